// Per-class selection of a whole batch around the batched NMS: MULTI_CLASSES_NMS of a multi-head detector
//
// replaces the frames x heads x classes loop of Detector3DTemplate.post_processing (pcdet/models/detectors/detector3d_template.py:
// 292-317) around model_nms_utils.multi_classes_nms (pcdet/models/model_utils/model_nms_utils.py:28-66): per iteration a boolean
// mask (a synchronising nonzero), a topk, an NMS and a slice — 48 iterations on 70,400 anchors each for the KITTI multi-head
// configuration at 16 frames. Here a segment is one (frame, head, class) triple and all S of them go through
//   crb_multiclass_candidates   (this file)            threshold + the best PRE per segment, in order
//   crb_decode_selected_anchors (proposal_layer.hip)   once per head, the picks only
//   crb_nms_batched             (iou3d_nms.hip)        S segments
//   crb_multiclass_finish       (this file)            survivors of a frame's segments one after another
// with no host synchronisation in between.
//
// Candidates: one 1024-thread workgroup per segment reads the segment's logit column in the head's own (B, A_h, C_h) layout
// (stride C_h) and orders anchors by the 64-bit key (f32 bits of the sigmoid score, ~anchor index): larger key = better score, then
// smaller index; keys are unique, so the result does not depend on the launch shape or on the order atomics retire.
//   pass 0      count the anchors at or above the threshold (n)
//   n > quota   radix select of the quota-th largest key: one 256-bin LDS histogram per 8-bit digit, most significant first; the
//               four digits of the index half are skipped when the cut does not fall inside a run of equal scores
//   last pass   keys at or above the cut into LDS (slot by LDS atomic: any order), bitonic sort, write
// The score of an anchor is recomputed in every pass (an exp and a divide on 69 logits per thread) instead of being stored.
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

constexpr int CT = 1024;              // threads of a candidates workgroup
constexpr int MAX_PRE = 4096;         // keys sorted in LDS (32 KB)
constexpr int MAX_SEG = CRB_MULTIHEAD_MAX_HEADS * 8;

struct McHead {
  const float* cls;                   // (B, A_h, C_h)
  int A, C, seg_start;
};

struct McArgs {
  McHead head[CRB_MULTIHEAD_MAX_HEADS];
  int num_heads, B, SEG;
};

// the f32 sigmoid the loop route's torch.sigmoid computes, as a sort key with the anchor index
__device__ __forceinline__ bool cand_key(const float* __restrict__ x, int i, int C, float thresh, unsigned long long& key) {
  const float v = x[(int64_t)i * C];
  const float p = 1.0f / (1.0f + expf(-v));
  if (!(p >= thresh)) return false;                                      // (NaN logits are no candidates)
  key = ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
  return true;
}

__global__ __launch_bounds__(CT) void multiclass_candidates_kernel(McArgs a, float thresh, int pre_max, int64_t* __restrict__ top_idx,
                                                                   float* __restrict__ top_logit, int32_t* __restrict__ counts) {
  __shared__ unsigned long long keys[MAX_PRE];
  __shared__ int hist[256];
  __shared__ int sh_n, sh_fill, sh_rem, sh_done;     // sh_n: anchors that pass; sh_fill: slots of keys[] handed out
  __shared__ unsigned long long sh_prefix;
  const int tid = threadIdx.x;
  const int s = blockIdx.x;                                              // head-major segment row
  int h = 0;
  for (int k = 1; k < a.num_heads; ++k)
    if (s >= a.B * a.head[k].seg_start) h = k;
  const int A = a.head[h].A, C = a.head[h].C;
  const int r = s - a.B * a.head[h].seg_start;
  const int b = r / C, c = r % C;
  const float* x = a.head[h].cls + (int64_t)b * A * C + c;
  const int K = min(pre_max, A);

  if (tid == 0) {
    sh_n = 0;
    sh_fill = 0;
  }
  __syncthreads();
  int cnt = 0;
  for (int i = tid; i < A; i += CT) {
    unsigned long long key;
    cnt += cand_key(x, i, C, thresh, key) ? 1 : 0;
  }
  if (cnt) atomicAdd(&sh_n, cnt);
  __syncthreads();
  const int n = sh_n;                                                    // (never written again: every wave reads the same count)
  unsigned long long cut = 0;                                            // keys >= cut are kept
  int m = n;
  if (n > K) {
    m = K;
    unsigned long long prefix = 0, mask = 0;
    if (tid == 0) {
      sh_rem = K;
      sh_done = 0;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
      for (int d = tid; d < 256; d += CT) hist[d] = 0;
      __syncthreads();
      for (int i = tid; i < A; i += CT) {
        unsigned long long key;
        if (cand_key(x, i, C, thresh, key) && (key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
      }
      __syncthreads();
      if (tid == 0) {
        int rem = sh_rem, d = 255;
        while (d > 0 && hist[d] < rem) rem -= hist[d--];
        sh_rem = rem;
        sh_prefix = prefix | ((unsigned long long)d << shift);
        // every anchor of the cut's score is taken: the index digits need no pass (prefix's low half stays 0)
        sh_done = (shift == 32 && hist[d] == rem) ? 1 : 0;
      }
      __syncthreads();
      prefix = sh_prefix;
      mask |= 255ull << shift;
      const int done = sh_done;
      __syncthreads();
      if (done) break;
    }
    cut = prefix;
  }

  for (int i = tid; i < A; i += CT) {
    unsigned long long key;
    if (cand_key(x, i, C, thresh, key) && key >= cut) {
      const int pos = atomicAdd(&sh_fill, 1);
      if (pos < MAX_PRE) keys[pos] = key;                                // (exactly m <= pre_max <= MAX_PRE keys pass)
    }
  }
  int P = 1;
  while (P < m) P <<= 1;
  __syncthreads();
  for (int t = m + tid; t < P; t += CT) keys[t] = 0;                     // below every key (the index half of a key is > 0)
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P; t += CT) {
        const int u = t ^ j;
        if (u > t) {
          const unsigned long long ka = keys[t], kb = keys[u];
          const bool desc = (t & k) == 0;
          if (desc ? ka < kb : ka > kb) {
            keys[t] = kb;
            keys[u] = ka;
          }
        }
      }
      __syncthreads();
    }
  for (int j = tid; j < pre_max; j += CT) {
    int64_t idx = 0;
    float v = 0.0f;
    if (j < m) {
      idx = (int64_t)(0xFFFFFFFFu - (uint32_t)(keys[j] & 0xFFFFFFFFull));
      v = x[idx * C];
    }
    top_idx[(int64_t)s * pre_max + j] = idx;
    top_logit[(int64_t)s * pre_max + j] = v;
  }
  if (tid == 0) counts[s] = m;
}

// one block per frame: the kept rows of the frame's SEG segments one after another
__global__ __launch_bounds__(256) void multiclass_finish_kernel(McArgs a, int pre_max, int post, const int32_t* __restrict__ keep,
                                                                const int32_t* __restrict__ num_keep, const int64_t* __restrict__ top_idx,
                                                                const float* __restrict__ top_logit, const float* __restrict__ top_boxes,
                                                                const int64_t* __restrict__ label_map, float* __restrict__ pred_boxes,
                                                                float* __restrict__ pred_logit, int64_t* __restrict__ pred_labels,
                                                                int64_t* __restrict__ pred_anchor, int32_t* __restrict__ seg_of,
                                                                int32_t* __restrict__ num) {
  __shared__ int off[MAX_SEG + 1];
  __shared__ int row_of[MAX_SEG];
  const int b = blockIdx.x, P = a.SEG * post;
  if (threadIdx.x == 0) {
    int o = 0, g = 0;
    for (int h = 0; h < a.num_heads; ++h)
      for (int c = 0; c < a.head[h].C; ++c, ++g) {
        const int row = a.B * a.head[h].seg_start + b * a.head[h].C + c;
        row_of[g] = row;
        off[g] = o;
        o += min(max(num_keep[row], 0), post);
      }
    off[a.SEG] = o;
    num[b] = o;
  }
  __syncthreads();
  const int64_t ob = (int64_t)b * P;
  for (int g = 0; g < a.SEG; ++g) {
    const int row = row_of[g], nk = off[g + 1] - off[g];
    const int64_t lab = label_map[g];
    for (int j = threadIdx.x; j < nk; j += blockDim.x) {
      const int k = keep[(int64_t)row * post + j];
      const int64_t o = ob + off[g] + j;
      const bool ok = k >= 0 && k < pre_max;
      const int64_t src = (int64_t)row * pre_max + (ok ? k : 0);
#pragma unroll
      for (int d = 0; d < 7; ++d) pred_boxes[o * 7 + d] = ok ? top_boxes[src * 7 + d] : 0.0f;
      pred_logit[o] = ok ? top_logit[src] : 0.0f;
      pred_labels[o] = ok ? lab : 0;
      pred_anchor[o] = ok ? top_idx[src] : 0;
      seg_of[o] = ok ? g : 0;
    }
  }
  for (int j = off[a.SEG] + threadIdx.x; j < P; j += blockDim.x) {
    const int64_t o = ob + j;
#pragma unroll
    for (int d = 0; d < 7; ++d) pred_boxes[o * 7 + d] = 0.0f;
    pred_logit[o] = 0.0f;
    pred_labels[o] = 0;
    pred_anchor[o] = 0;
    seg_of[o] = 0;
  }
}

bool fill_args(McArgs& a, const CrbMultiHeadEntry* heads, int num_heads, int B) {
  if (!heads || num_heads < 1 || num_heads > CRB_MULTIHEAD_MAX_HEADS || B < 0) return false;
  int seg = 0;
  for (int h = 0; h < CRB_MULTIHEAD_MAX_HEADS; ++h) {
    if (h < num_heads) {
      const CrbMultiHeadEntry& e = heads[h];
      if (!e.cls || e.anchor_count < 1 || e.class_count < 1 || e.class_count > 8) return false;
      a.head[h] = McHead{e.cls, e.anchor_count, e.class_count, seg};
      seg += e.class_count;
    } else {
      a.head[h] = McHead{nullptr, 0, 1, seg};
    }
  }
  a.num_heads = num_heads;
  a.B = B;
  a.SEG = seg;
  return true;
}

}  // namespace

extern "C" {

int crb_multiclass_candidates(const CrbMultiHeadEntry* heads, int num_heads, int B, float score_thresh, int pre_max, int64_t* top_idx,
                              float* top_logit, int32_t* counts, void* stream) {
  McArgs a;
  if (!fill_args(a, heads, num_heads, B) || pre_max < 1 || !top_idx || !top_logit || !counts) return CRB_ERR_ARG;
  if (pre_max > MAX_PRE) return CRB_ERR_UNSUPPORTED;
  if (B == 0) return CRB_OK;
  hipLaunchKernelGGL(multiclass_candidates_kernel, dim3(B * a.SEG), dim3(CT), 0, (hipStream_t)stream, a, score_thresh, pre_max,
                     top_idx, top_logit, counts);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

int crb_multiclass_finish(const CrbMultiHeadEntry* heads, int num_heads, int B, int pre_max, int post, const int32_t* keep,
                          const int32_t* num_keep, const int64_t* top_idx, const float* top_logit, const float* top_boxes,
                          const int64_t* label_map, float* pred_boxes, float* pred_logit, int64_t* pred_labels, int64_t* pred_anchor,
                          int32_t* seg_of, int32_t* num, void* stream) {
  McArgs a;
  if (!fill_args(a, heads, num_heads, B) || pre_max < 1 || post < 1 || !keep || !num_keep || !top_idx || !top_logit || !top_boxes ||
      !label_map || !pred_boxes || !pred_logit || !pred_labels || !pred_anchor || !seg_of || !num)
    return CRB_ERR_ARG;
  if (B == 0) return CRB_OK;
  hipLaunchKernelGGL(multiclass_finish_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a, pre_max, post, keep, num_keep, top_idx,
                     top_logit, top_boxes, label_map, pred_boxes, pred_logit, pred_labels, pred_anchor, seg_of, num);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

}  // extern "C"
