// RPN losses of AnchorHeadMulti as one forward kernel (+ the per-frame finalize of rpn_loss.hip) and one backward kernel over
// ALL heads and frames
//
// replaces, for one batch of head outputs:
//   AnchorHeadMulti.get_cls_layer_loss       (pcdet/models/dense_heads/anchor_head_multi.py:245-301)
//   AnchorHeadMulti.get_box_reg_layer_loss   (:303-373)
// which loop over the heads in Python: per head the ~45 elementwise / reduction launches of the single-head losses, on slices of
// the labels, targets and anchors. The single-head kernels of rpn_loss.hip cannot be called head by head: the three losses are
// normalised by a frame's positives over all heads TOGETHER, and each head has its own class columns.
//
// Anchors are indexed in the multi-head order (all anchors of head 0, then head 1, ...): labels (B,A), reg_targets (B,A,7) and
// anchors (A,7) are whole, the predictions (and gradients) live in one tensor per head. The forward pass walks the A anchors of a
// frame exactly as rpn_loss_partial_kernel does and looks the head of an anchor up in a table held in the kernel arguments (<= 16
// entries, scalar registers); the backward pass gives every head its own 256-anchor blocks so that each gradient tensor is
// written whole, as contiguous runs, in the head's own layout. Per-term arithmetic: rpn_loss_terms.h, shared with rpn_loss.hip.
// Sums are taken in a fixed order (per-thread, wave shuffle tree, 4 waves, blocks in index order): bit-reproducible.
#include "crb_common.h"
#include "../../include/crb_hip.h"
#include "rpn_loss_terms.h"

namespace {

constexpr int TPB = RPN_TPB;
constexpr int MAX_NC = 8, MAX_NB = 8;
constexpr int FWD_PER_THREAD = 4;

struct MhArgs {
  CrbMultiHeadEntry head[CRB_MULTIHEAD_MAX_HEADS];
  int blk_start[CRB_MULTIHEAD_MAX_HEADS + 1];   // backward: first 256-anchor block of every head
  int num_heads;
  const int32_t* labels;  // (B, A)  -1 ignored, 0 background, c > 0 class
  const float* tgt;       // (B, A, 7)
  const float* anchors;   // (A, 7)
  int B, A, num_class, NB, has_dir;
  float alpha, gamma, beta, dir_offset;
  float cw[7];
  float w_cls, w_loc, w_dir, w_pos, w_neg;
};

// head of global anchor i (the table is sorted by anchor_start and covers [0, A))
__device__ __forceinline__ int head_of(const MhArgs& a, int i) {
  int h = 0;
  for (int k = 1; k < a.num_heads; ++k)
    if (i >= a.head[k].anchor_start) h = k;
  return h;
}

// partial (B, nblk, 4) = {cls, loc, dir, npos} un-normalised sums of the block's anchors
__global__ __launch_bounds__(TPB) void multihead_loss_partial_kernel(MhArgs a, float* __restrict__ partial) {
  const int b = blockIdx.y, nblk = gridDim.x;
  const int64_t fb = (int64_t)b * a.A;
  float s_cls = 0.0f, s_loc = 0.0f, s_dir = 0.0f, s_pos = 0.0f;
#pragma unroll
  for (int it = 0; it < FWD_PER_THREAD; ++it) {
    const int i = (blockIdx.x * FWD_PER_THREAD + it) * TPB + threadIdx.x;
    if (i >= a.A) break;
    const int lab = a.labels[fb + i];
    if (lab < 0) continue;
    const int h = head_of(a, i);
    const CrbMultiHeadEntry& e = a.head[h];
    const int64_t row = (int64_t)b * e.anchor_count + (i - e.anchor_start);
    const int tc = lab > 0 ? (a.num_class == 1 ? 1 : lab) : 0;
    const float w = lab > 0 ? a.w_pos : a.w_neg;
    const float* x = e.cls + row * e.class_count;
    for (int c = 0; c < e.class_count; ++c) {
      float l, d;
      focal_term(x[c], tc == e.class_start + c + 1, a.alpha, a.gamma, l, d);
      s_cls += l * w;
    }
    if (lab > 0) {
      s_pos += 1.0f;
      const float* t = a.tgt + (fb + i) * 7;
      if (a.has_dir) {
        s_loc += box_term<true>(e.box + row * 7, t, a.cw, a.beta, nullptr);
        s_dir += dir_term(e.dir + row * a.NB, a.NB, dir_bin(t[6], a.anchors[(int64_t)i * 7 + 6], a.dir_offset, a.NB), nullptr);
      } else {
        s_loc += box_term<false>(e.box + row * 7, t, a.cw, a.beta, nullptr);
      }
    }
  }
  block_partial_store(s_cls, s_loc, s_dir, s_pos, partial + ((int64_t)b * nblk + blockIdx.x) * 4);
}

// gradients of sum_b sum_k gout[b,k] * loss[b,k] w.r.t. every head's three prediction tensors; a block = 256 consecutive anchors of
// one head of one frame, gradients staged in LDS and stored as contiguous runs
__global__ __launch_bounds__(TPB) void multihead_loss_backward_kernel(MhArgs a, const float* __restrict__ npos,
                                                                      const float* __restrict__ gout) {
  __shared__ float s_cls[TPB * MAX_NC];
  __shared__ float s_box[TPB * 7];
  __shared__ float s_dir[TPB * MAX_NB];
  const int b = blockIdx.y;
  int h = 0;
  for (int k = 1; k < a.num_heads; ++k)
    if ((int)blockIdx.x >= a.blk_start[k]) h = k;
  const CrbMultiHeadEntry& e = a.head[h];
  const int NC = e.class_count;
  const int l0 = ((int)blockIdx.x - a.blk_start[h]) * TPB, li = l0 + threadIdx.x;     // anchor inside the head
  const int cnt = min(TPB, e.anchor_count - l0);
  const int64_t hb = (int64_t)b * e.anchor_count;
  const float inv = 1.0f / fmaxf(npos[b], 1.0f);
  const float g_cls = gout[b * 3 + 0] * a.w_cls * inv, g_loc = gout[b * 3 + 1] * a.w_loc * inv,
              g_dir = gout[b * 3 + 2] * a.w_dir * inv;
  if (li < e.anchor_count) {
    const int i = e.anchor_start + li;                                                 // anchor in the multi-head order
    const int lab = a.labels[(int64_t)b * a.A + i];
    const int tc = lab > 0 ? (a.num_class == 1 ? 1 : lab) : 0;
    const float w = lab > 0 ? a.w_pos : a.w_neg;
    const float* x = e.cls + (hb + li) * NC;
    for (int c = 0; c < NC; ++c) {
      float l, d = 0.0f;
      if (lab >= 0) focal_term(x[c], tc == e.class_start + c + 1, a.alpha, a.gamma, l, d);
      s_cls[threadIdx.x * NC + c] = lab >= 0 ? d * w * g_cls : 0.0f;
    }
    float gb[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float gd[MAX_NB];
#pragma unroll
    for (int k = 0; k < MAX_NB; ++k) gd[k] = 0.0f;
    if (lab > 0) {
      const float* t = a.tgt + ((int64_t)b * a.A + i) * 7;
      if (a.has_dir) {
        box_term<true>(e.box + (hb + li) * 7, t, a.cw, a.beta, gb);
        dir_term(e.dir + (hb + li) * a.NB, a.NB, dir_bin(t[6], a.anchors[(int64_t)i * 7 + 6], a.dir_offset, a.NB), gd);
      } else {
        box_term<false>(e.box + (hb + li) * 7, t, a.cw, a.beta, gb);
      }
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) s_box[threadIdx.x * 7 + d] = gb[d] * g_loc;
    if (a.has_dir)
#pragma unroll
      for (int k = 0; k < MAX_NB; ++k)
        if (k < a.NB) s_dir[threadIdx.x * a.NB + k] = gd[k] * g_dir;
  }
  __syncthreads();
  float* oc = e.d_cls + (hb + l0) * NC;
  for (int k = threadIdx.x; k < cnt * NC; k += TPB) oc[k] = s_cls[k];
  float* ob = e.d_box + (hb + l0) * 7;
  for (int k = threadIdx.x; k < cnt * 7; k += TPB) ob[k] = s_box[k];
  if (a.has_dir) {
    float* od = e.d_dir + (hb + l0) * a.NB;
    for (int k = threadIdx.x; k < cnt * a.NB; k += TPB) od[k] = s_dir[k];
  }
}

bool fill_args(MhArgs& a, const CrbMultiHeadEntry* heads, int num_heads, const int32_t* labels, const float* tgt,
               const float* anchors, int B, int A, const CrbRpnLossCfg* cfg, float w_pos, float w_neg, bool backward) {
  if (!heads || num_heads < 1 || num_heads > CRB_MULTIHEAD_MAX_HEADS || !labels || !tgt || !cfg || B < 0 || A < 0) return false;
  if (cfg->num_class < 1) return false;
  const bool has_dir = heads[0].dir != nullptr;
  if (has_dir && (cfg->num_dir_bins < 1 || cfg->num_dir_bins > MAX_NB || !anchors)) return false;
  int next = 0, blk = 0;
  for (int h = 0; h < num_heads; ++h) {
    const CrbMultiHeadEntry& e = heads[h];
    // the heads tile [0, A) in order: no anchor is read or written through two entries, none past a tensor's end
    if (!e.cls || !e.box || (e.dir != nullptr) != has_dir || e.anchor_start != next || e.anchor_count < 1) return false;
    if (e.class_count < 1 || e.class_count > MAX_NC || e.class_start < 0) return false;
    if (backward && (!e.d_cls || !e.d_box || (has_dir && !e.d_dir))) return false;
    a.head[h] = e;
    a.blk_start[h] = blk;
    blk += (e.anchor_count + TPB - 1) / TPB;
    next += e.anchor_count;
  }
  if (next != A) return false;
  for (int h = num_heads; h < CRB_MULTIHEAD_MAX_HEADS; ++h) {
    a.head[h] = CrbMultiHeadEntry{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, A, 0, 0, 0};
    a.blk_start[h] = blk;
  }
  a.blk_start[CRB_MULTIHEAD_MAX_HEADS] = blk;
  a.num_heads = num_heads;
  a.labels = labels;
  a.tgt = tgt;
  a.anchors = anchors;
  a.B = B;
  a.A = A;
  a.num_class = cfg->num_class;
  a.has_dir = has_dir ? 1 : 0;
  a.NB = has_dir ? cfg->num_dir_bins : 1;
  a.alpha = cfg->alpha;
  a.gamma = cfg->gamma;
  a.beta = cfg->beta;
  a.dir_offset = cfg->dir_offset;
  for (int d = 0; d < 7; ++d) a.cw[d] = cfg->code_weights[d];
  a.w_cls = cfg->cls_weight;
  a.w_loc = cfg->loc_weight;
  a.w_dir = cfg->dir_weight;
  a.w_pos = w_pos;
  a.w_neg = w_neg;
  return true;
}

int fwd_blocks(int A) { return (A + TPB * FWD_PER_THREAD - 1) / (TPB * FWD_PER_THREAD); }

}  // namespace

extern "C" {

int64_t crb_multihead_loss_workspace_bytes(int B, int A) {
  if (B <= 0 || A <= 0) return 16;
  return (int64_t)B * fwd_blocks(A) * 4 * sizeof(float);
}

int crb_multihead_loss_forward(const CrbMultiHeadEntry* heads, int num_heads, const int32_t* labels, const float* reg_targets,
                               const float* anchors, int B, int A, const CrbRpnLossCfg* cfg, float pos_cls_weight,
                               float neg_cls_weight, float* loss, float* npos, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  if (B == 0 && loss && npos) return CRB_OK;
  if (A <= 0) return CRB_ERR_ARG;
  MhArgs a;
  if (!fill_args(a, heads, num_heads, labels, reg_targets, anchors, B, A, cfg, pos_cls_weight, neg_cls_weight, false) || !loss ||
      !npos)
    return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_multihead_loss_workspace_bytes(B, A)) return CRB_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = fwd_blocks(A);
  float* partial = (float*)workspace;
  hipLaunchKernelGGL(multihead_loss_partial_kernel, dim3(nblk, B), dim3(TPB), 0, s, a, partial);
  hipLaunchKernelGGL(rpn_loss_finalize_kernel, dim3(B), dim3(TPB), 0, s, partial, nblk, a.w_cls, a.w_loc,
                     a.has_dir ? a.w_dir : 0.0f, loss, npos);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

int crb_multihead_loss_backward(const CrbMultiHeadEntry* heads, int num_heads, const int32_t* labels, const float* reg_targets,
                                const float* anchors, int B, int A, const CrbRpnLossCfg* cfg, float pos_cls_weight,
                                float neg_cls_weight, const float* npos, const float* grad_loss, void* stream) {
  if (B == 0) return CRB_OK;
  if (A <= 0) return CRB_ERR_ARG;
  MhArgs a;
  if (!fill_args(a, heads, num_heads, labels, reg_targets, anchors, B, A, cfg, pos_cls_weight, neg_cls_weight, true) || !npos ||
      !grad_loss)
    return CRB_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(multihead_loss_backward_kernel, dim3(a.blk_start[CRB_MULTIHEAD_MAX_HEADS], B), dim3(TPB), 0, s, a, npos,
                     grad_loss);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

}  // extern "C"
