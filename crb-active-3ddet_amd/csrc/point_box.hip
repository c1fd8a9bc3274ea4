// Box branch of the point heads (PointIntraPartOffsetHead with TARGET_CONFIG.BOX_CODER: PartA2_free.yaml; PointHeadBox): box
// targets of every voxel centre in one launch, the focal + part-offset + box-regression losses with their gradients in two, and
// the decode of the per-point boxes into the dense, frame-padded tensors the proposal layer takes.
//
// replaces, per batch:
//   PointHeadTemplate.assign_stack_targets with ret_box_labels=True (pcdet/models/dense_heads/point_head_template.py:49-129): the loop
//       over the frames with a boolean-mask gather (a host sync) each, plus PointResidualCoder.encode_torch (box_coder_utils.py:153-187)
//   get_cls_layer_loss, get_part_layer_loss, get_box_layer_loss (:131-195) with WeightedSmoothL1Loss (loss_utils.py:75-134) and
//       their autograd
//   generate_predicted_boxes (:197-211) with PointResidualCoder.decode_torch (:189-221) and the per-frame mask loop of
//       RoIHeadTemplate.proposal_layer (roi_head_template.py:70-76)
// The target search and the tile / partials structure of the losses are those of csrc/part_head.hip (part_head_common.h): labels,
// owners and part labels are the same bits, sums are f64 in a fixed order, there are no atomics and no host read-back.
#include "crb_common.h"
#include "focal_term.h"
#include "part_head_common.h"
#include "../../include/crb_hip.h"

namespace {

struct CodeWeights { float w[8]; };

// a row of 8 codes as two 16-byte accesses (rows of (n,8) f32 tensors are 32-byte aligned)
__device__ __forceinline__ void load_row8(const float* __restrict__ p, float* v) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store_row8(float* __restrict__ p, const float* v) {
  reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// grid (cdiv(N, 256), B), as part_targets_kernel. mean (K,3): the anchor sizes of the classes 1 .. K
__global__ __launch_bounds__(256) void point_box_targets_kernel(int G, int num_class, int K, float ew0, float ew1, float ew2,
                                                                const float* __restrict__ pts, const int* __restrict__ off,
                                                                const float* __restrict__ gt, const float* __restrict__ mean,
                                                                int64_t* __restrict__ labels, int* __restrict__ owner,
                                                                float* __restrict__ box, float* __restrict__ part) {
  __shared__ PartBoxLds sb[PT_CHUNK];
  const int b = blockIdx.y;
  const int n0 = off[b], n1 = off[b + 1];
  const int base = n0 + (int)blockIdx.x * 256;
  if (base >= n1) return;                                   // uniform per workgroup
  const int i = base + (int)threadIdx.x;
  const bool active = i < n1;
  float x = 0.f, y = 0.f, z = 0.f;
  if (active) {
    const float* p = pts + (int64_t)i * 4;
    x = p[1]; y = p[2]; z = p[3];
  }
  const float* fb = gt + (int64_t)b * G * 8;
  bool shell;
  const int found = part_find_owner(sb, fb, G, ew0, ew1, ew2, active, x, y, z, shell);
  if (!active) return;
  float pl[3] = {0.f, 0.f, 0.f};
  float code[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (found >= 0) {
    const float* r = fb + (int64_t)found * 8;
    part_offsets(r, x, y, z, pl);
    // PointResidualCoder.encode_torch with use_mean_size, in f64 from the f32 inputs, rounded once. The anchor is the mean size of the
    // ground truth's class column (also when num_class == 1 labels the point 1); a class outside 1 .. K is clamped into it
    const int c = min(max((int)r[7], 1), K) - 1;
    const double dxa = (double)mean[c * 3], dya = (double)mean[c * 3 + 1], dza = (double)mean[c * 3 + 2];
    const double diag = sqrt(dxa * dxa + dya * dya);
    const double dxg = (double)fmaxf(r[3], 1e-5f), dyg = (double)fmaxf(r[4], 1e-5f), dzg = (double)fmaxf(r[5], 1e-5f);
    code[0] = (float)(((double)r[0] - (double)x) / diag);
    code[1] = (float)(((double)r[1] - (double)y) / diag);
    code[2] = (float)(((double)r[2] - (double)z) / dza);
    code[3] = (float)log(dxg / dxa);
    code[4] = (float)log(dyg / dya);
    code[5] = (float)log(dzg / dza);
    code[6] = (float)cos((double)r[6]);
    code[7] = (float)sin((double)r[6]);
  }
  labels[i] = part_label(fb, found, shell, num_class);
  owner[i] = found;
  store_row8(box + (int64_t)i * 8, code);
  if (part) { part[(int64_t)i * 3] = pl[0]; part[(int64_t)i * 3 + 1] = pl[1]; part[(int64_t)i * 3 + 2] = pl[2]; }
}

// WeightedSmoothL1Loss.forward for one code (loss_utils.py:104-134): a NaN target is replaced by the input, the difference is
// weighted, then smooth-L1 with beta (plain L1 below 1e-5). d: derivative w.r.t. the input. In f64 from the f32 inputs (a handful of
// multiplications per code): the difference of two close f32 numbers is then exact and the term carries no rounding of its own
__device__ __forceinline__ void box_term(float x, float t, float w, double bd, double& loss, double& d) {
  const double wd = (double)w;
  const double diff = (isnan(t) ? 0.0 : (double)x - (double)t) * wd;
  const double n = fabs(diff);
  if (bd < 1e-5) {
    loss = n;
    d = diff > 0.0 ? wd : (diff < 0.0 ? -wd : 0.0);
  } else if (n < bd) {
    loss = 0.5 * n * n / bd;
    d = diff / bd * wd;
  } else {
    loss = n - 0.5 * bd;
    d = diff > 0.0 ? wd : -wd;
  }
}

// partials (tiles, 4) f64 = {focal terms over rows with label >= 0, part terms, box terms, positives (the last three over label > 0)}
__global__ __launch_bounds__(LOSS_TPB) void point_box_loss_partial_kernel(const float* __restrict__ cls, const float* __restrict__ prt,
                                                                          const float* __restrict__ bx, const int64_t* __restrict__ labels,
                                                                          const float* __restrict__ pl, const float* __restrict__ bl,
                                                                          int64_t n, int C, float alpha, float gamma, CodeWeights cw,
                                                                          double beta, double* __restrict__ partials) {
  __shared__ double sh[LOSS_TPB / 64];
  double s_cls = 0.0, s_part = 0.0, s_box = 0.0, s_pos = 0.0;
#pragma unroll
  for (int k = 0; k < LOSS_ROWS; ++k) {
    const int64_t i = (int64_t)blockIdx.x * LOSS_TILE + k * LOSS_TPB + threadIdx.x;
    if (i >= n) continue;
    const int64_t lab = labels[i];
    if (lab >= 0)
      for (int c = 0; c < C; ++c) {
        float l, d;
        focal_term(cls[i * C + c], lab == c + 1, alpha, gamma, l, d);
        s_cls += (double)l;
      }
    if (lab > 0) {
      s_pos += 1.0;
      if (prt)
        for (int a = 0; a < 3; ++a) s_part += (double)part_bce(prt[i * 3 + a], pl[i * 3 + a]);
      float x[8], t[8];
      load_row8(bx + i * 8, x);
      load_row8(bl + i * 8, t);
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        double l, d;
        box_term(x[a], t[a], cw.w[a], beta, l, d);
        s_box += l;
      }
    }
  }
  const double t_cls = loss_block_sum(s_cls, sh), t_part = loss_block_sum(s_part, sh), t_box = loss_block_sum(s_box, sh),
               t_pos = loss_block_sum(s_pos, sh);
  if (threadIdx.x == 0) {
    double* o = partials + (int64_t)blockIdx.x * 4;
    o[0] = t_cls; o[1] = t_part; o[2] = t_box; o[3] = t_pos;
  }
}

// out (4) f64 = {point_loss_cls, point_loss_part, point_loss_box, positives}; d_cls (n,C), d_prt (n,3), d_box (n,8) = d loss / d
// prediction for unit upstream gradients
__global__ __launch_bounds__(LOSS_TPB) void point_box_loss_finish_kernel(const float* __restrict__ cls, const float* __restrict__ prt,
                                                                         const float* __restrict__ bx, const int64_t* __restrict__ labels,
                                                                         const float* __restrict__ pl, const float* __restrict__ bl,
                                                                         int64_t n, int C, float alpha, float gamma, CodeWeights cw,
                                                                         double beta, float w_cls, float w_part, float w_box,
                                                                         const double* __restrict__ partials, int tiles,
                                                                         double* __restrict__ out, float* __restrict__ d_cls,
                                                                         float* __restrict__ d_prt, float* __restrict__ d_box) {
  __shared__ double shd[LOSS_TPB / 64];
  double a_cls = 0.0, a_part = 0.0, a_box = 0.0, a_pos = 0.0;
  for (int t = threadIdx.x; t < tiles; t += LOSS_TPB) {
    a_cls += partials[(int64_t)t * 4];
    a_part += partials[(int64_t)t * 4 + 1];
    a_box += partials[(int64_t)t * 4 + 2];
    a_pos += partials[(int64_t)t * 4 + 3];
  }
  const double S_cls = loss_block_sum(a_cls, shd), S_part = loss_block_sum(a_part, shd), S_box = loss_block_sum(a_box, shd),
               pos = loss_block_sum(a_pos, shd);
  const double norm = pos > 1.0 ? pos : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = S_cls / norm * (double)w_cls;
    out[1] = S_part / (3.0 * norm) * (double)w_part;
    out[2] = S_box / norm * (double)w_box;
    out[3] = pos;
  }
  const float g_cls = (float)((double)w_cls / norm), g_part = (float)((double)w_part / (3.0 * norm));
  const double g_box = (double)w_box / norm;
#pragma unroll
  for (int k = 0; k < LOSS_ROWS; ++k) {
    const int64_t i = (int64_t)blockIdx.x * LOSS_TILE + k * LOSS_TPB + threadIdx.x;
    if (i >= n) continue;
    const int64_t lab = labels[i];
    for (int c = 0; c < C; ++c) {
      float l = 0.f, d = 0.f;
      if (lab >= 0) focal_term(cls[i * C + c], lab == c + 1, alpha, gamma, l, d);
      d_cls[i * C + c] = d * g_cls;
    }
    if (prt)
      for (int a = 0; a < 3; ++a) {
        float d = 0.f;
        if (lab > 0) {
          const float x = prt[i * 3 + a];
          d = (1.0f / (1.0f + expf(-x)) - pl[i * 3 + a]) * g_part;
        }
        d_prt[i * 3 + a] = d;
      }
    float db[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (lab > 0) {
      float x[8], t[8];
      load_row8(bx + i * 8, x);
      load_row8(bl + i * 8, t);
#pragma unroll
      for (int a = 0; a < 8; ++a) {
        double l, d;
        box_term(x[a], t[a], cw.w[a], beta, l, d);
        db[a] = (float)(d * g_box);
      }
    }
    store_row8(d_box + i * 8, db);
  }
}

// g (3) device = upstream gradients of {point_loss_cls, point_loss_part, point_loss_box}; d_prt may be null (no part branch)
__global__ __launch_bounds__(256) void point_box_loss_scale_kernel(const float* __restrict__ d_cls, const float* __restrict__ d_prt,
                                                                   const float* __restrict__ d_box, const float* __restrict__ g,
                                                                   int64_t n_cls, int64_t n_prt, int64_t n_box, float* __restrict__ o_cls,
                                                                   float* __restrict__ o_prt, float* __restrict__ o_box) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_cls) o_cls[i] = d_cls[i] * g[0];
  if (i < n_prt) o_prt[i] = d_prt[i] * g[1];
  if (i < n_box) o_box[i] = d_box[i] * g[2];
}

// grid (cdiv(amax, 256), B): row j of frame b. Rows of the frame: the argmax class (first maximum) picks the anchor size, then
// PointResidualCoder.decode_torch in f64 from the f32 inputs, rounded once; rows past the frame's count: logits -inf, a zero box
__global__ __launch_bounds__(256) void point_box_decode_kernel(const float* __restrict__ pts, const int* __restrict__ off,
                                                               const float* __restrict__ cls, const float* __restrict__ bx,
                                                               const float* __restrict__ mean, int64_t N, int amax, int C,
                                                               float* __restrict__ o_cls, float* __restrict__ o_box,
                                                               int* __restrict__ counts) {
  const int b = blockIdx.y;
  const int n0 = off[b], cnt = off[b + 1] - n0;
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[b] = max(cnt, 0);           // unclamped: a value above amax tells the caller that its bound dropped rows
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= amax) return;
  float* oc = o_cls + ((int64_t)b * amax + j) * C;
  float* ob = o_box + ((int64_t)b * amax + j) * 7;
  const int64_t i = (int64_t)n0 + j;
  if (j >= cnt || i < 0 || i >= N) {
    for (int c = 0; c < C; ++c) oc[c] = -INFINITY;
#pragma unroll
    for (int a = 0; a < 7; ++a) ob[a] = 0.f;
    return;
  }
  int best = 0;
  float top = cls[i * C];
  oc[0] = top;
  for (int c = 1; c < C; ++c) {
    const float v = cls[i * C + c];
    oc[c] = v;
    if (v > top) { top = v; best = c; }
  }
  const double dxa = (double)mean[best * 3], dya = (double)mean[best * 3 + 1], dza = (double)mean[best * 3 + 2];
  const double diag = sqrt(dxa * dxa + dya * dya);
  const float* e = bx + i * 8;
  const float* p = pts + i * 4;
  ob[0] = (float)((double)e[0] * diag + (double)p[1]);
  ob[1] = (float)((double)e[1] * diag + (double)p[2]);
  ob[2] = (float)((double)e[2] * dza + (double)p[3]);
  ob[3] = (float)(exp((double)e[3]) * dxa);
  ob[4] = (float)(exp((double)e[4]) * dya);
  ob[5] = (float)(exp((double)e[5]) * dza);
  ob[6] = (float)atan2((double)e[7], (double)e[6]);
}

inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

}  // namespace

extern "C" int crb_point_box_targets(const float* points, const int32_t* frame_offsets, const float* gt_boxes, int B, int64_t N, int G,
                                     const float* extra_width, int num_class, const float* mean_size, int K, int64_t* labels,
                                     int32_t* owner, float* box_labels, float* part_labels, void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || N >= (1LL << 31) - 256 || G < 0 || num_class <= 0 || K <= 0 || !extra_width) return CRB_ERR_ARG;
  if (N == 0) return CRB_OK;
  if (!points || !frame_offsets || (G > 0 && !gt_boxes) || !mean_size || !labels || !owner || !box_labels) return CRB_ERR_ARG;
  if (misaligned16(box_labels)) return CRB_ERR_ARG;
  hipLaunchKernelGGL(point_box_targets_kernel, dim3(crb_cdiv(N, 256), B), dim3(256), 0, (hipStream_t)stream, G, num_class, K,
                     extra_width[0], extra_width[1], extra_width[2], points, frame_offsets, gt_boxes, mean_size, labels, owner,
                     box_labels, part_labels);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_point_box_loss_workspace_bytes(int64_t n) {
  return (int64_t)sizeof(double) * 4 * (n <= 0 ? 1 : (n + LOSS_TILE - 1) / LOSS_TILE);
}

extern "C" int crb_point_box_loss_forward(const float* cls_preds, const float* part_preds, const float* box_preds, const int64_t* labels,
                                          const float* part_labels, const float* box_labels, int64_t n, int C, float alpha, float gamma,
                                          const float* code_weights, double beta, float cls_weight, float part_weight, float box_weight,
                                          double* loss, float* d_cls, float* d_part, float* d_box, void* workspace,
                                          int64_t workspace_bytes, void* stream) {
  if (n < 0 || n >= (1LL << 31) / 8 || C <= 0 || !loss || !code_weights || !(beta >= 0.0)) return CRB_ERR_ARG;
  if (workspace_bytes < crb_point_box_loss_workspace_bytes(n) || !workspace) return CRB_ERR_WORKSPACE;
  if (n > 0 && (!cls_preds || !box_preds || !labels || !box_labels || !d_cls || !d_box)) return CRB_ERR_ARG;
  if (n > 0 && part_preds && (!part_labels || !d_part)) return CRB_ERR_ARG;
  if (misaligned16(box_preds) || misaligned16(box_labels) || misaligned16(d_box)) return CRB_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)((n + LOSS_TILE - 1) / LOSS_TILE);
  double* partials = (double*)workspace;
  CodeWeights cw;
  for (int a = 0; a < 8; ++a) cw.w[a] = code_weights[a];
  if (tiles > 0)
    hipLaunchKernelGGL(point_box_loss_partial_kernel, dim3(tiles), dim3(LOSS_TPB), 0, st, cls_preds, part_preds, box_preds, labels,
                       part_labels, box_labels, n, C, alpha, gamma, cw, beta, partials);
  // (n == 0: one workgroup with no tile writes the four zeros)
  hipLaunchKernelGGL(point_box_loss_finish_kernel, dim3(tiles > 0 ? tiles : 1), dim3(LOSS_TPB), 0, st, cls_preds, part_preds, box_preds,
                     labels, part_labels, box_labels, n, C, alpha, gamma, cw, beta, cls_weight, part_weight, box_weight, partials, tiles,
                     loss, d_cls, d_part, d_box);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_point_box_loss_backward(const float* d_cls, const float* d_part, const float* d_box, const float* grad_losses,
                                           int64_t n, int C, float* grad_cls, float* grad_part, float* grad_box, void* stream) {
  if (n < 0 || n >= (1LL << 31) / 8 || C <= 0) return CRB_ERR_ARG;
  if (n == 0) return CRB_OK;
  if (!d_cls || !d_box || !grad_losses || !grad_cls || !grad_box || (d_part && !grad_part)) return CRB_ERR_ARG;
  const int64_t m = n * (C > 8 ? C : 8);
  hipLaunchKernelGGL(point_box_loss_scale_kernel, dim3(crb_cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, d_cls, d_part, d_box,
                     grad_losses, n * C, d_part ? n * 3 : 0, n * 8, grad_cls, grad_part, grad_box);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_point_box_decode(const float* points, const int32_t* frame_offsets, const float* cls_preds, const float* box_preds,
                                    const float* mean_size, int B, int64_t N, int amax, int C, int K, float* batch_cls_preds,
                                    float* batch_box_preds, int32_t* counts, void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || N >= (1LL << 31) / 8 || amax < 0 || C <= 0 || C > K || !frame_offsets || !counts)
    return CRB_ERR_ARG;
  if ((int64_t)B * amax * (C > 7 ? C : 7) >= (1LL << 40)) return CRB_ERR_ARG;
  if (N > 0 && (!points || !cls_preds || !box_preds)) return CRB_ERR_ARG;
  if (!mean_size || (amax > 0 && (!batch_cls_preds || !batch_box_preds))) return CRB_ERR_ARG;
  // (amax == 0: one workgroup per frame still writes the counts)
  hipLaunchKernelGGL(point_box_decode_kernel, dim3(amax > 0 ? crb_cdiv(amax, 256) : 1, B), dim3(256), 0, (hipStream_t)stream, points,
                     frame_offsets, cls_preds, box_preds, mean_size, N, amax, C, batch_cls_preds, batch_box_preds, counts);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
