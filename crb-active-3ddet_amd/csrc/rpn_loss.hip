// RPN losses of the anchor head as one forward kernel (+ a per-frame finalize) and one backward kernel  (row a11 of SURVEY §8)
//
// replaces, for one batch of head outputs:
//   AnchorHeadTemplate.get_cls_layer_loss      (pcdet/models/dense_heads/anchor_head_template.py:101-141)
//   AnchorHeadTemplate.add_sin_difference      (:143-152), get_direction_target (:154-166)
//   AnchorHeadTemplate.get_box_reg_layer_loss  (:168-214)
//   SigmoidFocalClassificationLoss.forward     (pcdet/utils/loss_utils.py:9-72)
//   WeightedSmoothL1Loss.forward               (:75-131), WeightedCrossEntropyLoss.forward (:168-188)
// which in torch are ~45 elementwise / reduction launches forward and as many backward over (B, A, .) tensors
// (A = 211,200 anchors per KITTI frame): 2.96 ms per SECOND step at bs = 16 (tools/time_rpn_loss.py).
//
// The three losses are sums over anchors of per-anchor terms divided by the frame's number of positive anchors, so one pass
// computes the un-normalised per-frame sums and the count, and a finalize divides (the reference multiplies every term by
// 1/max(npos,1) before summing: same value up to rounding of the sum). Only POSITIVE anchors (label > 0, ~0.1 %) have a
// regression / direction term: box and direction predictions and regression targets are read for those alone — the forward
// pass streams the labels and the class logits (16 B per anchor), the backward pass writes all three gradients (48 B per
// anchor, zeros for every anchor without a term) through LDS so the stores are whole contiguous runs.
// Sums are taken in a fixed order (per-thread, wave shuffle tree, 4 waves, blocks in index order): bit-reproducible.
#include "crb_common.h"
#include "../../include/crb_hip.h"
#include "rpn_loss_terms.h"      // the per-anchor terms and the fixed-order reductions, shared with multihead_loss.hip

namespace {

constexpr int TPB = RPN_TPB;
constexpr int MAX_NC = 8, MAX_NB = 8;

struct RpnArgs {
  const float* cls;       // (B, A, NC) logits
  const float* box;       // (B, A, 7)
  const float* dir;       // (B, A, NB) or null
  const int32_t* labels;  // (B, A)  -1 ignored, 0 background, c > 0 class
  const float* tgt;       // (B, A, 7) encoded regression targets
  const float* anchors;   // (A, 7)
  int B, A, NC, NB;
  float alpha, gamma, beta, dir_offset;
  float cw[7];
  float w_cls, w_loc, w_dir;
};

constexpr int FWD_PER_THREAD = 4;      // anchors per thread of the forward pass (strided by the block: coalesced label loads)

// partial (B, nblk, 4) = {cls, loc, dir, npos} un-normalised sums of the block's anchors
__global__ __launch_bounds__(TPB) void rpn_loss_partial_kernel(RpnArgs a, float* __restrict__ partial) {
  const int b = blockIdx.y, nblk = gridDim.x;
  const int64_t fb = (int64_t)b * a.A;
  float s_cls = 0.0f, s_loc = 0.0f, s_dir = 0.0f, s_pos = 0.0f;
#pragma unroll
  for (int it = 0; it < FWD_PER_THREAD; ++it) {
    const int i = (blockIdx.x * FWD_PER_THREAD + it) * TPB + threadIdx.x;
    if (i >= a.A) break;
    const int lab = a.labels[fb + i];
    if (lab >= 0) {
      const int tc = lab > 0 ? (a.NC == 1 ? 1 : lab) : 0;
      const float* x = a.cls + (fb + i) * a.NC;
      for (int c = 0; c < a.NC; ++c) {
        float l, d;
        focal_term(x[c], tc == c + 1, a.alpha, a.gamma, l, d);
        s_cls += l;
      }
    }
    if (lab > 0) {
      s_pos += 1.0f;
      const float* t = a.tgt + (fb + i) * 7;
      s_loc += box_term<true>(a.box + (fb + i) * 7, t, a.cw, a.beta, nullptr);
      if (a.dir)
        s_dir += dir_term(a.dir + (fb + i) * a.NB, a.NB, dir_bin(t[6], a.anchors[(int64_t)i * 7 + 6], a.dir_offset, a.NB), nullptr);
    }
  }
  block_partial_store(s_cls, s_loc, s_dir, s_pos, partial + ((int64_t)b * nblk + blockIdx.x) * 4);
}

// gradients of sum_b sum_k gout[b,k] * loss[b,k] w.r.t. the three prediction tensors; a block = 256 consecutive anchors of a
// frame, gradients staged in LDS and stored as contiguous runs
__global__ __launch_bounds__(TPB) void rpn_loss_backward_kernel(RpnArgs a, const float* __restrict__ npos,
                                                                const float* __restrict__ gout, float* __restrict__ dcls,
                                                                float* __restrict__ dbox, float* __restrict__ ddir) {
  __shared__ float s_cls[TPB * MAX_NC];
  __shared__ float s_box[TPB * 7];
  __shared__ float s_dir[TPB * MAX_NB];
  const int b = blockIdx.y;
  const int64_t fb = (int64_t)b * a.A;
  const int i0 = blockIdx.x * TPB, i = i0 + threadIdx.x;
  const int cnt = min(TPB, a.A - i0);
  const float inv = 1.0f / fmaxf(npos[b], 1.0f);
  const float g_cls = gout[b * 3 + 0] * a.w_cls * inv, g_loc = gout[b * 3 + 1] * a.w_loc * inv,
              g_dir = gout[b * 3 + 2] * a.w_dir * inv;
  if (i < a.A) {
    const int lab = a.labels[fb + i];
    const int tc = lab > 0 ? (a.NC == 1 ? 1 : lab) : 0;
    const float* x = a.cls + (fb + i) * a.NC;
    for (int c = 0; c < a.NC; ++c) {
      float l, d = 0.0f;
      if (lab >= 0) focal_term(x[c], tc == c + 1, a.alpha, a.gamma, l, d);
      s_cls[threadIdx.x * a.NC + c] = lab >= 0 ? d * g_cls : 0.0f;
    }
    float gb[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float gd[MAX_NB];
#pragma unroll
    for (int k = 0; k < MAX_NB; ++k) gd[k] = 0.0f;
    if (lab > 0) {
      const float* t = a.tgt + (fb + i) * 7;
      box_term<true>(a.box + (fb + i) * 7, t, a.cw, a.beta, gb);
      if (a.dir) dir_term(a.dir + (fb + i) * a.NB, a.NB, dir_bin(t[6], a.anchors[(int64_t)i * 7 + 6], a.dir_offset, a.NB), gd);
    }
#pragma unroll
    for (int d = 0; d < 7; ++d) s_box[threadIdx.x * 7 + d] = gb[d] * g_loc;
    if (a.dir)
#pragma unroll
      for (int k = 0; k < MAX_NB; ++k)
        if (k < a.NB) s_dir[threadIdx.x * a.NB + k] = gd[k] * g_dir;
  }
  __syncthreads();
  float* oc = dcls + (fb + i0) * a.NC;
  for (int k = threadIdx.x; k < cnt * a.NC; k += TPB) oc[k] = s_cls[k];
  float* ob = dbox + (fb + i0) * 7;
  for (int k = threadIdx.x; k < cnt * 7; k += TPB) ob[k] = s_box[k];
  if (a.dir) {
    float* od = ddir + (fb + i0) * a.NB;
    for (int k = threadIdx.x; k < cnt * a.NB; k += TPB) od[k] = s_dir[k];
  }
}

bool fill_args(RpnArgs& a, const float* cls, const float* box, const float* dir, const int32_t* labels, const float* tgt,
               const float* anchors, int B, int A, const CrbRpnLossCfg* cfg) {
  if (!cls || !box || !labels || !tgt || !cfg || B < 0 || A < 0) return false;
  if (cfg->num_class < 1 || cfg->num_class > MAX_NC) return false;
  if (dir && (cfg->num_dir_bins < 1 || cfg->num_dir_bins > MAX_NB || !anchors)) return false;
  a.cls = cls;
  a.box = box;
  a.dir = dir;
  a.labels = labels;
  a.tgt = tgt;
  a.anchors = anchors;
  a.B = B;
  a.A = A;
  a.NC = cfg->num_class;
  a.NB = dir ? cfg->num_dir_bins : 1;
  a.alpha = cfg->alpha;
  a.gamma = cfg->gamma;
  a.beta = cfg->beta;
  a.dir_offset = cfg->dir_offset;
  for (int d = 0; d < 7; ++d) a.cw[d] = cfg->code_weights[d];
  a.w_cls = cfg->cls_weight;
  a.w_loc = cfg->loc_weight;
  a.w_dir = cfg->dir_weight;
  return true;
}

int fwd_blocks(int A) { return (A + TPB * FWD_PER_THREAD - 1) / (TPB * FWD_PER_THREAD); }

}  // namespace

extern "C" {

int64_t crb_rpn_loss_workspace_bytes(int B, int A) {
  if (B <= 0 || A <= 0) return 16;
  return (int64_t)B * fwd_blocks(A) * 4 * sizeof(float);
}

int crb_rpn_loss_forward(const float* cls_preds, const float* box_preds, const float* dir_preds, const int32_t* labels,
                         const float* reg_targets, const float* anchors, int B, int A, const CrbRpnLossCfg* cfg,
                         float* loss, float* npos, void* workspace, int64_t workspace_bytes, void* stream) {
  RpnArgs a;
  if (!fill_args(a, cls_preds, box_preds, dir_preds, labels, reg_targets, anchors, B, A, cfg) || !loss || !npos)
    return CRB_ERR_ARG;
  if (B == 0) return CRB_OK;
  if (A == 0) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_rpn_loss_workspace_bytes(B, A)) return CRB_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int nblk = fwd_blocks(A);
  float* partial = (float*)workspace;
  hipLaunchKernelGGL(rpn_loss_partial_kernel, dim3(nblk, B), dim3(TPB), 0, s, a, partial);
  hipLaunchKernelGGL(rpn_loss_finalize_kernel, dim3(B), dim3(TPB), 0, s, partial, nblk, a.w_cls, a.w_loc,
                     dir_preds ? a.w_dir : 0.0f, loss, npos);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

int crb_rpn_loss_backward(const float* cls_preds, const float* box_preds, const float* dir_preds, const int32_t* labels,
                          const float* reg_targets, const float* anchors, int B, int A, const CrbRpnLossCfg* cfg,
                          const float* npos, const float* grad_loss, float* d_cls, float* d_box, float* d_dir, void* stream) {
  RpnArgs a;
  if (!fill_args(a, cls_preds, box_preds, dir_preds, labels, reg_targets, anchors, B, A, cfg) || !npos || !grad_loss ||
      !d_cls || !d_box || (dir_preds && !d_dir))
    return CRB_ERR_ARG;
  if (B == 0 || A == 0) return CRB_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rpn_loss_backward_kernel, dim3((A + TPB - 1) / TPB, B), dim3(TPB), 0, s, a, npos, grad_loss, d_cls, d_box,
                     d_dir);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

}  // extern "C"
