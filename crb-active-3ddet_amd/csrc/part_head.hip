// Point head of Part-A2 in training: segmentation and intra-object part targets of every voxel centre in one launch, and the focal
// + part-offset losses with their gradients in two.
//
// replaces, per batch:
//   PointHeadTemplate.assign_stack_targets in set_ignore_flag mode with ret_part_labels=True (pcdet/models/dense_heads/
//       point_head_template.py:49-129): a Python loop over the frames, each with a boolean-mask gather (a host sync), two
//       points_in_boxes_gpu launches and ~20 elementwise launches
//   PointHeadTemplate.get_cls_layer_loss (:131-158) and get_part_layer_loss (:160-173, whose max(1, pos.item()) is another host sync)
//       with their autograd: ~80 elementwise / reduction launches over (N, <= 3) tensors
// The head runs on every voxel of the batch (some 1e5 rows), so the losses use many workgroups where csrc/point_head.hip uses one:
//   launch 1  every workgroup reduces its tile of LOSS_TILE rows to three partial sums {focal terms, part terms, positives}
//   launch 2  every workgroup adds ALL partial sums in one fixed order (a few hundred numbers), which gives it the normaliser, and
//             writes the gradients of its tile; workgroup 0 also writes the losses
// No atomics, no ticket, no host read-back: losses and gradients are bit-identical from call to call. The terms are f32; every sum
// of them is f64 and so are the losses: the reference's own f32 error on these losses is about one f32 ulp (its pairwise sums), which
// f32 sums over 1,024 rows or an f32 result cannot stay within four times of.
#include "crb_common.h"
#include "focal_term.h"
#include "part_head_common.h"
#include "../../include/crb_hip.h"

namespace {

// grid (cdiv(N, 256), B): workgroup (x, b) takes rows off[b] + 256 x .. of frame b and leaves at once when the frame has fewer
__global__ __launch_bounds__(256) void part_targets_kernel(int G, int num_class, float ew0, float ew1, float ew2,
                                                           const float* __restrict__ pts, const int* __restrict__ off,
                                                           const float* __restrict__ gt, int64_t* __restrict__ labels,
                                                           float* __restrict__ part, int* __restrict__ owner) {
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
  bool shell;                                               // some enlarged box contains the point
  const int found = part_find_owner(sb, fb, G, ew0, ew1, ew2, active, x, y, z, shell);
  if (!active) return;
  const int64_t lab = part_label(fb, found, shell, num_class);
  float pl[3] = {0.f, 0.f, 0.f};
  if (found >= 0) part_offsets(fb + (int64_t)found * 8, x, y, z, pl);
  labels[i] = lab;
  owner[i] = found;
  part[(int64_t)i * 3] = pl[0]; part[(int64_t)i * 3 + 1] = pl[1]; part[(int64_t)i * 3 + 2] = pl[2];
}

// partials (tiles, 3) f64 = {sum of focal terms over rows with label >= 0, sum of part terms over rows with label > 0, positives}
__global__ __launch_bounds__(LOSS_TPB) void part_loss_partial_kernel(const float* __restrict__ cls, const float* __restrict__ prt,
                                                                     const int64_t* __restrict__ labels, const float* __restrict__ pl,
                                                                     int64_t n, int C, float alpha, float gamma,
                                                                     double* __restrict__ partials) {
  __shared__ double sh[LOSS_TPB / 64];
  double s_cls = 0.0, s_part = 0.0, s_pos = 0.0;
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
      for (int a = 0; a < 3; ++a) s_part += (double)part_bce(prt[i * 3 + a], pl[i * 3 + a]);
    }
  }
  const double t_cls = loss_block_sum(s_cls, sh), t_part = loss_block_sum(s_part, sh), t_pos = loss_block_sum(s_pos, sh);
  if (threadIdx.x == 0) {
    double* o = partials + (int64_t)blockIdx.x * 3;
    o[0] = t_cls; o[1] = t_part; o[2] = t_pos;
  }
}

// out (3) f64 = {point_loss_cls, point_loss_part, positives}; d_cls (n, C), d_prt (n, 3) = d loss / d logits for unit upstream gradients
__global__ __launch_bounds__(LOSS_TPB) void part_loss_finish_kernel(const float* __restrict__ cls, const float* __restrict__ prt,
                                                                    const int64_t* __restrict__ labels, const float* __restrict__ pl,
                                                                    int64_t n, int C, float alpha, float gamma, float w_cls, float w_part,
                                                                    const double* __restrict__ partials, int tiles, double* __restrict__ out,
                                                                    float* __restrict__ d_cls, float* __restrict__ d_prt) {
  __shared__ double shd[LOSS_TPB / 64];
  double a_cls = 0.0, a_part = 0.0, a_pos = 0.0;
  for (int t = threadIdx.x; t < tiles; t += LOSS_TPB) {
    a_cls += partials[(int64_t)t * 3];
    a_part += partials[(int64_t)t * 3 + 1];
    a_pos += partials[(int64_t)t * 3 + 2];
  }
  const double S_cls = loss_block_sum(a_cls, shd), S_part = loss_block_sum(a_part, shd), pos = loss_block_sum(a_pos, shd);
  const double norm = pos > 1.0 ? pos : 1.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[0] = S_cls / norm * (double)w_cls;
    out[1] = S_part / (3.0 * norm) * (double)w_part;
    out[2] = pos;
  }
  const float g_cls = (float)((double)w_cls / norm), g_part = (float)((double)w_part / (3.0 * norm));
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
    for (int a = 0; a < 3; ++a) {
      float d = 0.f;
      if (lab > 0) {
        const float x = prt[i * 3 + a];
        d = (1.0f / (1.0f + expf(-x)) - pl[i * 3 + a]) * g_part;
      }
      d_prt[i * 3 + a] = d;
    }
  }
}

// g (2) device = upstream gradients of {point_loss_cls, point_loss_part}
__global__ __launch_bounds__(256) void part_loss_scale_kernel(const float* __restrict__ d_cls, const float* __restrict__ d_prt,
                                                              const float* __restrict__ g, int64_t n_cls, int64_t n_prt,
                                                              float* __restrict__ o_cls, float* __restrict__ o_prt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_cls) o_cls[i] = d_cls[i] * g[0];
  if (i < n_prt) o_prt[i] = d_prt[i] * g[1];
}

}  // namespace

extern "C" int crb_part_targets(const float* points, const int32_t* frame_offsets, const float* gt_boxes, int B, int64_t N, int G,
                                const float* extra_width, int num_class, int64_t* labels, float* part_labels, int32_t* owner,
                                void* stream) {
  if (B <= 0 || B > 65535 || N < 0 || N >= (1LL << 31) - 256 || G < 0 || num_class <= 0 || !extra_width) return CRB_ERR_ARG;
  if (N == 0) return CRB_OK;
  if (!points || !frame_offsets || (G > 0 && !gt_boxes) || !labels || !part_labels || !owner) return CRB_ERR_ARG;
  hipLaunchKernelGGL(part_targets_kernel, dim3(crb_cdiv(N, 256), B), dim3(256), 0, (hipStream_t)stream, G, num_class, extra_width[0],
                     extra_width[1], extra_width[2], points, frame_offsets, gt_boxes, labels, part_labels, owner);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_part_loss_workspace_bytes(int64_t n) {
  return (int64_t)sizeof(double) * 3 * (n <= 0 ? 1 : (n + LOSS_TILE - 1) / LOSS_TILE);
}

extern "C" int crb_part_loss_forward(const float* cls_preds, const float* part_preds, const int64_t* labels, const float* part_labels,
                                     int64_t n, int C, float alpha, float gamma, float cls_weight, float part_weight, double* loss,
                                     float* d_cls, float* d_part, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || n >= (1LL << 31) || C <= 0 || !loss) return CRB_ERR_ARG;
  if (workspace_bytes < crb_part_loss_workspace_bytes(n) || !workspace) return CRB_ERR_WORKSPACE;
  if (n > 0 && (!cls_preds || !part_preds || !labels || !part_labels || !d_cls || !d_part)) return CRB_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (int)((n + LOSS_TILE - 1) / LOSS_TILE);
  double* partials = (double*)workspace;
  if (tiles > 0)
    hipLaunchKernelGGL(part_loss_partial_kernel, dim3(tiles), dim3(LOSS_TPB), 0, st, cls_preds, part_preds, labels, part_labels, n, C,
                       alpha, gamma, partials);
  // (n == 0: one workgroup with no tile writes the three zeros)
  hipLaunchKernelGGL(part_loss_finish_kernel, dim3(tiles > 0 ? tiles : 1), dim3(LOSS_TPB), 0, st, cls_preds, part_preds, labels,
                     part_labels, n, C, alpha, gamma, cls_weight, part_weight, partials, tiles, loss, d_cls, d_part);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_part_loss_backward(const float* d_cls, const float* d_part, const float* grad_losses, int64_t n, int C,
                                      float* grad_cls, float* grad_part, void* stream) {
  if (n < 0 || n >= (1LL << 31) || C <= 0) return CRB_ERR_ARG;
  if (n == 0) return CRB_OK;
  if (!d_cls || !d_part || !grad_losses || !grad_cls || !grad_part) return CRB_ERR_ARG;
  const int64_t m = n * (C > 3 ? C : 3);
  hipLaunchKernelGGL(part_loss_scale_kernel, dim3(crb_cdiv(m, 256)), dim3(256), 0, (hipStream_t)stream, d_cls, d_part, grad_losses,
                     n * C, n * 3, grad_cls, grad_part);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
