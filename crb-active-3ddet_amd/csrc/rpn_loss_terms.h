// Per-anchor terms of the anchor heads' RPN losses and the fixed-order reductions around them, shared by csrc/rpn_loss.hip (one
// head, one (B,A,NC) tensor) and csrc/multihead_loss.hip (a table of heads, each with its own class columns).
//   smooth_l1 / box_term   WeightedSmoothL1Loss.forward with add_sin_difference      (loss_utils.py:75-131, anchor_head_template.py:143-152)
//   dir_bin / dir_term     get_direction_target + WeightedCrossEntropyLoss.forward  (anchor_head_template.py:154-166, loss_utils.py:168-188)
//   focal_term             SigmoidFocalClassificationLoss.forward                   (focal_term.h)
//   wave_sum, rpn_loss_finalize_kernel: per-thread -> wave shuffle tree -> 4 waves -> blocks in index order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "focal_term.h"

namespace {

constexpr int RPN_TPB = 256;

// smooth-L1 of one weighted difference: loss, d loss / d diff      (loss_utils.py:98-107)
__device__ __forceinline__ void smooth_l1(float diff, float beta, float& loss, float& d) {
  const float n = fabsf(diff);
  if (beta < 1e-5f) {
    loss = n;
    d = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
  } else if (n < beta) {
    loss = 0.5f * n * n / beta;
    d = diff / beta;
  } else {
    loss = n - 0.5f * beta;
    d = diff > 0.0f ? 1.0f : -1.0f;
  }
}

// regression term of a positive anchor: sum over the 7 code entries, gradient w.r.t. the 7 predictions. SIN: the heading column
// goes through the sine difference (AnchorHeadMulti applies it only when the head has a direction classifier)
template <bool SIN>
__device__ __forceinline__ float box_term(const float* __restrict__ p, const float* __restrict__ t, const float* cw, float beta,
                                          float* __restrict__ g) {
  float sum = 0.0f;
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    float pv = p[d], tv = t[d], scale = 1.0f;
    if (SIN && d == 6) {                           // sin(a - b) = sin a cos b - cos a sin b, as the reference encodes it
      const float sp = sinf(p[6]), cp = cosf(p[6]), st = sinf(t[6]), ct = cosf(t[6]);
      pv = sp * ct;
      tv = cp * st;
      scale = cp * ct + sp * st;                   // d (pv - tv) / d p6
    }
    float diff = (tv != tv) ? 0.0f : (pv - tv);    // NaN target -> target := input (loss_utils.py:119)
    if (tv != tv) scale = 0.0f;
    diff *= cw[d];
    float l, dl;
    smooth_l1(diff, beta, l, dl);
    sum += l;
    if (g) g[d] = dl * cw[d] * scale;
  }
  return sum;
}

// direction bin of a positive anchor      (anchor_head_template.py:154-166, common_utils.limit_period)
__device__ __forceinline__ int dir_bin(float t6, float anchor_rot, float dir_offset, int nb) {
  const float two_pi = 6.283185307179586f;
  const float rot_gt = t6 + anchor_rot;
  const float val = rot_gt - dir_offset;
  const float off = val - floorf(val / two_pi + 0.0f) * two_pi;
  int bin = (int)floorf(off / (two_pi / (float)nb));
  return min(max(bin, 0), nb - 1);
}

// cross entropy of NB logits with target bin: loss, gradient = softmax - onehot
__device__ __forceinline__ float dir_term(const float* __restrict__ x, int nb, int bin, float* __restrict__ g) {
  float m = x[0];
  for (int k = 1; k < nb; ++k) m = fmaxf(m, x[k]);
  float s = 0.0f;
  for (int k = 0; k < nb; ++k) s += expf(x[k] - m);
  const float lse = logf(s);
  if (g)
    for (int k = 0; k < nb; ++k) g[k] = expf(x[k] - m - lse) - (k == bin ? 1.0f : 0.0f);
  return -(x[bin] - m - lse);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the block's four running sums {cls, loc, dir, npos} -> partial (B, nblk, 4), waves in index order
__device__ __forceinline__ void block_partial_store(float s_cls, float s_loc, float s_dir, float s_pos, float* __restrict__ out) {
  __shared__ float red[RPN_TPB / 64][4];
  s_cls = wave_sum(s_cls);
  s_loc = wave_sum(s_loc);
  s_dir = wave_sum(s_dir);
  s_pos = wave_sum(s_pos);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = s_cls;
    red[w][1] = s_loc;
    red[w][2] = s_dir;
    red[w][3] = s_pos;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < RPN_TPB / 64; ++k) v += red[k][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// one block per frame: partials summed in block order -> loss (B,3) weighted and normalised, npos (B)
__global__ __launch_bounds__(RPN_TPB) void rpn_loss_finalize_kernel(const float* __restrict__ partial, int nblk, float w_cls,
                                                                    float w_loc, float w_dir, float* __restrict__ loss,
                                                                    float* __restrict__ npos) {
  const int b = blockIdx.x;
  // thread t sums the partials t, t+256, ... (fixed order), then the fixed tree over the 256 threads
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int k = threadIdx.x; k < nblk; k += RPN_TPB) {
    const float4 p = *reinterpret_cast<const float4*>(partial + ((int64_t)b * nblk + k) * 4);
    v[0] += p.x;
    v[1] += p.y;
    v[2] += p.z;
    v[3] += p.w;
  }
  __shared__ float red[RPN_TPB / 64][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = wave_sum(v[j]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < 4; ++j) red[threadIdx.x >> 6][j] = v[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    float s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = 0.0f;
      for (int k = 0; k < RPN_TPB / 64; ++k) s[j] += red[k][j];
    }
    const float norm = fmaxf(s[3], 1.0f);
    loss[b * 3 + 0] = s[0] / norm * w_cls;
    loss[b * 3 + 1] = s[1] / norm * w_loc;
    loss[b * 3 + 2] = s[2] / norm * w_dir;
    npos[b] = s[3];
  }
}

}  // namespace
