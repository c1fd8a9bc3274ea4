// Two-layer pillar feature net of DynamicPillarVFE over variable-length segments (reference: PFNLayerV2 x 2 with NUM_FILTERS
// [64, 64], pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:14-142):
//   layer 1: Linear(K -> 32, no bias) + BatchNorm1d(32) + ReLU; x_max = per-pillar max, concatenated to each point (64 wide)
//   layer 2: Linear(64 -> 64, no bias) + BatchNorm1d(64) + ReLU + per-pillar max -> (M, 64)
// on the segments of crb_dyn_voxelize (perm, seg_offsets, coords) in pillar mode. The reference keeps six or seven (N, 64) f32
// tensors for the backward pass; here nothing of size (N, .) exists but the sorted point order: every kernel recomputes the values.
// The augmented point f = [point (C), xyz - pillar mean xyz (3), xyz - pillar centre (3)], K = C + 6, lives in LDS for the chunk a
// wave is walking and nowhere else. The pillar means come from crb_dyn_mean_vfe (f64 sums in segment order, rounded once).
//
// Work assignment: ONE WAVE PER WORKGROUP, a workgroup takes runs of DP_PPB neighbouring pillars (grid-stride), a pillar is walked
// in chunks of 64 points. Reason: segments have no length cap (1 .. several hundred points), so waves of one workgroup would meet
// their barriers after different numbers of chunks; with one wave per workgroup __syncthreads() is the wave's own LDS fence and
// costs nothing, and the CU still holds several such workgroups (LDS: 12 KB forward, 44 KB backward). Layer 1 (32 channels) runs
// as lane = (channel, point parity), two points per step; layer 2 as lane = output channel with its 32 weights for the per-point
// half of the input in registers, the per-pillar half (x_max) folded into a per-pillar base value. f32 FMAs, not MFMA: at K = 11
// and 32 inputs per point the launches are bound by the gathered point rows, and the values must be re-evaluated in the same order
// in every kernel so that forward and backward agree on each argmax (known limit: the backward kernel runs at 3 waves per CU).
// The sums run in segment order: crb_dyn_canonical_order makes that order a function of the points alone.
//   crb_dyn_pillar_moments     sum f and sum f f^T over all kept points, f64: the BatchNorm1d(32) statistics follow (n = Nk)
//   crb_dyn_pillar_stats2      sum y and sum y^2 of the layer-2 linear output y = W2 [x1; x_max], f64 (not linear in f)
//   crb_dyn_pillar_forward     out[m, c] = max_t relu(scale2 y + shift2); a pillar is walked twice (x_max, then the output)
//   crb_dyn_pillar_backward_a  hands grad_out to the first maximal point of each pillar and channel in segment order (none where
//                              the maximum is <= 0): sum dy2, sum dy2 yhat2 over the selected points; writes the argmax (M, 64)
//   crb_dyn_pillar_backward_b  over all points: dx2 = scale2 (dy2 - k1 - yhat2 k2), dW2 = sum dx2 [x1; x_max]^T, d[x1; x_max] =
//                              W2^T dx2; the x_max half summed over the pillar goes to the layer-1 argmax point of each channel;
//                              ReLU mask; G1 = sum dy1 f^T (32 x K), G0 = sum dy1. dW1, dgamma1, dbeta1 follow in closed form.
// Partial sums are f32 inside a workgroup at most, f64 across workgroups in a fixed order; no atomics: bit-reproducible.
#include "crb_common.h"
#include "../../include/crb_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int DP_PPB = 16;                     // neighbouring pillars per run
constexpr int DP_CHUNK = 64;
constexpr int DP_KS = 12;                      // LDS row stride of f (K <= 11)
constexpr int DP_H = 32;                       // layer-1 width
constexpr int DP_COUT = 64;
constexpr int DP_WS = 65;                      // LDS row stride of W2: rows and columns both read without bank conflicts
constexpr int DP_MAX_BLOCKS = 4096;             // moments, statistics, forward, pass A: 12 KB of LDS, 4 waves per SIMD on 256 CUs
constexpr int DP_MAX_BLOCKS_BWD = 1024;         // pass B: 44 KB of LDS and ~250 VGPRs hold 3 waves per CU
constexpr int DP_BWD_E = DP_COUT * DP_COUT + DP_H * DP_KS;
constexpr int DP_RED_E = 16, DP_RED_S = 256 / DP_RED_E;

struct DpArgs {
  const float* pts;          // (N, stride) rows [b, x, y, z, ...]
  const int* perm;           // (Nk)
  const int* seg;            // (M + 1)
  const int* coords;         // (M, 4) [b, 0, cy, cx]
  const float* pmean;        // (M, C): columns 0 .. 2 = pillar mean xyz
  const float* A1;           // (32, K) folded
  const float* b1;           // (32)
  const float* W2;           // (64, 64)
  const float* scale2;       // (64)
  const float* shift2;       // (64)
  const float* mean2;        // (64)  backward
  const float* isig2;        // (64)  backward
  const float* k1;           // (64)  backward_b: sum dy2 / n (0 in eval mode)
  const float* k2;           // (64)  backward_b: dgamma2 / n (0 in eval mode)
  const float* grad_out;     // (M, 64)
  int* arg2;                 // (M, 64)
  float* out;                // (M, 64)
  double* dpartial;          // f64 partials
  float* fpartial;           // f32 partials
  int64_t M;
  int stride;
  float vx, vy, ox, oy, oz;
};

__host__ __device__ constexpr int dp_nmom(int K) { return (K + 1) * (K + 2) / 2 - 1; }

// lanes t < cnt stage the augmented points of chunk [c0, c0 + cnt) of pillar m into fs (64 x DP_KS)
template <int C>
__device__ __forceinline__ void dp_stage(const DpArgs& a, int64_t m, int lo, int c0, int cnt, float* fs) {
  constexpr int K = C + 6;
  const int t = crb_lane();
  __syncthreads();                                            // the previous chunk's readers are done
  if (t < cnt) {
    const float* q = a.pts + (int64_t)a.perm[lo + c0 + t] * a.stride + 1;
    const float* pm = a.pmean + m * C;
    const int cy = a.coords[m * 4 + 2], cx = a.coords[m * 4 + 3];
    float* f = fs + t * DP_KS;
#pragma unroll
    for (int k = 0; k < C; ++k) f[k] = q[k];
    f[C + 0] = q[0] - pm[0]; f[C + 1] = q[1] - pm[1]; f[C + 2] = q[2] - pm[2];
    f[C + 3] = q[0] - ((float)cx * a.vx + a.ox);
    f[C + 4] = q[1] - ((float)cy * a.vy + a.oy);
    f[C + 5] = q[2] - a.oz;
#pragma unroll
    for (int k = K; k < DP_KS; ++k) f[k] = 0.f;                // the whole tail of the row: dp_value1 loads all DP_KS columns
  }
  __syncthreads();
}

template <int K>
__device__ __forceinline__ float dp_value1(const float* fs, int t, const float (&A)[DP_KS], float b) {
  const f32x4* r = reinterpret_cast<const f32x4*>(fs + t * DP_KS);
  const f32x4 r0 = r[0], r1 = r[1], r2 = r[2];
  const float x[DP_KS] = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3], r2[0], r2[1], r2[2], r2[3]};
  float v = b;
#pragma unroll
  for (int k = 0; k < K; ++k) v = fmaf(A[k], x[k], v);
  return v;
}

// layer 1 of a staged chunk: lane = (channel j, point parity); x1s[t][j] = relu(v); tracks the first maximal v > 0 (bt: its position
// in the segment, -1: none) and, when TRACK, its augmented point
template <int K, bool TRACK>
__device__ __forceinline__ void dp_layer1(const float* fs, int c0, int cnt, const float (&A)[DP_KS], float b, float* x1s, float& best,
                                          int& bt, float (&fb)[DP_KS]) {
  const int j = crb_lane() & 31, half = crb_lane() >> 5;
  for (int t = half; t < cnt; t += 2) {
    const float v = dp_value1<K>(fs, t, A, b);
    x1s[t * DP_H + j] = fmaxf(v, 0.f);
    if (v > best) {
      best = v; bt = c0 + t;
      if (TRACK) {
#pragma unroll
        for (int k = 0; k < DP_KS; ++k) fb[k] = fs[t * DP_KS + k];
      }
    }
  }
  __syncthreads();
}

// both parities agree on the first maximum of channel j; lanes < 32 publish x_max
template <bool TRACK>
__device__ __forceinline__ void dp_finish1(float& best, int& bt, float (&fb)[DP_KS], float* max1s) {
  const float ob = __shfl_xor(best, 32, 64);
  const int ot = __shfl_xor(bt, 32, 64);
  const bool take = ot >= 0 && (ob > best || (ob == best && (bt < 0 || ot < bt)));
  if (TRACK) {
#pragma unroll
    for (int k = 0; k < DP_KS; ++k) {
      const float o = __shfl_xor(fb[k], 32, 64);
      if (take) fb[k] = o;
    }
  }
  if (take) { best = ob; bt = ot; }
  __syncthreads();
  if (crb_lane() < DP_H) max1s[crb_lane()] = best;            // best starts at 0: the maximum of the ReLU outputs
  __syncthreads();
}

// y of output channel `lane` at staged point t: base (the x_max half) + the 32 per-point inputs, always in this order
__device__ __forceinline__ float dp_value2(const float* x1s, int t, const float (&w)[DP_H], float base) {
  const f32x4* r = reinterpret_cast<const f32x4*>(x1s + t * DP_H);
  float y = base;
#pragma unroll
  for (int q = 0; q < DP_H / 4; ++q) {
    const f32x4 v = r[q];
    y = fmaf(w[4 * q + 0], v[0], y); y = fmaf(w[4 * q + 1], v[1], y); y = fmaf(w[4 * q + 2], v[2], y); y = fmaf(w[4 * q + 3], v[3], y);
  }
  return y;
}

__device__ __forceinline__ float dp_base2(const float* W2, const float* max1s) {
  const float* w = W2 + crb_lane() * DP_COUT + DP_H;
  float y = 0.f;
#pragma unroll
  for (int j = 0; j < DP_H; ++j) y = fmaf(w[j], max1s[j], y);
  return y;
}

template <int C>
__global__ __launch_bounds__(64) void dp_moments_kernel(DpArgs a) {
  constexpr int K = C + 6, NMOM = dp_nmom(K);
  __shared__ __attribute__((aligned(16))) float fs[DP_CHUNK * DP_KS];
  const int lane = crb_lane();
  int ei[2], ej[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int e = lane + 64 * s, i = 0;
    if (e >= NMOM) e = 0;
    while (e >= K + 1 - i) { e -= K + 1 - i; ++i; }
    ei[s] = i; ej[s] = i + e;
  }
  double acc[2] = {0, 0};
  const int64_t runs = (a.M + DP_PPB - 1) / DP_PPB;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t m1 = min((run + 1) * (int64_t)DP_PPB, a.M);
    for (int64_t m = run * DP_PPB; m < m1; ++m) {
      const int lo = a.seg[m], n = a.seg[m + 1] - lo;
      for (int c0 = 0; c0 < n; c0 += DP_CHUNK) {
        const int cnt = min(DP_CHUNK, n - c0);
        dp_stage<C>(a, m, lo, c0, cnt, fs);
        for (int t = 0; t < cnt; ++t) {
          const float* f = fs + t * DP_KS;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const double fi = f[ei[s]], fj = ej[s] == K ? 1.0 : (double)f[ej[s]];
            acc[s] += fi * fj;
          }
        }
      }
    }
  }
  if (lane < NMOM) a.dpartial[(int64_t)blockIdx.x * NMOM + lane] = acc[0];
  if (lane + 64 < NMOM) a.dpartial[(int64_t)blockIdx.x * NMOM + lane + 64] = acc[1];
}

// MODE 0: sum y, sum y^2 (f64 partials, 128 per workgroup); 1: out = max relu; 2: backward pass A (argmax, sum dy2, sum dy2 yhat2)
template <int C, int MODE>
__global__ __launch_bounds__(64) void dp_layer2_kernel(DpArgs a) {
  constexpr int K = C + 6;
  __shared__ __attribute__((aligned(16))) float fs[DP_CHUNK * DP_KS];
  __shared__ __attribute__((aligned(16))) float x1s[DP_CHUNK * DP_H];
  __shared__ float max1s[DP_H];
  const int lane = crb_lane(), j = lane & 31;
  float A1[DP_KS], w2[DP_H], fb[DP_KS];
#pragma unroll
  for (int k = 0; k < DP_KS; ++k) { A1[k] = k < K ? a.A1[j * K + k] : 0.f; fb[k] = 0.f; }
  const float b1 = a.b1[j];
#pragma unroll
  for (int q = 0; q < DP_H; ++q) w2[q] = a.W2[lane * DP_COUT + q];
  const float sc = MODE == 0 ? 0.f : a.scale2[lane], sh = MODE == 0 ? 0.f : a.shift2[lane];
  const float mu = MODE == 2 ? a.mean2[lane] : 0.f, is = MODE == 2 ? a.isig2[lane] : 0.f;
  double s0 = 0, s1 = 0;
  const int64_t runs = (a.M + DP_PPB - 1) / DP_PPB;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t m1 = min((run + 1) * (int64_t)DP_PPB, a.M);
    for (int64_t m = run * DP_PPB; m < m1; ++m) {
      const int lo = a.seg[m], n = a.seg[m + 1] - lo;
      float best1 = 0.f;
      int bt1 = -1;
      for (int c0 = 0; c0 < n; c0 += DP_CHUNK) {
        const int cnt = min(DP_CHUNK, n - c0);
        dp_stage<C>(a, m, lo, c0, cnt, fs);
        dp_layer1<K, false>(fs, c0, cnt, A1, b1, x1s, best1, bt1, fb);
      }
      dp_finish1<false>(best1, bt1, fb, max1s);
      const float base = dp_base2(a.W2, max1s);
      float best2 = 0.f, ybest = 0.f;
      int arg = -1;
      for (int c0 = 0; c0 < n; c0 += DP_CHUNK) {
        const int cnt = min(DP_CHUNK, n - c0);
        if (n > DP_CHUNK) {                                   // (a single chunk is still staged)
          float bb = 0.f;
          int tt = -1;
          dp_stage<C>(a, m, lo, c0, cnt, fs);
          dp_layer1<K, false>(fs, c0, cnt, A1, b1, x1s, bb, tt, fb);
        }
        for (int t = 0; t < cnt; ++t) {
          const float y = dp_value2(x1s, t, w2, base);
          if (MODE == 0) { s0 += (double)y; s1 += (double)y * (double)y; }
          else {
            const float v = fmaf(sc, y, sh);
            if (v > best2) { best2 = v; ybest = y; arg = c0 + t; }
          }
        }
      }
      if (MODE == 1) a.out[m * DP_COUT + lane] = best2;
      if (MODE == 2) {
        a.arg2[m * DP_COUT + lane] = arg;
        if (arg >= 0) {
          const float g = a.grad_out[m * DP_COUT + lane];
          s0 += (double)g;
          s1 += (double)g * (double)((ybest - mu) * is);
        }
      }
    }
  }
  if (MODE != 1) {
    a.dpartial[(int64_t)blockIdx.x * 2 * DP_COUT + lane] = s0;
    a.dpartial[(int64_t)blockIdx.x * 2 * DP_COUT + DP_COUT + lane] = s1;
  }
}

template <int C>
__global__ __launch_bounds__(64) void dp_backward_kernel(DpArgs a) {
  constexpr int K = C + 6;
  __shared__ __attribute__((aligned(16))) float fs[DP_CHUNK * DP_KS];
  __shared__ __attribute__((aligned(16))) float x1s[DP_CHUNK * DP_H];
  __shared__ __attribute__((aligned(16))) float dxs[DP_CHUNK * DP_COUT];
  __shared__ float W2s[DP_COUT * DP_WS];
  __shared__ float max1s[DP_H];
  __shared__ float sdxs[DP_COUT];
  const int lane = crb_lane(), j = lane & 31, half = lane >> 5;
  for (int e = lane; e < DP_COUT * DP_COUT; e += 64) W2s[(e >> 6) * DP_WS + (e & 63)] = a.W2[e];
  float A1[DP_KS], w2[DP_H], acc2a[DP_H], acc2b[DP_H], accG[DP_KS], fb[DP_KS];
#pragma unroll
  for (int k = 0; k < DP_KS; ++k) { A1[k] = k < K ? a.A1[j * K + k] : 0.f; accG[k] = 0.f; fb[k] = 0.f; }
  const float b1 = a.b1[j];
#pragma unroll
  for (int q = 0; q < DP_H; ++q) { w2[q] = a.W2[lane * DP_COUT + q]; acc2a[q] = 0.f; acc2b[q] = 0.f; }
  const float sc = a.scale2[lane], mu = a.mean2[lane], is = a.isig2[lane], k1 = a.k1[lane], k2 = a.k2[lane];
  const int64_t runs = (a.M + DP_PPB - 1) / DP_PPB;
  for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
    const int64_t m1 = min((run + 1) * (int64_t)DP_PPB, a.M);
    for (int64_t m = run * DP_PPB; m < m1; ++m) {
      const int lo = a.seg[m], n = a.seg[m + 1] - lo;
      float best1 = 0.f;
      int bt1 = -1;
      for (int c0 = 0; c0 < n; c0 += DP_CHUNK) {
        const int cnt = min(DP_CHUNK, n - c0);
        dp_stage<C>(a, m, lo, c0, cnt, fs);
        dp_layer1<K, true>(fs, c0, cnt, A1, b1, x1s, best1, bt1, fb);
      }
      dp_finish1<true>(best1, bt1, fb, max1s);
      const float base = dp_base2(a.W2, max1s);
      const float g = a.grad_out[m * DP_COUT + lane];
      const int arg = a.arg2[m * DP_COUT + lane];
      float sdx = 0.f;
      for (int c0 = 0; c0 < n; c0 += DP_CHUNK) {
        const int cnt = min(DP_CHUNK, n - c0);
        if (n > DP_CHUNK) {
          float bb = 0.f, fdummy[DP_KS];
          int tt = -1;
          dp_stage<C>(a, m, lo, c0, cnt, fs);
          dp_layer1<K, false>(fs, c0, cnt, A1, b1, x1s, bb, tt, fdummy);
        }
        for (int t = 0; t < cnt; ++t) {                       // lane = output channel of layer 2
          const float y = dp_value2(x1s, t, w2, base);
          const float dy = (c0 + t == arg) ? g : 0.f;
          const float dx = sc * (dy - k1 - (y - mu) * is * k2);
          sdx += dx;
          const f32x4* r = reinterpret_cast<const f32x4*>(x1s + t * DP_H);
#pragma unroll
          for (int q = 0; q < DP_H / 4; ++q) {
            const f32x4 v = r[q];
            acc2a[4 * q + 0] = fmaf(dx, v[0], acc2a[4 * q + 0]); acc2a[4 * q + 1] = fmaf(dx, v[1], acc2a[4 * q + 1]);
            acc2a[4 * q + 2] = fmaf(dx, v[2], acc2a[4 * q + 2]); acc2a[4 * q + 3] = fmaf(dx, v[3], acc2a[4 * q + 3]);
          }
          dxs[t * DP_COUT + lane] = dx;
        }
        __syncthreads();
        for (int t = half; t < cnt; t += 2) {                 // lane = (layer-1 channel j, point parity): d x1 = W2[:, j]^T dx2
          if (x1s[t * DP_H + j] > 0.f) {                      // ReLU mask
            float d = 0.f;
            for (int c = 0; c < DP_COUT; ++c) d = fmaf(W2s[c * DP_WS + j], dxs[t * DP_COUT + c], d);
#pragma unroll
            for (int k = 0; k < K; ++k) accG[k] = fmaf(d, fs[t * DP_KS + k], accG[k]);
            accG[K] += d;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < DP_H; ++q) acc2b[q] = fmaf(sdx, max1s[q], acc2b[q]);
      __syncthreads();
      sdxs[lane] = sdx;
      __syncthreads();
      if (half == 0 && bt1 >= 0) {                            // the x_max half of d in2, summed over the pillar, to the argmax point
        float d = 0.f;
        for (int c = 0; c < DP_COUT; ++c) d = fmaf(W2s[c * DP_WS + DP_H + j], sdxs[c], d);
#pragma unroll
        for (int k = 0; k < K; ++k) accG[k] = fmaf(d, fb[k], accG[k]);
        accG[K] += d;
      }
    }
  }
  float* p = a.fpartial + (int64_t)blockIdx.x * DP_BWD_E;
#pragma unroll
  for (int q = 0; q < DP_H; ++q) { p[lane * DP_COUT + q] = acc2a[q]; p[lane * DP_COUT + DP_H + q] = acc2b[q]; }
#pragma unroll
  for (int k = 0; k < DP_KS; ++k) {
    const float v = accG[k] + __shfl_xor(accG[k], 32, 64);
    if (half == 0) p[DP_COUT * DP_COUT + j * DP_KS + k] = k <= K ? v : 0.f;
  }
}

// out[e] (E) = sum over the nb partial rows in f64, a fixed tree (the scheme of pillar_vfe.hip)
template <typename TIn>
__global__ __launch_bounds__(256) void dp_reduce_kernel(const TIn* __restrict__ partial, int64_t nb, int E, double* __restrict__ out) {
  __shared__ double sh[DP_RED_S][DP_RED_E];
  const int s = threadIdx.x / DP_RED_E, jj = threadIdx.x - s * DP_RED_E;
  const int e = blockIdx.x * DP_RED_E + jj;
  double v = 0;
  if (e < E)
    for (int64_t i = s; i < nb; i += DP_RED_S) v += (double)partial[i * E + e];
  sh[s][jj] = v;
  __syncthreads();
  for (int w = DP_RED_S / 2; w > 0; w >>= 1) {
    if (s < w) sh[s][jj] += sh[s + w][jj];
    __syncthreads();
  }
  if (s == 0 && e < E) out[e] = sh[0][jj];
}

int dp_blocks(int64_t M, int cap = DP_MAX_BLOCKS) {
  const int64_t runs = (M + DP_PPB - 1) / DP_PPB;
  return (int)(runs < cap ? (runs < 1 ? 1 : runs) : cap);
}

int dp_args_ok(const CrbDynPillarArgs* g) {
  if (!g || g->M < 1 || g->n_points < 1 || g->M > g->n_points || g->n_points >= (1LL << 31) - 1) return CRB_ERR_ARG;
  if (g->C != 4 && g->C != 5) return CRB_ERR_UNSUPPORTED;
  if (g->row_stride < 1 + g->C || !g->points || !g->perm || !g->seg_offsets || !g->coords || !g->pillar_mean) return CRB_ERR_ARG;
  return CRB_OK;
}

DpArgs dp_args(const CrbDynPillarArgs* g) {
  DpArgs a = {};
  a.pts = g->points; a.perm = g->perm; a.seg = g->seg_offsets; a.coords = g->coords; a.pmean = g->pillar_mean; a.M = g->M;
  a.stride = g->row_stride; a.vx = g->voxel_xy[0]; a.vy = g->voxel_xy[1]; a.ox = g->offsets[0]; a.oy = g->offsets[1]; a.oz = g->offsets[2];
  a.A1 = g->A1; a.b1 = g->b1; a.W2 = g->W2; a.scale2 = g->scale2; a.shift2 = g->shift2; a.mean2 = g->mean2; a.isig2 = g->inv_sigma2;
  a.k1 = g->k1; a.k2 = g->k2;
  return a;
}

template <typename TIn>
void dp_reduce(const TIn* partial, int nb, int E, double* out, hipStream_t st) {
  hipLaunchKernelGGL(dp_reduce_kernel<TIn>, dim3(crb_cdiv(E, DP_RED_E)), dim3(256), 0, st, partial, (int64_t)nb, E, out);
}

}  // namespace

extern "C" int crb_dyn_pillar_vfe_supported(int C, int num_layers, int filters0, int filters1) {
  return ((C == 4 || C == 5) && num_layers == 2 && filters0 == 64 && filters1 == 64) ? 1 : 0;
}

extern "C" int crb_dyn_pillar_num_moments(int C) { return dp_nmom(C + 6); }

extern "C" int64_t crb_dyn_pillar_workspace_bytes(int64_t M) {
  const int64_t light = (int64_t)dp_blocks(M) * 2 * DP_COUT * (int64_t)sizeof(double);      // 128 f64 partials (the moments: fewer)
  const int64_t bwd = (int64_t)dp_blocks(M, DP_MAX_BLOCKS_BWD) * DP_BWD_E * (int64_t)sizeof(float);
  return light > bwd ? light : bwd;
}

extern "C" int crb_dyn_pillar_moments(const CrbDynPillarArgs* g, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = dp_args_ok(g);
  if (rc != CRB_OK) return rc;
  if (!sums) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_dyn_pillar_workspace_bytes(g->M) || ((uintptr_t)workspace & 7)) return CRB_ERR_WORKSPACE;
  DpArgs a = dp_args(g);
  a.dpartial = (double*)workspace;
  const int nb = dp_blocks(g->M), E = dp_nmom(g->C + 6);
  if (g->C == 4) hipLaunchKernelGGL(dp_moments_kernel<4>, dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(dp_moments_kernel<5>, dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  dp_reduce((const double*)workspace, nb, E, sums, (hipStream_t)stream);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_dyn_pillar_stats2(const CrbDynPillarArgs* g, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = dp_args_ok(g);
  if (rc != CRB_OK) return rc;
  if (!sums || !g->A1 || !g->b1 || !g->W2) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_dyn_pillar_workspace_bytes(g->M) || ((uintptr_t)workspace & 7)) return CRB_ERR_WORKSPACE;
  DpArgs a = dp_args(g);
  a.dpartial = (double*)workspace;
  const int nb = dp_blocks(g->M);
  if (g->C == 4) hipLaunchKernelGGL((dp_layer2_kernel<4, 0>), dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((dp_layer2_kernel<5, 0>), dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  dp_reduce((const double*)workspace, nb, 2 * DP_COUT, sums, (hipStream_t)stream);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_dyn_pillar_forward(const CrbDynPillarArgs* g, float* out, void* stream) {
  const int rc = dp_args_ok(g);
  if (rc != CRB_OK) return rc;
  if (!out || !g->A1 || !g->b1 || !g->W2 || !g->scale2 || !g->shift2) return CRB_ERR_ARG;
  DpArgs a = dp_args(g);
  a.out = out;
  const int nb = dp_blocks(g->M);
  if (g->C == 4) hipLaunchKernelGGL((dp_layer2_kernel<4, 1>), dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((dp_layer2_kernel<5, 1>), dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_dyn_pillar_backward_a(const CrbDynPillarArgs* g, const float* grad_out, int32_t* arg2, double* sums, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
  const int rc = dp_args_ok(g);
  if (rc != CRB_OK) return rc;
  if (!grad_out || !arg2 || !sums || !g->A1 || !g->b1 || !g->W2 || !g->scale2 || !g->shift2 || !g->mean2 || !g->inv_sigma2) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_dyn_pillar_workspace_bytes(g->M) || ((uintptr_t)workspace & 7)) return CRB_ERR_WORKSPACE;
  DpArgs a = dp_args(g);
  a.grad_out = grad_out; a.arg2 = arg2; a.dpartial = (double*)workspace;
  const int nb = dp_blocks(g->M);
  if (g->C == 4) hipLaunchKernelGGL((dp_layer2_kernel<4, 2>), dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((dp_layer2_kernel<5, 2>), dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  dp_reduce((const double*)workspace, nb, 2 * DP_COUT, sums, (hipStream_t)stream);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_dyn_pillar_backward_b(const CrbDynPillarArgs* g, const float* grad_out, const int32_t* arg2, double* d_sums,
                                         void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = dp_args_ok(g);
  if (rc != CRB_OK) return rc;
  if (!grad_out || !arg2 || !d_sums || !g->A1 || !g->b1 || !g->W2 || !g->scale2 || !g->mean2 || !g->inv_sigma2 || !g->k1 || !g->k2)
    return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_dyn_pillar_workspace_bytes(g->M) || ((uintptr_t)workspace & 7)) return CRB_ERR_WORKSPACE;
  DpArgs a = dp_args(g);
  a.grad_out = grad_out; a.arg2 = (int*)arg2; a.fpartial = (float*)workspace;
  const int nb = dp_blocks(g->M, DP_MAX_BLOCKS_BWD);
  if (g->C == 4) hipLaunchKernelGGL(dp_backward_kernel<4>, dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(dp_backward_kernel<5>, dim3(nb), dim3(64), 0, (hipStream_t)stream, a);
  dp_reduce((const float*)workspace, nb, DP_BWD_E, d_sums, (hipStream_t)stream);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
