// Pillar feature net of PointPillars: PillarVFE with one PFNLayer (reference: pcdet/models/backbones_3d/vfe/pillar_vfe.py:8-123),
// Linear(K -> 64, no bias) + BatchNorm1d(64) + ReLU + max over the T slots of a pillar.
//
// The reference builds (M, T, K) augmented points, (M, T, 64) three times (linear, BatchNorm, ReLU), keeps them for the backward
// and takes the max over T. Here the augmented point f = [point (C), xyz - mean_xyz (3), xyz - pillar centre (3)], K = C + 6, lives
// in LDS for the pillar a wave is working on and nowhere else:
//   crb_pillar_vfe_moments   sum f (K) and sum f f^T (upper triangle) over the valid slots, f64, per-workgroup partials reduced in
//                            a fixed order: the batch statistics of the BatchNorm1d follow from them (the linear layer has no bias;
//                            padded slots are exact zeros and only count in n = M * T).
//   crb_pillar_vfe_forward   out[m, c] = max_t relu(A[c, :] . f[m, t] + b[c]) with the folded affine A = diag(scale) W, b = shift;
//                            a padded slot takes part with relu(b[c]). One lane per output channel, A in registers.
//   crb_pillar_vfe_backward  recomputes the values, hands grad_out to the first maximal slot (none where the maximum is <= 0) and
//                            sums dy f^T (64 x K) and dy (64) over the selected slots: f32 inside a workgroup, f64 across them in a
//                            fixed order. dW, dgamma and dbeta follow in closed form on the host side of the binding.
// Only the slots t < num_points[m] of `voxels` are read. No atomics anywhere: every result is bit-reproducible.
#include "crb_common.h"
#include "../../include/crb_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PV_TPB = 256;
constexpr int PV_WAVES = PV_TPB / 64;
constexpr int PV_PPB = 64;                     // pillars per workgroup (16 per wave)
constexpr int PV_MAX_T = 32;
constexpr int PV_COUT = 64;
constexpr int PV_KS = 12;                      // LDS row stride of f (K <= 11), 16-byte rows
constexpr int PV_RED_E = 16, PV_RED_S = PV_TPB / PV_RED_E;

struct PillarArgs {
  const float* voxels;       // (M, T, C)
  const int* num_points;     // (M)
  const int* coords;         // (M, 4) [b, z, y, x]
  const float* A;            // (64, K)
  const float* bias;         // (64)
  float* out;                // forward: (M, 64)
  const float* grad_out;     // backward: (M, 64)
  float* partial;            // backward: (blocks, 64, K + 1) f32
  double* mpartial;          // moments: (blocks, NMOM) f64
  int64_t M;
  int T;
  float vx, vy, vz, ox, oy, oz;
};

__host__ __device__ constexpr int pv_nmom(int K) { return (K + 1) * (K + 2) / 2 - 1; }

// One wave stages pillar m: raw (T * C) <- the valid slots of voxels, then f (T, PV_KS) <- the augmented points. All four waves
// of the workgroup call it together (two __syncthreads inside); a wave whose m is past the end stages nothing. -> valid slots
template <int C>
__device__ __forceinline__ int stage_pillar(const PillarArgs& a, int64_t m, float* raw, float* f) {
  constexpr int K = C + 6;
  const int lane = crb_lane();
  int cnt = 0;
  if (m < a.M) {
    cnt = min(max(a.num_points[m], 0), a.T);
    const float* src = a.voxels + m * (int64_t)a.T * C;
    for (int i = lane; i < cnt * C; i += 64) raw[i] = src[i];
  }
  __syncthreads();
  if (cnt > 0) {
    double sx = 0, sy = 0, sz = 0;                            // wave-uniform: LDS broadcast reads
    for (int t = 0; t < cnt; ++t) { sx += raw[t * C + 0]; sy += raw[t * C + 1]; sz += raw[t * C + 2]; }
    const float mean[3] = {(float)(sx / cnt), (float)(sy / cnt), (float)(sz / cnt)};
    const int4 c = *reinterpret_cast<const int4*>(a.coords + m * 4);
    const float ctr[3] = {(float)c.w * a.vx + a.ox, (float)c.z * a.vy + a.oy, (float)c.y * a.vz + a.oz};
    for (int i = lane; i < cnt * K; i += 64) {
      const int t = i / K, k = i - t * K;
      float v;
      if (k < C) v = raw[t * C + k];
      else if (k < C + 3) v = raw[t * C + (k - C)] - (k == C ? mean[0] : k == C + 1 ? mean[1] : mean[2]);
      else v = raw[t * C + (k - C - 3)] - (k == C + 3 ? ctr[0] : k == C + 4 ? ctr[1] : ctr[2]);
      f[t * PV_KS + k] = v;
    }
  }
  __syncthreads();
  return cnt;
}

// value of channel `lane` at staged slot t (A row in registers)
template <int K>
__device__ __forceinline__ float slot_value(const float* f, int t, const float (&A)[PV_KS], float b) {
  const f32x4* r = reinterpret_cast<const f32x4*>(f + t * PV_KS);
  const f32x4 r0 = r[0], r1 = r[1], r2 = r[2];
  const float x[PV_KS] = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3], r2[0], r2[1], r2[2], r2[3]};
  float v = b;
#pragma unroll
  for (int k = 0; k < K; ++k) v = fmaf(A[k], x[k], v);
  return v;
}

template <int C>
__global__ __launch_bounds__(PV_TPB) void pillar_moments_kernel(PillarArgs a) {
  constexpr int K = C + 6, NMOM = pv_nmom(K);
  __shared__ float raw[PV_WAVES][PV_MAX_T * C];
  __shared__ __attribute__((aligned(16))) float fs[PV_WAVES][PV_MAX_T * PV_KS];
  __shared__ double red[PV_WAVES][2][64];
  const int wave = threadIdx.x >> 6, lane = crb_lane();
  // entry e of the upper triangle of [f, 1] [f, 1]^T without the (K, K) corner: lane owns e = lane and e = lane + 64
  int ei[2], ej[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    int e = lane + 64 * s, i = 0;
    if (e >= NMOM) e = 0;
    while (e >= K + 1 - i) { e -= K + 1 - i; ++i; }
    ei[s] = i; ej[s] = i + e;
  }
  double acc[2] = {0, 0};
  for (int it = 0; it < PV_PPB / PV_WAVES; ++it) {
    const int64_t m = (int64_t)blockIdx.x * PV_PPB + it * PV_WAVES + wave;
    const int cnt = stage_pillar<C>(a, m, raw[wave], fs[wave]);
    for (int t = 0; t < cnt; ++t) {
      const float* f = fs[wave] + t * PV_KS;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const double fi = f[ei[s]], fj = ej[s] == K ? 1.0 : (double)f[ej[s]];
        acc[s] += fi * fj;
      }
    }
  }
  red[wave][0][lane] = acc[0]; red[wave][1][lane] = acc[1];
  __syncthreads();
  if ((int)threadIdx.x < NMOM) {
    const int s = threadIdx.x >> 6, l = threadIdx.x & 63;
    double v = red[0][s][l];
#pragma unroll
    for (int w = 1; w < PV_WAVES; ++w) v += red[w][s][l];
    a.mpartial[(int64_t)blockIdx.x * NMOM + threadIdx.x] = v;
  }
}

template <int C>
__global__ __launch_bounds__(PV_TPB) void pillar_forward_kernel(PillarArgs a) {
  constexpr int K = C + 6;
  __shared__ float raw[PV_WAVES][PV_MAX_T * C];
  __shared__ __attribute__((aligned(16))) float fs[PV_WAVES][PV_MAX_T * PV_KS];
  const int wave = threadIdx.x >> 6, lane = crb_lane();
  float A[PV_KS];
#pragma unroll
  for (int k = 0; k < PV_KS; ++k) A[k] = k < K ? a.A[lane * K + k] : 0.f;
  const float b = a.bias[lane];
  for (int it = 0; it < PV_PPB / PV_WAVES; ++it) {
    const int64_t m = (int64_t)blockIdx.x * PV_PPB + it * PV_WAVES + wave;
    const int cnt = stage_pillar<C>(a, m, raw[wave], fs[wave]);
    if (m >= a.M) continue;                                   // (the barriers are inside stage_pillar: every wave has passed them)
    float best = cnt < a.T ? fmaxf(b, 0.f) : 0.f;             // padded slots: relu(b); relu output >= 0
    for (int t = 0; t < cnt; ++t) best = fmaxf(best, slot_value<K>(fs[wave], t, A, b));
    a.out[m * PV_COUT + lane] = best;
  }
}

template <int C>
__global__ __launch_bounds__(PV_TPB) void pillar_backward_kernel(PillarArgs a) {
  constexpr int K = C + 6;
  __shared__ float raw[PV_WAVES][PV_MAX_T * C];
  __shared__ __attribute__((aligned(16))) float fs[PV_WAVES][PV_MAX_T * PV_KS];
  __shared__ float red[PV_WAVES][PV_COUT][K + 1];
  const int wave = threadIdx.x >> 6, lane = crb_lane();
  float A[PV_KS];
#pragma unroll
  for (int k = 0; k < PV_KS; ++k) A[k] = k < K ? a.A[lane * K + k] : 0.f;
  const float b = a.bias[lane];
  float acc[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) acc[k] = 0.f;
  for (int it = 0; it < PV_PPB / PV_WAVES; ++it) {
    const int64_t m = (int64_t)blockIdx.x * PV_PPB + it * PV_WAVES + wave;
    const int cnt = stage_pillar<C>(a, m, raw[wave], fs[wave]);
    if (m >= a.M) continue;
    float best = 0.f;                                         // a maximum of 0 (ReLU inactive) passes no gradient
    int sel = -1;                                             // -1: none, 0 .. cnt - 1: a valid slot, PV_MAX_T: a padded slot (f = 0)
    for (int t = 0; t < cnt; ++t) {
      const float v = slot_value<K>(fs[wave], t, A, b);
      if (v > best) { best = v; sel = t; }                    // first maximum in slot order
    }
    if (cnt < a.T && b > best) sel = PV_MAX_T;
    if (sel >= 0) {
      const float g = a.grad_out[m * PV_COUT + lane];
      acc[K] += g;
      if (sel < PV_MAX_T) {
        const float* f = fs[wave] + sel * PV_KS;
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += g * f[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k <= K; ++k) red[wave][lane][k] = acc[k];
  __syncthreads();
  for (int e = threadIdx.x; e < PV_COUT * (K + 1); e += PV_TPB) {
    const float* r = &red[0][0][0] + e;
    float v = r[0];
#pragma unroll
    for (int w = 1; w < PV_WAVES; ++w) v += r[w * PV_COUT * (K + 1)];
    a.partial[(int64_t)blockIdx.x * PV_COUT * (K + 1) + e] = v;
  }
}

// out[e] (E) = sum over the nb partial rows in f64: a workgroup takes 16 neighbouring outputs (64-byte reads), 16 threads per
// output each a strided sequential sum, then a fixed tree
template <typename TIn>
__global__ __launch_bounds__(PV_TPB) void pillar_reduce_kernel(const TIn* __restrict__ partial, int64_t nb, int E, double* __restrict__ out) {
  __shared__ double sh[PV_RED_S][PV_RED_E];
  const int s = threadIdx.x / PV_RED_E, j = threadIdx.x - s * PV_RED_E;
  const int e = blockIdx.x * PV_RED_E + j;
  double v = 0;
  if (e < E)
    for (int64_t i = s; i < nb; i += PV_RED_S) v += (double)partial[i * E + e];
  sh[s][j] = v;
  __syncthreads();
  for (int w = PV_RED_S / 2; w > 0; w >>= 1) {
    if (s < w) sh[s][j] += sh[s + w][j];
    __syncthreads();
  }
  if (s == 0 && e < E) out[e] = sh[0][j];
}

bool pillar_shape_ok(int C, int T, int Cout) { return (C == 4 || C == 5) && T >= 1 && T <= PV_MAX_T && Cout == PV_COUT; }

int pillar_args_ok(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M, int T, int C, int Cout,
                   const float* voxel_size, const float* offsets) {
  if (M < 1 || T < 1 || C < 1 || Cout < 1) return CRB_ERR_ARG;
  if (!pillar_shape_ok(C, T, Cout)) return CRB_ERR_UNSUPPORTED;
  if (!voxels || !num_points || !coords || !voxel_size || !offsets || ((uintptr_t)coords & 15) || M >= (1LL << 31) * PV_PPB) return CRB_ERR_ARG;
  return CRB_OK;
}

PillarArgs pillar_args(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M, int T, const float* voxel_size,
                       const float* offsets) {
  PillarArgs a = {};
  a.voxels = voxels; a.num_points = num_points; a.coords = coords; a.M = M; a.T = T;
  a.vx = voxel_size[0]; a.vy = voxel_size[1]; a.vz = voxel_size[2]; a.ox = offsets[0]; a.oy = offsets[1]; a.oz = offsets[2];
  return a;
}

}  // namespace

extern "C" int crb_pillar_vfe_supported(int C, int T, int Cout) { return pillar_shape_ok(C, T, Cout) ? 1 : 0; }

extern "C" int crb_pillar_vfe_num_moments(int C) { return pv_nmom(C + 6); }

extern "C" int64_t crb_pillar_vfe_moments_workspace_bytes(int64_t M, int C) {
  return (int64_t)crb_cdiv(M < 1 ? 1 : M, PV_PPB) * pv_nmom(C + 6) * (int64_t)sizeof(double);
}

extern "C" int crb_pillar_vfe_moments(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M, int T, int C,
                                      const float* voxel_size, const float* offsets, double* sums, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  const int rc = pillar_args_ok(voxels, num_points, coords, M, T, C, PV_COUT, voxel_size, offsets);
  if (rc != CRB_OK) return rc;
  if (!sums) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_pillar_vfe_moments_workspace_bytes(M, C) || ((uintptr_t)workspace & 7)) return CRB_ERR_WORKSPACE;
  PillarArgs a = pillar_args(voxels, num_points, coords, M, T, voxel_size, offsets);
  a.mpartial = (double*)workspace;
  const int nb = crb_cdiv(M, PV_PPB), E = pv_nmom(C + 6);
  if (C == 4) hipLaunchKernelGGL(pillar_moments_kernel<4>, dim3(nb), dim3(PV_TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pillar_moments_kernel<5>, dim3(nb), dim3(PV_TPB), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(pillar_reduce_kernel<double>, dim3(crb_cdiv(E, PV_RED_E)), dim3(PV_TPB), 0, (hipStream_t)stream,
                     (const double*)workspace, (int64_t)nb, E, sums);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_pillar_vfe_forward(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M, int T, int C,
                                      const float* voxel_size, const float* offsets, const float* A, const float* b, int Cout,
                                      float* out, void* stream) {
  const int rc = pillar_args_ok(voxels, num_points, coords, M, T, C, Cout, voxel_size, offsets);
  if (rc != CRB_OK) return rc;
  if (!A || !b || !out) return CRB_ERR_ARG;
  PillarArgs a = pillar_args(voxels, num_points, coords, M, T, voxel_size, offsets);
  a.A = A; a.bias = b; a.out = out;
  const int nb = crb_cdiv(M, PV_PPB);
  if (C == 4) hipLaunchKernelGGL(pillar_forward_kernel<4>, dim3(nb), dim3(PV_TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pillar_forward_kernel<5>, dim3(nb), dim3(PV_TPB), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_pillar_vfe_backward_workspace_bytes(int64_t M, int C, int Cout) {
  return (int64_t)crb_cdiv(M < 1 ? 1 : M, PV_PPB) * (Cout < 1 ? 1 : Cout) * (C + 7) * (int64_t)sizeof(float);
}

extern "C" int crb_pillar_vfe_backward(const float* grad_out, const float* voxels, const int32_t* num_points, const int32_t* coords,
                                       int64_t M, int T, int C, const float* voxel_size, const float* offsets, const float* A,
                                       const float* b, int Cout, double* d_sums, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = pillar_args_ok(voxels, num_points, coords, M, T, C, Cout, voxel_size, offsets);
  if (rc != CRB_OK) return rc;
  if (!grad_out || !A || !b || !d_sums) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_pillar_vfe_backward_workspace_bytes(M, C, Cout) || ((uintptr_t)workspace & 3)) return CRB_ERR_WORKSPACE;
  PillarArgs a = pillar_args(voxels, num_points, coords, M, T, voxel_size, offsets);
  a.A = A; a.bias = b; a.grad_out = grad_out; a.partial = (float*)workspace;
  const int nb = crb_cdiv(M, PV_PPB), E = PV_COUT * (C + 7);
  if (C == 4) hipLaunchKernelGGL(pillar_backward_kernel<4>, dim3(nb), dim3(PV_TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(pillar_backward_kernel<5>, dim3(nb), dim3(PV_TPB), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(pillar_reduce_kernel<float>, dim3(crb_cdiv(E, PV_RED_E)), dim3(PV_TPB), 0, (hipStream_t)stream,
                     (const float*)workspace, (int64_t)nb, E, d_sums);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
