// VectorPool aggregation of PV-RCNN++ (reference: pointnet2_stack/src/vector_pool_gpu.cu and the host loops of
// ThreeNNForVectorPoolByTwoStep / VectorPoolWithVoxelQuery, pointnet2_utils.py:302-448).
// The reference builds a neighbour list per new point through a global atomic cursor, reads the cursor back, grows the list and
// retries, then runs a 3-NN launch over the list, three_interpolate, a coordinate gather, two cats, a mask write and a permute. Here:
//   vp_three_nn_kernel   one wave per new point. The lanes stride over the frame's support points; the in-range ones of each 64 are
//                        visited in ascending row order (ballot + lowest set bit), which IS the reference's list order, and lanes
//                        0 .. G-1 each keep the three nearest of their cell with the reference's strict-< insertion. No list is stored.
//   vp_interp_kernel     one thread per output element of the (G, M, C + 9) matrix the grouped 1x1 convolution reads as G GEMMs:
//                        inverse-distance weights, the interpolated channels, centre - xyz[idx_j]; empty cells are zeros.
//   vp_voxel_kernel      voxel_random_choice, one wave per new point: lane g owns cell g; in-range points are visited in row order and
//                        the first to reach an empty cell fills it. The picked row per cell replaces grouped_idxs and its cursor.
//   vp_gather_sum_kernel both backward passes: one thread per (support row, channel) finds the row's run in the stably sorted inverse
//                        list and adds its contributions in that order. No float atomics: the same bits on every run.
// Every row index and loop bound that comes from device memory is clamped to the array it indexes.
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

constexpr int VP_WAVES = 4;            // new points per 256-thread workgroup
constexpr int VP_MAX_CAND = 1000;      // the reference's temp_idxs[1000]

struct VpFrame {
  int64_t start;                       // first support row of the frame, in [0, N]
  int n;                               // support rows of the frame, start + n <= N
};

// the reference's walk: the frame whose running sum of new_xyz_batch_cnt first exceeds m, else the last frame
__device__ __forceinline__ VpFrame vp_frame(const int* __restrict__ xyz_cnt, const int* __restrict__ new_cnt, int B, int64_t m, int64_t N) {
  int b = 0;
  int64_t covered = new_cnt[0];
  for (int k = 1; k < B; ++k) {
    if (m < covered) break;
    covered += new_cnt[k];
    b = k;
  }
  int64_t start = 0;
  for (int k = 0; k < b; ++k) start += xyz_cnt[k];
  start = start < 0 ? 0 : (start > N ? N : start);
  int64_t n = xyz_cnt[b];
  n = n < 0 ? 0 : (n > N - start ? N - start : n);
  VpFrame f;
  f.start = start;
  f.n = (int)n;
  return f;
}

__device__ __forceinline__ bool vp_in_range(float lx, float ly, float lz, float dist, float dist2, int neighbor_type) {
  if (neighbor_type == 1) return !(lx * lx + ly * ly + lz * lz > dist2);
  return !(fabsf(lx) > dist || fabsf(ly) > dist || fabsf(lz) > dist);
}

__global__ __launch_bounds__(256) void vp_three_nn_kernel(const float* __restrict__ xyz, int64_t N, const int* __restrict__ xyz_cnt,
                                                          const float* __restrict__ new_xyz, int64_t M, const int* __restrict__ new_cnt,
                                                          int B, const float* __restrict__ centers, int G, float dist, int nsample,
                                                          int neighbor_type, int* __restrict__ out_idx, float* __restrict__ out_dist) {
  const int lane = crb_lane();
  const int64_t m = (int64_t)blockIdx.x * VP_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;                                   // (whole waves: the kernel has no workgroup barrier)
  const VpFrame f = vp_frame(xyz_cnt, new_cnt, B, m, N);
  const float* p = xyz + f.start * 3;
  const float nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
  const float dist2 = dist * dist;
  const int cap = (nsample > 0 && nsample < VP_MAX_CAND) ? nsample : VP_MAX_CAND;
  float cx = 0.f, cy = 0.f, cz = 0.f;
  if (lane < G) {
    const float* c = centers + (m * G + lane) * 3;
    cx = c[0]; cy = c[1]; cz = c[2];
  }
  float b1 = __builtin_inff(), b2 = __builtin_inff(), b3 = __builtin_inff();
  int i1 = -1, i2 = -1, i3 = -1;
  int total = 0;
  for (int base = 0; base < f.n && total < cap; base += 64) {
    const int k = base + lane;
    float x = 0.f, y = 0.f, z = 0.f;
    bool in = false;
    if (k < f.n) {
      x = p[(int64_t)k * 3 + 0]; y = p[(int64_t)k * 3 + 1]; z = p[(int64_t)k * 3 + 2];
      in = vp_in_range(x - nx, y - ny, z - nz, dist, dist2, neighbor_type);
    }
    unsigned long long mask = __ballot(in);
    while (mask != 0ull && total < cap) {
      const int l = __ffsll(mask) - 1;
      mask &= mask - 1ull;
      ++total;
      const float X = __shfl(x, l, 64), Y = __shfl(y, l, 64), Z = __shfl(z, l, 64);
      const float d = (cx - X) * (cx - X) + (cy - Y) * (cy - Y) + (cz - Z) * (cz - Z);
      const int row = base + l;
      if (d < b1) {
        b3 = b2; i3 = i2;
        b2 = b1; i2 = i1;
        b1 = d; i1 = row;
      } else if (d < b2) {
        b3 = b2; i3 = i2;
        b2 = d; i2 = row;
      } else if (d < b3) {
        b3 = d; i3 = row;
      }
    }
  }
  if (lane >= G) return;
  if (i2 == -1) { i2 = i1; b2 = b1; }
  if (i3 == -1) { i3 = i1; b3 = b1; }
  const int s = (int)f.start;
  int* oi = out_idx + (m * G + lane) * 3;
  float* od = out_dist + (m * G + lane) * 3;
  oi[0] = i1 < 0 ? -1 : s + i1;
  oi[1] = i2 < 0 ? -1 : s + i2;
  oi[2] = i3 < 0 ? -1 : s + i3;
  od[0] = sqrtf(b1);
  od[1] = sqrtf(b2);
  od[2] = sqrtf(b3);
}

__device__ __forceinline__ void vp_weights(const float* __restrict__ d, float* w) {
  const float r0 = 1.f / (d[0] + 1e-8f), r1 = 1.f / (d[1] + 1e-8f), r2 = 1.f / (d[2] + 1e-8f);
  const float den = fmaxf(r0 + r1 + r2, 1e-8f);
  w[0] = r0 / den; w[1] = r1 / den; w[2] = r2 / den;
}

__global__ __launch_bounds__(256) void vp_interp_kernel(const int* __restrict__ idx, const float* __restrict__ dist,
                                                        const float* __restrict__ centers, const float* __restrict__ xyz,
                                                        const float* __restrict__ feat, int64_t N, int64_t M, int G, int C,
                                                        float* __restrict__ out) {
  const int K = C + 9;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)G * M * K) return;
  const int c = (int)(t % K);
  const int64_t row = t / K;
  const int64_t m = row % M;
  const int g = (int)(row / M);
  const int64_t cell = m * G + g;
  int64_t i[3] = {idx[cell * 3 + 0], idx[cell * 3 + 1], idx[cell * 3 + 2]};
  float v = 0.f;
  if (i[0] >= 0 && N > 0) {
#pragma unroll
    for (int j = 0; j < 3; ++j) i[j] = i[j] < 0 ? 0 : (i[j] > N - 1 ? N - 1 : i[j]);
    if (c < C) {
      float w[3];
      vp_weights(dist + cell * 3, w);
      v = w[0] * feat[i[0] * C + c] + w[1] * feat[i[1] * C + c] + w[2] * feat[i[2] * C + c];
    } else {
      const int j = (c - C) / 3, a = (c - C) % 3;
      v = centers[cell * 3 + a] - xyz[i[j] * 3 + a];
    }
  }
  out[t] = v;
}

__global__ __launch_bounds__(256) void vp_voxel_kernel(const float* __restrict__ xyz, const float* __restrict__ feat, int64_t N,
                                                       const int* __restrict__ xyz_cnt, const float* __restrict__ new_xyz, int64_t M,
                                                       const int* __restrict__ new_cnt, int B, int gy, int gz, int G, float R, float sx,
                                                       float sy, float sz, int C, int nsample, int neighbor_type,
                                                       float* __restrict__ new_feat, float* __restrict__ new_local, int* __restrict__ cnt,
                                                       int* __restrict__ pick_out) {
  const int lane = crb_lane();
  const int64_t m = (int64_t)blockIdx.x * VP_WAVES + (threadIdx.x >> 6);
  if (m >= M) return;
  const VpFrame f = vp_frame(xyz_cnt, new_cnt, B, m, N);
  const float* p = xyz + f.start * 3;
  const float nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
  const float R2 = R * R;
  const int limit = (nsample > 0 && nsample < G) ? nsample : G;
  int pick = -1;                                        // lane g: the frame-local row that filled cell g
  int filled = 0;
  for (int base = 0; base < f.n && filled < limit; base += 64) {
    const int k = base + lane;
    bool in = false;
    int cell = 0;
    if (k < f.n) {
      const float lx = p[(int64_t)k * 3 + 0] - nx, ly = p[(int64_t)k * 3 + 1] - ny, lz = p[(int64_t)k * 3 + 2] - nz;
      in = vp_in_range(lx, ly, lz, R, R2, neighbor_type);
      if (in) {
        const int ix = (int)floorf((lx + R) / sx), iy = (int)floorf((ly + R) / sy), iz = (int)floorf((lz + R) / sz);
        cell = ix * gy * gz + iy * gz + iz;
        cell = cell < 0 ? 0 : (cell > G - 1 ? G - 1 : cell);
      }
    }
    unsigned long long mask = __ballot(in);
    while (mask != 0ull && filled < limit) {
      const int l = __ffsll(mask) - 1;
      mask &= mask - 1ull;
      const int c = __shfl(cell, l, 64);
      const int cur = __shfl(pick, c, 64);
      if (cur < 0) {
        if (lane == c) pick = base + l;
        ++filled;
      }
    }
  }
  const int GC = G * C;
  for (int t0 = 0; t0 < GC; t0 += 64) {
    const int t = t0 + lane;
    const int g = t < GC ? t / C : G - 1;
    const int src = __shfl(pick, g, 64);
    if (t < GC) new_feat[m * GC + t] = src >= 0 ? feat[(f.start + src) * C + (t % C)] : 0.f;
  }
  if (lane >= G) return;
  float lx = 0.f, ly = 0.f, lz = 0.f;
  if (pick >= 0) {
    lx = p[(int64_t)pick * 3 + 0] - nx; ly = p[(int64_t)pick * 3 + 1] - ny; lz = p[(int64_t)pick * 3 + 2] - nz;
  }
  float* o = new_local + (m * G + lane) * 3;
  o[0] = lx; o[1] = ly; o[2] = lz;
  cnt[m * G + lane] = pick >= 0 ? 1 : 0;
  pick_out[m * G + lane] = pick >= 0 ? (int)f.start + pick : -1;
}

// INTERP: entry e = (m G + g) 3 + j of grad (G, M, C + 9) with weight w_j; else: entry e = m G + g of grad (M, G C) with weight 1
template <bool INTERP>
__global__ __launch_bounds__(256) void vp_gather_sum_kernel(const float* __restrict__ grad, const float* __restrict__ dist,
                                                            const int* __restrict__ rows, const int64_t* __restrict__ order, int64_t E,
                                                            int64_t N, int64_t M, int G, int C, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= N * C) return;
  const int c = (int)(t % C);
  const int n = (int)(t / C);
  int64_t lo = 0, hi = E;                               // first k with rows[k] >= n
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rows[mid] < n) lo = mid + 1; else hi = mid;
  }
  float acc = 0.f;
  for (int64_t k = lo; k < E && rows[k] == n; ++k) {
    int64_t e = order[k];
    e = e < 0 ? 0 : (e > E - 1 ? E - 1 : e);
    if (INTERP) {
      const int j = (int)(e % 3);
      const int64_t cell = e / 3;
      const int64_t m = cell / G;
      const int g = (int)(cell % G);
      float w[3];
      vp_weights(dist + cell * 3, w);
      acc += grad[((int64_t)g * M + m) * (C + 9) + c] * w[j];
    } else {
      acc += grad[e * C + c];
    }
  }
  out[t] = acc;
}

bool vp_counts_ok(int64_t N, int64_t M, int B, int G, int C) {
  return N >= 0 && M >= 0 && B >= 0 && G > 0 && C >= 0 && N < (1ll << 31) && M * (int64_t)G * 3 < (1ll << 40);
}

}  // namespace

extern "C" int crb_vector_pool_three_nn(const float* support_xyz, int64_t N, const int32_t* xyz_batch_cnt, const float* new_xyz, int64_t M,
                                        const int32_t* new_xyz_batch_cnt, int B, const float* grid_centers, int G, float query_dist,
                                        int nsample, int neighbor_type, int32_t* idx, float* dist, void* stream) {
  if (!vp_counts_ok(N, M, B, G, 0)) return CRB_ERR_ARG;
  if (G > CRB_WAVE) return CRB_ERR_UNSUPPORTED;
  if (M == 0) return CRB_OK;
  if (B < 1 || !xyz_batch_cnt || !new_xyz || !new_xyz_batch_cnt || !grid_centers || !idx || !dist || (N > 0 && !support_xyz))
    return CRB_ERR_ARG;
  hipLaunchKernelGGL(vp_three_nn_kernel, dim3(crb_cdiv(M, VP_WAVES)), dim3(256), 0, (hipStream_t)stream, support_xyz, N, xyz_batch_cnt,
                     new_xyz, M, new_xyz_batch_cnt, B, grid_centers, G, query_dist, nsample, neighbor_type, idx, dist);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_vector_pool_interp_forward(const int32_t* idx, const float* dist, const float* grid_centers, const float* support_xyz,
                                              const float* features, int64_t N, int64_t M, int G, int C, float* out, void* stream) {
  if (!vp_counts_ok(N, M, 1, G, C)) return CRB_ERR_ARG;
  if (M == 0) return CRB_OK;
  if (!idx || !dist || !grid_centers || !out || (N > 0 && (!support_xyz || (C > 0 && !features)))) return CRB_ERR_ARG;
  const int64_t total = (int64_t)G * M * (C + 9);
  hipLaunchKernelGGL(vp_interp_kernel, dim3(crb_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, idx, dist, grid_centers, support_xyz,
                     features, N, M, G, C, out);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_vector_pool_interp_backward(const float* grad_out, const float* dist, const int32_t* sorted_rows, const int64_t* order,
                                               int64_t N, int64_t M, int G, int C, float* grad_features, void* stream) {
  if (!vp_counts_ok(N, M, 1, G, C)) return CRB_ERR_ARG;
  if (N == 0 || C == 0) return CRB_OK;
  const int64_t E = M * G * 3;
  if (!grad_features || (E > 0 && (!grad_out || !dist || !sorted_rows || !order))) return CRB_ERR_ARG;
  hipLaunchKernelGGL(vp_gather_sum_kernel<true>, dim3(crb_cdiv(N * C, 256)), dim3(256), 0, (hipStream_t)stream, grad_out, dist,
                     sorted_rows, order, E, N, M, G, C, grad_features);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_vector_pool_voxel_forward(const float* support_xyz, const float* features, int64_t N, const int32_t* xyz_batch_cnt,
                                             const float* new_xyz, int64_t M, const int32_t* new_xyz_batch_cnt, int B, int num_grid_x,
                                             int num_grid_y, int num_grid_z, float max_distance, float grid_size_x, float grid_size_y,
                                             float grid_size_z, int C, int nsample, int neighbor_type, float* new_features,
                                             float* new_local_xyz, int32_t* point_cnt, int32_t* pick, void* stream) {
  if (num_grid_x < 1 || num_grid_y < 1 || num_grid_z < 1 || num_grid_x > CRB_WAVE || num_grid_y > CRB_WAVE || num_grid_z > CRB_WAVE)
    return CRB_ERR_ARG;
  const int G = num_grid_x * num_grid_y * num_grid_z;
  if (!vp_counts_ok(N, M, B, G, C)) return CRB_ERR_ARG;
  if (G > CRB_WAVE) return CRB_ERR_UNSUPPORTED;
  if (M == 0) return CRB_OK;
  if (B < 1 || !xyz_batch_cnt || !new_xyz || !new_xyz_batch_cnt || !new_local_xyz || !point_cnt || !pick || (C > 0 && !new_features) ||
      (N > 0 && (!support_xyz || (C > 0 && !features))))
    return CRB_ERR_ARG;
  hipLaunchKernelGGL(vp_voxel_kernel, dim3(crb_cdiv(M, VP_WAVES)), dim3(256), 0, (hipStream_t)stream, support_xyz, features, N,
                     xyz_batch_cnt, new_xyz, M, new_xyz_batch_cnt, B, num_grid_y, num_grid_z, G, max_distance, grid_size_x, grid_size_y,
                     grid_size_z, C, nsample, neighbor_type, new_features, new_local_xyz, point_cnt, pick);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_vector_pool_voxel_backward(const float* grad_new_features, const int32_t* sorted_rows, const int64_t* order, int64_t N,
                                              int64_t M, int G, int C, float* grad_features, void* stream) {
  if (!vp_counts_ok(N, M, 1, G, C)) return CRB_ERR_ARG;
  if (N == 0 || C == 0) return CRB_OK;
  const int64_t E = M * G;
  if (!grad_features || (E > 0 && (!grad_new_features ||!sorted_rows || !order))) return CRB_ERR_ARG;
  hipLaunchKernelGGL(vp_gather_sum_kernel<false>, dim3(crb_cdiv(N * C, 256)), dim3(256), 0, (hipStream_t)stream, grad_new_features,
                     (const float*)nullptr, sorted_rows, order, E, N, M, G, C, grad_features);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
