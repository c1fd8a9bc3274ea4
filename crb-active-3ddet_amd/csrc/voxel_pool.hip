// Voxel-neighbourhood RoI grid pooling of Voxel R-CNN: the voxel query and the fused body of one NeighborVoxelSAModuleMSG scale
// (reference: pointnet2_stack/src/voxel_query_gpu.cu:10-89, voxel_query_utils.py:10-100, voxel_pool_modules.py:70-130).
//
// The reference scatters a dense (B, Z, Y, X) int32 row index per level (757 MB for x_conv2 at bs = 16), probes it over a
// (2 rz + 1)(2 ry + 1)(2 rx + 1) window per grid point, gathers (M, C, nsample) / (M, 3, nsample) tensors and pushes them through
// Conv2d + BatchNorm2d + ReLU + max / avg pooling. Here:
//   crb_voxel_query          one thread per grid point scans the window in the reference's order (dz, dy, dx ascending) and looks
//                            every site up in the x-grouped site hash of crb_sparse_hash_build (any row order, 12 bytes per slot);
//                            the scan stops at the nsample-th hit (later hits change nothing). No dense index exists.
//   crb_voxel_pool_moments   sums of d and d d^T over all M * nsample slots (d = neighbour centre - grid point, duplicated fill
//                            slots and the zeroed slots of empty balls included) in f64, fixed order: the nine numbers from which
//                            the batch statistics of the folded BatchNorm2d follow (mlps_pos is linear in d).
//   crb_voxel_pool_forward   out[m, c] = pool_s relu(features_in[idx[m, s], c] + A[c, :] . d[m, s] + b[c]): one thread per (grid
//                            point, channel quad), 16-byte gathers along C, nothing of size (M, C, nsample) is ever written.
//   crb_voxel_pool_backward  recomputes the same values from idx: d features_in (f32 atomics, or compact rows for a deterministic
//                            scatter by the caller), dA, db (per-workgroup partials reduced in a fixed order in f64: reproducible).
// An empty ball reads row 0 with features and d zeroed: its output is relu(b) (the reference's quirk), its feature gradient nothing.
#include "crb_common.h"
#include "../../include/crb_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int VP_TPB = 256;
constexpr int VP_MAX_NSAMPLE = 32;
constexpr int VP_MAX_RANGE = 4;

struct VoxelQueryArgs {
  const float* xyz;          // (N, 3) voxel centres
  const float* new_xyz;      // (M, 3)
  const int* new_coords;     // (M, 4) [b, z, y, x]
  const long long* hkeys;
  const int* hvals;
  int* idx;                  // (M, nsample)
  int* cnt;                  // (M)
  int64_t M;
  uint32_t hmask;
  int B, D, H, W, rz, ry, rx, nsample;
  float radius2;
};

__global__ __launch_bounds__(VP_TPB) void voxel_query_kernel(VoxelQueryArgs a) {
  const int64_t m = (int64_t)blockIdx.x * VP_TPB + threadIdx.x;
  if (m >= a.M) return;
  const float nx = a.new_xyz[m * 3 + 0], ny = a.new_xyz[m * 3 + 1], nz = a.new_xyz[m * 3 + 2];
  const int4 c = *reinterpret_cast<const int4*>(a.new_coords + m * 4);
  const int b = c.x, z0 = c.y, y0 = c.z, x0 = c.w;
  int* out = a.idx + m * a.nsample;
  int cnt = 0, first = 0;
  if (b >= 0 && b < a.B) {
    for (int dz = -a.rz; dz <= a.rz && cnt < a.nsample; ++dz) {
      const int zc = z0 + dz;
      if (zc < 0 || zc >= a.D) continue;
      for (int dy = -a.ry; dy <= a.ry && cnt < a.nsample; ++dy) {
        const int yc = y0 + dy;
        if (yc < 0 || yc >= a.H) continue;
        const int64_t base = (((int64_t)b * a.D + zc) * a.H + yc) * (int64_t)a.W;
        for (int dx = -a.rx; dx <= a.rx && cnt < a.nsample; ++dx) {
          const int xc = x0 + dx;
          if (xc < 0 || xc >= a.W) continue;
          const uint32_t slot = crb_ghash_find(a.hkeys, a.hmask, base + xc);
          if (slot == 0xffffffffu) continue;
          const int row = a.hvals[slot];
          const float px = a.xyz[(int64_t)row * 3 + 0], py = a.xyz[(int64_t)row * 3 + 1], pz = a.xyz[(int64_t)row * 3 + 2];
          const float d2 = (px - nx) * (px - nx) + (py - ny) * (py - ny) + (pz - nz) * (pz - nz);
          if (d2 > a.radius2) continue;
          if (cnt == 0) first = row;
          out[cnt++] = row;
        }
      }
    }
  }
  for (int l = cnt; l < a.nsample; ++l) out[l] = first;      // fill with the first hit; an empty ball reads row 0
  a.cnt[m] = cnt;
}

// ---- moments of d ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VP_TPB) void voxel_moments_partial_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                                       const int* __restrict__ idx, const int* __restrict__ cnt, int64_t M,
                                                                       int nsample, double* __restrict__ partial) {
  __shared__ double sh[9][VP_TPB];
  const int64_t m = (int64_t)blockIdx.x * VP_TPB + threadIdx.x;
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (m < M && cnt[m] > 0) {
    const float nx = new_xyz[m * 3 + 0], ny = new_xyz[m * 3 + 1], nz = new_xyz[m * 3 + 2];
    for (int k = 0; k < nsample; ++k) {
      const int64_t row = idx[m * nsample + k];
      const double dx = xyz[row * 3 + 0] - nx, dy = xyz[row * 3 + 1] - ny, dz = xyz[row * 3 + 2] - nz;   // f32 differences, as grouped
      s[0] += dx; s[1] += dy; s[2] += dz;
      s[3] += dx * dx; s[4] += dx * dy; s[5] += dx * dz; s[6] += dy * dy; s[7] += dy * dz; s[8] += dz * dz;
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) sh[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int w = VP_TPB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < 9; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 9) partial[(int64_t)blockIdx.x * 9 + threadIdx.x] = sh[threadIdx.x][0];
}

// one workgroup: out[k] = sum over the nb partial rows, every thread a strided sequential sum, then the same tree
template <int K>
__global__ __launch_bounds__(VP_TPB) void reduce_partials_kernel(const double* __restrict__ partial, int64_t nb, double* __restrict__ out) {
  __shared__ double sh[VP_TPB];
  const int k = blockIdx.x;
  double s = 0;
  for (int64_t i = threadIdx.x; i < nb; i += VP_TPB) s += partial[i * K + k];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = VP_TPB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[k] = sh[0];
}

// ---- pooling -----------------------------------------------------------------------------------------------------------
struct VoxelPoolArgs {
  const float* feat;         // (N, C)
  const float* xyz;          // (N, 3)
  const float* new_xyz;      // (M, 3)
  const int* idx;            // (M, nsample)
  const int* cnt;            // (M)
  const float* A;            // (C, 3)
  const float* bias;         // (C)
  float* out;                // forward: (M, C)
  const float* grad_out;     // backward: (M, C)
  float* d_feat;             // backward: (N, C) accumulated with atomics, or NULL
  float* g_sel;              // backward, max pooling, d_feat == NULL: (M, C) gradient that reaches the selected row
  int* a_row;                //                                         (M, C) the selected row, -1 = none
  float* partial;            // backward: (blocks, C, 4) {dA x, dA y, dA z, db} per workgroup
  int64_t M;
  int C, nsample, avg;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

template <int C>
__global__ __launch_bounds__(VP_TPB) void voxel_pool_forward_kernel(VoxelPoolArgs a) {
  constexpr int Q = C / 4;
  const int64_t t = (int64_t)blockIdx.x * VP_TPB + threadIdx.x;
  const int64_t m = t / Q;
  if (m >= a.M) return;
  const int c0 = (int)(t - m * Q) * 4;
  float A0[4], A1[4], A2[4], bb[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A0[j] = a.A[(c0 + j) * 3 + 0]; A1[j] = a.A[(c0 + j) * 3 + 1]; A2[j] = a.A[(c0 + j) * 3 + 2]; bb[j] = a.bias[c0 + j];
  }
  const int cnt = a.cnt[m];
  f32x4 acc;
  if (cnt <= 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = fmaxf(bb[j], 0.f);
  } else {
    const float nx = a.new_xyz[m * 3 + 0], ny = a.new_xyz[m * 3 + 1], nz = a.new_xyz[m * 3 + 2];
    const int* id = a.idx + m * a.nsample;
    // max pooling: the fill slots repeat the first hit and cannot change the maximum; avg pooling counts them like the reference
    const int ns = a.avg ? a.nsample : min(cnt, a.nsample);
    acc = (f32x4){0.f, 0.f, 0.f, 0.f};                        // relu output >= 0: 0 is the identity of both pools
    for (int k = 0; k < ns; ++k) {
      const int64_t row = id[k];
      const float dx = a.xyz[row * 3 + 0] - nx, dy = a.xyz[row * 3 + 1] - ny, dz = a.xyz[row * 3 + 2] - nz;
      const f32x4 f = ld4(a.feat + row * C + c0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float v = fmaxf(f[j] + (A0[j] * dx + A1[j] * dy + A2[j] * dz + bb[j]), 0.f);
        acc[j] = a.avg ? acc[j] + v : fmaxf(acc[j], v);
      }
    }
    if (a.avg) acc = acc / (float)a.nsample;
  }
  *reinterpret_cast<f32x4*>(a.out + m * C + c0) = acc;
}

template <int C>
__global__ __launch_bounds__(VP_TPB) void voxel_pool_backward_kernel(VoxelPoolArgs a) {
  constexpr int Q = C / 4, MPB = VP_TPB / Q;                  // grid points per workgroup
  __shared__ float sh[VP_TPB][17];                            // 16 sums per thread (+1: bank spread)
  const int ml = threadIdx.x / Q, q = threadIdx.x - ml * Q;
  const int64_t m = (int64_t)blockIdx.x * MPB + ml;
  const int c0 = q * 4;
  float acc[4][4];                                            // [channel][dA x, dA y, dA z, db]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[j][k] = 0.f;
  if (m < a.M) {
    float A0[4], A1[4], A2[4], bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      A0[j] = a.A[(c0 + j) * 3 + 0]; A1[j] = a.A[(c0 + j) * 3 + 1]; A2[j] = a.A[(c0 + j) * 3 + 2]; bb[j] = a.bias[c0 + j];
    }
    const f32x4 g = ld4(a.grad_out + m * C + c0);
    const int cnt = a.cnt[m];
    int sel_row[4] = {-1, -1, -1, -1};
    float sel_g[4] = {0.f, 0.f, 0.f, 0.f};
    if (cnt <= 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (bb[j] > 0.f) acc[j][3] = g[j];                    // relu(b): d is zero, the zeroed features take no gradient
    } else {
      const float nx = a.new_xyz[m * 3 + 0], ny = a.new_xyz[m * 3 + 1], nz = a.new_xyz[m * 3 + 2];
      const int* id = a.idx + m * a.nsample;
      if (a.avg) {
        const float inv = 1.f / (float)a.nsample;
        for (int k = 0; k < a.nsample; ++k) {
          const int64_t row = id[k];
          const float dx = a.xyz[row * 3 + 0] - nx, dy = a.xyz[row * 3 + 1] - ny, dz = a.xyz[row * 3 + 2] - nz;
          const f32x4 f = ld4(a.feat + row * C + c0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v = f[j] + (A0[j] * dx + A1[j] * dy + A2[j] * dz + bb[j]);
            if (v > 0.f) {
              const float gj = g[j] * inv;
              acc[j][0] += gj * dx; acc[j][1] += gj * dy; acc[j][2] += gj * dz; acc[j][3] += gj;
              atomicAdd(a.d_feat + row * C + c0 + j, gj);
            }
          }
        }
      } else {
        const int ns = min(cnt, a.nsample);
        float best[4] = {0.f, 0.f, 0.f, 0.f}, bd[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) bd[j][0] = bd[j][1] = bd[j][2] = 0.f;
        for (int k = 0; k < ns; ++k) {
          const int64_t row = id[k];
          const float dx = a.xyz[row * 3 + 0] - nx, dy = a.xyz[row * 3 + 1] - ny, dz = a.xyz[row * 3 + 2] - nz;
          const f32x4 f = ld4(a.feat + row * C + c0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v = f[j] + (A0[j] * dx + A1[j] * dy + A2[j] * dz + bb[j]);
            if (v > best[j]) {                                // first maximum in slot order; a maximum of 0 passes no gradient
              best[j] = v; sel_row[j] = (int)row; bd[j][0] = dx; bd[j][1] = dy; bd[j][2] = dz;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (sel_row[j] >= 0) {
            sel_g[j] = g[j];
            acc[j][0] = g[j] * bd[j][0]; acc[j][1] = g[j] * bd[j][1]; acc[j][2] = g[j] * bd[j][2]; acc[j][3] = g[j];
            if (a.d_feat) atomicAdd(a.d_feat + (int64_t)sel_row[j] * C + c0 + j, g[j]);
          }
        }
      }
    }
    if (a.g_sel) {
      *reinterpret_cast<f32x4*>(a.g_sel + m * C + c0) = (f32x4){sel_g[0], sel_g[1], sel_g[2], sel_g[3]};
      *reinterpret_cast<int4*>(a.a_row + m * C + c0) = make_int4(sel_row[0], sel_row[1], sel_row[2], sel_row[3]);
    }
  }
  // sums over the workgroup's grid points, fixed order: thread (ml, q) holds 16 numbers, tree over ml
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[threadIdx.x][j * 4 + k] = acc[j][k];
  __syncthreads();
  for (int w = MPB / 2; w > 0; w >>= 1) {
    if (ml < w) {
#pragma unroll
      for (int e = 0; e < 16; ++e) sh[threadIdx.x][e] += sh[threadIdx.x + w * Q][e];
    }
    __syncthreads();
  }
  if (ml == 0) {
    float* p = a.partial + ((int64_t)blockIdx.x * C + c0) * 4;
#pragma unroll
    for (int e = 0; e < 16; ++e) p[e] = sh[threadIdx.x][e];
  }
}

// out[e] (C * 4) = sum over the workgroups' partial rows in f64, one wave-sized strided sum per output and a fixed tree
__global__ __launch_bounds__(VP_TPB) void voxel_pool_dab_kernel(const float* __restrict__ partial, int64_t nb, int E, float* __restrict__ out) {
  __shared__ double sh[VP_TPB];
  const int e = blockIdx.x;
  double s = 0;
  for (int64_t i = threadIdx.x; i < nb; i += VP_TPB) s += (double)partial[i * E + e];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = VP_TPB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[e] = (float)sh[0];
}

bool pool_shape_ok(int C, int nsample) { return (C == 32 || C == 64) && nsample >= 1 && nsample <= VP_MAX_NSAMPLE; }

}  // namespace

extern "C" int crb_voxel_pool_supported(int C, int nsample) { return pool_shape_ok(C, nsample) ? 1 : 0; }

extern "C" int crb_voxel_query(const float* xyz, int64_t N, const float* new_xyz, const int32_t* new_coords, int64_t M, int B,
                               const int32_t* shape_dhw, const int32_t* ranges_zyx, float radius, int nsample, const int64_t* hkeys,
                               const int32_t* hvals, int64_t capacity, int32_t* idx, int32_t* cnt, void* stream) {
  if (M < 0 || N < 0 || B <= 0 || !shape_dhw || !ranges_zyx || nsample < 1 || !(radius >= 0.f)) return CRB_ERR_ARG;
  if (shape_dhw[0] <= 0 || shape_dhw[1] <= 0 || shape_dhw[2] <= 0 || ranges_zyx[0] < 0 || ranges_zyx[1] < 0 || ranges_zyx[2] < 0)
    return CRB_ERR_ARG;
  if (nsample > VP_MAX_NSAMPLE || ranges_zyx[0] > VP_MAX_RANGE || ranges_zyx[1] > VP_MAX_RANGE || ranges_zyx[2] > VP_MAX_RANGE)
    return CRB_ERR_UNSUPPORTED;
  if (capacity < 8 || (capacity & (capacity - 1)) || capacity > (1LL << 32) || N >= (1LL << 31) || M * nsample >= (1LL << 40))
    return CRB_ERR_ARG;
  if (M == 0) return CRB_OK;
  if (!xyz || !new_xyz || !new_coords || !hkeys || !hvals || !idx || !cnt || ((uintptr_t)new_coords & 15)) return CRB_ERR_ARG;
  VoxelQueryArgs a;
  a.xyz = xyz; a.new_xyz = new_xyz; a.new_coords = new_coords; a.hkeys = (const long long*)hkeys; a.hvals = hvals; a.idx = idx; a.cnt = cnt;
  a.M = M; a.hmask = (uint32_t)(capacity - 1); a.B = B; a.D = shape_dhw[0]; a.H = shape_dhw[1]; a.W = shape_dhw[2];
  a.rz = ranges_zyx[0]; a.ry = ranges_zyx[1]; a.rx = ranges_zyx[2]; a.nsample = nsample; a.radius2 = radius * radius;
  hipLaunchKernelGGL(voxel_query_kernel, dim3(crb_cdiv(M, VP_TPB)), dim3(VP_TPB), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_voxel_pool_moments_workspace_bytes(int64_t M) {
  return (int64_t)crb_cdiv(M < 1 ? 1 : M, VP_TPB) * 9 * (int64_t)sizeof(double);
}

extern "C" int crb_voxel_pool_moments(const float* xyz, const float* new_xyz, const int32_t* idx, const int32_t* cnt, int64_t M,
                                      int nsample, double* sums, void* workspace, int64_t workspace_bytes, void* stream) {
  if (M < 1 || nsample < 1 || !xyz || !new_xyz || !idx || !cnt || !sums) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_voxel_pool_moments_workspace_bytes(M) || ((uintptr_t)workspace & 7)) return CRB_ERR_WORKSPACE;
  const int nb = crb_cdiv(M, VP_TPB);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(voxel_moments_partial_kernel, dim3(nb), dim3(VP_TPB), 0, (hipStream_t)stream, xyz, new_xyz, idx, cnt, M, nsample, partial);
  hipLaunchKernelGGL(reduce_partials_kernel<9>, dim3(9), dim3(VP_TPB), 0, (hipStream_t)stream, partial, (int64_t)nb, sums);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

static int pool_args_ok(const float* feat, int64_t N, int C, const float* xyz, const float* new_xyz, const int32_t* idx, const int32_t* cnt,
                        int64_t M, int nsample, int pool, const float* A, const float* b) {
  if (M < 1 || N < 1 || C < 1 || nsample < 1 || (pool != 0 && pool != 1)) return CRB_ERR_ARG;
  if (!pool_shape_ok(C, nsample)) return CRB_ERR_UNSUPPORTED;
  if (!feat || !xyz || !new_xyz || !idx || !cnt || !A || !b || ((uintptr_t)feat & 15) || N >= (1LL << 31)) return CRB_ERR_ARG;
  return CRB_OK;
}

extern "C" int crb_voxel_pool_forward(const float* features_in, int64_t N, int C, const float* xyz, const float* new_xyz,
                                      const int32_t* idx, const int32_t* cnt, int64_t M, int nsample, int pool, const float* A,
                                      const float* b, float* out, void* stream) {
  const int rc = pool_args_ok(features_in, N, C, xyz, new_xyz, idx, cnt, M, nsample, pool, A, b);
  if (rc != CRB_OK) return rc;
  if (!out || ((uintptr_t)out & 15)) return CRB_ERR_ARG;
  VoxelPoolArgs a = {};
  a.feat = features_in; a.xyz = xyz; a.new_xyz = new_xyz; a.idx = idx; a.cnt = cnt; a.A = A; a.bias = b; a.out = out;
  a.M = M; a.C = C; a.nsample = nsample; a.avg = pool;
  const int blocks = crb_cdiv(M * (C / 4), VP_TPB);
  if (C == 32) hipLaunchKernelGGL(voxel_pool_forward_kernel<32>, dim3(blocks), dim3(VP_TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(voxel_pool_forward_kernel<64>, dim3(blocks), dim3(VP_TPB), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_voxel_pool_backward_workspace_bytes(int64_t M, int C) {
  if (C < 4 || M < 1) return 0;
  const int mpb = VP_TPB / (C / 4);
  return (int64_t)crb_cdiv(M, mpb < 1 ? 1 : mpb) * C * 4 * (int64_t)sizeof(float);
}

extern "C" int crb_voxel_pool_backward(const float* grad_out, const float* features_in, int64_t N, int C, const float* xyz,
                                       const float* new_xyz, const int32_t* idx, const int32_t* cnt, int64_t M, int nsample, int pool,
                                       const float* A, const float* b, float* d_features, float* g_sel, int32_t* a_row, float* d_Ab,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = pool_args_ok(features_in, N, C, xyz, new_xyz, idx, cnt, M, nsample, pool, A, b);
  if (rc != CRB_OK) return rc;
  if (!grad_out || !d_Ab || ((uintptr_t)grad_out & 15)) return CRB_ERR_ARG;
  if (!d_features && (!g_sel || !a_row)) return CRB_ERR_ARG;
  if (!d_features && pool == 1) return CRB_ERR_UNSUPPORTED;        // avg pooling has no single selected row per output
  if (g_sel && (!a_row || ((uintptr_t)g_sel & 15) || ((uintptr_t)a_row & 15))) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_voxel_pool_backward_workspace_bytes(M, C) || ((uintptr_t)workspace & 15)) return CRB_ERR_WORKSPACE;
  VoxelPoolArgs a = {};
  a.feat = features_in; a.xyz = xyz; a.new_xyz = new_xyz; a.idx = idx; a.cnt = cnt; a.A = A; a.bias = b; a.grad_out = grad_out;
  a.d_feat = d_features; a.g_sel = g_sel; a.a_row = g_sel ? a_row : nullptr; a.partial = (float*)workspace;
  a.M = M; a.C = C; a.nsample = nsample; a.avg = pool;
  const int blocks = crb_cdiv(M, VP_TPB / (C / 4));
  if (C == 32) hipLaunchKernelGGL(voxel_pool_backward_kernel<32>, dim3(blocks), dim3(VP_TPB), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(voxel_pool_backward_kernel<64>, dim3(blocks), dim3(VP_TPB), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(voxel_pool_dab_kernel, dim3(C * 4), dim3(VP_TPB), 0, (hipStream_t)stream, (const float*)workspace, (int64_t)blocks,
                     C * 4, d_Ab);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
