// Dynamic voxelization (reference: DynamicPillarVFE.forward, pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:93-103,132-138, and
// DynamicMeanVFE.forward, dynamic_mean_vfe.py:53-72): every point in range belongs to its voxel, no cap on points per voxel, no cap
// on voxels, voxels in ascending key order (torch.unique's order), points of a voxel in input order. The reference builds this from
// torch.unique(return_inverse) and torch_scatter; here it is one stable radix sort of (key, point index) pairs:
//   dyn_keys_kernel     per point the 64-bit cell key, or the sentinel `cells` (= one past the largest key) for a dropped point, so
//                       that the dropped points sort behind every kept one
//   hipCUB SortPairs    stable LSD radix sort over the bits of `cells` only -> perm = the sorted point indices
//   dyn_heads           a device-wide exclusive scan of the segment-head flags numbers the voxels; the head of voxel v writes
//                       seg_offsets[v] and coords[v], the element at the kept / dropped boundary writes seg_offsets[M], M and Nk
//   dyn_mean_kernel     (M, C) means over the segments: one thread per (voxel, feature), an f64 sum in segment order, rounded once
// crb_dyn_canonical_order re-orders the points inside every voxel by their content (the bit patterns of feature columns 1 .. C,
// column 1 most significant), so that sums taken in segment order no longer depend on the order of the input rows: C stable 32-bit
// radix sorts, last column first, of the positions in the sorted order, then one stable sort by voxel number. Rows of equal content
// are interchangeable in any sum, so the result is a function of the multiset of rows alone.
// One thread per point / per output everywhere: the work is a handful of loads per point, bound by the sort. No atomics at all:
// every output is a function of the input alone, bit-reproducible from call to call.
#include <hipcub/hipcub.hpp>
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

struct DynParams {
  float min_x, min_y, min_z;
  float vs_x, vs_y, vs_z;
  int gx, gy, gz;
  int B;
  int mode;                  // CRB_DYN_PILLAR: x, y masked, key over (b, x, y); CRB_DYN_VOXEL: x, y, z masked, key over (b, x, y, z)
  uint64_t cells;            // number of keys = the sentinel
};

// cell index along one axis, the f32 arithmetic of voxelize.hip's vox_insert (= torch's (p - min) / voxel, floor); -1: outside or NaN
__device__ __forceinline__ int dyn_cell(float p, float mn, float vs, int g) {
  const float c = floorf(__fdiv_rn(__fsub_rn(p, mn), vs));
  return (c >= 0.f && c < (float)g) ? (int)c : -1;          // a NaN fails both comparisons: the point is dropped
}

__global__ __launch_bounds__(256) void dyn_keys_kernel(const float* __restrict__ pts, int n, int stride, DynParams p,
                                                       uint64_t* __restrict__ keys, int* __restrict__ vals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* q = pts + (int64_t)i * stride;
  const float bf = q[0];
  uint64_t key = p.cells;
  if (bf > -1.f && bf < (float)p.B) {                       // .int() truncates towards zero; NaN is dropped
    const int b = (int)bf;
    const int cx = dyn_cell(q[1], p.min_x, p.vs_x, p.gx), cy = dyn_cell(q[2], p.min_y, p.vs_y, p.gy);
    if (cx >= 0 && cy >= 0) {
      if (p.mode == CRB_DYN_PILLAR) {
        if (q[3] == q[3]) key = ((uint64_t)b * p.gx + cx) * p.gy + cy;      // z is not masked, but a NaN z still drops the point
      } else {
        const int cz = dyn_cell(q[3], p.min_z, p.vs_z, p.gz);
        if (cz >= 0) key = (((uint64_t)b * p.gx + cx) * p.gy + cy) * p.gz + cz;
      }
    }
  }
  keys[i] = key;
  vals[i] = i;
}

struct HeadFlag {
  const uint64_t* keys;      // sorted
  uint64_t cells;
  __device__ int operator()(int64_t j) const {
    const uint64_t k = keys[j];
    return (k < cells && (j == 0 || keys[j - 1] != k)) ? 1 : 0;
  }
};

struct HeadWrite {
  const uint64_t* keys;      // sorted
  DynParams p;
  int n, cap;
  int* seg_offsets;          // (cap + 1)
  int* coords;               // (cap, 4) [b, z, y, x]
  int* counts;               // {M, Nk}
  __device__ void operator()(int64_t j, int ex, int v) const {
    const uint64_t k = keys[j];
    if (v && ex < cap) {
      seg_offsets[ex] = (int)j;
      uint64_t r = k;
      int cz = 0;
      if (p.mode == CRB_DYN_VOXEL) { cz = (int)(r % p.gz); r /= p.gz; }
      const int cy = (int)(r % p.gy); r /= p.gy;
      const int cx = (int)(r % p.gx); r /= p.gx;
      int* c = coords + (int64_t)ex * 4;
      c[0] = (int)r; c[1] = cz; c[2] = cy; c[3] = cx;
    }
    // exactly one element sits at the kept / dropped boundary: the first dropped one, or the last element when none is dropped
    const bool kept = k < p.cells;
    int M = -1, Nk = 0;
    if (!kept && (j == 0 || keys[j - 1] < p.cells)) { M = ex; Nk = (int)j; }
    else if (kept && j == n - 1) { M = ex + v; Nk = n; }
    if (M >= 0) {
      if (M <= cap) seg_offsets[M] = Nk;
      counts[0] = M; counts[1] = Nk;
    }
  }
};

__global__ __launch_bounds__(256) void dyn_mean_kernel(const float* __restrict__ pts, int stride, int C, const int* __restrict__ perm,
                                                       const int* __restrict__ seg_offsets, int64_t M, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= M * C) return;
  const int64_t m = e / C;
  const int c = (int)(e - m * C);
  const int lo = seg_offsets[m], hi = seg_offsets[m + 1];
  double s = 0;
  for (int j = lo; j < hi; ++j) s += (double)pts[(int64_t)perm[j] * stride + 1 + c];
  out[e] = (float)(s / (double)(hi > lo ? hi - lo : 1));
}

// keys[i] = the bits of feature column `col` of the point at position pos[i] of the sorted order (pos == nullptr: position i)
__global__ __launch_bounds__(256) void dyn_colkeys_kernel(const float* __restrict__ pts, int stride, int col, const int* __restrict__ perm,
                                                          const int* __restrict__ pos, int n, uint32_t* __restrict__ keys,
                                                          int* __restrict__ ident) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = pos ? pos[i] : i;
  keys[i] = __float_as_uint(pts[(int64_t)perm[p] * stride + 1 + col]);
  if (ident) ident[i] = i;
}

// keys[i] = the voxel that owns position pos[i]: the last v with seg_offsets[v] <= pos[i]
__global__ __launch_bounds__(256) void dyn_segkeys_kernel(const int* __restrict__ seg_offsets, int M, const int* __restrict__ pos, int n,
                                                          uint32_t* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = pos[i];
  int lo = 0, hi = M - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_offsets[mid] <= p) lo = mid; else hi = mid - 1;
  }
  keys[i] = (uint32_t)lo;
}

__global__ __launch_bounds__(256) void dyn_gather_kernel(const int* __restrict__ perm, const int* __restrict__ pos, int n,
                                                         int* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = perm[pos[i]];
}

size_t dyn_sort32_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int*)nullptr, (int*)nullptr,
                                           (int)n, 0, 32, (hipStream_t)0);
  return b;
}

size_t dyn_sort_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int*)nullptr, (int*)nullptr,
                                           (int)n, 0, 64, (hipStream_t)0);
  return b;
}

}  // namespace

extern "C" int64_t crb_dyn_voxelize_workspace_bytes(int64_t n_points) {
  if (n_points <= 0) return 256;
  return 2 * crb_align_up(8 * n_points, 256) + crb_align_up(4 * n_points, 256) +
         crb_align_up((int64_t)crb_scan_num_tiles(n_points) * 4, 256) + crb_align_up((int64_t)dyn_sort_temp_bytes(n_points), 256) + 256;
}

extern "C" int crb_dyn_voxelize(const float* points, int64_t n_points, int row_stride, int B, int mode, const float* range_min_xyz,
                                const float* voxel_size_xyz, const int32_t* grid_xyz, int64_t max_voxels, int32_t* perm,
                                int32_t* seg_offsets, int32_t* coords, int32_t* counts, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  if (n_points < 0 || n_points >= (1LL << 31) - 1 || row_stride < 4 || B <= 0 || (mode != CRB_DYN_PILLAR && mode != CRB_DYN_VOXEL) ||
      !range_min_xyz || !voxel_size_xyz || !grid_xyz || !seg_offsets || !counts || max_voxels < 0 || max_voxels >= (1LL << 31) - 1)
    return CRB_ERR_ARG;
  const int64_t gx = grid_xyz[0], gy = grid_xyz[1], gz = mode == CRB_DYN_VOXEL ? grid_xyz[2] : 1;
  if (gx < 1 || gy < 1 || gz < 1 || gx >= (1 << 24) || gy >= (1 << 24) || gz >= (1 << 24)) return CRB_ERR_ARG;   // (float)g is exact
  if ((double)B * (double)gx * (double)gy * (double)gz >= 4.0e18) return CRB_ERR_ARG;
  const uint64_t cells = (uint64_t)B * gx * gy * gz;
  hipStream_t st = (hipStream_t)stream;
  if (n_points == 0) {
    CRB_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), st));
    CRB_HIP(hipMemsetAsync(seg_offsets, 0, sizeof(int32_t), st));
    return CRB_OK;
  }
  const int64_t need = n_points < (int64_t)cells ? n_points : (int64_t)cells;      // the most voxels the input can give
  if (!points || !perm || !coords || max_voxels < need) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_dyn_voxelize_workspace_bytes(n_points)) return CRB_ERR_WORKSPACE;
  const int n = (int)n_points;
  CrbArena ar(workspace, (size_t)workspace_bytes);
  uint64_t* kin = ar.take<uint64_t>(n);
  uint64_t* kout = ar.take<uint64_t>(n);
  int* vin = ar.take<int>(n);
  int* tile_sums = ar.take<int>(crb_scan_num_tiles(n));
  const size_t tb = dyn_sort_temp_bytes(n);
  char* temp = ar.take<char>((int64_t)tb);
  if (!ar.ok) return CRB_ERR_WORKSPACE;

  DynParams p;
  p.min_x = range_min_xyz[0]; p.min_y = range_min_xyz[1]; p.min_z = range_min_xyz[2];
  p.vs_x = voxel_size_xyz[0]; p.vs_y = voxel_size_xyz[1]; p.vs_z = voxel_size_xyz[2];
  p.gx = (int)gx; p.gy = (int)gy; p.gz = (int)gz; p.B = B; p.mode = mode; p.cells = cells;
  hipLaunchKernelGGL(dyn_keys_kernel, dim3(crb_cdiv(n, 256)), dim3(256), 0, st, points, n, row_stride, p, kin, vin);
  int bits = 1;
  while (bits < 64 && (1ULL << bits) <= cells) ++bits;       // keys 0 .. cells
  size_t tbytes = tb;
  if (hipcub::DeviceRadixSort::SortPairs(temp, tbytes, (const uint64_t*)kin, kout, (const int*)vin, perm, n, 0, bits, st) != hipSuccess)
    return CRB_ERR_LAUNCH;
  HeadFlag hf{kout, cells};
  HeadWrite hw{kout, p, n, (int)max_voxels, seg_offsets, coords, counts};
  const int rc = crb_device_excl_scan(hf, hw, (int64_t)n, tile_sums, (int*)nullptr, st);
  if (rc != CRB_OK) return rc;
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_dyn_mean_vfe(const float* points, int64_t n_points, int row_stride, int C, const int32_t* perm,
                                const int32_t* seg_offsets, int64_t M, float* out, void* stream) {
  if (n_points < 0 || n_points >= (1LL << 31) - 1 || C < 1 || row_stride < 1 + C || M < 0 || M > n_points) return CRB_ERR_ARG;
  if (M == 0) return CRB_OK;
  if (!points || !perm || !seg_offsets || !out) return CRB_ERR_ARG;
  hipLaunchKernelGGL(dyn_mean_kernel, dim3(crb_cdiv(M * C, 256)), dim3(256), 0, (hipStream_t)stream, points, row_stride, C, perm,
                     seg_offsets, M, out);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_dyn_canonical_order_workspace_bytes(int64_t n_kept) {
  if (n_kept <= 0) return 256;
  return 4 * crb_align_up(4 * n_kept, 256) + crb_align_up((int64_t)dyn_sort32_temp_bytes(n_kept), 256) + 256;
}

extern "C" int crb_dyn_canonical_order(const float* points, int64_t n_points, int row_stride, int C, const int32_t* perm, int64_t n_kept,
                                       const int32_t* seg_offsets, int64_t M, int32_t* perm_out, void* workspace,
                                       int64_t workspace_bytes, void* stream) {
  if (n_points < 0 || n_points >= (1LL << 31) - 1 || C < 1 || row_stride < 1 + C || n_kept < 0 || n_kept > n_points || M < 0 ||
      M > n_kept || (M == 0) != (n_kept == 0))
    return CRB_ERR_ARG;
  if (n_kept == 0) return CRB_OK;
  if (!points || !perm || !seg_offsets || !perm_out || perm_out == perm) return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_dyn_canonical_order_workspace_bytes(n_kept)) return CRB_ERR_WORKSPACE;
  const int n = (int)n_kept;
  hipStream_t st = (hipStream_t)stream;
  CrbArena ar(workspace, (size_t)workspace_bytes);
  uint32_t* kin = ar.take<uint32_t>(n);
  uint32_t* kout = ar.take<uint32_t>(n);
  int* vin = ar.take<int>(n);
  int* vout = ar.take<int>(n);
  const size_t tb = dyn_sort32_temp_bytes(n);
  char* temp = ar.take<char>((int64_t)tb);
  if (!ar.ok) return CRB_ERR_WORKSPACE;
  const dim3 grid(crb_cdiv(n, 256)), block(256);
  for (int col = C - 1; col >= 0; --col) {                    // least significant column first
    const bool first = col == C - 1;
    hipLaunchKernelGGL(dyn_colkeys_kernel, grid, block, 0, st, points, row_stride, col, perm, first ? (const int*)nullptr : (const int*)vin,
                       n, kin, first ? vin : (int*)nullptr);
    size_t tbytes = tb;
    if (hipcub::DeviceRadixSort::SortPairs(temp, tbytes, (const uint32_t*)kin, kout, (const int*)vin, vout, n, 0, 32, st) != hipSuccess)
      return CRB_ERR_LAUNCH;
    int* t = vin; vin = vout; vout = t;
  }
  hipLaunchKernelGGL(dyn_segkeys_kernel, grid, block, 0, st, seg_offsets, (int)M, (const int*)vin, n, kin);
  int bits = 1;
  while (bits < 32 && (1LL << bits) < M) ++bits;             // keys 0 .. M - 1
  size_t tbytes = tb;
  if (hipcub::DeviceRadixSort::SortPairs(temp, tbytes, (const uint32_t*)kin, kout, (const int*)vin, vout, n, 0, bits, st) != hipSuccess)
    return CRB_ERR_LAUNCH;
  hipLaunchKernelGGL(dyn_gather_kernel, grid, block, 0, st, perm, (const int*)vout, n, perm_out);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
