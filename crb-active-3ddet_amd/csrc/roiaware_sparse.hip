// RoI-aware pooling of all frames straight into the rows of the sparse RoI-grid tensor (PartA2FCHead) for gfx950.
//
// Replaces, for the head's use, the per-frame loop over crb_roiaware_pool3d_forward (csrc/roiaware_pool3d.hip): two collect
// passes per frame into (R, o,o,o, max_pts) tables, two dense (R, o,o,o, C) grids, `sum(-1).nonzero()` and a gather. Same
// semantics, cell by cell: pt_in_box + the unsigned cell index of roiaware_collect_kernel, the first max_pts - 1 points of a
// cell in ascending point index, avg = sequential f32 sum / (float)n, max = first largest value.
//
// Shape: one WAVE per RoI (b * R + r) walks the points of its frame in 64-point rounds and bins them into a per-wave LDS
// histogram over the o^3 cells with the ordered ballot placement of the dense collect kernel (a group of lanes that hit the
// same cell takes consecutive positions by lane rank, so point order survives).
//   count  histogram -> per RoI {rows, kept hits}; a cell is a row iff one of its KEPT points has a non-zero part feature
//          (the dense rule `sum of the four averages != 0` for non-negative features; a negative feature inside a RoI raises
//          the device flag and the caller takes the dense route)
//   (the caller scans the per-RoI pairs and reads back the two totals and the flag: the one read-back)
//   fill   histogram again, a wave scan over the cells in lexicographic order gives every row its number and its slice of
//          the hit list, a second walk over the points writes the CSR list row -> kept points
//   pool   one thread per (row, channel)
// Backward: the kept (point, row) pairs are stable-sorted by point (hipCUB LSD radix sort; the list is in row order, so the
// rows of a point stay ascending) and one thread per (point, channel) sums its rows in that order: no float atomics.
//
// Memory: 2 ints per RoI, 5 ints per row, 2 ints per kept hit (+ the sort's double buffer in backward). Nothing of size
// B*R*o^3.
#include <hipcub/hipcub.hpp>

#include "crb_common.h"
#include "pt_in_box.h"
#include "../../include/crb_hip.h"

namespace {

constexpr int RS_MAX_CELLS = 4096;          // 3 int tables of o^3 cells per wave in LDS: 48 KB at the limit
constexpr int RS_ROW_FLAG = 1 << 30;        // bit 30 of a histogram word: the cell is a row; bits 0..29: saturated count
constexpr int RS_CNT_MASK = RS_ROW_FLAG - 1;

struct RoiGeom { BoxLds b; float x_res, y_res, z_res; int ox, oy, oz; };

// cell of point (x,y,z) in the RoI or -1: roiaware_collect_kernel's arithmetic
__device__ __forceinline__ int rs_cell_code(const RoiGeom& g, float x, float y, float z) {
  float lx, ly;
  if (!pt_in_box(x, y, z, g.b, lx, ly)) return -1;
  const float lz = z - g.b.cz;
  unsigned xi = (unsigned)(int)((lx + g.b.dx / 2) / g.x_res);
  unsigned yi = (unsigned)(int)((ly + g.b.dy / 2) / g.y_res);
  unsigned zi = (unsigned)(int)((lz + g.b.dz / 2) / g.z_res);
  xi = min(max(xi, 0u), (unsigned)(g.ox - 1));
  yi = min(max(yi, 0u), (unsigned)(g.oy - 1));
  zi = min(max(zi, 0u), (unsigned)(g.oz - 1));
  return (int)((xi * g.oy + yi) * g.oz + zi);
}

__device__ __forceinline__ RoiGeom rs_load_roi(const float* r, int ox, int oy, int oz) {
  RoiGeom g;
  g.b = load_box(r);
  g.x_res = g.b.dx / ox; g.y_res = g.b.dy / oy; g.z_res = g.b.dz / oz;
  g.ox = ox; g.oy = oy; g.oz = oz;
  return g;
}

// The histogram pass shared by count and fill: hist[cell] = min(hits, cap) | RS_ROW_FLAG when a kept point of the cell has a
// non-zero part feature. Returns (wave-uniform) whether a point inside the RoI carries a negative part feature.
__device__ __forceinline__ bool rs_histogram(const RoiGeom& g, int n0, int n1, int cap, const float* __restrict__ pts,
                                             const float* __restrict__ part, volatile int* hist) {
  const int lane = crb_lane();
  bool neg = false;
  for (int k0 = n0; k0 < n1; k0 += 64) {
    const int k = k0 + lane;
    int code = -1;
    if (k < n1) code = rs_cell_code(g, pts[(int64_t)k * 3], pts[(int64_t)k * 3 + 1], pts[(int64_t)k * 3 + 2]);
    unsigned long long todo = __ballot(code >= 0);
    if (!todo) continue;
    bool nz = false;
    if (code >= 0) {
      const float4 f = *reinterpret_cast<const float4*>(part + (int64_t)k * 4);
      nz = f.x != 0.f || f.y != 0.f || f.z != 0.f || f.w != 0.f;
      neg = neg || f.x < 0.f || f.y < 0.f || f.z < 0.f || f.w < 0.f;
    }
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int c0 = __shfl(code, leader, 64);
      const unsigned long long same = __ballot(code == c0);
      const int old = hist[c0];                                  // every lane reads before the leader writes
      const int pos = (old & RS_CNT_MASK) + __popcll(same & ((1ULL << lane) - 1ULL));
      const unsigned long long live = __ballot(code == c0 && pos < cap && nz);
      if (lane == leader)
        hist[c0] = min((old & RS_CNT_MASK) + (int)__popcll(same), cap) | (old & RS_ROW_FLAG) | (live ? RS_ROW_FLAG : 0);
      todo &= ~same;
    }
  }
  return __ballot(neg) != 0ULL;
}

// one wave per RoI -> roi_counts[roi] = {rows, kept hits}
__global__ __launch_bounds__(64) void rs_count_kernel(int R, int ox, int oy, int oz, int max_pts,
                                                      const float* __restrict__ rois, const float* __restrict__ pts,
                                                      const int* __restrict__ off, const float* __restrict__ part,
                                                      int* __restrict__ roi_counts, int* __restrict__ flag) {
  extern __shared__ int rs_lds[];
  const int roi = blockIdx.x, lane = crb_lane();
  const int ncell = ox * oy * oz;
  for (int c = lane; c < ncell; c += 64) rs_lds[c] = 0;
  __syncthreads();
  const RoiGeom g = rs_load_roi(rois + (int64_t)roi * 7, ox, oy, oz);
  const int b = roi / R;
  const bool neg = rs_histogram(g, off[b], off[b + 1], max_pts - 1, pts, part, rs_lds);
  __syncthreads();
  int rows = 0, hits = 0;
  for (int c = lane; c < ncell; c += 64) {
    const int v = rs_lds[c];
    if (v & RS_ROW_FLAG) { rows += 1; hits += v & RS_CNT_MASK; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    rows += __shfl_xor(rows, d, 64);
    hits += __shfl_xor(hits, d, 64);
  }
  if (lane == 0) {
    roi_counts[roi * 2] = rows;
    roi_counts[roi * 2 + 1] = hits;
    if (neg) atomicOr(flag, 1);
  }
}

// one wave per RoI; roi_starts[roi] = exclusive scan of roi_counts: {first row, first hit}
__global__ __launch_bounds__(64) void rs_fill_kernel(int R, int ox, int oy, int oz, int max_pts, int T, int H,
                                                     const float* __restrict__ rois, const float* __restrict__ pts,
                                                     const int* __restrict__ off, const float* __restrict__ part,
                                                     const int* __restrict__ roi_starts, int* __restrict__ coords,
                                                     int* __restrict__ row_ptr, int* __restrict__ hit_pt,
                                                     int* __restrict__ hit_row) {
  extern __shared__ int rs_lds[];
  const int roi = blockIdx.x, lane = crb_lane();
  const int ncell = ox * oy * oz;
  int* hist = rs_lds;                      // histogram, then the running position of the second walk
  int* start = rs_lds + ncell;             // first hit of the cell's row, relative to the RoI's first hit; -1: no row
  int* rowrel = rs_lds + 2 * ncell;        // row of the cell, relative to the RoI's first row
  if (roi == 0 && lane == 0) row_ptr[T] = H;
  for (int c = lane; c < ncell; c += 64) hist[c] = 0;
  __syncthreads();
  const RoiGeom g = rs_load_roi(rois + (int64_t)roi * 7, ox, oy, oz);
  const int b = roi / R;
  const int n0 = off[b], n1 = off[b + 1];
  const int cap = max_pts - 1;
  rs_histogram(g, n0, n1, cap, pts, part, hist);
  __syncthreads();
  const int row0 = roi_starts[roi * 2], hit0 = roi_starts[roi * 2 + 1];
  int row_run = 0, hit_run = 0;
  for (int c0 = 0; c0 < ncell; c0 += 64) {           // cells in lexicographic (x, y, z) order
    const int c = c0 + lane;
    const int v = c < ncell ? hist[c] : 0;
    const int is_row = (v & RS_ROW_FLAG) ? 1 : 0;
    const int kept = is_row ? (v & RS_CNT_MASK) : 0;
    const int row_inc = crb_wave_incl_scan(is_row), hit_inc = crb_wave_incl_scan(kept);
    if (c < ncell) {
      hist[c] = 0;
      start[c] = is_row ? hit_run + hit_inc - kept : -1;
      rowrel[c] = row_run + row_inc - 1;
      const int row = row0 + row_run + row_inc - 1;
      if (is_row && row < T) {
        const int z = c % oz, y = (c / oz) % oy, x = c / (oz * oy);
        coords[(int64_t)row * 4] = roi;
        coords[(int64_t)row * 4 + 1] = x;
        coords[(int64_t)row * 4 + 2] = y;
        coords[(int64_t)row * 4 + 3] = z;
        row_ptr[row] = hit0 + hit_run + hit_inc - kept;
      }
    }
    row_run += __shfl(row_inc, 63, 64);
    hit_run += __shfl(hit_inc, 63, 64);
  }
  __syncthreads();
  volatile int* run = hist;
  for (int k0 = n0; k0 < n1; k0 += 64) {
    const int k = k0 + lane;
    int code = -1;
    if (k < n1) code = rs_cell_code(g, pts[(int64_t)k * 3], pts[(int64_t)k * 3 + 1], pts[(int64_t)k * 3 + 2]);
    unsigned long long todo = __ballot(code >= 0);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const int c0 = __shfl(code, leader, 64);
      const unsigned long long same = __ballot(code == c0);
      const int base = run[c0];
      const int st = start[c0];
      if (code == c0 && st >= 0) {
        const int pos = base + __popcll(same & ((1ULL << lane) - 1ULL));
        const int h = hit0 + st + pos;
        if (pos < cap && h < H) {
          hit_pt[h] = k;
          hit_row[h] = row0 + rowrel[c0];
        }
      }
      if (lane == leader) run[c0] = min(base + (int)__popcll(same), cap);
      todo &= ~same;
    }
  }
}

// one thread per (row, channel): channels 0..3 avg of the part features, 4..4+C-1 max of the point features
__global__ __launch_bounds__(256) void rs_pool_kernel(int64_t total, int C, const int* __restrict__ row_ptr,
                                                      const int* __restrict__ hit_pt, const float* __restrict__ part,
                                                      const float* __restrict__ feat, float* __restrict__ out_part,
                                                      float* __restrict__ out_feat, int* __restrict__ argmax) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int W = 4 + C;
  const int64_t row = t / W;
  const int c = (int)(t - row * W);
  const int lo = row_ptr[row], n = row_ptr[row + 1] - lo;
  if (c < 4) {
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += part[(int64_t)hit_pt[lo + k] * 4 + c];
    out_part[row * 4 + c] = n > 0 ? s / (float)n : 0.f;
  } else {
    const int cc = c - 4;
    int am = -1;
    float mx = -INFINITY;
    for (int k = 0; k < n; ++k) {
      const int p = hit_pt[lo + k];
      const float f = feat[(int64_t)p * C + cc];
      if (f > mx) { mx = f; am = p; }
    }
    out_feat[row * C + cc] = am != -1 ? mx : 0.f;
    argmax[row * C + cc] = am;
  }
}

// first position of every point in the sorted pair list: pt_start[p] = lower_bound(keys, p), p = 0..N
__global__ __launch_bounds__(256) void rs_point_start_kernel(int N, int H, const uint32_t* __restrict__ keys,
                                                             int* __restrict__ pt_start) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p > N) return;
  int lo = 0, hi = H;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < (uint32_t)p) lo = mid + 1; else hi = mid;
  }
  pt_start[p] = lo;
}

// one thread per (point, channel), summing over the point's rows in ascending row order
__global__ __launch_bounds__(256) void rs_bwd_kernel(int64_t total, int C, const int* __restrict__ pt_start,
                                                     const int* __restrict__ rows, const int* __restrict__ row_ptr,
                                                     const int* __restrict__ argmax, const float* __restrict__ g_part,
                                                     const float* __restrict__ g_feat, float* __restrict__ grad_part,
                                                     float* __restrict__ grad_feat) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int W = 4 + C;
  const int64_t p = t / W;
  const int c = (int)(t - p * W);
  const int lo = pt_start[p], hi = pt_start[p + 1];
  float acc = 0.f;
  if (c < 4) {
    for (int j = lo; j < hi; ++j) {
      const int row = rows[j];
      const int n = row_ptr[row + 1] - row_ptr[row];
      acc += g_part[(int64_t)row * 4 + c] * (1 / fmaxf((float)n, 1.0f));
    }
    grad_part[p * 4 + c] = acc;
  } else {
    const int cc = c - 4;
    for (int j = lo; j < hi; ++j) {
      const int row = rows[j];
      if (argmax[(int64_t)row * C + cc] == (int)p) acc += g_feat[(int64_t)row * C + cc];
    }
    grad_feat[p * C + cc] = acc;
  }
}

size_t rs_sort_temp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int*)nullptr,
                                           (int*)nullptr, (int)n, 0, 32, (hipStream_t)0);
  return b;
}

// (B >= 1 frames of R >= 1 RoIs: a caller without RoIs has nothing to pool and does not call)
bool rs_bad_shape(int n_rois, int R, int B, int64_t N, int max_pts, int ox, int oy, int oz) {
  return R <= 0 || B <= 0 || n_rois != B * R || N < 0 || N >= (1LL << 30) || max_pts < 2 ||
         max_pts > RS_CNT_MASK || ox <= 0 || oy <= 0 || oz <= 0;
}

}  // namespace

extern "C" int crb_roiaware_sparse_max_cells(void) { return RS_MAX_CELLS; }

extern "C" int crb_roiaware_sparse_count(int n_rois, int R, int B, int64_t N, int max_pts_each_voxel, int out_x, int out_y,
                                         int out_z, const float* rois, const float* pts, const int32_t* frame_offsets,
                                         const float* part, int32_t* roi_counts, int32_t* flag, void* stream) {
  if (rs_bad_shape(n_rois, R, B, N, max_pts_each_voxel, out_x, out_y, out_z) || !flag) return CRB_ERR_ARG;
  if ((int64_t)out_x * out_y * out_z > RS_MAX_CELLS) return CRB_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  CRB_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), st));
  if (!rois || !frame_offsets || !roi_counts || (N > 0 && (!pts || !part))) return CRB_ERR_ARG;
  const int ncell = out_x * out_y * out_z;
  hipLaunchKernelGGL(rs_count_kernel, dim3(n_rois), dim3(64), (size_t)ncell * sizeof(int), st, R, out_x, out_y, out_z,
                     max_pts_each_voxel, rois, pts, frame_offsets, part, roi_counts, flag);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_roiaware_sparse_fill(int n_rois, int R, int B, int64_t N, int max_pts_each_voxel, int out_x, int out_y,
                                        int out_z, const float* rois, const float* pts, const int32_t* frame_offsets,
                                        const float* part, const int32_t* roi_starts, int64_t T, int64_t H, int32_t* coords,
                                        int32_t* row_ptr, int32_t* hit_pt, int32_t* hit_row, void* stream) {
  if (rs_bad_shape(n_rois, R, B, N, max_pts_each_voxel, out_x, out_y, out_z) || T < 0 || H < T || H >= (1LL << 31) - 1 ||
      !row_ptr)
    return CRB_ERR_ARG;
  if ((int64_t)out_x * out_y * out_z > RS_MAX_CELLS) return CRB_ERR_UNSUPPORTED;
  if (!rois || !frame_offsets || !roi_starts || (N > 0 && (!pts || !part)) || (T > 0 && !coords) || (H > 0 && (!hit_pt || !hit_row)))
    return CRB_ERR_ARG;
  const int ncell = out_x * out_y * out_z;
  hipLaunchKernelGGL(rs_fill_kernel, dim3(n_rois), dim3(64), (size_t)ncell * 3 * sizeof(int), (hipStream_t)stream, R, out_x,
                     out_y, out_z, max_pts_each_voxel, (int)T, (int)H, rois, pts, frame_offsets, part, roi_starts, coords,
                     row_ptr, hit_pt, hit_row);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_roiaware_sparse_pool(int64_t T, int C, const int32_t* row_ptr, const int32_t* hit_pt, const float* part,
                                        const float* feat, float* out_part, float* out_feat, int32_t* argmax, void* stream) {
  if (T < 0 || C <= 0 || T * (4 + (int64_t)C) >= (1LL << 31) * 256) return CRB_ERR_ARG;
  if (T == 0) return CRB_OK;
  if (!row_ptr || !hit_pt || !part || !feat || !out_part || !out_feat || !argmax) return CRB_ERR_ARG;
  const int64_t total = T * (4 + C);
  hipLaunchKernelGGL(rs_pool_kernel, dim3(crb_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, total, C, row_ptr, hit_pt,
                     part, feat, out_part, out_feat, argmax);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_roiaware_sparse_backward_workspace_bytes(int64_t N, int64_t H) {
  if (N < 0 || H < 0) return 256;
  return 2 * crb_align_up(4 * (H + 1), 256) + crb_align_up(4 * (N + 1), 256) +
         crb_align_up((int64_t)rs_sort_temp_bytes(H > 0 ? H : 1), 256) + 256;
}

extern "C" int crb_roiaware_sparse_backward(int64_t N, int64_t T, int64_t H, int C, const int32_t* row_ptr,
                                            const int32_t* hit_pt, const int32_t* hit_row, const int32_t* argmax,
                                            const float* g_part, const float* g_feat, float* grad_part, float* grad_feat,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (N < 0 || N >= (1LL << 30) || T < 0 || H < 0 || H >= (1LL << 31) - 1 || C <= 0) return CRB_ERR_ARG;
  if (N == 0) return CRB_OK;
  if (!grad_part || !grad_feat || (H > 0 && (!row_ptr || !hit_pt || !hit_row || !argmax || !g_part || !g_feat)))
    return CRB_ERR_ARG;
  if (!workspace || workspace_bytes < crb_roiaware_sparse_backward_workspace_bytes(N, H)) return CRB_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CrbArena ar(workspace, (size_t)workspace_bytes);
  uint32_t* keys = ar.take<uint32_t>(H + 1);
  int* rows = ar.take<int>(H + 1);
  int* pt_start = ar.take<int>(N + 1);
  const size_t tb = rs_sort_temp_bytes(H > 0 ? H : 1);
  char* temp = ar.take<char>((int64_t)tb);
  if (!ar.ok) return CRB_ERR_WORKSPACE;
  if (H > 0) {
    int bits = 1;
    while (bits < 32 && (1LL << bits) < N) ++bits;             // keys 0 .. N - 1
    size_t tbytes = tb;
    if (hipcub::DeviceRadixSort::SortPairs(temp, tbytes, (const uint32_t*)hit_pt, keys, (const int*)hit_row, rows, (int)H, 0,
                                           bits, st) != hipSuccess)
      return CRB_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(rs_point_start_kernel, dim3(crb_cdiv(N + 1, 256)), dim3(256), 0, st, (int)N, (int)H, keys, pt_start);
  const int64_t total = N * (4 + C);
  hipLaunchKernelGGL(rs_bwd_kernel, dim3(crb_cdiv(total, 256)), dim3(256), 0, st, total, C, pt_start, rows, row_ptr, argmax,
                     g_part, g_feat, grad_part, grad_feat);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
