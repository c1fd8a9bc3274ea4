// Sectorized proposal-centric keypoint sampling (reference: sample_points_with_roi / sector_fps of pcdet/models/backbones_3d/pfe/
// voxel_set_abstraction.py:45-121 and stack_farthest_point_sampling_kernel of pointnet2_stack/src/sampling_gpu.cu:187-319).
// The reference walks the frames and the sectors on the host: B x S boolean masks with a .sum().item() each and an (N, R) distance
// tensor per frame. Here all frames go through four launches and nothing is read back in between:
//   roi_mask_kernel      per point the f32 distance to every RoI centre of its frame, the nearest RoI (lowest index on a tie) and the
//                        bit  min_dis < |dims / 2| + radius; no (N, R) tensor exists
//   spc_sector_kernel    per point the azimuth sector (f32, torch's device arithmetic: the division by the sector size is the
//                        multiplication by its f32 reciprocal), and the (frame, sector) counts of the kept points (integer atomics:
//                        a sum of ones does not depend on the order of arrival)
//   spc_quota_kernel     one workgroup: the points[:1] rule, the per-segment quota  min(n_k, ceil((double(n_k) / double(N)) * double(K))),
//                        the clamped fallback segment, the segment table and the keypoint counts of the frames
//   spc_compact_kernel   one workgroup per (frame, sector): stable compaction (input order, as a boolean mask keeps it) of its points
//   fps_segments_kernel  one 1024-thread workgroup per segment, all segments of all frames in one launch. Tie rule of the reference's
//                        1024-thread strided scan + LDS tree as a strict total order on the candidates k: larger running distance, then
//                        smaller bit-reversed (k mod 1024), then smaller k. Segments up to 20,480 points keep coordinates and distances
//                        in registers (the formulation of fps2_kernel, pointnet2_stack.hip), longer ones keep the distances in a caller-provided
//                        array (fps_large_kernel's way; a 40-distances-per-thread variant beside the others spilled). The choice is made
//                        per workgroup inside the launch.
// No float atomics; every output is a function of the input alone.
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

constexpr int SPC_THREADS = 1024;
constexpr int SPC_MAX_KEYS = 4096;          // B * (S + 1) of one call (LDS of the quota kernel)

// frame of row i: the last b with off[b] <= i (off: B + 1 ascending row offsets)
__device__ __forceinline__ int spc_frame_of(const int* __restrict__ off, int B, int64_t i) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void roi_mask_kernel(const float* __restrict__ pts, int64_t n, int stride, const int* __restrict__ off,
                                                       int B, const float* __restrict__ rois, int R, int roi_stride, float radius,
                                                       uint8_t* __restrict__ mask, int* __restrict__ nearest) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = spc_frame_of(off, B, i);
  const float* p = pts + i * stride;
  const float x = p[0], y = p[1], z = p[2];
  const float* rb = rois + (int64_t)b * R * roi_stride;
  float best = __builtin_inff();
  int bi = 0;
  for (int r = 0; r < R; ++r) {
    const float* q = rb + (int64_t)r * roi_stride;
    const float dx = x - q[0], dy = y - q[1], dz = z - q[2];
    const float d = sqrtf(dx * dx + dy * dy + dz * dz);
    if (d < best || r == 0) { best = d; bi = r; }       // strict: the lowest index of the minimum (a NaN distance never wins after r = 0)
  }
  bool keep = false;
  if (R > 0) {
    const float* q = rb + (int64_t)bi * roi_stride;
    const float hx = q[3] / 2.f, hy = q[4] / 2.f, hz = q[5] / 2.f;
    keep = best < sqrtf(hx * hx + hy * hy + hz * hz) + radius;
  }
  mask[i] = keep ? 1 : 0;
  if (nearest) nearest[i] = bi;
}

// floor((atan2(y, x) + pi) / sector_size) clamped to [0, S]: f32 throughout; inv_size = 1.f / (float)sector_size
__device__ __forceinline__ int spc_sector(float x, float y, float inv_size, int S) {
  const float a = atan2f(y, x) + 3.14159274101257324f;
  float s = floorf(a * inv_size);
  s = s < 0.f ? 0.f : s;                 // (clamp(min, max) of torch: a NaN stays a NaN and equals no sector)
  s = s > (float)S ? (float)S : s;
  return s == s ? (int)s : S;            // NaN: no sector, dropped like sector S
}

__global__ __launch_bounds__(256) void spc_sector_kernel(const float* __restrict__ pts, int64_t n, int stride, const int* __restrict__ off,
                                                         int B, const uint8_t* __restrict__ mask, int S, float inv_size,
                                                         uint8_t* __restrict__ sector, int* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = pts + i * stride;
  const int s = spc_sector(p[0], p[1], inv_size, S);
  sector[i] = (uint8_t)s;
  if (mask[i]) atomicAdd(&cnt[spc_frame_of(off, B, i) * (S + 1) + s], 1);
}

// segment table row: {start in the compacted array, n, m, start in the output, frame, 0, 0, 0}
constexpr int SEG_ROW = 8;

// hdr: [0] segments, [1] compacted rows, [2] keypoints, [3 + b] keypoints of frame b
__global__ __launch_bounds__(256) void spc_quota_kernel(const int* __restrict__ off, int64_t n, int B, int S, int K, const uint8_t* __restrict__ sector,
                                                        int* __restrict__ cnt, int* __restrict__ key_start, int* __restrict__ seg,
                                                        int* __restrict__ hdr, uint8_t* __restrict__ first_rule) {
  __shared__ int c[SPC_MAX_KEYS];
  const int S1 = S + 1;
  for (int b = threadIdx.x; b < B; b += 256) {             // the points[:1] rule, per frame
    int kept = 0;
    for (int s = 0; s < S1; ++s) kept += cnt[b * S1 + s];
    const bool first = kept == 0 && off[b + 1] > off[b] && off[b] >= 0 && (int64_t)off[b] < n;     // (offsets past the array: no row is read)
    first_rule[b] = first ? 1 : 0;
    for (int s = 0; s < S1; ++s) c[b * S1 + s] = cnt[b * S1 + s];
    if (first) c[b * S1 + sector[off[b]]] = 1;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int nseg = 0, rows = 0, picks = 0;
  for (int b = 0; b < B; ++b) {
    int kept = 0;
    for (int s = 0; s < S1; ++s) kept += c[b * S1 + s];
    const bool fallback = kept > 0 && kept == c[b * S1 + S];        // every kept point fell to the clamp: one segment of all of them
    int frame_picks = 0;
    for (int s = 0; s < S1; ++s) {
      const int nk = c[b * S1 + s];
      const bool is_seg = nk > 0 && (s < S || fallback);
      key_start[b * S1 + s] = is_seg ? rows : -1;
      if (!is_seg) continue;
      int m;
      if (s < S) {
        const double ratio = (double)nk / (double)kept;
        const double want = ceil(ratio * (double)K);
        m = want < (double)nk ? (int)want : nk;
      } else {
        m = nk < K ? nk : K;
      }
      m = m < 0 ? 0 : m;
      int* row = seg + (int64_t)nseg * SEG_ROW;
      row[0] = rows; row[1] = nk; row[2] = m; row[3] = picks; row[4] = b; row[5] = 0; row[6] = 0; row[7] = 0;
      rows += nk; picks += m; frame_picks += m; ++nseg;
    }
    hdr[3 + b] = frame_picks;
  }
  hdr[0] = nseg; hdr[1] = rows; hdr[2] = picks;
}

__global__ __launch_bounds__(SPC_THREADS) void spc_compact_kernel(const float* __restrict__ pts, int stride, const int* __restrict__ off, int S,
                                                                  const uint8_t* __restrict__ mask, const uint8_t* __restrict__ sector,
                                                                  const uint8_t* __restrict__ first_rule, const int* __restrict__ key_start,
                                                                  int64_t cap, float* __restrict__ xyz_out, int* __restrict__ src_idx) {
  __shared__ int wave_cnt[16];
  const int key = blockIdx.x, b = key / (S + 1), s = key - b * (S + 1);
  const int start = key_start[key];
  if (start < 0) return;
  const int beg = off[b] < 0 ? 0 : off[b], end = (int64_t)off[b + 1] < cap ? off[b + 1] : (int)cap;      // (cap = rows of the inputs)
  const bool first = first_rule[b] != 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int at = start;
  for (int i0 = beg; i0 < end; i0 += SPC_THREADS) {
    const int i = i0 + tid;
    const bool in = i < end && (int)sector[i < end ? i : beg] == s && (first ? i == beg : mask[i < end ? i : beg] != 0);
    const unsigned long long bal = __ballot(in);
    if (lane == 0) wave_cnt[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int v = wave_cnt[w];
      before += w < wave ? v : 0;
      total += v;
    }
    const int pos = at + before + __popcll(bal & ((1ULL << lane) - 1ULL));
    if (in && (int64_t)pos < cap) {
      const float* p = pts + (int64_t)i * stride;
      xyz_out[(int64_t)pos * 3 + 0] = p[0]; xyz_out[(int64_t)pos * 3 + 1] = p[1]; xyz_out[(int64_t)pos * 3 + 2] = p[2];
      src_idx[pos] = i;
    }
    at += total;
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ segmented FPS
typedef float seg_f2 __attribute__((ext_vector_type(2)));

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float seg_dpp_f(float old, float src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), CTRL, ROW_MASK, 0xf, false));
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ unsigned seg_dpp_u(unsigned old, unsigned src) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ float seg_wave_max(float v) {
  v = fmaxf(v, seg_dpp_f<0x111>(v, v));          // row_shr:1
  v = fmaxf(v, seg_dpp_f<0x112>(v, v));          // row_shr:2
  v = fmaxf(v, seg_dpp_f<0x114>(v, v));          // row_shr:4
  v = fmaxf(v, seg_dpp_f<0x118>(v, v));          // row_shr:8   -> lane 15 of every row: the row's maximum
  v = fmaxf(v, seg_dpp_f<0x142, 0xa>(v, v));     // row_bcast:15 into rows 1, 3
  v = fmaxf(v, seg_dpp_f<0x143, 0xc>(v, v));     // row_bcast:31 into rows 2, 3
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ unsigned seg_wave_min_u(unsigned v) {
  v = min(v, seg_dpp_u<0x111>(v, v));
  v = min(v, seg_dpp_u<0x112>(v, v));
  v = min(v, seg_dpp_u<0x114>(v, v));
  v = min(v, seg_dpp_u<0x118>(v, v));
  v = min(v, seg_dpp_u<0x142, 0xa>(v, v));
  v = min(v, seg_dpp_u<0x143, 0xc>(v, v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

struct SegOut {
  int* idx;          // (m) global rows of the compacted array, or NULL
  float* kp;         // (m, 4) [frame, x, y, z], or NULL
  int base;          // the segment's first row
  float frame;
};
__device__ __forceinline__ void seg_emit(const SegOut& o, int j, int sel, float x, float y, float z) {
  if (o.idx) o.idx[j] = o.base + sel;
  if (o.kp) { o.kp[(int64_t)j * 4 + 0] = o.frame; o.kp[(int64_t)j * 4 + 1] = x; o.kp[(int64_t)j * 4 + 2] = y; o.kp[(int64_t)j * 4 + 3] = z; }
}

// n <= 1024 * PPT: coordinates and running distances in registers, one barrier per round (fps2_kernel with the block size fixed at 1024)
template <int PPT>
__device__ __forceinline__ void fps_seg_regs(int n, int m, const float* __restrict__ xyz, const SegOut& o, float (*slot)[16][8]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  seg_f2 px[PPT / 2], py[PPT / 2], pz[PPT / 2], dist[PPT / 2];      // element e of pair h: point tid + (2 h + e) * 1024
#pragma unroll
  for (int h = 0; h < PPT / 2; ++h)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int k = tid + (2 * h + e) * SPC_THREADS;
      const bool in = k < n;
      px[h][e] = in ? xyz[k * 3 + 0] : 0.f; py[h][e] = in ? xyz[k * 3 + 1] : 0.f; pz[h][e] = in ? xyz[k * 3 + 2] : 0.f;
      dist[h][e] = in ? 1e10f : -1.f;              // a slot past the end never wins: min(d, -1) = -1 < every real distance
    }
  float x1 = xyz[0], y1 = xyz[1], z1 = xyz[2];
  if (tid == 0) seg_emit(o, 0, 0, x1, y1, z1);
  for (int j = 1; j < m; ++j) {
    const seg_f2 X1 = (seg_f2){x1, x1}, Y1 = (seg_f2){y1, y1}, Z1 = (seg_f2){z1, z1};
    float lmax = -1.f;
#pragma unroll
    for (int h = 0; h < PPT / 2; ++h) {
      const seg_f2 dx = px[h] - X1, dy = py[h] - Y1, dz = pz[h] - Z1;
      const seg_f2 d = dx * dx + dy * dy + dz * dz;
      float d0, d1;                                 // (no NaNs in a distance to a real point: plain v_min / v_max3, no canonicalising copies)
      asm("v_min_f32 %0, %1, %2" : "=v"(d0) : "v"(d[0]), "v"(dist[h][0]));
      asm("v_min_f32 %0, %1, %2" : "=v"(d1) : "v"(d[1]), "v"(dist[h][1]));
      dist[h] = (seg_f2){d0, d1};
      asm("v_max3_f32 %0, %1, %2, %3" : "=v"(lmax) : "v"(lmax), "v"(d0), "v"(d1));
    }
    const float bestd = lmax;
    const float M = seg_wave_max(bestd);
    int bestt = 0;                                  // the lane's first maximum (descending scan: the smallest t is written last)
#pragma unroll
    for (int t = PPT - 1; t >= 0; --t) bestt = dist[t >> 1][t & 1] == bestd ? t : bestt;
    const int bestk = tid + bestt * SPC_THREADS;
    const unsigned br = __brev((unsigned)bestk & 1023u) >> 22;
    const unsigned key = (bestd == M && bestd >= 0.f) ? ((br << 20) | (unsigned)bestk) : 0xffffffffu;
    const unsigned K = seg_wave_min_u(key);
    float* sl = slot[j & 1][0];
    if (key == K && K != 0xffffffffu) {
      const float* p = xyz + (int64_t)bestk * 3;
      float* w = sl + wave * 8;
      w[0] = M; w[1] = __uint_as_float(K); w[2] = p[0]; w[3] = p[1]; w[4] = p[2];
    } else if (K == 0xffffffffu && lane == 0) {
      float* w = sl + wave * 8;
      w[0] = -1.f; w[1] = __uint_as_float(K);
    }
    __syncthreads();
    const int w16 = lane & 15;
    const float sd = sl[w16 * 8];
    const unsigned sk = __float_as_uint(sl[w16 * 8 + 1]);
    float gm = sd;
    gm = fmaxf(gm, seg_dpp_f<0x111>(gm, gm));
    gm = fmaxf(gm, seg_dpp_f<0x112>(gm, gm));
    gm = fmaxf(gm, seg_dpp_f<0x114>(gm, gm));
    gm = fmaxf(gm, seg_dpp_f<0x118>(gm, gm));
    const float GM = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, gm), 15));
    unsigned gk = sd == GM ? sk : 0xffffffffu;
    gk = min(gk, seg_dpp_u<0x111>(gk, gk));
    gk = min(gk, seg_dpp_u<0x112>(gk, gk));
    gk = min(gk, seg_dpp_u<0x114>(gk, gk));
    gk = min(gk, seg_dpp_u<0x118>(gk, gk));
    const unsigned GK = (unsigned)__builtin_amdgcn_readlane((int)gk, 15);
    const unsigned long long wb = __ballot(sd == GM && sk == GK) & 0xffffULL;
    const int ww = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(wb ? wb : 1ULL));
    x1 = sl[ww * 8 + 2]; y1 = sl[ww * 8 + 3]; z1 = sl[ww * 8 + 4];
    if (tid == 0) seg_emit(o, j, (int)(GK & 0xfffffu), x1, y1, z1);
  }
}

// the workgroup's best candidate from every thread's (distance, first index): 64-bit keys, larger wins. The low word orders
// (bit-reversed k mod 1024, k div 1024), which identifies k: any segment length below 2^31 fits
__device__ __forceinline__ int fps_seg_reduce(float bestd, int bestk, unsigned long long* wave_best) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long best = 0ULL;
  if (bestd >= 0.f) {
    const unsigned br = __brev((unsigned)bestk & 1023u) >> 22;
    best = ((unsigned long long)__float_as_uint(bestd) << 32) | (0xffffffffu - ((br << 22) | ((unsigned)bestk >> 10)));
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const unsigned long long v = __shfl_xor(best, s, 64);
    best = v > best ? v : best;
  }
  if (lane == 0) wave_best[wave] = best;
  __syncthreads();
  unsigned long long b2 = wave_best[lane & 15];
#pragma unroll
  for (int s = 8; s > 0; s >>= 1) {
    const unsigned long long v = __shfl_xor(b2, s, 64);
    b2 = v > b2 ? v : b2;
  }
  const unsigned low = 0xffffffffu - (unsigned)(b2 & 0xffffffffULL);
  return (int)(((low & 0x3fffffu) << 10) | (__brev(low >> 22) >> 22));
}

// any n: running distances in the caller's array
__device__ __forceinline__ void fps_seg_global(int n, int m, const float* __restrict__ xyz, float* __restrict__ dist, const SegOut& o,
                                               unsigned long long* wave_best, float* sel_xyz) {
  const int tid = threadIdx.x;
  for (int k = tid; k < n; k += SPC_THREADS) dist[k] = 1e10f;
  if (tid == 0) { sel_xyz[0] = xyz[0]; sel_xyz[1] = xyz[1]; sel_xyz[2] = xyz[2]; seg_emit(o, 0, 0, xyz[0], xyz[1], xyz[2]); }
  __syncthreads();
  for (int j = 1; j < m; ++j) {
    const float x1 = sel_xyz[0], y1 = sel_xyz[1], z1 = sel_xyz[2];
    float bestd = -1.f;
    int bestk = 0;
    for (int k = tid; k < n; k += SPC_THREADS) {
      const float dx = xyz[(int64_t)k * 3 + 0] - x1, dy = xyz[(int64_t)k * 3 + 1] - y1, dz = xyz[(int64_t)k * 3 + 2] - z1;
      const float d2 = fminf(dx * dx + dy * dy + dz * dz, dist[k]);
      dist[k] = d2;
      if (d2 > bestd) { bestd = d2; bestk = k; }
    }
    const int sel = fps_seg_reduce(bestd, bestk, wave_best);
    if (tid == 0) {
      const float x = xyz[(int64_t)sel * 3 + 0], y = xyz[(int64_t)sel * 3 + 1], z = xyz[(int64_t)sel * 3 + 2];
      seg_emit(o, j, sel, x, y, z);
      sel_xyz[0] = x; sel_xyz[1] = y; sel_xyz[2] = z;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SPC_THREADS) void fps_segments_kernel(const float* __restrict__ xyz, int64_t rows, const int* __restrict__ seg,
                                                                   const int* __restrict__ nseg_dev, int nseg_host, int64_t out_cap,
                                                                   float* __restrict__ temp, int* __restrict__ idx, float* __restrict__ kp) {
  __shared__ float slot[2][16][8];
  __shared__ unsigned long long wave_best[16];
  __shared__ float sel_xyz[3];
  const int nseg = nseg_dev ? min(*nseg_dev, nseg_host) : nseg_host;
  if ((int)blockIdx.x >= nseg) return;
  const int* row = seg + (int64_t)blockIdx.x * SEG_ROW;
  const int start = row[0], n = row[1], out_start = row[3];
  const int m = min(row[2], n);
  // (a table that points outside the arrays is skipped, never followed)
  if (n <= 0 || m <= 0 || start < 0 || (int64_t)start + n > rows || out_start < 0 || (int64_t)out_start + m > out_cap) return;
  const float* p = xyz + (int64_t)start * 3;
  SegOut o;
  o.idx = idx ? idx + out_start : nullptr;
  o.kp = kp ? kp + (int64_t)out_start * 4 : nullptr;
  o.base = start;
  o.frame = (float)row[4];
  if (n <= 2 * SPC_THREADS) fps_seg_regs<2>(n, m, p, o, slot);
  else if (n <= 4 * SPC_THREADS) fps_seg_regs<4>(n, m, p, o, slot);
  else if (n <= 8 * SPC_THREADS) fps_seg_regs<8>(n, m, p, o, slot);
  else if (n <= 20 * SPC_THREADS) fps_seg_regs<20>(n, m, p, o, slot);
  else if (temp) fps_seg_global(n, m, p, temp + start, o, wave_best, sel_xyz);
}

}  // namespace

extern "C" int crb_roi_proximity_mask(const float* points, int64_t n, int row_stride, const int32_t* frame_offsets, int B, const float* rois,
                                      int R, int roi_stride, float radius, uint8_t* mask, int32_t* nearest, void* stream) {
  if (n < 0 || B <= 0 || R < 0 || row_stride < 3 || (R > 0 && roi_stride < 6) || n > 0x7fffffffLL) return CRB_ERR_ARG;
  if (n == 0) return CRB_OK;
  hipLaunchKernelGGL(roi_mask_kernel, dim3(crb_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, points, n, row_stride, frame_offsets, B,
                     rois, R, roi_stride, radius, mask, nearest);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_spc_plan_workspace_bytes(int B, int S) {
  if (B <= 0 || S <= 0) return 0;
  return 2 * crb_align_up((int64_t)B * (S + 1) * 4, 256) + crb_align_up(B, 256);
}

extern "C" int crb_spc_plan(const float* points, int64_t n, int row_stride, const int32_t* frame_offsets, int B, const uint8_t* mask, int S,
                            int K, float inv_sector_size, uint8_t* sector, float* xyz_out, int32_t* src_idx, int32_t* seg_table,
                            int32_t* header, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n < 0 || B <= 0 || S <= 0 || S > 254 || K < 0 || row_stride < 3 || n > 0x7fffffffLL) return CRB_ERR_ARG;
  if ((int64_t)B * (S + 1) > SPC_MAX_KEYS) return CRB_ERR_UNSUPPORTED;
  CrbArena a(workspace, (size_t)workspace_bytes);
  int* cnt = a.take<int>((int64_t)B * (S + 1));
  int* key_start = a.take<int>((int64_t)B * (S + 1));
  uint8_t* first_rule = a.take<uint8_t>(B);
  if (!a.ok) return CRB_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  CRB_HIP(hipMemsetAsync(cnt, 0, (size_t)B * (S + 1) * 4, st));
  if (n > 0)
    hipLaunchKernelGGL(spc_sector_kernel, dim3(crb_cdiv(n, 256)), dim3(256), 0, st, points, n, row_stride, frame_offsets, B, mask, S,
                       inv_sector_size, sector, cnt);
  hipLaunchKernelGGL(spc_quota_kernel, dim3(1), dim3(256), 0, st, frame_offsets, n, B, S, K, sector, cnt, key_start, seg_table, header, first_rule);
  if (n > 0)
    hipLaunchKernelGGL(spc_compact_kernel, dim3(B * (S + 1)), dim3(SPC_THREADS), 0, st, points, row_stride, frame_offsets, S, mask, sector,
                       first_rule, key_start, n, xyz_out, src_idx);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_fps_segments(const float* xyz, int64_t rows, const int32_t* seg_table, const int32_t* num_segments, int max_segments,
                                int64_t out_capacity, float* temp, int32_t* out_idx, float* out_keypoints, void* stream) {
  if (rows < 0 || max_segments < 0 || out_capacity < 0 || rows > 0x7fffffffLL) return CRB_ERR_ARG;
  if (max_segments == 0 || rows == 0 || out_capacity == 0) return CRB_OK;
  if (rows > 20LL * SPC_THREADS && !temp) return CRB_ERR_WORKSPACE;       // a segment may be as long as the whole array
  hipLaunchKernelGGL(fps_segments_kernel, dim3(max_segments), dim3(SPC_THREADS), 0, (hipStream_t)stream, xyz, rows, seg_table, num_segments,
                     max_segments, out_capacity, temp, out_idx, out_keypoints);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
