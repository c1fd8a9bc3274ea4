// Training-time world augmentation for gfx950, fused with the point-range mask (C-ABI in include/crb_hip.h).
//
// Replaces, for a whole batch on the device, what the reference does per frame in loader workers:
//   pcdet/datasets/augmentor/augmentor_utils.py:8-81,124-175 (random_flip_along_x/y, global_rotation, global_scaling,
//   random_translation_along_x/y/z) as queued by pcdet/datasets/augmentor/data_augmentor.py:43-117,229-258, followed by
//   pcdet/datasets/processor/data_processor.py:78-91 (mask_points_and_boxes_outside_range: common_utils.mask_points_by_range,
//   box_utils.mask_boxes_outside_range_numpy).
//
// The random draws stay on the host (np.random, the reference's calls in the reference's order); the kernels receive one row of
// eight f32 per frame: [flip_x, flip_y, c, s, scale, tx, ty, tz]. Arithmetic definition (pcdet/datasets/augmentor/augmentor_utils.py
// of this repository is the same sequence in numpy, and the two agree bit for bit): f32, one rounding per operation, in the fixed
// order flip x, flip y, rotation, scaling, translation. A step whose parameter is the identity is SKIPPED, not computed (x * 1 and
// x + 0 are not the identity on every bit pattern: -0.0 + 0.0 = +0.0), so identity parameters copy the rows.
//
// Points: three launches, no atomics, stable order.
//   K1 aug_count  one thread per point: transform x/y, range test, wave ballot -> kept rows per 256-point block
//   K2 aug_scan   one block: exclusive scan of the block counts, total, new offsets of the frames that start at or past the end
//   K3 aug_emit   one thread per point: the same test, rank = block base + waves before + lanes before (ballot prefix), write the
//                 transformed row; the first point of a frame writes that frame's new offset (its own rank)
// Boxes: one 256-thread block per frame, stable in-frame compaction by a block scan per 256 boxes.
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

#define AUG_PI_F 3.14159274101257324f        // f32(pi)
#define AUG_TWO_PI_F 6.28318548202514648f    // f32(2 pi)

struct AugFrame {
  float flip_x, flip_y, c, s, scale, tx, ty, tz;
};

__device__ __forceinline__ AugFrame aug_load(const float* __restrict__ params, int b) {
  const float4 lo = *reinterpret_cast<const float4*>(params + (int64_t)b * 8);
  const float4 hi = *reinterpret_cast<const float4*>(params + (int64_t)b * 8 + 4);
  AugFrame f;
  f.flip_x = lo.x; f.flip_y = lo.y; f.c = lo.z; f.s = lo.w;
  f.scale = hi.x; f.tx = hi.y; f.ty = hi.z; f.tz = hi.w;
  return f;
}

__device__ __forceinline__ bool aug_rotates(const AugFrame& f) { return !(f.c == 1.f && f.s == 0.f); }

// (x, y) -> rotated about +z: x' = x c - y s, y' = x s + y c, every product and sum rounded on its own
__device__ __forceinline__ void aug_rot(const AugFrame& f, float& x, float& y) {
  const float nx = __fsub_rn(__fmul_rn(x, f.c), __fmul_rn(y, f.s));
  const float ny = __fadd_rn(__fmul_rn(x, f.s), __fmul_rn(y, f.c));
  x = nx;
  y = ny;
}

__device__ __forceinline__ void aug_point(const AugFrame& f, float& x, float& y, float& z) {
  if (f.flip_x != 0.f) y = -y;
  if (f.flip_y != 0.f) x = -x;
  if (aug_rotates(f)) aug_rot(f, x, y);
  if (f.scale != 1.f) {
    x = __fmul_rn(x, f.scale);
    y = __fmul_rn(y, f.scale);
    z = __fmul_rn(z, f.scale);
  }
  if (f.tx != 0.f) x = __fadd_rn(x, f.tx);
  if (f.ty != 0.f) y = __fadd_rn(y, f.ty);
  if (f.tz != 0.f) z = __fadd_rn(z, f.tz);
}

struct AugRange {
  float x0, y0, z0, x1, y1, z1;
};

// last frame b with frame_off[b] <= i (frame_off ascending, B + 1 entries; empty frames share a start with their successor)
__device__ __forceinline__ int aug_frame_of(const int* __restrict__ frame_off, int B, int i) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (frame_off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

struct AugPoints {
  const float* pts;
  int64_t row_stride;
  int xyz_col;
  int n, B;
  const int* frame_off;
  const float* params;
  AugRange r;
  int do_mask;
  int vec4;      // rows are aligned 16-byte lines with xyz first and a fourth column: one dwordx4 load per row
};

// transformed xyz of point i and whether it survives the range test (mask_points_by_range: x and y only, bounds inclusive; a NaN
// coordinate fails every comparison and is dropped, as in numpy)
__device__ __forceinline__ bool aug_eval(const AugPoints& a, int i, int& b, float& x, float& y, float& z, float& w) {
  const float* q = a.pts + (int64_t)i * a.row_stride + a.xyz_col;
  if (a.vec4) {
    const float4 t = *reinterpret_cast<const float4*>(q);
    x = t.x; y = t.y; z = t.z; w = t.w;
  } else {
    x = q[0]; y = q[1]; z = q[2];
  }
  b = aug_frame_of(a.frame_off, a.B, i);
  const AugFrame f = aug_load(a.params, b);
  aug_point(f, x, y, z);
  return !a.do_mask || (x >= a.r.x0 && x <= a.r.x1 && y >= a.r.y0 && y <= a.r.y1);
}

__global__ __launch_bounds__(256) void aug_count(AugPoints a, int* __restrict__ block_counts) {
  __shared__ int sh[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  if (i < a.n) {
    int b;
    float x, y, z, w;
    keep = aug_eval(a, i, b, x, y, z, w);
  }
  const unsigned long long m = __ballot(keep);
  if (crb_lane() == 0) sh[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// one block: block_counts -> exclusive bases in place; new_off[b] = total for every frame that starts at or past the last point
// (b = B always; trailing empty frames too). Frames that start at a point get their offset from that point's thread in aug_emit.
__global__ __launch_bounds__(256) void aug_scan(int* __restrict__ block_counts, int m, const int* __restrict__ frame_off, int B,
                                                int n, int* __restrict__ new_off) {
  __shared__ int sh[4];
  int carry = 0;
  for (int base = 0; base < m; base += 256) {
    const int i = base + (int)threadIdx.x;
    const int v = i < m ? block_counts[i] : 0;
    int tot;
    const int ex = crb_block_excl_scan_256(v, sh, &tot);
    if (i < m) block_counts[i] = carry + ex;
    carry += tot;
  }
  for (int b = threadIdx.x; b <= B; b += 256)
    if (frame_off[b] >= n) new_off[b] = carry;
}

__global__ __launch_bounds__(256) void aug_emit(AugPoints a, int C, const int* __restrict__ block_base, float* __restrict__ out,
                                                int frame_col, int* __restrict__ new_off) {
  __shared__ int sh[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = crb_lane(), wave = (int)(threadIdx.x >> 6);
  bool keep = false;
  int b = 0;
  float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
  if (i < a.n) keep = aug_eval(a, i, b, x, y, z, w);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) sh[wave] = __popcll(m);
  __syncthreads();
  int rank = block_base[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += sh[w];
  if (i >= a.n) return;
  // the first point of frame b (and of the empty frames just before it, which start at the same point) carries their new offset
  for (int f = b; f >= 0 && a.frame_off[f] == i; --f) new_off[f] = rank;
  if (!keep) return;
  const float* q = a.pts + (int64_t)i * a.row_stride + a.xyz_col;
  float* o = out + (int64_t)rank * (C + frame_col);
  if (frame_col) *o++ = (float)b;
  o[0] = x; o[1] = y; o[2] = z;
  int k = 3;
  if (a.vec4) o[k++] = w;
  for (; k < C; ++k) o[k] = q[k];
}

// ------------------------------------------------------------------------------------------------------------------------------
// boxes
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int AUG_MAX_W = 10;

// at least min_corners of the 8 corners inside the range on all three axes (box_utils.mask_boxes_outside_range_numpy). Corner
// arithmetic of boxes_to_corners_3d: half extents (size * +-0.5), rotation about z by the heading, plus the centre; the rotation
// uses c = f32(cos(f64 heading)), s = f32(sin(f64 heading)) and separately rounded products, the definition the host mirror
// (augmentor_utils.box_corners_f32) shares.
__device__ __forceinline__ bool aug_box_inside(const float* v, const AugRange& r, int min_corners) {
  const float c = (float)cos((double)v[6]), s = (float)sin((double)v[6]);
  int inside = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // template order of box_utils.boxes_to_corners_3d: x + + - - + + - -, y + - - + + - - +, z - - - - + + + +
    const float sx = (k & 3) < 2 ? 0.5f : -0.5f;
    const float sy = ((k & 3) == 0 || (k & 3) == 3) ? 0.5f : -0.5f;
    const float sz = k < 4 ? -0.5f : 0.5f;
    const float lx = __fmul_rn(v[3], sx), ly = __fmul_rn(v[4], sy), lz = __fmul_rn(v[5], sz);
    const float cx = __fadd_rn(__fsub_rn(__fmul_rn(lx, c), __fmul_rn(ly, s)), v[0]);
    const float cy = __fadd_rn(__fadd_rn(__fmul_rn(lx, s), __fmul_rn(ly, c)), v[1]);
    const float cz = __fadd_rn(lz, v[2]);
    inside += (cx >= r.x0 && cx <= r.x1 && cy >= r.y0 && cy <= r.y1 && cz >= r.z0 && cz <= r.z1) ? 1 : 0;
  }
  return inside >= min_corners;
}

__global__ __launch_bounds__(256) void aug_boxes(const float* __restrict__ boxes, const int* __restrict__ counts, int G, int W,
                                                 const float* __restrict__ params, const float* __restrict__ angles, AugRange r,
                                                 int do_mask, int min_corners, float* __restrict__ out, int* __restrict__ new_counts) {
  __shared__ int sh[4];
  const int b = blockIdx.x;
  int cnt = counts[b];
  cnt = cnt < 0 ? 0 : (cnt > G ? G : cnt);
  const AugFrame f = aug_load(params, b);
  const float angle = angles ? angles[b] : 0.f;
  const bool vel = W - 1 > 7;
  const float* src = boxes + (int64_t)b * G * W;
  float* dst = out + (int64_t)b * G * W;
  int kept = 0;
  for (int base = 0; base < cnt; base += 256) {          // (cnt is uniform over the block: every thread takes every round)
    const int g = base + (int)threadIdx.x;
    float v[AUG_MAX_W];
    bool keep = false;
    if (g < cnt) {
#pragma unroll
      for (int k = 0; k < AUG_MAX_W; ++k) v[k] = k < W ? src[(int64_t)g * W + k] : 0.f;
      if (f.flip_x != 0.f) {
        v[1] = -v[1];
        v[6] = -v[6];
        if (vel) v[8] = -v[8];
      }
      if (f.flip_y != 0.f) {
        v[0] = -v[0];
        v[6] = -__fadd_rn(v[6], AUG_PI_F);
        if (vel) v[7] = -v[7];
      }
      if (aug_rotates(f)) {
        aug_rot(f, v[0], v[1]);
        v[6] = __fadd_rn(v[6], angle);
        if (vel) aug_rot(f, v[7], v[8]);
      }
      if (f.scale != 1.f) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = __fmul_rn(v[k], f.scale);
      }
      if (f.tx != 0.f) v[0] = __fadd_rn(v[0], f.tx);
      if (f.ty != 0.f) v[1] = __fadd_rn(v[1], f.ty);
      if (f.tz != 0.f) v[2] = __fadd_rn(v[2], f.tz);
      // limit_period(heading, 0.5, 2 pi)
      v[6] = __fsub_rn(v[6], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(v[6], AUG_TWO_PI_F), 0.5f)), AUG_TWO_PI_F));
      keep = !do_mask || aug_box_inside(v, r, min_corners);
    }
    int tot;
    const int ex = crb_block_excl_scan_256(keep ? 1 : 0, sh, &tot);
    if (keep) {
      float* o = dst + (int64_t)(kept + ex) * W;
#pragma unroll
      for (int k = 0; k < AUG_MAX_W; ++k)
        if (k < W) o[k] = v[k];
    }
    kept += tot;
  }
  // everything behind the kept rows: removed boxes and the frame's padding
  for (int64_t t = (int64_t)kept * W + threadIdx.x; t < (int64_t)G * W; t += 256) dst[t] = 0.f;
  if (threadIdx.x == 0) new_counts[b] = kept;
}

}  // namespace

extern "C" int64_t crb_augment_mask_points_workspace_bytes(int64_t n_points, int B) {
  (void)B;
  if (n_points < 0) n_points = 0;
  return crb_align_up((int64_t)(crb_cdiv(n_points, 256) + 1) * 4, 256) + 256;
}

extern "C" int crb_augment_mask_points(const float* points, int64_t n_points, int64_t row_stride, int xyz_col, int num_features,
                                       const int32_t* frame_offsets, int B, const float* params, const float* range6,
                                       int do_mask, float* out_points, int out_frame_col, int32_t* new_frame_offsets,
                                       void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_points < 0 || n_points >= (int64_t)0x7fffff00 || B <= 0 || num_features < 3 || xyz_col < 0 ||
      row_stride < (int64_t)xyz_col + num_features || !frame_offsets || !params || !new_frame_offsets || (do_mask && !range6))
    return CRB_ERR_ARG;
  if (n_points > 0 && (!points || !out_points)) return CRB_ERR_ARG;
  if (((uintptr_t)params & 15) != 0) return CRB_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)n_points;
  if (n == 0) {
    CRB_HIP(hipMemsetAsync(new_frame_offsets, 0, sizeof(int32_t) * (B + 1), st));
    return CRB_OK;
  }
  const int blocks = crb_cdiv(n, 256);
  CrbArena arena(workspace, (size_t)workspace_bytes);
  int* block_counts = arena.take<int>(blocks + 1);
  if (!arena.ok) return CRB_ERR_WORKSPACE;
  AugPoints a;
  a.pts = points; a.row_stride = row_stride; a.xyz_col = xyz_col; a.n = n; a.B = B;
  a.frame_off = frame_offsets; a.params = params; a.do_mask = do_mask ? 1 : 0;
  a.vec4 = (xyz_col == 0 && num_features >= 4 && (row_stride & 3) == 0 && ((uintptr_t)points & 15) == 0) ? 1 : 0;
  a.r = AugRange{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (range6) a.r = AugRange{range6[0], range6[1], range6[2], range6[3], range6[4], range6[5]};
  hipLaunchKernelGGL(aug_count, dim3(blocks), dim3(256), 0, st, a, block_counts);
  hipLaunchKernelGGL(aug_scan, dim3(1), dim3(256), 0, st, block_counts, blocks, frame_offsets, B, n, new_frame_offsets);
  hipLaunchKernelGGL(aug_emit, dim3(blocks), dim3(256), 0, st, a, num_features, (const int*)block_counts, out_points,
                     out_frame_col ? 1 : 0, new_frame_offsets);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_augment_boxes(const float* gt_boxes, const int32_t* counts, int B, int G, int W, const float* params,
                                 const float* rot_angles, const float* range6, int do_mask, int min_num_corners,
                                 float* out_boxes, int32_t* new_counts, void* stream) {
  if (B <= 0 || G < 0 || (W != 8 && W != 10) || !counts || !params || !new_counts || (do_mask && !range6)) return CRB_ERR_ARG;
  if (G > 0 && (!gt_boxes || !out_boxes || gt_boxes == out_boxes)) return CRB_ERR_ARG;
  if (((uintptr_t)params & 15) != 0) return CRB_ERR_ARG;
  AugRange r{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (range6) r = AugRange{range6[0], range6[1], range6[2], range6[3], range6[4], range6[5]};
  hipLaunchKernelGGL(aug_boxes, dim3(B), dim3(256), 0, (hipStream_t)stream, gt_boxes, counts, G, W, params, rot_angles, r,
                     do_mask ? 1 : 0, min_num_corners, out_boxes, new_counts);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
