// What csrc/part_head.hip and csrc/point_box.hip share: the search for the ground truth that owns a voxel centre (so both target
// launches give the same labels, owners and part labels bit for bit), the workgroup sum in a fixed order and the tile constants of
// the loss launches.
#pragma once
#include <hip/hip_runtime.h>
#include "pt_in_box.h"

namespace {

constexpr int PT_CHUNK = 64;     // ground truths staged per pass
constexpr int LOSS_TPB = 256;
constexpr int LOSS_ROWS = 4;     // rows per thread
constexpr int LOSS_TILE = LOSS_TPB * LOSS_ROWS;

// a ground truth and its enlarged twin (box_utils.enlarge_box3d: dims + extra width, centre and heading unchanged -> the same sin / cos)
struct PartBoxLds { BoxLds box; float ex, ey, ez; };

// The first ground truth of frame rows fb (G,8), in index order, that contains (x, y, z), or -1; shell: some enlarged ground truth
// does. Every thread of the 256-wide workgroup calls it (it stages the boxes through sb and synchronises); inactive threads search nothing.
__device__ __forceinline__ int part_find_owner(PartBoxLds* sb, const float* __restrict__ fb, int G, float ew0, float ew1, float ew2,
                                               bool active, float x, float y, float z, bool& shell) {
  int found = -1;
  shell = false;
  for (int t0 = 0; t0 < G; t0 += PT_CHUNK) {
    __syncthreads();
    const int tc = min(PT_CHUNK, G - t0);
    if ((int)threadIdx.x < tc) {
      const float* r = fb + (int64_t)(t0 + threadIdx.x) * 8;
      PartBoxLds v;
      v.box = load_box(r);
      v.ex = r[3] + ew0; v.ey = r[4] + ew1; v.ez = r[5] + ew2;
      sb[threadIdx.x] = v;
    }
    __syncthreads();
    if (active && found < 0) {
      float lx, ly;
      for (int k = 0; k < tc; ++k) {
        if (pt_in_box(x, y, z, sb[k].box, lx, ly)) { found = t0 + k; break; }
        if (!shell) {
          BoxLds e = sb[k].box;
          e.dx = sb[k].ex; e.dy = sb[k].ey; e.dz = sb[k].ez;
          shell = pt_in_box(x, y, z, e, lx, ly);
        }
      }
    }
  }
  return found;
}

// fg ^ (enlarged hit), then the foreground class on top: an owned point keeps its class whatever the enlarged query says
__device__ __forceinline__ int64_t part_label(const float* __restrict__ fb, int found, bool shell, int num_class) {
  if (found < 0) return shell ? -1 : 0;
  return num_class == 1 ? 1 : (int64_t)fb[(int64_t)found * 8 + 7];
}

// rotate_z(p - c, -rz) / dims + 0.5 of ground truth r (8) in f64 from the f32 inputs, rounded once
__device__ __forceinline__ void part_offsets(const float* __restrict__ r, float x, float y, float z, float* pl) {
  const double sx = (double)x - (double)r[0], sy = (double)y - (double)r[1], sz = (double)z - (double)r[2];
  const double ca = cos((double)r[6]), sa = sin((double)r[6]);
  pl[0] = (float)((sx * ca + sy * sa) / (double)r[3] + 0.5);
  pl[1] = (float)((sy * ca - sx * sa) / (double)r[4] + 0.5);
  pl[2] = (float)(sz / (double)r[5] + 0.5);
}

// sum over the workgroup in a fixed order: xor butterflies inside each wave, then the four wave sums left to right
template <typename T>
__device__ __forceinline__ T loss_block_sum(T v, T* sh) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  T t = 0;
#pragma unroll
  for (int w = 0; w < LOSS_TPB / 64; ++w) t += sh[w];
  return t;
}

// stable binary cross entropy of sigmoid(x) against t
__device__ __forceinline__ float part_bce(float x, float t) { return fmaxf(x, 0.0f) - x * t + log1pf(expf(-fabsf(x))); }

}  // namespace
