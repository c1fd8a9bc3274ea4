// The point-in-box test shared by csrc/roiaware_pool3d.hip and csrc/part_head.hip: one definition, so every route that asks
// "which ground truth owns this point" answers alike, faces included.
//
// |z-cz| <= dz/2 and the rotated |lx| < dx/2 + 1e-5, |ly| < dy/2 + 1e-5, evaluated like the reference's device function (f32 sin/cos
// of -heading, the half-extent comparisons promoted to double by its `/ 2.0` literals, roiaware_pool3d_kernel.cu:23-36).
#pragma once
#include <hip/hip_runtime.h>

namespace {

struct BoxLds { float cx, cy, cz, dx, dy, dz, ca, sa; };

__device__ __forceinline__ bool pt_in_box(float x, float y, float z, const BoxLds& b, float& lx, float& ly) {
  if ((double)fabsf(z - b.cz) > (double)b.dz / 2.0) return false;
  const float sx = x - b.cx, sy = y - b.cy;
  lx = sx * b.ca + sy * (-b.sa);
  ly = sx * b.sa + sy * b.ca;
  const double margin = (double)1e-5f;
  return ((double)fabsf(lx) < (double)b.dx / 2.0 + margin) && ((double)fabsf(ly) < (double)b.dy / 2.0 + margin);
}

__device__ __forceinline__ BoxLds load_box(const float* p) {
  BoxLds b;
  b.cx = p[0]; b.cy = p[1]; b.cz = p[2]; b.dx = p[3]; b.dy = p[4]; b.dz = p[5];
  b.ca = cosf(-p[6]); b.sa = sinf(-p[6]);
  return b;
}

}  // namespace
