// Rotated-rectangle BEV overlap and IoU: the device functions shared by csrc/iou3d_nms.hip (crb_boxes_pairwise, NMS) and
// csrc/gt_sampling.hip (collision test of gt_sampling). One definition, so that both callers decide with the same bits.
//
// Parity contract (see csrc/iou3d_nms.hip): the reference's geometric definition step for step (iou3d_nms_kernel.cu:104-225) in
// the same f32 operation order; the translation unit must be compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr float kEps = 1e-8f;

struct P2 { float x, y; };

__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) {
  return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ bool bbox_cross(P2 p1, P2 p2, P2 q1, P2 q2) {
  return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
         fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}

// segment (p0,p1) x segment (q0,q1); returns true and the crossing point when they properly cross
__device__ __forceinline__ bool seg_cross(P2 p1, P2 p0, P2 q1, P2 q0, P2& out) {
  if (!bbox_cross(p0, p1, q0, q1)) return false;
  float s1 = cross3(q0, p1, p0);
  float s2 = cross3(p1, q1, p0);
  float s3 = cross3(p0, q1, q0);
  float s4 = cross3(q1, p1, q0);
  if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
  float s5 = cross3(q1, p1, p0);
  if (fabsf(s5 - s1) > kEps) {
    out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
    out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
  } else {
    float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
    float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
    float D = a0 * b1 - a1 * b0;
    out.x = (b0 * c1 - b1 * c0) / D;
    out.y = (a1 * c0 - a0 * c1) / D;
  }
  return true;
}

__device__ __forceinline__ bool in_box_margin(const float* b, P2 p, float margin) {
  float ac = cosf(-b[6]), as = sinf(-b[6]);
  float rx = (p.x - b[0]) * ac + (p.y - b[1]) * (-as);
  float ry = (p.x - b[0]) * as + (p.y - b[1]) * ac;
  return fabsf(rx) < b[3] / 2 + margin && fabsf(ry) < b[4] / 2 + margin;
}

__device__ __forceinline__ void box_corners(const float* b, P2* c /*5*/) {
  float hx = b[3] / 2, hy = b[4] / 2;
  float x1 = b[0] - hx, y1 = b[1] - hy, x2 = b[0] + hx, y2 = b[1] + hy;
  float ca = cosf(b[6]), sa = sinf(b[6]);
  const float px[4] = {x1, x2, x2, x1};
  const float py[4] = {y1, y1, y2, y2};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float nx = (px[k] - b[0]) * ca + (py[k] - b[1]) * (-sa) + b[0];
    float ny = (px[k] - b[0]) * sa + (py[k] - b[1]) * ca + b[1];
    c[k].x = nx; c[k].y = ny;
  }
  c[4] = c[0];
}

// rotated-rectangle intersection area (reference: box_overlap, iou3d_nms_kernel.cu:104-225). margin: how far outside a box a corner of
// the other one still counts as inside. The reference's NMS uses 1e-2 (a centimetre); csrc/kitti_eval.hip, whose bar is an f64
// overlap, passes boxes translated to their own neighbourhood and a margin just above their f32 rounding.
__device__ float rect_overlap(const float* a, const float* b, const float margin = 1e-2f) {
  P2 ca[5], cb[5];
  box_corners(a, ca);
  box_corners(b, cb);
  P2 pts[16];
  float sx = 0.f, sy = 0.f;
  int cnt = 0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      P2 q;
      if (seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], q)) {
        sx = sx + q.x; sy = sy + q.y;
        pts[cnt++] = q;
      }
    }
  for (int k = 0; k < 4; ++k) {
    if (in_box_margin(a, cb[k], margin)) { sx = sx + cb[k].x; sy = sy + cb[k].y; pts[cnt++] = cb[k]; }
    if (in_box_margin(b, ca[k], margin)) { sx = sx + ca[k].x; sy = sy + ca[k].y; pts[cnt++] = ca[k]; }
  }
  float cx = sx / cnt, cy = sy / cnt;    // cnt == 0 -> NaN centre, loops below do nothing, area 0 (as the reference)
  // bubble sort by polar angle about the centroid (same comparison sequence as the reference => same permutation)
  float ang[16];
  for (int k = 0; k < cnt; ++k) ang[k] = atan2f(pts[k].y - cy, pts[k].x - cx);
  for (int j = 0; j < cnt - 1; ++j)
    for (int i = 0; i < cnt - j - 1; ++i)
      if (ang[i] > ang[i + 1]) {
        P2 t = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = t;
        float ta = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = ta;
      }
  float area = 0.f;
  for (int k = 0; k < cnt - 1; ++k) {
    float ax = pts[k].x - pts[0].x, ay = pts[k].y - pts[0].y;
    float bx = pts[k + 1].x - pts[0].x, by = pts[k + 1].y - pts[0].y;
    area += ax * by - ay * bx;
  }
  return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev_rot(const float* a, const float* b) {
  float sa = a[3] * a[4], sb = b[3] * b[4];
  float so = rect_overlap(a, b);
  return so / fmaxf(sa + sb - so, kEps);
}

}  // namespace
