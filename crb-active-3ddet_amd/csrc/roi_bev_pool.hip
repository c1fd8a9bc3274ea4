// Rotated G x G grid pooling of the BEV feature map under every first-stage proposal, all frames in ONE launch
// (reference: SECONDHead.roi_grid_pool, pcdet/models/roi_heads/second_head.py:53-110: per frame an affine_grid + grid_sample over a
// (R, C, H, W) expand of the NCHW map, with torch's defaults align_corners=False / bilinear / zeros although theta is written in the
// W - 1 convention - the quirk is what the reference executes and is kept).
//
// The map stays NHWC (the 16 x 200 x 176 x 512 map of a bs=16 step is 1.15 GB: it is never transposed). One workgroup per RoI:
//   phase 1: thread g < G*G forms the sampling position of grid point g in f64 (theta, the affine map, the un-normalisation: a few
//            dozen operations per grid point, once per RoI and not once per channel quad), its four corner rows as float offsets
//            into the frame's map (-1 = the corner lies outside the map: zero padding, the corner contributes NOTHING, it is not
//            clamped) and the four bilinear weights from the UNCLAMPED coordinates, into LDS;
//   phase 2: the threads walk (grid point, channel quad): four 16-byte gathers along C, one 16-byte store. Output rows are
//            (RoI, grid point, channel): the host hands them back as a permuted (B*R, C, G, G) view.
// The products are added in grid_sample's order (north-west, north-east, south-west, south-east), no atomics: the output is
// bit-identical from call to call. Nothing here has a backward: the reference detaches the map and the RoIs before it pools.
#include "crb_common.h"
#include "../../include/crb_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int RBP_TPB = 256;
constexpr int RBP_MAX_G = 16;                       // G * G grid points of a RoI = one per thread of phase 1
constexpr int RBP_MAX_G2 = RBP_MAX_G * RBP_MAX_G;

struct RoiBevPoolArgs {
  const float* bev;      // (B, H, W, C)
  const float* rois;     // (B * R, roi_c)
  float* out;            // (B * R, G * G, C)
  int R, H, W, C, G, roi_c;
  double x_min, y_min, cell_x, cell_y;
};

__global__ __launch_bounds__(RBP_TPB) void roi_bev_pool_kernel(RoiBevPoolArgs a) {
  __shared__ int s_off[4][RBP_MAX_G2];              // nw, ne, sw, se
  __shared__ float s_w[4][RBP_MAX_G2];
  const int64_t n = blockIdx.x;
  const int G = a.G, G2 = G * G, H = a.H, W = a.W, C = a.C;
  if ((int)threadIdx.x < G2) {
    const int g = threadIdx.x, j = g / G, i = g - j * G;             // j = row (v, y), i = column (u, x)
    const float* r = a.rois + n * a.roi_c;
    const double x = r[0], y = r[1], dx = r[3], dy = r[4], rz = r[6];
    const double x1 = (x - dx / 2 - a.x_min) / a.cell_x, x2 = (x + dx / 2 - a.x_min) / a.cell_x;
    const double y1 = (y - dy / 2 - a.y_min) / a.cell_y, y2 = (y + dy / 2 - a.y_min) / a.cell_y;
    const double c = cos(rz), s = sin(rz);
    const double W1 = (double)(W - 1), H1 = (double)(H - 1);
    const double t00 = (x2 - x1) / W1 * c, t01 = (x2 - x1) / W1 * (-s), t02 = (x1 + x2 - W + 1) / W1;
    const double t10 = (y2 - y1) / H1 * s, t11 = (y2 - y1) / H1 * c, t12 = (y1 + y2 - H + 1) / H1;
    const double u = (double)(2 * i + 1) / G - 1, v = (double)(2 * j + 1) / G - 1;
    const double gx = t00 * u + t01 * v + t02, gy = t10 * u + t11 * v + t12;
    const double ix = ((gx + 1) * W - 1) / 2, iy = ((gy + 1) * H - 1) / 2;
    const double fx = floor(ix), fy = floor(iy);
    // (comparisons in f64 before any conversion: a NaN / infinite coordinate is outside the map)
    const bool xw = fx >= 0 && fx <= W - 1, xe = fx + 1 >= 0 && fx + 1 <= W - 1;
    const bool yn = fy >= 0 && fy <= H - 1, ys = fy + 1 >= 0 && fy + 1 <= H - 1;
    const int x0 = (xw || xe) ? (int)fx : 0, y0 = (yn || ys) ? (int)fy : 0;       // in [-1, W - 1] / [-1, H - 1] where it is read
    const double ax = ix - fx, ay = iy - fy;                         // distance to the west / north corner, in [0, 1)
    s_off[0][g] = (xw && yn) ? (y0 * W + x0) * C : -1;
    s_off[1][g] = (xe && yn) ? (y0 * W + x0 + 1) * C : -1;
    s_off[2][g] = (xw && ys) ? ((y0 + 1) * W + x0) * C : -1;
    s_off[3][g] = (xe && ys) ? ((y0 + 1) * W + x0 + 1) * C : -1;
    s_w[0][g] = (float)((1 - ax) * (1 - ay));
    s_w[1][g] = (float)(ax * (1 - ay));
    s_w[2][g] = (float)((1 - ax) * ay);
    s_w[3][g] = (float)(ax * ay);
  }
  __syncthreads();
  const int q = C >> 2;
  const float* map = a.bev + (n / a.R) * ((int64_t)H * W * C);
  float* dst = a.out + n * ((int64_t)G2 * C);
  for (int t = threadIdx.x; t < G2 * q; t += RBP_TPB) {
    const int g = t / q, c4 = (t - g * q) * 4;
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int o = s_off[k][g];
      if (o >= 0) acc = acc + *reinterpret_cast<const f32x4*>(map + o + c4) * s_w[k][g];
    }
    *reinterpret_cast<f32x4*>(dst + g * C + c4) = acc;
  }
}

}  // namespace

extern "C" int crb_roi_bev_pool(const float* bev, int B, int H, int W, int C, const float* rois, int roi_row_stride, int R, int grid_size,
                                double x_min, double y_min, double cell_x, double cell_y, float* out, void* stream) {
  if (B <= 0 || R <= 0 || H < 2 || W < 2 || C <= 0 || (C & 3) || grid_size < 1 || roi_row_stride < 7 || !(cell_x > 0.0) ||
      !(cell_y > 0.0) || !(x_min == x_min) || !(y_min == y_min))
    return CRB_ERR_ARG;
  if (grid_size > RBP_MAX_G) return CRB_ERR_UNSUPPORTED;
  if ((int64_t)H * W * C >= (1LL << 31) || (int64_t)B * R >= (1LL << 31)) return CRB_ERR_ARG;
  if (!bev || !rois || !out || ((uintptr_t)bev & 15) || ((uintptr_t)out & 15)) return CRB_ERR_ARG;
  RoiBevPoolArgs a;
  a.bev = bev; a.rois = rois; a.out = out;
  a.R = R; a.H = H; a.W = W; a.C = C; a.G = grid_size; a.roi_c = roi_row_stride;
  a.x_min = x_min; a.y_min = y_min; a.cell_x = cell_x; a.cell_y = cell_y;
  hipLaunchKernelGGL(roi_bev_pool_kernel, dim3((unsigned)((int64_t)B * R)), dim3(RBP_TPB), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
