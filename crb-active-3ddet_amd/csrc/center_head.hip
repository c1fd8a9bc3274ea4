// The anchor-free centre head of CenterPoint: target assignment, losses and box decoding as a handful of launches.
//
// replaces, for one batch:
//   CenterHead.assign_targets / assign_target_of_single_head   (pcdet/models/dense_heads/center_head.py:103-219)
//   centernet_utils.gaussian_radius / gaussian2D / draw_gaussian_to_heatmap   (pcdet/models/model_utils/centernet_utils.py:9-69)
//   CenterHead.get_loss (:225-251), neg_loss_cornernet / _reg_loss / _transpose_and_gather_feat   (pcdet/utils/loss_utils.py:264-386)
//   centernet_utils.decode_bbox_from_heatmap behind its top-K   (centernet_utils.py:154-216)
// The reference assigns targets in three nested Python loops on the host (a .cpu() per frame, an .item() and a numpy window per
// box, an upload per frame), takes the loss in ~25 launches per head with an .item() per term, and decodes through seven
// permute().contiguous() + gather passes over whole maps.
//
// Maps are addressed as b * C*H*W + c * stride_c + cell * stride_p, so NCHW and channels_last memory are read where the
// convolutions left them. A workgroup of the loss kernels owns 256 consecutive cells of one frame; a thread owns one cell.
// Every sum is taken in f64 in a fixed order (thread: channels in order; workgroup: LDS tree; launch: partials in index order),
// the heatmap maximum is an integer maximum: all results are bit-reproducible.
// f64 on purpose: the terms of the focal loss (exp, two logs per logit) and the few transcendental target / box entries are
// formed in f64 and rounded once, so the results sit at the f64 definition instead of a few f32 ulp away from it. The maps are
// small (C * H * W = 105,600 logits per KITTI frame).
#include "crb_common.h"
#include "../../include/crb_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_CLS = 16, MAX_HEADS = 8, MAX_EXTRA = 8, MAX_SLOTS = 4096;

struct AssignArgs {
  const float* gt;          // (B, M, box_dim)
  int B, M, box_dim, E, num_class, num_heads, H, W, nmax;
  int class_head[MAX_CLS], class_local[MAX_CLS];
  int64_t heat_off[MAX_HEADS];      // offset of the head's (B, C_h, H, W) block in `heat`
  int head_channels[MAX_HEADS];
  float rx, ry, vx, vy, stride;
  double overlap;           // the Python scalar: constants derived from it are formed in f64 and rounded to f32 once, as torch does
  int min_radius;
  float* heat;
  float* tb;                // (num_heads, B, nmax, 8 + E)
  int64_t* inds;            // (num_heads, B, nmax)
  int64_t* masks;
  int4* obj;                // (num_heads, B, nmax) {x, y, radius (-1: nothing to draw), class in head}
};

// block-wide exclusive scan of one int per thread through LDS (no cross-lane instruction: the same code runs in the host check)
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < TPB; d <<= 1) {
    const int add = t >= d ? sh[t - d] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int inc = sh[t];
  *total = sh[TPB - 1];
  __syncthreads();
  return inc - v;
}

// centernet_utils.gaussian_radius (:9-35) with height = dx, width = dy, operation by operation in f32 (scalars rounded to f32 as
// torch rounds a Python scalar that meets an f32 tensor); sqrtf is correctly rounded (hipcc's default for f32 sqrt and division)
__device__ __forceinline__ float gaussian_radius(float h, float w, double mo) {
  const float s1 = (float)(1.0 - mo), s2 = (float)(1.0 + mo);
  const float b1 = h + w;
  const float c1 = w * h * s1 / s2;
  const float r1 = (b1 + sqrtf(b1 * b1 - 4.0f * c1)) / 2.0f;
  const float b2 = 2.0f * (h + w);
  const float c2 = s1 * w * h;
  const float r2 = (b2 + sqrtf(b2 * b2 - 16.0f * c2)) / 2.0f;
  const float a3x4 = (float)(4.0 * (4.0 * mo));
  const float b3 = (float)(-2.0 * mo) * (h + w);
  const float c3 = (float)(mo - 1.0) * w * h;
  const float r3 = (b3 + sqrtf(b3 * b3 - a3x4 * c3)) / 2.0f;
  return fminf(fminf(r1, r2), r3);
}

// one workgroup per frame: slot = rank of the box among the frame's boxes of its head (input order), target row, cell, mask and
// the descriptor the drawing kernel reads
__global__ __launch_bounds__(TPB) void center_slots_kernel(AssignArgs a) {
  __shared__ int sh[TPB];
  const int b = blockIdx.x;
  const int D = 8 + a.E;
  for (int h = 0; h < a.num_heads; ++h) {
    int carry = 0;
    for (int base = 0; base < a.M && carry < a.nmax; base += TPB) {
      const int i = base + (int)threadIdx.x;
      const float* box = a.gt + ((int64_t)b * a.M + (i < a.M ? i : 0)) * a.box_dim;
      int cls = 0;
      if (i < a.M) {
        const float c = box[a.box_dim - 1];
        if (c >= 1.0f && c <= (float)a.num_class) cls = (int)c;
      }
      const int mine = (cls > 0 && a.class_head[cls - 1] == h) ? 1 : 0;
      int total;
      const int slot = carry + block_excl_scan(mine, sh, &total);
      carry += total;
      if (!mine || slot >= a.nmax) continue;
      const float dx = box[3], dy = box[4];
      if (!(dx > 0.0f) || !(dy > 0.0f)) continue;                      // (:137) the slot stays zero
      // (:121-127) two f32 divisions, clamp to [0, size - 0.5], truncate
      float cx = (box[0] - a.rx) / a.vx / a.stride, cy = (box[1] - a.ry) / a.vy / a.stride;
      cx = fminf(fmaxf(cx, 0.0f), (float)a.W - 0.5f);
      cy = fminf(fmaxf(cy, 0.0f), (float)a.H - 0.5f);
      if (!(cx >= 0.0f) || !(cy >= 0.0f)) continue;                    // NaN centre: no object
      const int xi = (int)cx, yi = (int)cy;
      const float rad = gaussian_radius(dx / a.vx / a.stride, dy / a.vy / a.stride, a.overlap);
      const int r = max((int)rad, a.min_radius);
      const int64_t s = ((int64_t)h * a.B + b) * a.nmax + slot;
      a.inds[s] = (int64_t)yi * a.W + xi;
      a.masks[s] = 1;
      float* t = a.tb + s * D;
      t[0] = cx - (float)xi;
      t[1] = cy - (float)yi;
      t[2] = box[2];
      t[3] = (float)log((double)box[3]);
      t[4] = (float)log((double)box[4]);
      t[5] = (float)log((double)box[5]);
      t[6] = (float)cos((double)box[6]);
      t[7] = (float)sin((double)box[6]);
      for (int e = 0; e < a.E; ++e) t[8 + e] = box[7 + e];
      a.obj[s] = make_int4(xi, yi, r, a.class_local[cls - 1]);
    }
  }
}

// one workgroup per slot: the window of draw_gaussian_to_heatmap (:47-69), clipped as there, exp(-(i^2 + j^2) / (2 sigma^2)) with
// sigma = (2 r + 1) / 6 in f64 as numpy forms it, rounded to f32 once. The reference zeroes entries below eps * max of the window
// (gaussian2D :43): with sigma = diameter / 6 the smallest entry is exp(-9 r^2 / (2r+1)^2 * 2) > exp(-4.5) at every radius, far above
// 2.2e-16, so the cut never triggers and is not implemented. Values are >= 0, so the integer order of their bit patterns is
// their order: atomicMax on int is the order-independent maximum.
__global__ __launch_bounds__(TPB) void center_draw_kernel(AssignArgs a) {
  const int slot = blockIdx.x, b = blockIdx.y, h = blockIdx.z;
  const int4 o = a.obj[((int64_t)h * a.B + b) * a.nmax + slot];
  const int r = o.z;
  if (r < 0) return;
  const int x = o.x, y = o.y;
  const int left = min(x, r), right = min(a.W - x, r + 1), top = min(y, r), bottom = min(a.H - y, r + 1);
  const int ww = left + right, wh = top + bottom;
  if (ww <= 0 || wh <= 0) return;
  const double sigma = (double)(2 * r + 1) / 6.0;
  const double den = 2.0 * sigma * sigma;
  float* map = a.heat + a.heat_off[h] + ((int64_t)b * a.head_channels[h] + o.w) * a.H * a.W;
  for (int k = threadIdx.x; k < ww * wh; k += TPB) {
    const int j = k / ww - top, i = k % ww - left;                     // offsets from the centre cell
    const float v = (float)exp(-(double)(i * i + j * j) / den);
    atomicMax(reinterpret_cast<int*>(map + (int64_t)(y + j) * a.W + (x + i)), __float_as_int(v));
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
struct LossArgs {
  const float* hm;          // logits
  int64_t hm_sc, hm_sp;
  const float* heat;        // (B, C, H, W) NCHW
  int B, C, H, W, nmax, D;  // D = number of regression columns
  CrbCenterMaps reg;
  int col_map[CRB_CENTER_MAX_CODE], col_ch[CRB_CENTER_MAX_CODE];
  const float* tb;          // (B, nmax, D)
  const int64_t* inds;
  const int64_t* masks;
  float cw[CRB_CENTER_MAX_CODE];
  float w_cls, w_loc;
};

__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = TPB / 2; d > 0; d >>= 1) {
    if (t < d) sh[t] += sh[t + d];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// CenterHead.sigmoid (:221-223): clamp(sigmoid(x), 1e-4, 1 - 1e-4); inside = the clamp passes the gradient
__device__ __forceinline__ double clamped_sigmoid(float x, bool& inside) {
  const double p = 1.0 / (1.0 + exp(-(double)x));
  inside = p >= 1e-4 && p <= 1.0 - 1e-4;
  return p < 1e-4 ? 1e-4 : (p > 1.0 - 1e-4 ? 1.0 - 1e-4 : p);
}

// partial (nblk, 3) f64 = {pos_loss, neg_loss, num_pos} of the workgroup's cells     (neg_loss_cornernet, loss_utils.py:264-299)
__global__ __launch_bounds__(TPB) void center_loss_partial_kernel(LossArgs a, double* __restrict__ partial) {
  __shared__ double sh[TPB];
  const int b = blockIdx.y, HW = a.H * a.W;
  const int cell = blockIdx.x * TPB + (int)threadIdx.x;
  double pos = 0.0, neg = 0.0, np = 0.0;
  if (cell < HW) {
    const float* x = a.hm + (int64_t)b * a.C * HW + (int64_t)cell * a.hm_sp;
    const float* g = a.heat + (int64_t)b * a.C * HW + cell;
    for (int c = 0; c < a.C; ++c) {
      bool inside;
      const double p = clamped_sigmoid(x[c * a.hm_sc], inside);
      const double gt = (double)g[(int64_t)c * HW];
      if (gt == 1.0) {
        pos += log(p) * ((1.0 - p) * (1.0 - p));
        np += 1.0;
      } else if (gt < 1.0) {
        const double w = (1.0 - gt) * (1.0 - gt);
        neg += log(1.0 - p) * (p * p) * (w * w);
      }
    }
  }
  pos = block_sum(pos, sh);
  neg = block_sum(neg, sh);
  np = block_sum(np, sh);
  if (threadIdx.x == 0) {
    double* o = partial + ((int64_t)b * gridDim.x + blockIdx.x) * 3;
    o[0] = pos;
    o[1] = neg;
    o[2] = np;
  }
}

// one workgroup: the partials in index order -> hm loss; RegLossCenterNet (loss_utils.py:314-386) over the B * nmax slots -> loc loss
__global__ __launch_bounds__(TPB) void center_loss_finalize_kernel(LossArgs a, const double* __restrict__ partial, int nblk,
                                                                  double* __restrict__ loss, double* __restrict__ stats) {
  __shared__ double sh[TPB];
  double v[3] = {0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < nblk; k += TPB)
    for (int j = 0; j < 3; ++j) v[j] += partial[(int64_t)k * 3 + j];
  for (int j = 0; j < 3; ++j) v[j] = block_sum(v[j], sh);
  const int HW = a.H * a.W;
  double col[CRB_CENTER_MAX_CODE], num = 0.0;
  for (int d = 0; d < CRB_CENTER_MAX_CODE; ++d) col[d] = 0.0;
  for (int s = threadIdx.x; s < a.B * a.nmax; s += TPB) {
    if (a.masks[s] == 0) continue;
    num += 1.0;
    const int b = s / a.nmax;
    const int64_t cell = a.inds[s];
    if (cell < 0 || cell >= HW) continue;
    for (int d = 0; d < a.D; ++d) {
      const int m = a.col_map[d];
      const float t = a.tb[(int64_t)s * a.D + d];
      if (t != t) continue;                                            // NaN target: no term (:326)
      const float p = a.reg.ptr[m][(int64_t)b * a.reg.channels[m] * HW + (int64_t)a.col_ch[d] * a.reg.stride_c[m] + cell * a.reg.stride_p[m]];
      col[d] += fabs((double)p - (double)t);
    }
  }
  num = block_sum(num, sh);
  double loc = 0.0;
  for (int d = 0; d < a.D; ++d) {
    const double c = block_sum(col[d], sh);
    loc += c / fmax(num, 1.0) * (double)a.cw[d];
  }
  if (threadIdx.x == 0) {
    const double hm = v[2] == 0.0 ? -v[1] : -(v[0] + v[1]) / v[2];
    loss[0] = hm * (double)a.w_cls;
    loss[1] = loc * (double)a.w_loc;
    stats[0] = v[2];
    stats[1] = num;
  }
}

// gradients of gout[0] * loss[0] + gout[1] * loss[1]: the hm logits of the workgroup's cells, and the regression maps - zero but for
// the cells named by inds, where the slots of the frame that fall into this workgroup's cells are listed in LDS and every thread
// counts the signs of its own cell's slots in integers: two objects in one cell add without any float atomic, in no order at all.
__global__ __launch_bounds__(TPB) void center_loss_backward_kernel(LossArgs a, const double* __restrict__ stats,
                                                                  const float* __restrict__ gout, float* __restrict__ d_hm) {
  __shared__ int s_list[MAX_SLOTS];
  __shared__ int s_n;
  const int b = blockIdx.y, HW = a.H * a.W;
  const int c0 = blockIdx.x * TPB, cell = c0 + (int)threadIdx.x;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < a.nmax; k += TPB) {
    const int64_t s = (int64_t)b * a.nmax + k;
    if (a.masks[s] == 0) continue;
    const int64_t ci = a.inds[s];
    if (ci >= c0 && ci < c0 + TPB && ci < HW) s_list[atomicAdd(&s_n, 1)] = k;
  }
  __syncthreads();
  if (cell >= HW) return;
  const double npos = stats[0], num = fmax(stats[1], 1.0);
  const double g_hm = (double)gout[0] * (double)a.w_cls, g_loc = (double)gout[1] * (double)a.w_loc / num;
  {
    const float* x = a.hm + (int64_t)b * a.C * HW + (int64_t)cell * a.hm_sp;
    float* dx = d_hm + (int64_t)b * a.C * HW + (int64_t)cell * a.hm_sp;
    const float* g = a.heat + (int64_t)b * a.C * HW + cell;
    for (int c = 0; c < a.C; ++c) {
      bool inside;
      const double p = clamped_sigmoid(x[c * a.hm_sc], inside);
      const double gt = (double)g[(int64_t)c * HW];
      double dl = 0.0;                                                 // d (pos_loss + neg_loss) / d p
      if (inside) {
        if (gt == 1.0) {
          if (npos != 0.0) dl = (1.0 - p) * (1.0 - p) / p - 2.0 * (1.0 - p) * log(p);
        } else if (gt < 1.0) {
          const double w = (1.0 - gt) * (1.0 - gt);
          dl = (w * w) * (2.0 * p * log(1.0 - p) - p * p / (1.0 - p));
        }
      }
      const double scale = npos == 0.0 ? -1.0 : -1.0 / npos;
      dx[c * a.hm_sc] = (float)(g_hm * scale * dl * (p * (1.0 - p)));
    }
  }
  int cnt[CRB_CENTER_MAX_CODE];
  for (int d = 0; d < CRB_CENTER_MAX_CODE; ++d) cnt[d] = 0;
  const int n = s_n;
  for (int q = 0; q < n; ++q) {
    const int k = s_list[q];
    const int64_t s = (int64_t)b * a.nmax + k;
    if (a.inds[s] != cell) continue;
    for (int d = 0; d < a.D; ++d) {
      const int m = a.col_map[d];
      const float t = a.tb[s * a.D + d];
      if (t != t) continue;
      const float p = a.reg.ptr[m][(int64_t)b * a.reg.channels[m] * HW + (int64_t)a.col_ch[d] * a.reg.stride_c[m] + (int64_t)cell * a.reg.stride_p[m]];
      cnt[d] += p > t ? 1 : (p < t ? -1 : 0);
    }
  }
  for (int d = 0; d < a.D; ++d) {
    const int m = a.col_map[d];
    a.reg.grad[m][(int64_t)b * a.reg.channels[m] * HW + (int64_t)a.col_ch[d] * a.reg.stride_c[m] + (int64_t)cell * a.reg.stride_p[m]] =
        cnt[d] == 0 ? 0.0f : (float)((double)cnt[d] * (g_loc * (double)a.cw[d]));
  }
}

bool fill_loss(LossArgs& a, const float* hm, int64_t sc, int64_t sp, const float* heat, int B, int C, int H, int W,
               const CrbCenterMaps* reg, const float* tb, const int64_t* inds, const int64_t* masks, int nmax,
               const CrbCenterLossCfg* cfg, bool need_grad) {
  if (!hm || !heat || !reg || !tb || !inds || !masks || !cfg || B < 0 || C < 1 || H < 1 || W < 1 || nmax < 1) return false;
  if (reg->num_maps < 1 || reg->num_maps > CRB_CENTER_MAX_MAPS || (int64_t)C * H * W >= (1LL << 31)) return false;
  a.hm = hm;
  a.hm_sc = sc;
  a.hm_sp = sp;
  a.heat = heat;
  a.B = B;
  a.C = C;
  a.H = H;
  a.W = W;
  a.nmax = nmax;
  a.reg = *reg;
  a.D = 0;
  for (int m = 0; m < reg->num_maps; ++m) {
    if (!reg->ptr[m] || reg->channels[m] < 1 || (need_grad && !reg->grad[m])) return false;
    for (int c = 0; c < reg->channels[m]; ++c) {
      if (a.D >= CRB_CENTER_MAX_CODE) return false;
      a.col_map[a.D] = m;
      a.col_ch[a.D] = c;
      ++a.D;
    }
  }
  for (int d = 0; d < CRB_CENTER_MAX_CODE; ++d) a.cw[d] = cfg->code_weights[d];
  a.w_cls = cfg->cls_weight;
  a.w_loc = cfg->loc_weight;
  a.tb = tb;
  a.inds = inds;
  a.masks = masks;
  return true;
}

int tiles(int H, int W) { return (H * W + TPB - 1) / TPB; }

// ---------------------------------------------------------------------------------------------------------------------------
struct DecodeArgs {
  const float* val;
  const int64_t* idx;
  int B, K, C, H, W, cl, nbox;
  CrbCenterMaps reg;
  float rx, ry, vx, vy, stride, lim[6], thresh;
  float* boxes;
  float* scores;
  int64_t* labels;
  uint8_t* keep;
};

__device__ __forceinline__ float map_at(const CrbCenterMaps& r, int m, int c, int b, int64_t cell, int HW) {
  return r.ptr[m][(int64_t)b * r.channels[m] * HW + (int64_t)c * r.stride_c[m] + cell * r.stride_p[m]];
}

// decode_bbox_from_heatmap (:164-192) for the picked cells: x, y as the reference's f32 operations, exp / atan2 / sigmoid in f64
__global__ __launch_bounds__(TPB) void center_decode_kernel(DecodeArgs a) {
  const int i = blockIdx.x * TPB + (int)threadIdx.x;
  if (i >= a.B * a.K) return;
  const int b = i / a.K, HW = a.H * a.W;
  int64_t f = a.idx[i];
  if (f < 0 || f >= (int64_t)a.C * HW) f = 0;
  const int cls = a.cl ? (int)(f % a.C) : (int)(f / HW);
  const int64_t cell = a.cl ? f / a.C : f % HW;
  const float xs = (float)(cell % a.W), ys = (float)(cell / a.W);
  float* o = a.boxes + (int64_t)i * a.nbox;
  const float x = (xs + map_at(a.reg, 0, 0, b, cell, HW)) * a.stride * a.vx + a.rx;
  const float y = (ys + map_at(a.reg, 0, 1, b, cell, HW)) * a.stride * a.vy + a.ry;
  const float z = map_at(a.reg, 1, 0, b, cell, HW);
  o[0] = x;
  o[1] = y;
  o[2] = z;
  for (int d = 0; d < 3; ++d) o[3 + d] = (float)exp((double)map_at(a.reg, 2, d, b, cell, HW));
  o[6] = (float)atan2((double)map_at(a.reg, 3, 1, b, cell, HW), (double)map_at(a.reg, 3, 0, b, cell, HW));
  for (int d = 7; d < a.nbox; ++d) o[d] = map_at(a.reg, 4, d - 7, b, cell, HW);
  const float score = (float)(1.0 / (1.0 + exp(-(double)a.val[i])));
  a.scores[i] = score;
  a.labels[i] = cls;
  a.keep[i] = (x >= a.lim[0] && y >= a.lim[1] && z >= a.lim[2] && x <= a.lim[3] && y <= a.lim[4] && z <= a.lim[5] && score > a.thresh) ? 1 : 0;
}

}  // namespace

extern "C" {

int64_t crb_center_assign_workspace_bytes(int num_heads, int B, int num_max_objs) {
  if (num_heads <= 0 || B <= 0 || num_max_objs <= 0) return 16;
  return (int64_t)num_heads * B * num_max_objs * (int64_t)sizeof(int4);
}

int crb_center_assign_targets(const float* gt_boxes, int B, int M, int box_dim, int num_class, const int32_t* class_head,
                              const int32_t* class_local, int num_heads, const int32_t* head_channels, int H, int W,
                              const float* pc_range_xy, const float* voxel_size_xy, int feature_map_stride, int num_max_objs,
                              double gaussian_overlap, int min_radius, float* heatmaps, float* target_boxes, int64_t* inds,
                              int64_t* masks, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!class_head || !class_local || !head_channels || !pc_range_xy || !voxel_size_xy || !heatmaps || !target_boxes || !inds ||
      !masks || B < 0 || M < 0 || box_dim < 8 || H < 1 || W < 1 || num_max_objs < 1 || feature_map_stride < 1 || num_class < 1 ||
      num_heads < 1 || (M > 0 && B > 0 && !gt_boxes) || !(voxel_size_xy[0] > 0.0f) || !(voxel_size_xy[1] > 0.0f) ||
      (int64_t)H * W >= (1LL << 31))
    return CRB_ERR_ARG;
  if (num_class > MAX_CLS || num_heads > MAX_HEADS || box_dim - 8 > MAX_EXTRA) return CRB_ERR_UNSUPPORTED;
  if (B == 0) return CRB_OK;
  if (!workspace || workspace_bytes < crb_center_assign_workspace_bytes(num_heads, B, num_max_objs)) return CRB_ERR_WORKSPACE;
  AssignArgs a;
  a.gt = gt_boxes;
  a.B = B;
  a.M = M;
  a.box_dim = box_dim;
  a.E = box_dim - 8;
  a.num_class = num_class;
  a.num_heads = num_heads;
  a.H = H;
  a.W = W;
  a.nmax = num_max_objs;
  int64_t off = 0;
  for (int h = 0; h < num_heads; ++h) {
    if (head_channels[h] < 1) return CRB_ERR_ARG;
    a.head_channels[h] = head_channels[h];
    a.heat_off[h] = off;
    off += (int64_t)B * head_channels[h] * H * W;
  }
  for (int c = 0; c < num_class; ++c) {
    const int h = class_head[c];
    if (h >= num_heads || (h >= 0 && (class_local[c] < 0 || class_local[c] >= head_channels[h]))) return CRB_ERR_ARG;
    a.class_head[c] = h;
    a.class_local[c] = class_local[c];
  }
  a.rx = pc_range_xy[0];
  a.ry = pc_range_xy[1];
  a.vx = voxel_size_xy[0];
  a.vy = voxel_size_xy[1];
  a.stride = (float)feature_map_stride;
  a.overlap = gaussian_overlap;
  a.min_radius = min_radius;
  a.heat = heatmaps;
  a.tb = target_boxes;
  a.inds = inds;
  a.masks = masks;
  a.obj = (int4*)workspace;
  hipStream_t s = (hipStream_t)stream;
  const int64_t slots = (int64_t)num_heads * B * num_max_objs;
  CRB_HIP(hipMemsetAsync(heatmaps, 0, (size_t)off * sizeof(float), s));
  CRB_HIP(hipMemsetAsync(target_boxes, 0, (size_t)slots * (8 + a.E) * sizeof(float), s));
  CRB_HIP(hipMemsetAsync(inds, 0, (size_t)slots * sizeof(int64_t), s));
  CRB_HIP(hipMemsetAsync(masks, 0, (size_t)slots * sizeof(int64_t), s));
  CRB_HIP(hipMemsetAsync(workspace, 0xFF, (size_t)slots * sizeof(int4), s));
  if (M == 0) return CRB_OK;
  hipLaunchKernelGGL(center_slots_kernel, dim3(B), dim3(TPB), 0, s, a);
  hipLaunchKernelGGL(center_draw_kernel, dim3(num_max_objs, B, num_heads), dim3(TPB), 0, s, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

int64_t crb_center_loss_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 16;
  return (int64_t)B * tiles(H, W) * 3 * (int64_t)sizeof(double);
}

int crb_center_loss_forward(const float* hm, int64_t hm_stride_c, int64_t hm_stride_p, const float* heatmap, int B, int C, int H, int W,
                            const CrbCenterMaps* reg, const float* target_boxes, const int64_t* inds, const int64_t* masks,
                            int num_max_objs, const CrbCenterLossCfg* cfg, double* loss, double* stats, void* workspace,
                            int64_t workspace_bytes, void* stream) {
  LossArgs a;
  if (!fill_loss(a, hm, hm_stride_c, hm_stride_p, heatmap, B, C, H, W, reg, target_boxes, inds, masks, num_max_objs, cfg, false) ||
      !loss || !stats || B < 1)
    return CRB_ERR_ARG;
  if (num_max_objs > MAX_SLOTS) return CRB_ERR_UNSUPPORTED;       // (the backward's limit: refuse before anything is computed)
  if (!workspace || workspace_bytes < crb_center_loss_workspace_bytes(B, H, W)) return CRB_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int nt = tiles(H, W);
  double* partial = (double*)workspace;
  hipLaunchKernelGGL(center_loss_partial_kernel, dim3(nt, B), dim3(TPB), 0, s, a, partial);
  hipLaunchKernelGGL(center_loss_finalize_kernel, dim3(1), dim3(TPB), 0, s, a, (const double*)partial, nt * B, loss, stats);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

int crb_center_loss_backward(const float* hm, int64_t hm_stride_c, int64_t hm_stride_p, const float* heatmap, int B, int C, int H, int W,
                             const CrbCenterMaps* reg, const float* target_boxes, const int64_t* inds, const int64_t* masks,
                             int num_max_objs, const CrbCenterLossCfg* cfg, const double* stats, const float* grad_loss, float* d_hm,
                             void* stream) {
  LossArgs a;
  if (!fill_loss(a, hm, hm_stride_c, hm_stride_p, heatmap, B, C, H, W, reg, target_boxes, inds, masks, num_max_objs, cfg, true) ||
      !stats || !grad_loss || !d_hm || B < 1)
    return CRB_ERR_ARG;
  if (num_max_objs > MAX_SLOTS) return CRB_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(center_loss_backward_kernel, dim3(tiles(H, W), B), dim3(TPB), 0, (hipStream_t)stream, a, stats, grad_loss, d_hm);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

int crb_center_decode(const float* top_val, const int64_t* top_idx, int B, int K, int C, int H, int W, int idx_channels_last,
                      const CrbCenterMaps* reg, const float* pc_range_xy, const float* voxel_size_xy, int feature_map_stride,
                      const float* limit_range, float score_thresh, float* boxes, float* scores, int64_t* labels, uint8_t* keep,
                      void* stream) {
  if (!top_val || !top_idx || !reg || !pc_range_xy || !voxel_size_xy || !limit_range || !boxes || !scores || !labels || !keep ||
      B < 0 || K < 0 || C < 1 || H < 1 || W < 1 || feature_map_stride < 1 || (int64_t)C * H * W >= (1LL << 31))
    return CRB_ERR_ARG;
  // center (2), center_z (1), dim (3), rot (2) and optionally vel
  if (reg->num_maps < 4 || reg->num_maps > 5 || reg->channels[0] != 2 || reg->channels[1] != 1 || reg->channels[2] != 3 ||
      reg->channels[3] != 2 || (reg->num_maps == 5 && (reg->channels[4] < 1 || reg->channels[4] > MAX_EXTRA)))
    return CRB_ERR_ARG;
  for (int m = 0; m < reg->num_maps; ++m)
    if (!reg->ptr[m]) return CRB_ERR_ARG;
  if (B == 0 || K == 0) return CRB_OK;
  DecodeArgs a;
  a.val = top_val;
  a.idx = top_idx;
  a.B = B;
  a.K = K;
  a.C = C;
  a.H = H;
  a.W = W;
  a.cl = idx_channels_last ? 1 : 0;
  a.nbox = 7 + (reg->num_maps == 5 ? reg->channels[4] : 0);
  a.reg = *reg;
  a.rx = pc_range_xy[0];
  a.ry = pc_range_xy[1];
  a.vx = voxel_size_xy[0];
  a.vy = voxel_size_xy[1];
  a.stride = (float)feature_map_stride;
  for (int k = 0; k < 6; ++k) a.lim[k] = limit_range[k];
  a.thresh = score_thresh;
  a.boxes = boxes;
  a.scores = scores;
  a.labels = labels;
  a.keep = keep;
  hipLaunchKernelGGL(center_decode_kernel, dim3((B * K + TPB - 1) / TPB), dim3(TPB), 0, (hipStream_t)stream, a);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

}  // extern "C"
