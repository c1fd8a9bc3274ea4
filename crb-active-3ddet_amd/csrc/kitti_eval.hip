// KITTI object AP on gfx950: overlaps, ignore flags, true-positive scores, score thresholds and the precision / recall counts of
// every (frame, combination, threshold) (C-ABI in include/crb_hip.h).
//
// Replaces pcdet/datasets/kitti/kitti_object_eval_python/rotate_iou.py (numba.cuda) and the numba.jit loops of eval.py there:
// image_box_overlap, d3_box_overlap_kernel, clean_data, compute_statistics_jit, get_thresholds, fused_compute_statistics.
//
// Layout. Boxes of all frames are stacked: frame f owns ground-truth rows gt_off[f] .. gt_off[f + 1], detection rows dt_off[f] ..
// dt_off[f + 1], and its (detection, ground truth) pairs lie at pair_off[f] as a row-major [n_dt, n_gt] matrix, the orientation of
// the reference's overlaps[i]. Pairs of different frames do not exist. A combination is (metric, class, difficulty, overlap row);
// the caller lists them as arrays (metric, class * 3 + difficulty, minimum overlap, slot of its similarity sums or -1).
//
// Arithmetic. Image overlaps and everything the matching compares (scores, thresholds, minimum overlaps) are f64. The rotated
// intersection is the f32 routine of csrc/iou3d_bev.h: the pair is translated so that the ground-truth box is centred at the origin
// (the subtraction in f64, rounded once), the angle is negated (rbbox_to_corners turns clockwise for a positive angle, box_corners
// counter-clockwise), and a corner counts as inside up to kMargin outside, which only has to cover the f32 rounding of a corner
// lying exactly on the other box's boundary (identical boxes). BEV IoU is then f32 as in the reference, the 3D IoU takes the height
// overlap and the volumes in f64 and is rounded to f32 where the reference stores it.
//
// Launches. overlaps: one thread per pair. match_scores: one thread per (frame, combination). match_pr: one 64-thread workgroup
// (one wave) per (frame, combination), lane = threshold; the frame's overlaps of the metric, flags and scores are staged in LDS when
// n_gt <= 64, n_dt <= 512 and n_gt * n_dt <= 2048, otherwise the same walk reads them from global memory and keeps its
// assigned-detection bits in a caller-provided buffer. tp / fp / fn accumulate with integer atomics, the similarity as per-frame
// partial sums that one thread per (combination, threshold) adds in frame order: the result is the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/crb_hip.h"
#include "crb_common.h"
#include "iou3d_bev.h"

namespace {

constexpr int kPts = 41;                  // N_SAMPLE_PTS
constexpr int kStageGt = 64, kStageDt = 512, kStagePairs = 2048;
constexpr float kMargin = 4e-6f;
constexpr double kNoDetection = -10000000.0;

__device__ __forceinline__ int64_t frame_of_pair(const int64_t* pair_off, int64_t F, int64_t p) {
  int64_t lo = 0, hi = F;                 // the last f with pair_off[f] <= p (frames without pairs repeat an offset)
  while (hi - lo > 1) {
    int64_t mid = (lo + hi) >> 1;
    if (pair_off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void kitti_overlaps_kernel(const int64_t* __restrict__ gt_off, const int64_t* __restrict__ dt_off,
                                                             const int64_t* __restrict__ pair_off, int64_t F, int64_t P,
                                                             const double* __restrict__ gt_bbox, const double* __restrict__ dt_bbox,
                                                             const double* __restrict__ gt_cam, const double* __restrict__ dt_cam,
                                                             double* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const int64_t f = frame_of_pair(pair_off, F, p);
  const int64_t ng = gt_off[f + 1] - gt_off[f], local = p - pair_off[f];
  const double* gb = gt_bbox + 4 * (gt_off[f] + local % ng);
  const double* db = dt_bbox + 4 * (dt_off[f] + local / ng);
  const double* gc = gt_cam + 7 * (gt_off[f] + local % ng);
  const double* dc = dt_cam + 7 * (dt_off[f] + local / ng);
  // image boxes (image_box_overlap, criterion -1 and 0 with boxes = detections)
  double iou = 0.0, over_dt = 0.0;
  const double iw = fmin(db[2], gb[2]) - fmax(db[0], gb[0]);
  if (iw > 0) {
    const double ih = fmin(db[3], gb[3]) - fmax(db[1], gb[1]);
    if (ih > 0) {
      const double da = (db[2] - db[0]) * (db[3] - db[1]), ga = (gb[2] - gb[0]) * (gb[3] - gb[1]);
      iou = iw * ih / (da + ga - iw * ih);
      over_dt = iw * ih / da;
    }
  }
  out[p] = iou;
  out[3 * P + p] = over_dt;
  // rotated rectangles in the camera's x-z plane: [x, z, l, w, ry] = columns 0, 2, 3, 5, 6
  const float a[7] = {0.f, 0.f, 0.f, (float)gc[3], (float)gc[5], 0.f, -(float)gc[6]};
  const float b[7] = {(float)(dc[0] - gc[0]), (float)(dc[2] - gc[2]), 0.f, (float)dc[3], (float)dc[5], 0.f, -(float)dc[6]};
  const float reach = 0.5f * (sqrtf(a[3] * a[3] + a[4] * a[4]) + sqrtf(b[3] * b[3] + b[4] * b[4]));
  // The reach does not include kMargin, on purpose: the yardstick here is the reference's f64 clipper, which has no margin and
  // gives disjoint rectangles exactly 0 - as this reject does. (The NMS reject of csrc/iou3d_nms.hip has to include its margin:
  // its reference counts corners inside the margin and returns a non-zero overlap for disjoint boxes.)
  float inter = 0.f;
  if (b[0] * b[0] + b[1] * b[1] <= reach * reach) inter = rect_overlap(a, b, kMargin);
  double bev = 0.0, d3 = 0.0;
  if (inter > 0.f) {
    bev = (double)(inter / (a[3] * a[4] + b[3] * b[4] - inter));
    const double h = fmin(dc[1], gc[1]) - fmax(dc[1] - dc[4], gc[1] - gc[4]);     // boxes are bottom-centred, y points down
    if (h > 0) {
      const double inc = h * (double)inter;
      d3 = (double)(float)(inc / (dc[3] * dc[4] * dc[5] + gc[3] * gc[4] * gc[5] - inc));
    }
  }
  out[P + p] = bev;
  out[2 * P + p] = d3;
}

// clean_data: flag[(c * 3 + l) * n + box], 0 counts, 1 ignored, -1 another class
__global__ __launch_bounds__(256) void kitti_flags_kernel(const int32_t* __restrict__ gt_cls, const double* __restrict__ gt_occ,
                                                          const double* __restrict__ gt_trunc, const double* __restrict__ gt_bbox,
                                                          int64_t G, const int32_t* __restrict__ dt_cls,
                                                          const double* __restrict__ dt_bbox, int64_t D,
                                                          const int32_t* __restrict__ classes, int C, int8_t* __restrict__ gt_flag,
                                                          int8_t* __restrict__ dt_flag) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (G + D) * C * 3) return;
  const int cl = (int)(t / (G + D)), c = classes[cl / 3], l = cl % 3;
  const int64_t box = t % (G + D);
  const double min_height = l == 0 ? 40.0 : 25.0;
  if (box < G) {
    const int cls = gt_cls[box];
    const int valid = cls == c ? 1 : ((c == 1 && cls == 4) || (c == 0 && cls == 3)) ? 0 : -1;
    const double max_trunc = l == 0 ? 0.15 : l == 1 ? 0.3 : 0.5;
    const bool ignore = gt_occ[box] > (double)l || gt_trunc[box] > max_trunc || gt_bbox[4 * box + 3] - gt_bbox[4 * box + 1] <= min_height;
    gt_flag[(int64_t)cl * G + box] = (valid == 1 && !ignore) ? 0 : (valid == 0 || (ignore && valid == 1)) ? 1 : -1;
  } else {
    const int64_t d = box - G;
    const double height = fabs(dt_bbox[4 * d + 3] - dt_bbox[4 * d + 1]);
    dt_flag[(int64_t)cl * D + d] = height < min_height ? 1 : dt_cls[d] == c ? 0 : -1;
  }
}

// compute_statistics_jit of one frame for one threshold. ov / ovdc [nd][ng]; asg: the bits of the assigned detections, word w at
// asg[w * astride]. kFp false: the thresh = 0, compute_fp = False pass, which leaves the matched score of every ground-truth box
// in tp_slot (-inf: none).
template <bool kFp>
__device__ void greedy_match(const double* ov, int ng, int nd, const int8_t* gf, const int8_t* df, const double* score, double min_ov,
                             double thresh, uint32_t* asg, int astride, double* tp_slot, const double* ovdc, const uint8_t* gdc,
                             int metric, bool aos, const double* galpha, const double* dalpha, int& tp_o, int& fp_o, int& fn_o,
                             double& sim_o) {
  const int nw = (nd + 31) >> 5;
  for (int w = 0; w < nw; ++w) asg[w * astride] = 0u;
  int tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  for (int i = 0; i < ng; ++i) {
    if (!kFp) tp_slot[i] = -INFINITY;
    const int gfi = gf[i];
    if (gfi == -1) continue;
    int det = -1;
    double valid = kNoDetection, max_ov = 0.0;
    bool ignored_det = false;
    for (int j = 0; j < nd; ++j) {
      const int dfj = df[j];
      if (dfj == -1) continue;
      if ((asg[(j >> 5) * astride] >> (j & 31)) & 1u) continue;
      const double s = score[j];
      if (kFp && s < thresh) continue;
      const double o = ov[(int64_t)j * ng + i];
      if (!(o > min_ov)) continue;
      if (!kFp) {
        if (s > valid) { det = j; valid = s; }
      } else if ((o > max_ov || ignored_det) && dfj == 0) {
        max_ov = o; det = j; valid = 1.0; ignored_det = false;
      } else if (valid == kNoDetection && dfj == 1) {
        det = j; valid = 1.0; ignored_det = true;
      }
    }
    if (valid == kNoDetection) {
      if (gfi == 0) ++fn;
    } else {
      if (!(gfi == 1 || df[det] == 1)) {
        ++tp;
        if (!kFp) tp_slot[i] = score[det];
        if (aos) sim += (1.0 + cos(galpha[i] - dalpha[det])) / 2.0;
      }
      asg[(det >> 5) * astride] |= 1u << (det & 31);
    }
  }
  if (kFp) {
    for (int j = 0; j < nd; ++j)
      if (df[j] == 0 && !((asg[(j >> 5) * astride] >> (j & 31)) & 1u) && !(score[j] < thresh)) ++fp;
    if (metric == 0) {                       // false positives inside DontCare regions are nobody's fault
      for (int i = 0; i < ng; ++i) {
        if (!gdc[i]) continue;
        for (int j = 0; j < nd; ++j) {
          if (df[j] != 0 || ((asg[(j >> 5) * astride] >> (j & 31)) & 1u) || score[j] < thresh) continue;
          if (ovdc[(int64_t)j * ng + i] > min_ov) {
            asg[(j >> 5) * astride] |= 1u << (j & 31);
            --fp;
          }
        }
      }
    }
  }
  tp_o = tp; fp_o = fp; fn_o = fn; sim_o = sim;
}

__global__ __launch_bounds__(256) void kitti_match_scores_kernel(
    const int64_t* __restrict__ gt_off, const int64_t* __restrict__ dt_off, const int64_t* __restrict__ pair_off,
    const int64_t* __restrict__ asg_off, int64_t F, int64_t G, int64_t D, int64_t P, const double* __restrict__ overlaps,
    const int8_t* __restrict__ gt_flag, const int8_t* __restrict__ dt_flag, const double* __restrict__ dt_score,
    const int32_t* __restrict__ combo_metric, const int32_t* __restrict__ combo_flags, const double* __restrict__ combo_min_overlap,
    int NC, uint32_t* __restrict__ asg, double* __restrict__ tp_scores) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= F * NC) return;
  const int64_t f = t / NC;
  const int q = (int)(t % NC);
  const int ng = (int)(gt_off[f + 1] - gt_off[f]), nd = (int)(dt_off[f + 1] - dt_off[f]);
  const int nw = (nd + 31) >> 5;
  int tp, fp, fn;
  double sim;
  greedy_match<false>(overlaps + (int64_t)combo_metric[q] * P + pair_off[f], ng, nd, gt_flag + (int64_t)combo_flags[q] * G + gt_off[f],
                      dt_flag + (int64_t)combo_flags[q] * D + dt_off[f], dt_score + dt_off[f], combo_min_overlap[q], 0.0,
                      asg + asg_off[f] * NC + (int64_t)q * nw, 1, tp_scores + (int64_t)q * G + gt_off[f], nullptr, nullptr, 0, false,
                      nullptr, nullptr, tp, fp, fn, sim);
}

// get_thresholds on the descending scores of a combination; one thread each (the scan carries current_recall)
__global__ __launch_bounds__(64) void kitti_thresholds_kernel(const double* __restrict__ sorted_scores, const int32_t* __restrict__ num_scores,
                                                              const int32_t* __restrict__ num_valid_gt, int NC, int64_t G,
                                                              double* __restrict__ thresholds, int32_t* __restrict__ num_thresholds) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= NC) return;
  const double* s = sorted_scores + (int64_t)q * G;
  const int64_t n = num_scores[q];
  const double num_gt = (double)num_valid_gt[q];
  double current_recall = 0.0;
  int cnt = 0;
  for (int64_t i = 0; i < n && cnt < kPts; ++i) {
    const double l_recall = (double)(i + 1) / num_gt;
    const double r_recall = i < n - 1 ? (double)(i + 2) / num_gt : l_recall;
    if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
    thresholds[q * kPts + cnt++] = s[i];
    current_recall += 1.0 / ((double)kPts - 1.0);
  }
  for (int k = cnt; k < kPts; ++k) thresholds[q * kPts + k] = 0.0;
  num_thresholds[q] = cnt;
}

__global__ __launch_bounds__(64) void kitti_match_pr_kernel(
    const int64_t* __restrict__ gt_off, const int64_t* __restrict__ dt_off, const int64_t* __restrict__ pair_off,
    const int64_t* __restrict__ big_off, int64_t F, int64_t G, int64_t D, int64_t P, const double* __restrict__ overlaps,
    const int8_t* __restrict__ gt_flag, const int8_t* __restrict__ dt_flag, const double* __restrict__ dt_score,
    const uint8_t* __restrict__ gt_dc, const double* __restrict__ gt_alpha, const double* __restrict__ dt_alpha,
    const int32_t* __restrict__ combo_metric, const int32_t* __restrict__ combo_flags, const double* __restrict__ combo_min_overlap,
    const int32_t* __restrict__ combo_aos, int NC, int num_aos, const double* __restrict__ thresholds,
    const int32_t* __restrict__ num_thresholds, uint32_t* __restrict__ asg_big, int32_t* __restrict__ counts,
    double* __restrict__ sim_part) {
  __shared__ double s_ov[kStagePairs];
  __shared__ double s_score[kStageDt];
  __shared__ uint32_t s_asg[(kStageDt / 32) * 64];
  __shared__ int8_t s_gf[kStageGt];
  __shared__ int8_t s_df[kStageDt];
  const int64_t f = (int64_t)blockIdx.x / NC;
  const int q = (int)((int64_t)blockIdx.x % NC);
  const int lane = threadIdx.x;
  const int nthr = num_thresholds[q];
  const int slot = combo_aos[q];
  if (nthr == 0) {
    if (slot >= 0 && lane < kPts) sim_part[(f * num_aos + slot) * kPts + lane] = 0.0;
    return;
  }
  const int ng = (int)(gt_off[f + 1] - gt_off[f]), nd = (int)(dt_off[f + 1] - dt_off[f]);
  const int metric = combo_metric[q];
  const double* ov = overlaps + (int64_t)metric * P + pair_off[f];
  const int8_t* gf = gt_flag + (int64_t)combo_flags[q] * G + gt_off[f];
  const int8_t* df = dt_flag + (int64_t)combo_flags[q] * D + dt_off[f];
  const double* score = dt_score + dt_off[f];
  const int nw = (nd + 31) >> 5;
  uint32_t* asg;
  int astride = 64;
  const bool staged = ng <= kStageGt && nd <= kStageDt && (int64_t)ng * nd <= kStagePairs;
  if (staged) {
    for (int k = lane; k < ng * nd; k += 64) s_ov[k] = ov[k];
    for (int k = lane; k < nd; k += 64) { s_score[k] = score[k]; s_df[k] = df[k]; }
    for (int k = lane; k < ng; k += 64) s_gf[k] = gf[k];
    __syncthreads();
    ov = s_ov; gf = s_gf; df = s_df; score = s_score;
    asg = s_asg + lane;
  } else {
    asg = asg_big + (big_off[f] * NC + (int64_t)q * nw) * 64 + lane;
  }
  int tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  if (lane < nthr) {
    greedy_match<true>(ov, ng, nd, gf, df, score, combo_min_overlap[q], thresholds[q * kPts + lane], asg, astride, nullptr,
                       overlaps + 3 * P + pair_off[f], gt_dc + gt_off[f], metric, slot >= 0, gt_alpha + gt_off[f], dt_alpha + dt_off[f],
                       tp, fp, fn, sim);
    int32_t* c = counts + ((int64_t)q * kPts + lane) * 3;
    if (tp) atomicAdd(c, tp);
    if (fp) atomicAdd(c + 1, fp);
    if (fn) atomicAdd(c + 2, fn);
  }
  if (slot >= 0 && lane < kPts) sim_part[(f * num_aos + slot) * kPts + lane] = sim;
}

// result[(q * 41 + t) * 5 ..] = tp, fp, fn, similarity (frames added in order), threshold; result[NC * 41 * 5 + q] = thresholds of q
__global__ __launch_bounds__(64) void kitti_finish_kernel(int64_t F, int NC, int num_aos, const int32_t* __restrict__ combo_aos,
                                                          const int32_t* __restrict__ counts, const double* __restrict__ sim_part,
                                                          const double* __restrict__ thresholds,
                                                          const int32_t* __restrict__ num_thresholds, double* __restrict__ result) {
  const int q = blockIdx.x, t = threadIdx.x;
  if (t >= kPts) return;
  double sim = 0.0;
  const int slot = combo_aos[q];
  if (slot >= 0)
    for (int64_t f = 0; f < F; ++f) sim += sim_part[(f * num_aos + slot) * kPts + t];
  double* r = result + ((int64_t)q * kPts + t) * 5;
  const int32_t* c = counts + ((int64_t)q * kPts + t) * 3;
  r[0] = (double)c[0]; r[1] = (double)c[1]; r[2] = (double)c[2]; r[3] = sim; r[4] = thresholds[q * kPts + t];
  if (t == 0) result[(int64_t)NC * kPts * 5 + q] = (double)num_thresholds[q];
}

}  // namespace

extern "C" int crb_kitti_stage_limit(int which) {
  return which == 0 ? kStageGt : which == 1 ? kStageDt : which == 2 ? kStagePairs : -1;
}

extern "C" int crb_kitti_overlaps(const int64_t* gt_off, const int64_t* dt_off, const int64_t* pair_off, int64_t num_frames,
                                  int64_t num_pairs, const double* gt_bbox, const double* dt_bbox, const double* gt_cam,
                                  const double* dt_cam, double* overlaps, void* stream) {
  if (num_frames < 0 || num_pairs < 0 || num_pairs > 256LL * 0x7fffffffLL) return CRB_ERR_ARG;
  if (num_pairs == 0) return CRB_OK;
  hipLaunchKernelGGL(kitti_overlaps_kernel, dim3(crb_cdiv(num_pairs, 256)), dim3(256), 0, (hipStream_t)stream, gt_off, dt_off, pair_off,
                     num_frames, num_pairs, gt_bbox, dt_bbox, gt_cam, dt_cam, overlaps);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_kitti_ignore_flags(const int32_t* gt_cls, const double* gt_occ, const double* gt_trunc, const double* gt_bbox,
                                      int64_t G, const int32_t* dt_cls, const double* dt_bbox, int64_t D, const int32_t* classes,
                                      int num_classes, int8_t* gt_flag, int8_t* dt_flag, void* stream) {
  if (G < 0 || D < 0 || num_classes <= 0 || (G + D) * num_classes * 3 > 256LL * 0x7fffffffLL) return CRB_ERR_ARG;
  if (G + D == 0) return CRB_OK;
  hipLaunchKernelGGL(kitti_flags_kernel, dim3(crb_cdiv((G + D) * num_classes * 3, 256)), dim3(256), 0, (hipStream_t)stream, gt_cls, gt_occ,
                     gt_trunc, gt_bbox, G, dt_cls, dt_bbox, D, classes, num_classes, gt_flag, dt_flag);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_kitti_match_scores(const int64_t* gt_off, const int64_t* dt_off, const int64_t* pair_off, const int64_t* asg_off,
                                      int64_t num_frames, int64_t G, int64_t D, int64_t num_pairs, const double* overlaps,
                                      const int8_t* gt_flag, const int8_t* dt_flag, const double* dt_score,
                                      const int32_t* combo_metric, const int32_t* combo_flags, const double* combo_min_overlap,
                                      int num_combos, uint32_t* asg_workspace, double* tp_scores, void* stream) {
  if (num_frames < 0 || G < 0 || D < 0 || num_pairs < 0 || num_combos <= 0 || num_frames * num_combos > 256LL * 0x7fffffffLL)
    return CRB_ERR_ARG;
  if (num_frames == 0) return CRB_OK;
  hipLaunchKernelGGL(kitti_match_scores_kernel, dim3(crb_cdiv(num_frames * num_combos, 256)), dim3(256), 0, (hipStream_t)stream, gt_off,
                     dt_off, pair_off, asg_off, num_frames, G, D, num_pairs, overlaps, gt_flag, dt_flag, dt_score, combo_metric,
                     combo_flags, combo_min_overlap, num_combos, asg_workspace, tp_scores);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_kitti_thresholds(const double* sorted_scores, const int32_t* num_scores, const int32_t* num_valid_gt, int num_combos,
                                    int64_t G, double* thresholds, int32_t* num_thresholds, void* stream) {
  if (num_combos <= 0 || G < 0) return CRB_ERR_ARG;
  hipLaunchKernelGGL(kitti_thresholds_kernel, dim3(crb_cdiv(num_combos, 64)), dim3(64), 0, (hipStream_t)stream, sorted_scores, num_scores,
                     num_valid_gt, num_combos, G, thresholds, num_thresholds);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int crb_kitti_match_pr(const int64_t* gt_off, const int64_t* dt_off, const int64_t* pair_off, const int64_t* big_off,
                                  int64_t num_frames, int64_t G, int64_t D, int64_t num_pairs, const double* overlaps,
                                  const int8_t* gt_flag, const int8_t* dt_flag, const double* dt_score, const uint8_t* gt_dc,
                                  const double* gt_alpha, const double* dt_alpha, const int32_t* combo_metric,
                                  const int32_t* combo_flags, const double* combo_min_overlap, const int32_t* combo_aos, int num_combos,
                                  int num_aos, const double* thresholds, const int32_t* num_thresholds, uint32_t* asg_big,
                                  int32_t* counts, double* sim_part, double* result, void* stream) {
  if (num_frames < 0 || G < 0 || D < 0 || num_pairs < 0 || num_combos <= 0 || num_aos < 0 || num_aos > num_combos ||
      num_frames * num_combos > 0x7fffffffLL)
    return CRB_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  CRB_HIP(hipMemsetAsync(counts, 0, (size_t)num_combos * kPts * 3 * sizeof(int32_t), st));
  if (num_frames > 0)
    hipLaunchKernelGGL(kitti_match_pr_kernel, dim3((unsigned)(num_frames * num_combos)), dim3(64), 0, st, gt_off, dt_off, pair_off, big_off,
                       num_frames, G, D, num_pairs, overlaps, gt_flag, dt_flag, dt_score, gt_dc, gt_alpha, dt_alpha, combo_metric,
                       combo_flags, combo_min_overlap, combo_aos, num_combos, num_aos, thresholds, num_thresholds, asg_big, counts,
                       sim_part);
  hipLaunchKernelGGL(kitti_finish_kernel, dim3(num_combos), dim3(64), 0, st, num_frames, num_combos, num_aos, combo_aos, counts, sim_part,
                     thresholds, num_thresholds, result);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
