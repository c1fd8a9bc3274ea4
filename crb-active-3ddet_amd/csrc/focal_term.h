// The sigmoid focal term of one logit, shared by csrc/point_head.hip, csrc/part_head.hip and, through csrc/rpn_loss_terms.h,
// csrc/rpn_loss.hip and csrc/multihead_loss.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// focal term of one logit and its derivative w.r.t. the logit, the expressions of rpn_loss.hip (loss_utils.py:47-72)
__device__ __forceinline__ void focal_term(float x, bool t, float alpha, float gamma, float& loss, float& d) {
  const float p = 1.0f / (1.0f + expf(-x));
  const float bce = fmaxf(x, 0.0f) - (t ? x : 0.0f) + log1pf(expf(-fabsf(x)));
  const float pt = t ? 1.0f - p : p;
  const float aw = t ? alpha : 1.0f - alpha;
  float ptg, ptg1;
  if (gamma == 2.0f) {
    ptg = pt * pt;
    ptg1 = 2.0f * pt;
  } else {
    ptg = powf(pt, gamma);
    ptg1 = gamma * powf(pt, gamma - 1.0f);
  }
  loss = aw * ptg * bce;
  const float dpt = t ? -p * (1.0f - p) : p * (1.0f - p);
  const float dbce = x == 0.0f ? (t ? 0.0f : 1.0f) : (t ? p - 1.0f : p);
  d = aw * (ptg1 * dpt * bce + ptg * dbce);
}

}  // namespace
