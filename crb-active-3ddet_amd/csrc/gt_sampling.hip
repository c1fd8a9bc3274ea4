// gt_sampling for a batch of training frames on gfx950: collision test of the drawn database objects and paste of the accepted
// ones (C-ABI in include/crb_hip.h).
//
// Replaces, for a whole batch on the device, what the reference does per frame in loader workers:
//   pcdet/datasets/augmentor/database_sampler.py:150-234 (DataBaseSampler.__call__ from the IoU tests on, add_sampled_boxes_to_scene)
//   with pcdet/ops/iou3d_nms/src/iou3d_cpu.cpp:232-252 (boxes_iou_bev_cpu), pcdet/utils/box_utils.py:75-89,145-158
//   (remove_points_in_boxes3d, enlarge_box3d) and pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-167 (points_in_boxes_cpu).
//
// The random draws stay on the host (the candidate walk of sample_with_fixed_number never depends on a collision result), and so
// does the arithmetic on the few dozen candidate boxes of a frame; the kernels receive one record of GS_REC = 20 f32 per candidate:
//   [0..6]   box x, y, z, dx, dy, dz, heading as it enters the collision test (z BEFORE the road-plane shift)
//   [7]      class as f32
//   [8]      shift: the road-plane z shift of the object (0 when unused)
//   [9..16]  removal box: cx, cy, cz (after the shift), dx, dy, dz with REMOVE_EXTRA_WIDTH added, cosa = f32(cos(-(double)rz)),
//            sina = f32(sin(-(double)rz))
//   [17..19] the offset added to the object's database points (the database box centre)
// Arithmetic definition (pcdet/datasets/augmentor/database_sampler.py of this repository is the same sequence in numpy, and the two
// agree bit for bit):
//   collision  candidate s of group k is valid iff iou_bev_rot(s, o) == 0.0f for every box o that exists when group k is tested - the
//              frame's own boxes and the valid candidates of groups < k - and for every other candidate o of group k. iou_bev_rot is
//              the device function of crb_boxes_pairwise(mode 1) (csrc/iou3d_bev.h), candidate first.
//   appended   box row = [x, y, z - shift, dx, dy, dz, heading, class]: one f32 subtraction.
//   pasted     point row = database row with x + ox, y + oy, (z + oz) - shift: separate f32 additions, then one f32 subtraction that
//              is skipped when shift == 0 (the reference only subtracts with USE_ROAD_PLANE).
//   removal    (the CPU twin's rule, roiaware_pool3d.cpp:121-140) a scene point is inside a removal box iff
//              !(fabsf(z - cz) > dz / 2) and, with sx = x - cx, sy = y - cy, lx = sx * cosa + sy * (-sina), ly = sx * sina + sy * cosa
//              (every f32 product and sum rounded once, no FMA), (double)fabsf(lx) < (double)dx / 2 + (double)1e-2f and the same
//              for ly / dy. A scene point inside the removal box of any VALID candidate of its frame is dropped.
//
// Launches. select: one 256-thread workgroup per frame; the groups in order with barriers between them, (candidate, box) pairs spread
// over the lanes, flags OR-ed in LDS, accepted candidates appended to the frame's box list in LDS. paste: count / scan / emit over the
// scene points as in csrc/augment.hip (wave ballots, no atomics, stable order) and one block per (candidate, frame) for the objects.
#include "crb_common.h"
#include "../../include/crb_hip.h"
#include "iou3d_bev.h"

namespace {

constexpr int GS_REC = 20;
constexpr int GS_MAX_S = 256;       // candidates per frame
constexpr int GS_MAX_BOXES = 512;   // frame boxes + candidates per frame
constexpr int GS_W = 8;

// ------------------------------------------------------------------------------------------------------------------------------
// select
// ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gs_select(const float* __restrict__ gt_boxes, const int* __restrict__ gt_counts, int G,
                                                 const float* __restrict__ cand, const int* __restrict__ cand_obj,
                                                 const int* __restrict__ group_off, int S, int K,
                                                 const int* __restrict__ obj_off, int num_objects,
                                                 unsigned char* __restrict__ valid, float* __restrict__ out_boxes,
                                                 int* __restrict__ new_counts, int* __restrict__ cand_rows,
                                                 int* __restrict__ paste_counts) {
  __shared__ float sbox[GS_MAX_BOXES * 7];     // the boxes that exist so far, then (behind them) the current group's candidates
  __shared__ int flag[GS_MAX_S];
  __shared__ int sh[4];
  const int b = blockIdx.x, tid = (int)threadIdx.x;
  int cnt = gt_counts[b];
  cnt = cnt < 0 ? 0 : (cnt > G ? G : cnt);
  const float* fb = gt_boxes + (int64_t)b * G * GS_W;
  const float* fc = cand + (int64_t)b * S * GS_REC;
  const int* go = group_off + (int64_t)b * (K + 1);
  float* ob = out_boxes + (int64_t)b * (G + S) * GS_W;
  unsigned char* fv = valid + (int64_t)b * S;
  int n_cand = go[K];
  n_cand = n_cand < 0 ? 0 : (n_cand > S ? S : n_cand);

  for (int t = tid; t < cnt * 7; t += 256) sbox[t] = fb[(int64_t)(t / 7) * GS_W + t % 7];
  for (int t = tid; t < cnt * GS_W; t += 256) ob[t] = fb[t];
  for (int t = tid; t < S; t += 256) fv[t] = 0;       // padding and candidates outside every group
  __syncthreads();
  int n_exist = cnt;
  for (int k = 0; k < K; ++k) {
    // (all of these are uniform over the block: every thread takes every barrier)
    int s0 = go[k], s1 = go[k + 1];
    s0 = s0 < 0 ? 0 : (s0 > n_cand ? n_cand : s0);
    s1 = s1 < s0 ? s0 : (s1 > n_cand ? n_cand : s1);
    const int ns = s1 - s0;
    if (ns == 0) continue;
    float* sc = sbox + n_exist * 7;            // n_exist + ns <= cnt + n_cand <= GS_MAX_BOXES
    __syncthreads();                           // the appends of the group before
    for (int t = tid; t < ns * 7; t += 256) sc[t] = fc[(int64_t)(s0 + t / 7) * GS_REC + t % 7];
    if (tid < ns) flag[tid] = 0;
    __syncthreads();
    const int others = n_exist + ns;
    for (int t = tid; t < ns * others; t += 256) {
      const int c = t / others, j = t - c * others;
      if (j == n_exist + c) continue;          // the candidate itself
      const float iou = iou_bev_rot(sc + c * 7, sbox + j * 7);
      if (!(iou == 0.0f)) flag[c] = 1;         // (every writer stores the same value)
    }
    __syncthreads();
    const bool ok = tid < ns && flag[tid] == 0;
    float row[7];
    if (ok) {
#pragma unroll
      for (int q = 0; q < 7; ++q) row[q] = sc[tid * 7 + q];
    }
    int tot;
    const int ex = crb_block_excl_scan_256(ok ? 1 : 0, sh, &tot);   // (barriers inside: every row[] is read before sc is overwritten)
    if (tid < ns) fv[s0 + tid] = ok ? 1 : 0;
    if (ok) {
      float* dst = sbox + (n_exist + ex) * 7;
#pragma unroll
      for (int q = 0; q < 7; ++q) dst[q] = row[q];
      const float* rec = fc + (int64_t)(s0 + tid) * GS_REC;
      float* o = ob + (int64_t)(n_exist + ex) * GS_W;
#pragma unroll
      for (int q = 0; q < 7; ++q) o[q] = row[q];
      o[2] = __fsub_rn(row[2], rec[8]);
      o[7] = rec[7];
    }
    n_exist += tot;
  }
  __syncthreads();                             // fv[] below is read by another thread than the one that wrote it
  for (int64_t t = (int64_t)n_exist * GS_W + tid; t < (int64_t)(G + S) * GS_W; t += 256) ob[t] = 0.f;
  // rows of every valid candidate's points inside the frame's pasted block: exclusive scan of the point counts in candidate order
  int np = 0;
  if (tid < n_cand && fv[tid]) {
    const int o = cand_obj[(int64_t)b * S + tid];
    if (o >= 0 && o < num_objects) np = obj_off[o + 1] - obj_off[o];
    np = np < 0 ? 0 : np;
  }
  int tot;
  const int ex = crb_block_excl_scan_256(np, sh, &tot);
  if (tid < S) cand_rows[(int64_t)b * S + tid] = (tid < n_cand && fv[tid]) ? ex : -1;
  if (tid == 0) {
    new_counts[b] = n_exist;
    paste_counts[b] = tot;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// paste
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool gs_in_removal_box(float x, float y, float z, const float* __restrict__ r /* rec + 9 */) {
  if (fabsf(__fsub_rn(z, r[2])) > r[5] / 2.0f) return false;
  const float sx = __fsub_rn(x, r[0]), sy = __fsub_rn(y, r[1]);
  const float cosa = r[6], sina = r[7];
  const float lx = __fadd_rn(__fmul_rn(sx, cosa), __fmul_rn(sy, -sina));
  const float ly = __fadd_rn(__fmul_rn(sx, sina), __fmul_rn(sy, cosa));
  const double margin = (double)1e-2f;
  return (double)fabsf(lx) < (double)r[3] / 2.0 + margin && (double)fabsf(ly) < (double)r[4] / 2.0 + margin;
}

// last frame b with frame_off[b] <= i (as aug_frame_of in csrc/augment.hip)
__device__ __forceinline__ int gs_frame_of(const int* __restrict__ frame_off, int B, int i) {
  int lo = 0, hi = B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (frame_off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

struct GsScene {
  const float* pts;
  int n, C, B, S;
  const int* frame_off;
  const float* cand;
  const unsigned char* valid;
};

__device__ __forceinline__ bool gs_keep(const GsScene& a, int i, int& b) {
  const float* q = a.pts + (int64_t)i * a.C;
  const float x = q[0], y = q[1], z = q[2];
  b = gs_frame_of(a.frame_off, a.B, i);
  const unsigned char* fv = a.valid + (int64_t)b * a.S;
  const float* fc = a.cand + (int64_t)b * a.S * GS_REC;
  for (int s = 0; s < a.S; ++s)
    if (fv[s] && gs_in_removal_box(x, y, z, fc + (int64_t)s * GS_REC + 9)) return false;
  return true;
}

__global__ __launch_bounds__(256) void gs_count(GsScene a, int* __restrict__ block_counts) {
  __shared__ int sh[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool keep = false;
  int b;
  if (i < a.n) keep = gs_keep(a, i, b);
  const unsigned long long m = __ballot(keep);
  if (crb_lane() == 0) sh[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// one block: block_counts (m) -> exclusive bases in place; paste_prefix[b] = pasted rows of the frames before b (B + 1 entries);
// new_off[b] for every frame that starts at or past the last scene point (b = B always), new_off[B + 1] = capacity. Frames that
// start at a scene point get their offset from that point's thread in gs_emit.
__global__ __launch_bounds__(256) void gs_scan(int* __restrict__ block_counts, int m, const int* __restrict__ frame_off, int B,
                                               int n, const int* __restrict__ paste_counts, int* __restrict__ paste_prefix,
                                               int* __restrict__ new_off, int capacity) {
  __shared__ int sh[4];
  int carry = 0;
  for (int base = 0; base < m; base += 256) {
    const int i = base + (int)threadIdx.x;
    const int v = i < m ? block_counts[i] : 0;
    int tot;
    const int ex = crb_block_excl_scan_256(v, sh, &tot);
    if (i < m) block_counts[i] = carry + ex;
    carry += tot;
    __syncthreads();
  }
  int pcarry = 0;
  for (int base = 0; base <= B; base += 256) {
    const int f = base + (int)threadIdx.x;
    const int v = f < B ? paste_counts[f] : 0;
    int tot;
    const int ex = crb_block_excl_scan_256(v, sh, &tot);
    if (f <= B) {
      paste_prefix[f] = pcarry + ex;
      if (frame_off[f] >= n) new_off[f] = carry + pcarry + ex;
    }
    pcarry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) new_off[B + 1] = capacity;
}

__global__ __launch_bounds__(256) void gs_emit(GsScene a, const int* __restrict__ block_base, const int* __restrict__ paste_prefix,
                                               float* __restrict__ out, int64_t capacity, int* __restrict__ new_off) {
  __shared__ int sh[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = crb_lane(), wave = (int)(threadIdx.x >> 6);
  bool keep = false;
  int b = 0;
  if (i < a.n) keep = gs_keep(a, i, b);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) sh[wave] = __popcll(m);
  __syncthreads();
  int rank = block_base[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) rank += sh[w];
  if (i >= a.n) return;
  // the first scene point of frame b (and of the empty frames just before it) carries their new offset: the kept scene rows before
  // it plus the pasted rows of the frames before
  for (int f = b; f >= 0 && a.frame_off[f] == i; --f) new_off[f] = rank + paste_prefix[f];
  if (!keep) return;
  const int64_t row = (int64_t)rank + paste_prefix[b + 1];      // behind this frame's own pasted rows
  if (row >= capacity) return;
  const float* q = a.pts + (int64_t)i * a.C;
  float* o = out + row * a.C;
  for (int k = 0; k < a.C; ++k) o[k] = q[k];
}

// grid (S, B): the points of candidate s of frame b, if valid, to rows new_off[b] + cand_rows[b, s] + p
__global__ __launch_bounds__(64) void gs_objects(const float* __restrict__ cand, const int* __restrict__ cand_obj, int S,
                                                 const unsigned char* __restrict__ valid, const int* __restrict__ cand_rows,
                                                 const float* __restrict__ db_points, const int* __restrict__ obj_off,
                                                 int num_objects, int C, const int* __restrict__ new_off, float* __restrict__ out,
                                                 int64_t capacity) {
  const int s = blockIdx.x, b = blockIdx.y;
  const int64_t cs = (int64_t)b * S + s;
  if (!valid[cs]) return;
  const int o = cand_obj[cs];
  if (o < 0 || o >= num_objects) return;
  const int p0 = obj_off[o], np = obj_off[o + 1] - p0;
  const float* rec = cand + cs * GS_REC;
  const float shift = rec[8], ox = rec[17], oy = rec[18], oz = rec[19];
  const int64_t row0 = (int64_t)new_off[b] + cand_rows[cs];
  for (int p = threadIdx.x; p < np; p += 64) {
    const int64_t row = row0 + p;
    if (row < 0 || row >= capacity) continue;
    const float* q = db_points + (int64_t)(p0 + p) * C;
    float* w = out + row * C;
    w[0] = __fadd_rn(q[0], ox);
    w[1] = __fadd_rn(q[1], oy);
    float z = __fadd_rn(q[2], oz);
    if (shift != 0.f) z = __fsub_rn(z, shift);
    w[2] = z;
    for (int k = 3; k < C; ++k) w[k] = q[k];
  }
}

}  // namespace

extern "C" int crb_gt_sample_select(const float* gt_boxes, const int32_t* gt_counts, int B, int G, const float* cand,
                                    const int32_t* cand_obj, const int32_t* group_offsets, int S, int K,
                                    const int32_t* obj_offsets, int64_t num_objects, uint8_t* valid, float* out_boxes,
                                    int32_t* new_counts, int32_t* cand_rows, int32_t* paste_counts, void* stream) {
  if (B <= 0 || G < 0 || S < 0 || K < 0 || num_objects < 0 || num_objects >= (int64_t)0x7fffffff || !gt_counts || !group_offsets ||
      !obj_offsets || !new_counts || !paste_counts)
    return CRB_ERR_ARG;
  if (S > GS_MAX_S || G + S > GS_MAX_BOXES) return CRB_ERR_UNSUPPORTED;
  if (G > 0 && !gt_boxes) return CRB_ERR_ARG;
  if (S > 0 && (!cand || !cand_obj || !valid || !cand_rows)) return CRB_ERR_ARG;
  if (G + S > 0 && (!out_boxes || out_boxes == gt_boxes)) return CRB_ERR_ARG;
  hipLaunchKernelGGL(gs_select, dim3(B), dim3(256), 0, (hipStream_t)stream, gt_boxes, gt_counts, G, cand, cand_obj, group_offsets, S,
                     K, obj_offsets, (int)num_objects, valid, out_boxes, new_counts, cand_rows, paste_counts);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}

extern "C" int64_t crb_gt_sample_paste_workspace_bytes(int64_t n_points, int B) {
  if (n_points < 0) n_points = 0;
  if (B < 0) B = 0;
  return crb_align_up((int64_t)(crb_cdiv(n_points, 256) + 1) * 4, 256) + crb_align_up((int64_t)(B + 2) * 4, 256) + 256;
}

extern "C" int crb_gt_sample_paste(const float* points, int64_t n_points, int num_features, const int32_t* frame_offsets, int B,
                                   const float* cand, const int32_t* cand_obj, int S, const uint8_t* valid,
                                   const int32_t* cand_rows, const int32_t* paste_counts, const float* db_points,
                                   const int32_t* obj_offsets, int64_t num_objects, int64_t capacity, float* out_points,
                                   int32_t* new_frame_offsets, void* workspace, int64_t workspace_bytes, void* stream) {
  if (n_points < 0 || n_points >= (int64_t)0x7fffff00 || capacity < n_points || capacity >= (int64_t)0x7fffff00 || B <= 0 ||
      B > 65535 || num_features < 3 || S < 0 || S > GS_MAX_S || num_objects < 0 || num_objects >= (int64_t)0x7fffffff ||
      !frame_offsets || !paste_counts || !obj_offsets || !new_frame_offsets)
    return CRB_ERR_ARG;
  if (n_points > 0 && !points) return CRB_ERR_ARG;
  if (capacity > 0 && !out_points) return CRB_ERR_ARG;
  if (S > 0 && (!cand || !cand_obj || !valid || !cand_rows)) return CRB_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int n = (int)n_points;
  const int blocks = crb_cdiv(n, 256);
  CrbArena arena(workspace, (size_t)workspace_bytes);
  int* block_counts = arena.take<int>(blocks + 1);
  int* paste_prefix = arena.take<int>(B + 2);
  if (!arena.ok) return CRB_ERR_WORKSPACE;
  GsScene a;
  a.pts = points; a.n = n; a.C = num_features; a.B = B; a.S = S;
  a.frame_off = frame_offsets; a.cand = cand; a.valid = valid;
  if (blocks > 0) hipLaunchKernelGGL(gs_count, dim3(blocks), dim3(256), 0, st, a, block_counts);
  hipLaunchKernelGGL(gs_scan, dim3(1), dim3(256), 0, st, block_counts, blocks, frame_offsets, B, n, paste_counts, paste_prefix,
                     new_frame_offsets, (int)capacity);
  if (blocks > 0)
    hipLaunchKernelGGL(gs_emit, dim3(blocks), dim3(256), 0, st, a, (const int*)block_counts, (const int*)paste_prefix, out_points,
                       capacity, new_frame_offsets);
  if (S > 0 && db_points)
    hipLaunchKernelGGL(gs_objects, dim3(S, B), dim3(64), 0, st, cand, cand_obj, S, valid, cand_rows, db_points, obj_offsets,
                       (int)num_objects, num_features, (const int*)new_frame_offsets, out_points, capacity);
  CRB_CHECK_LAUNCH();
  return CRB_OK;
}
