/*
 * libcrbhip.so — C-ABI of the MI355X (gfx950) hot path of CRB-active-3Ddet.
 *
 * Every entry point: plain device pointers + sizes, caller-owned outputs AND workspace, launches on the
 * hipStream_t passed as `void* stream`, never synchronises unless stated, returns 0 or a negative
 * CRB_ERR_* code (never exit()). No torch / pybind types cross this boundary.
 *
 * Each declaration cites the reference interface (file:line under the upstream tree) it replaces.
 * The Python host side (crb-active-3ddet_amd/crbhip/_lib.py) binds these with ctypes; INTEGRATION.md
 * shows the stub a pcdet maintainer would add.
 */
#ifndef CRB_HIP_H
#define CRB_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRB_OK 0
#define CRB_ERR_ARG (-1)
#define CRB_ERR_WORKSPACE (-2)
#define CRB_ERR_LAUNCH (-3)
#define CRB_ERR_UNSUPPORTED (-4)

/* ABI version of this header; bumped on any signature change. */
int crb_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * a1/a2/a3  VoxelGenerator (+ collate + MeanVFE)
 * replaces: spconv.utils.Point2VoxelCPU3d.point_to_voxel as called from
 *           pcdet/datasets/processor/data_processor.py:44-60 (VoxelGeneratorWrapper.generate),
 *           the voxel concat / batch-index pad of pcdet/datasets/dataset.py:160-229 (collate_batch),
 *           and pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31 (MeanVFE.forward) when mean_features != NULL.
 *
 * points          (n_points, num_features) f32, frames concatenated, xyz first
 * frame_offsets   (B+1) i32 device, frame b owns points [off[b], off[b+1])
 * range_min_xyz / voxel_size_xyz / grid_xyz : HOST arrays of 3
 * outputs sized for cap = min(B*max_voxels, n_points) rows:
 *   voxels (cap, max_points, num_features) f32 or NULL; coords (cap,4) i32 [b,z,y,x];
 *   num_points (cap) i32; mean_features (cap, num_features) f32 or NULL;
 *   num_voxels_out (B+1) i32 device: per-frame kept voxel count, [B] = total rows written.
 * Rows beyond the total are left untouched.
 * ---------------------------------------------------------------------------------------------- */
int64_t crb_voxelize_workspace_bytes(int64_t n_points, int B, int max_voxels, int max_points);
int crb_voxelize(const float* points, int64_t n_points, int num_features,
                 const int32_t* frame_offsets, int B,
                 const float* range_min_xyz, const float* voxel_size_xyz, const int32_t* grid_xyz,
                 int max_voxels, int max_points,
                 float* voxels, int32_t* coords, int32_t* num_points, float* mean_features,
                 int32_t* num_voxels_out,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a0  World augmentation (+ range mask + frame concat) for a batch of training frames
 * replaces: pcdet/datasets/augmentor/augmentor_utils.py:8-81 (random_flip_along_x / _y, global_rotation, global_scaling) and
 *           :124-175 (random_translation_along_x / _y / _z) as queued by pcdet/datasets/augmentor/data_augmentor.py:43-117 and
 *           finished by :229-258 (limit_period of the heading), then pcdet/datasets/processor/data_processor.py:78-91
 *           (mask_points_and_boxes_outside_range) with pcdet/utils/common_utils.py:60-63 (mask_points_by_range) and
 *           pcdet/utils/box_utils.py:56-72 (mask_boxes_outside_range_numpy, corners of :28-53), and the frame-index column of
 *           pcdet/datasets/dataset.py:160-229 (collate_batch).
 *
 * params (B, 8) f32 device, 16-byte aligned, one row per frame: [flip_x, flip_y, c, s, scale, tx, ty, tz]. flip_* != 0 flips;
 *   c = f32(cos a), s = f32(sin a) of the drawn angle a. The random draws are the caller's (host, np.random). Steps run in the fixed
 *   order flip x (y = -y), flip y (x = -x), rotation (x' = x c - y s, y' = x s + y c), scaling (xyz *= scale), translation; f32,
 *   one rounding per operation. A step at its identity value (flip 0, (c, s) = (1, 0), scale 1, offset 0) is skipped, so identity
 *   parameters reproduce every bit of the input. range6: HOST array [x0, y0, z0, x1, y1, z1].
 *
 * crb_augment_mask_points: points = n_points rows, row_stride floats apart, xyz at column xyz_col followed by num_features - 3
 *   feature columns that pass through (xyz_col = 0: raw (N, C) rows; 1: the batch layout (N, 1 + C)); frame_offsets (B+1) i32
 *   device. Each transformed point is kept if !do_mask or x0 <= x <= x1 and y0 <= y <= y1 (x and y only, bounds inclusive).
 *   Kept rows go to out_points in their original order, frame after frame, as dense rows of out_frame_col + num_features floats
 *   (out_frame_col = 1: column 0 = frame index as f32); out_points holds n_points rows, rows past the total stay untouched.
 *   new_frame_offsets (B+1) i32 device: offsets of the kept rows, [B] = total. Three launches, no atomics: same bits every call.
 * crb_augment_boxes: gt_boxes (B, G, W) f32, W = 8 or 10: W - 1 box coordinates [x, y, z, dx, dy, dz, heading, (vx, vy)] + class;
 *   counts (B) i32: valid rows per frame, the rest is padding. Centre, size, heading and velocity get the same transforms
 *   (flip x: heading = -heading, vy = -vy; flip y: heading = -(heading + f32(pi)), vx = -vx; rotation: heading += rot_angles[b],
 *   the f32 of the drawn angle, (vx, vy) rotated; scaling: columns 0..5), then heading = h - floor(h / f32(2 pi) + 0.5) * f32(2 pi),
 *   then, if do_mask, boxes with fewer than min_num_corners corners inside range6 on all three axes are removed (corners:
 *   size * (+-0.5) rotated by c = f32(cos((double)heading)), s = f32(sin((double)heading)), plus the centre). Kept rows are compacted
 *   in order inside each frame of out_boxes (B, G, W) (must not alias gt_boxes), all other rows are zero; new_counts (B) i32.
 *   rot_angles (B) f32 device or NULL (= 0). One launch.
 * ---------------------------------------------------------------------------------------------- */
int64_t crb_augment_mask_points_workspace_bytes(int64_t n_points, int B);
int crb_augment_mask_points(const float* points, int64_t n_points, int64_t row_stride, int xyz_col, int num_features,
                            const int32_t* frame_offsets, int B, const float* params, const float* range6, int do_mask,
                            float* out_points, int out_frame_col, int32_t* new_frame_offsets,
                            void* workspace, int64_t workspace_bytes, void* stream);
int crb_augment_boxes(const float* gt_boxes, const int32_t* counts, int B, int G, int W, const float* params,
                      const float* rot_angles, const float* range6, int do_mask, int min_num_corners,
                      float* out_boxes, int32_t* new_counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a0' gt_sampling for a batch of training frames: collision test of the drawn database objects, paste of the accepted ones
 * replaces: pcdet/datasets/augmentor/database_sampler.py:150-234 (the IoU tests of DataBaseSampler.__call__ and
 *           add_sampled_boxes_to_scene) with pcdet/ops/iou3d_nms/src/iou3d_cpu.cpp:232-252 (boxes_iou_bev_cpu),
 *           pcdet/utils/box_utils.py:75-89,145-158 (remove_points_in_boxes3d, enlarge_box3d) and
 *           pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-167 (points_in_boxes_cpu, the CPU twin's rule).
 *
 * The candidate walk (sample_with_fixed_number, np.random) and the arithmetic on the candidate boxes are the caller's (host).
 * cand (B, S, 20) f32 device, one record per candidate, a frame's candidates group after group in the order of SAMPLE_GROUPS:
 *   [0..6]   x, y, z, dx, dy, dz, heading as they enter the collision test (after the fake-lidar conversion, before the road plane)
 *   [7]      class as f32            [8] shift: road-plane z shift of the object, 0 when unused
 *   [9..16]  removal box: cx, cy, cz (z - shift), dx, dy, dz (+ REMOVE_EXTRA_WIDTH), cosa = f32(cos(-(double)rz)),
 *            sina = f32(sin(-(double)rz))
 *   [17..19] offset added to the object's database points (xyz of the database box)
 * cand_obj (B, S) i32 device: database object of each candidate; group_offsets (B, K + 1) i32 device: candidates [off[k], off[k+1])
 *   of a frame form group k, off[K] = the frame's candidate count (<= S, the rest of the frame's S records is padding).
 * Database: db_points (P, num_features) f32 with xyz relative to the box centre, obj_offsets (num_objects + 1) i32, both device.
 *
 * crb_gt_sample_select: gt_boxes (B, G, 8) f32 [x, y, z, dx, dy, dz, heading, class] with gt_counts (B) i32 valid rows. One
 *   workgroup per frame walks the groups in order. Candidate s of group k is valid iff iou(s, o) == 0.0f for every box o existing
 *   when group k is tested (the frame's own boxes and the valid candidates of earlier groups) and for every other candidate o of
 *   group k; iou is the rotated BEV IoU of crb_boxes_pairwise(mode 1), the very same device function, candidate first. So two
 *   candidates of one group that touch each other are both dropped, and a candidate whose only overlap is with a dropped candidate
 *   of an earlier group is accepted.
 *   valid (B, S) u8 (padding 0). out_boxes (B, G + S, 8): the frame's own rows, behind them the valid candidates in candidate order
 *   as [x, y, z - shift, dx, dy, dz, heading, class] (one f32 subtraction), the rest zero; new_counts (B) i32.
 *   cand_rows (B, S) i32: first row of a valid candidate's points inside its frame's pasted block (exclusive scan of the point counts
 *   of the valid candidates in candidate order), -1 for the others; paste_counts (B) i32: pasted rows per frame.
 *   Capacity: S <= 256 and G + S <= 512, else CRB_ERR_UNSUPPORTED. One launch.
 * crb_gt_sample_paste: points (n_points, num_features) f32 dense rows, frame_offsets (B+1) i32. Output rows, frame after frame:
 *   first the points of the frame's valid candidates in candidate order - database row with x + ox, y + oy, z + oz (separate f32
 *   additions) and then z - shift (one more f32 subtraction, skipped when shift == 0), features copied - then the frame's own
 *   points that lie in no valid candidate's removal box, in their original order, unchanged. A point is inside a removal box iff
 *   !(fabsf(z - cz) > dz / 2) and, with sx = x - cx, sy = y - cy, lx = sx * cosa + sy * (-sina), ly = sx * sina + sy * cosa (every f32
 *   product and sum rounded once, no FMA), (double)fabsf(lx) < (double)dx / 2 + (double)1e-2f and the same for ly / dy.
 *   out_points holds `capacity` rows (>= n_points + the point counts of ALL candidates, which the host knows: no read-back); rows past
 *   the total stay untouched. new_frame_offsets (B + 2) i32: offsets of the frames' rows, [B] = total, [B + 1] = capacity - to a
 *   consumer that takes its row count from the host (crb_augment_mask_points) the untouched tail is one more frame whose rows land
 *   behind the total. Count, scan and emit launches plus one for the objects, no atomics: the same bits every call.
 * ---------------------------------------------------------------------------------------------- */
int crb_gt_sample_select(const float* gt_boxes, const int32_t* gt_counts, int B, int G, const float* cand,
                         const int32_t* cand_obj, const int32_t* group_offsets, int S, int K,
                         const int32_t* obj_offsets, int64_t num_objects, uint8_t* valid, float* out_boxes,
                         int32_t* new_counts, int32_t* cand_rows, int32_t* paste_counts, void* stream);
int64_t crb_gt_sample_paste_workspace_bytes(int64_t n_points, int B);
int crb_gt_sample_paste(const float* points, int64_t n_points, int num_features, const int32_t* frame_offsets, int B,
                        const float* cand, const int32_t* cand_obj, int S, const uint8_t* valid,
                        const int32_t* cand_rows, const int32_t* paste_counts, const float* db_points,
                        const int32_t* obj_offsets, int64_t num_objects, int64_t capacity, float* out_points,
                        int32_t* new_frame_offsets, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a4  Sparse 3D convolution: rulebooks + gather-GEMM fwd / dgrad / wgrad
 * replaces: spconv.pytorch.SubMConv3d / SparseConv3d / SparseConvTensor (third-party spconv-cu113 v2.1.21,
 *           not vendored) as used by pcdet/models/backbones_3d/spconv_backbone.py:8-27,77-117,141-157 and
 *           pcdet/utils/spconv_utils.py:3-34.
 *
 * coords (N,4) i32 [b,z,y,x]; shape_dhw = spatial shape [D,H,W] (HOST int32[3]); ksize/stride/padding HOST int32[3].
 * Kernel offset index o = (kz*KH + ky)*KW + kx; weights are (K, Cin, Cout) f32 contiguous.
 * ---------------------------------------------------------------------------------------------- */
int64_t crb_hash_capacity_for(int64_t n);   /* power of two >= 2n */
/* site -> row hash for a coordinate set in ANY row order (the voxelizer's output): hkeys (capacity) i64, hvals (capacity) i32.
 * Slots are grouped by 8 consecutive x-sites (slot = group(site / 8) * 8 + site % 8, whole groups probe linearly), so the
 * three x-neighbours of a kernel row usually share one 64-byte line of keys. Duplicate coordinates: the smallest row wins.
 * Consumed by crb_subm_rows; sets that come out of crb_spconv_chain_emit need no hash (rank tables). */
int crb_sparse_hash_build(const int32_t* coords, int64_t n, const int32_t* shape_dhw,
                          int64_t* hkeys, int32_t* hvals, int64_t capacity, void* stream);
/* Y (n_out,cout) = sum_o X[nbr[:,o]] @ W[o]; also used for dgrad with the transposed table / weights.
 * Optional row permutation: when perm != NULL, `nbr` holds the table rows in permuted order (nbr_sorted[s] =
 * nbr[perm[s]]) and the result of sorted row s is written to Y[perm[s]]. Sorting rows by their neighbour bit-mask
 * (crb_nbr_masks -> sort -> crb_nbr_permute) lets a wave skip every kernel offset none of its 16 rows uses. */
int crb_sparse_conv_supported(int cin, int cout);
int crb_nbr_masks(const int32_t* nbr, int64_t n, int K, int32_t* mask, void* stream);
/* stable sort of the rows of every chunk of crb_mask_sort_chunk_rows() consecutive rows by mask, DESCENDING (rows with the
 * most neighbours first) -> perm (n) */
int crb_mask_sort_chunk_rows(void);
/* sort key of crb_mask_sort_chunks: the mask with its bits re-ranked rarest offset first by frequency inside the chunk
 * (A/B alternatives: crb_hip_measure.h). The gather-GEMM's results do not depend on the row order; the MFMA tile fill does. */
int crb_mask_sort_chunks(const int32_t* mask, int64_t n, int32_t* perm, void* stream);
/* the same order for chunks of chunk_rows rows (a multiple of 1024; chunks too large for one workgroup's LDS): keys ranked
 * per chunk, then one stable device radix sort (hipCUB) of (chunk, key, row) */
int64_t crb_mask_sort_rows_workspace_bytes(int64_t n);
int crb_mask_sort_rows(const int32_t* mask, int64_t n, int chunk_rows, int32_t* perm, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* perm_out = perm_in with the full 64-row tiles of each of crb_tile_lpt_ranges() contiguous tile ranges (one per XCD, the
 * split the gather-GEMM's workgroup->tile map uses) re-ordered heaviest first; weight = kernel offsets present in any row
 * of the tile = phases its workgroup will run. A launch then ends on light tiles instead of idling behind 27-phase ones,
 * and a range's gathers stay in one XCD's L2. mask as written by crb_nbr_masks (indexed by original row). The order among
 * equal weights is arbitrary; the trailing partial tile stays last. */
int crb_tile_lpt_ranges(void);
int64_t crb_tile_lpt_workspace_bytes(int64_t n);
int crb_tile_lpt_perm(const int32_t* mask, const int32_t* perm_in, int64_t n, int32_t* perm_out, void* workspace,
                      int64_t workspace_bytes, void* stream);
int crb_nbr_permute(const int32_t* nbr, const int32_t* perm, int64_t n, int K, int32_t* nbr_sorted, void* stream);
/* Compact neighbour table of the gather-GEMM: cmask (n) u32 = kernel offsets present in row i of the KERNEL order (row
 * perm[i] of nbr; perm NULL = identity), cbase (n+1) i32 = exclusive prefix of the masks' popcounts, packed (>= cbase[n],
 * caller allocates n*K) = the present neighbour indices row after row, offsets ascending. 8 + 4 P/n bytes per row instead
 * of 4 K. crb_sparse_conv_forward_compact is crb_sparse_conv_forward on that table (bit-identical results); shapes for
 * which crb_sparse_conv_compact_supported() is 0 keep the (n,K) table. Supported: the phase kernel's shapes (Cin, Cout multiples of
 * 16, Cin <= 64) and, since round 4, the low-channel forward instance (Cin, Cout) = (4, 16) of the KITTI input layer (a wave owns a
 * 16-row tile end to end). */
int crb_sparse_conv_compact_supported(int cin, int cout);
int64_t crb_nbr_compact_workspace_bytes(int64_t n);
int crb_nbr_compact(const int32_t* nbr, const int32_t* perm, int64_t n, int K, uint32_t* cmask, int32_t* cbase,
                    int32_t* packed, void* workspace, int64_t workspace_bytes, void* stream);
/* tile_order (ceil(n_out/64)) or NULL: position -> 64-row tile of the kernel order, the heaviest-first dispatch order inside
 * each XCD's contiguous range of tiles (crb_tables_finish); results do not depend on it. */
int crb_sparse_conv_forward_compact(const float* X, const float* W, const uint32_t* cmask, const int32_t* cbase,
                                    const int32_t* packed, const int32_t* perm, const int32_t* tile_order, float* Y,
                                    int64_t n_out, int K, int cin, int cout, void* stream);

/* ---- the whole backbone's tables in ~26 launches and ONE host read-back (csrc/rulebook_plan.hip) --------------------------
 * replaces: the indice-pair generation of every spconv.pytorch.SubMConv3d / SparseConv3d of
 *   pcdet/models/backbones_3d/spconv_backbone.py:77-117 (VoxelBackBone8x: 4 SubM keys + 4 strided keys), which spconv builds
 *   layer by layer inside forward with one synchronisation per strided layer.
 * chain: output sets of a chain of strided convs (level l+1 = conv l+1 applied to level l's set). geoms = n_levels x 9 ints
 *   {k,s,p} (d,h,w), out_shapes = n_levels x 3; the bitmaps of all levels live in one caller-owned buffer, level l at word
 *   word_off[l] (n_levels+1 entries, multiples of 2048, word_off[l+1]-word_off[l] >= crb_spconv_padded_words of level l);
 *   tile_sums_all holds one int per 2048-word tile. crb_spconv_chain_mark zero-fills and marks every level and writes the
 *   per-level site counts to counts_dev (device; the caller reads them back ONCE and sizes every later buffer).
 *   crb_spconv_chain_emit: per level the coordinates (ascending (b,z,y,x), n_out[l] rows, host array of device pointers) and
 *   the rank table: 8 bytes per bitmap word {bits, rows before the word} so that site -> row is ONE load. */
int64_t crb_spconv_padded_words(int B, const int32_t* out_shape_dhw);
int crb_spconv_chain_mark(const int32_t* coords, int64_t n, int B, const int32_t* in_shape_dhw, int n_levels,
                          const int32_t* geoms, const int32_t* out_shapes, const int64_t* word_off, uint32_t* bitmap_all,
                          int32_t* tile_sums_all, int32_t* counts_dev, void* stream);
/* the same with the input row count still on the device: coords holds n_cap rows of which the first *n_dev are valid (the voxel
 * generator's coordinate buffer and its total, crb_voxelize's counts[B]). The chain is marked and counted before the host knows
 * the voxel count; ONE read-back then returns it together with the level sizes (the reference path synchronises twice here:
 * Point2VoxelCPU3d returns host arrays, spconv's indice generation returns host-side counts per strided layer). */
int crb_spconv_chain_mark_lazy(const int32_t* coords, int64_t n_cap, const int32_t* n_dev, int B, const int32_t* in_shape_dhw,
                               int n_levels, const int32_t* geoms, const int32_t* out_shapes, const int64_t* word_off,
                               uint32_t* bitmap_all, int32_t* tile_sums_all, int32_t* counts_dev, void* stream);
int crb_spconv_chain_emit(int B, int n_levels, const int32_t* out_shapes, const int64_t* word_off,
                          const uint32_t* bitmap_all, const int32_t* tile_sums_all, void* rank_all,
                          int32_t* const* out_coords, const int64_t* n_out, void* stream);
/* rows: ONE kernel per table writes the neighbour rows (n,K), mask (n) u32 = offsets present per row and hist
 * (ceil(n / crb_table_chunk_rows()), 32) i32 += per-chunk count of every offset (caller zero-fills hist).
 * crb_subm_rows: SubM table of a site set; sites are looked up in `rank` (rank table of THIS set from crb_spconv_chain_emit:
 *   rows are bitmap ranks) or, rank == NULL, in the site hash of crb_sparse_hash_build (any row order).
 * crb_spconv_rows: strided conv from the input rows `coords` to the set whose rank table is rank_out: nbr_t (n,K) = output row
 *   per (input row, offset) with its mask / hist, and nbr (n_out,K) filled by the unique writer of every entry (the launch
 *   first fills it with -1). No existence test is needed (every site an input reaches is an output).
 * crb_table_masks: mask + hist of an existing (n,K) table. */
int crb_table_chunk_rows(void);
int crb_subm_rows(const int32_t* coords, int64_t n, const int32_t* shape_dhw, const int32_t* ksize, const int64_t* hkeys,
                  const int32_t* hvals, int64_t capacity, const void* rank, int32_t* nbr, uint32_t* mask, int32_t* hist,
                  void* stream);
int crb_spconv_rows(const int32_t* coords, int64_t n, const int32_t* ksize, const int32_t* stride, const int32_t* padding,
                    const int32_t* out_shape_dhw, const void* rank_out, int64_t n_out, int32_t* nbr, int32_t* nbr_t,
                    uint32_t* mask_t, int32_t* hist_t, void* stream);
int crb_table_masks(const int32_t* nbr, int64_t n, int K, uint32_t* mask, int32_t* hist, void* stream);
/* finish: everything the kernels read, for any number of tables, in THREE launches per 16 tables (sort pass: one
 * workgroup per 4096-row chunk, register/shuffle bitonic network; fill pass: one workgroup per 256 rows; tile order).
 * per table (host array of CrbTablePlan; all pointers device, caller-owned):
 *   in : nbr (n,K), mask (n), hist (chunks,32) as written by the rows kernels
 *   out: perm (n) kernel order of the rows (every 4096-row chunk sorted by mask, rarest offset first, descending, stable);
 *        cmask (n) / cbase (n+1) / packed (>= P, caller allocates n*K) the compact table of crb_nbr_compact in that order;
 *        tile_weight / tile_order (ceil(n/64)) offsets present per 64-row tile and the heaviest-first order of the tiles
 *        inside each of the 8 XCD ranges (stable: deterministic);
 *        pair_in / pair_out (>= P) / pair_start (K+1) + workspace pair_unit_base, or all four NULL: the wgrad pair lists of
 *        wgrad kernels: pair_in / pair_out sorted by (offset, output row), pair_start[o] = first pair of offset o, [K] = P. */
typedef struct CrbTablePlan {
  const int32_t* nbr;
  const uint32_t* mask;
  const int32_t* hist;
  int32_t* perm;
  uint32_t* cmask;
  int32_t* cbase;
  int32_t* packed;
  int32_t* tile_weight;
  int32_t* tile_order;
  int32_t* pair_in;
  int32_t* pair_out;
  int32_t* pair_start;
  int32_t* pair_unit_base;      /* workspace, ceil(n/64) x 32 ints (NULL with the pair lists): first pair of every (64-row unit, offset) */
  int64_t n;
  int32_t K;
  int32_t reserved;
} CrbTablePlan;
int crb_tables_finish(const CrbTablePlan* tables, int n_tables, void* stream);

/* Inference epilogue in the gather-GEMM: y = relu(gamma * ((conv + bias - running_mean) * rsqrt(running_var + eps)) + beta),
 * i.e. the (bias,) nn.BatchNorm1d in eval mode and nn.ReLU that follow a sparse conv in post_act_block
 * (pcdet/models/backbones_3d/spconv_backbone.py:8-31), evaluated on the accumulator before the store instead of in two more
 * passes over the rows; same arithmetic order as crb_bn_relu_apply. bias may be NULL; relu 0/1. Shapes of
 * crb_sparse_conv_compact_supported only. */
int crb_sparse_conv_forward_compact_bn(const float* X, const float* W, const uint32_t* cmask, const int32_t* cbase,
                                       const int32_t* packed, const int32_t* perm, const int32_t* tile_order, float* Y,
                                       int64_t n_out, int K, int cin, int cout, const float* bias, const float* gamma, const float* beta,
                                       const float* running_mean, const float* running_var, float eps, int relu,
                                       void* stream);

/* the weight layouts of n <= 32 layers in one launch: w[j] = a spconv layer's parameter (Cout_j, K_j, Cin_j) contiguous (spconv 2.x
 * checkpoint layout, spconv/pytorch/conv.py) -> w_kio[j] (K, Cin, Cout) = the forward operand W[o] of crb_sparse_conv_forward*, and
 * w_dgrad[j] (K, Cout, Cin) (NULL = not wanted) = the input gradient's operand: W[o]^T, at K-1-o when flip[j] (submanifold layers).
 * Replaces a permuted copy per layer forward and a flip + transposed copy per layer backward. Host arrays of pointers / ints. */
int crb_sparse_weights_multi(int n, const float* const* w, const int32_t* K, const int32_t* cin, const int32_t* cout,
                             const int32_t* flip, float* const* w_kio, float* const* w_dgrad, void* stream);
int crb_sparse_conv_forward(const float* X, const float* W, const int32_t* nbr, const int32_t* perm, float* Y,
                            int64_t n_out, int K, int cin, int cout, void* stream);
/* dW (K,cin,cout) = sum over pairs X[pin]^T dY[pout] */
int crb_sparse_conv_wgrad_splits(void);
int crb_sparse_conv_wgrad_occupancy(int cin, int cout); /* measurement helper: resident workgroups per CU of the v2 wgrad instance */
int64_t crb_sparse_conv_wgrad_workspace_bytes(int K, int cin, int cout);
/* Windowed wgrad (tiles of <= 4 blocks of 32x32): work is cut by WINDOWS OF OUTPUT ROWS instead of per-offset pair ranges —
 * XCD x owns the x-th eighth of the rows, all kernel offsets' workgroups of an XCD walk the same window at the same time,
 * so gathered rows are served by the XCD's L2 instead of being fetched once per offset. bounds (K, crb_wgrad_num_windows()+1)
 * = first pair of every window per offset (crb_wgrad_window_bounds, once per rulebook; pair_out ascending inside an offset).
 * Same deterministic partial + fixed-order reduction scheme as crb_sparse_conv_wgrad, same result up to f32 summation
 * order. */
int crb_wgrad_num_windows(void);
int crb_wgrad_window_bounds(const int32_t* pair_out, const int32_t* pair_start, int K, int64_t n_out, int32_t* bounds,
                            void* stream);
int crb_sparse_conv_wgrad_windowed_supported(int cin, int cout);
int64_t crb_sparse_conv_wgrad_windowed_workspace_bytes(int K, int cin, int cout);
int crb_sparse_conv_wgrad_windowed(const float* X, const float* dY, const int32_t* pair_in, const int32_t* pair_out,
                                   const int32_t* pair_start, const int32_t* bounds, float* dW, int K, int cin, int cout,
                                   void* workspace, int64_t workspace_bytes, void* stream);
int crb_sparse_conv_wgrad(const float* X, const float* dY, const int32_t* pair_in, const int32_t* pair_out,
                          const int32_t* pair_start, float* dW, int K, int cin, int cout,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a6  SparseConvTensor.dense() and its backward
 * replaces: spconv SparseConvTensor.dense() as used by
 *           pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-24.
 * out (B,C,D,H,W) f32. zero_fill != 0 clears `out` first.
 * ---------------------------------------------------------------------------------------------- */
int crb_sparse_to_dense(const float* feat, const int32_t* coords, float* out, int64_t n, int B, int C,
                        int D, int H, int W, int zero_fill, void* stream);
int crb_dense_to_sparse(const float* dense, const int32_t* coords, float* feat, int64_t n, int B, int C,
                        int D, int H, int W, void* stream);
/* same, BEV channels-last memory: out is (B, H, W, C*D) with channel index c*D + z — the layout of a
 * torch (B, C*D, H, W) tensor in channels_last format, i.e. HeightCompression's view without NCHW<->NHWC transposes */
int crb_sparse_to_dense_nhwc(const float* feat, const int32_t* coords, float* out, int64_t n, int B, int C,
                             int D, int H, int W, int zero_fill, void* stream);
int crb_dense_to_sparse_nhwc(const float* dense, const int32_t* coords, float* feat, int64_t n, int B, int C,
                             int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a13/a14  rotated BEV overlap / IoU / 3-D IoU and NMS
 * replaces: the pybind surface of pcdet/ops/iou3d_nms/src/iou3d_nms_api.cpp:11-17
 *   boxes_overlap_bev_gpu (iou3d_nms.cpp:46-66)  -> crb_boxes_pairwise(mode 0)
 *   boxes_iou_bev_gpu     (iou3d_nms.cpp:68-88)  -> crb_boxes_pairwise(mode 1)
 *   boxes_iou3d_gpu       (iou3d_nms_utils.py:48-81, fused) -> crb_boxes_pairwise(mode 2)
 *   nms_gpu / nms_normal_gpu (iou3d_nms.cpp:90-185: device mask + D2H + host greedy scan) -> crb_nms_batched
 * boxes are (n,7) f32 [x,y,z,dx,dy,dz,heading]; out (na,nb) f32.
 * crb_nms_batched: boxes_sorted (B,nmax,7) already in descending score order, counts (B) i32 device or NULL (= nmax
 * everywhere); keep (B,max_keep) i32 indices into the sorted order, -1 padded; num_keep (B) i32. Greedy scan runs on
 * the device; no synchronisation. workspace >= crb_nms_workspace_bytes(B,nmax).
 * ---------------------------------------------------------------------------------------------- */
int crb_boxes_pairwise(const float* boxes_a, int64_t na, const float* boxes_b, int64_t nb, float* out,
                       int mode, void* stream);
int64_t crb_nms_workspace_bytes(int B, int64_t nmax);
int crb_nms_batched(const float* boxes_sorted, const int32_t* counts, int B, int64_t nmax, float thresh,
                    int rotated, int max_keep, int32_t* keep, int32_t* num_keep, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a16-a18  PointNet++ stack ops
 * replaces: the pybind surface of pcdet/ops/pointnet2/pointnet2_stack/src/pointnet2_api.cpp:12-31
 *   ball_query_wrapper (ball_query.cpp:31-47), group_points_wrapper / group_points_grad_wrapper
 *   (group_points.cpp), farthest_point_sampling_wrapper (sampling.cpp), three_nn_wrapper,
 *   three_interpolate_wrapper / three_interpolate_grad_wrapper (interpolate.cpp).
 * Stacked layout: xyz (N1+N2+..,3) f32 + *_batch_cnt (B) i32 on the device; idx int32.
 * ball query: idx (M,nsample): hits in scan order, padded with the first hit; empty ball: idx[m][0] = -1, rest 0.
 * grad kernels accumulate with atomics into PRE-ZEROED outputs.
 * ---------------------------------------------------------------------------------------------- */
int crb_ball_query_stack(int B, int64_t M, float radius, int nsample, const float* new_xyz,
                         const int32_t* new_xyz_batch_cnt, const float* xyz, const int32_t* xyz_batch_cnt,
                         int32_t* idx, void* stream);
/* two radii, same centres, one scan. idx_a (M,nsample_a) / idx_b (M,nsample_b) already in the grouping kernels' form (an
 * empty ball is all zeros, flagged in empty_a / empty_b (M) u8): replaces two ball_query_wrapper calls plus the Python
 * fix-up `empty = idx[:,0]==-1; idx[empty]=0` (pointnet2_utils.py:31-38) */
int crb_ball_query2_stack(int B, int64_t M, float radius_a, int nsample_a, float radius_b, int nsample_b,
                          const float* new_xyz, const int32_t* new_xyz_batch_cnt, const float* xyz,
                          const int32_t* xyz_batch_cnt, int32_t* idx_a, int32_t* idx_b, uint8_t* empty_a,
                          uint8_t* empty_b, void* stream);
/* crb_ball_query2_stack on a per-call cell grid (round 6): the call's source points are counting-sorted into a hashed grid of cells
 * of edge 1.001 radius_b (histogram, exclusive scan, cursor fill), a query tests the points of the 27 cells around its own and
 * keeps the nsample smallest indices of each radius in ascending order - the lists of crb_ball_query2_stack, index for index
 * (replaces the same ball_query_wrapper calls, pointnet2_utils.py:31-38 / ball_query_gpu.cu:47-66: hits in scan order, first
 * nsample, padded with the first hit). radius_a <= radius_b. n_total = rows of xyz. workspace: crb_ball_query2_grid_workspace_bytes. */
int64_t crb_ball_query2_grid_workspace_bytes(int64_t n_total);
int crb_ball_query2_grid_stack(int B, int64_t M, float radius_a, int nsample_a, float radius_b, int nsample_b,
                               const float* new_xyz, const int32_t* new_xyz_batch_cnt, const float* xyz,
                               const int32_t* xyz_batch_cnt, int64_t n_total, int32_t* idx_a, int32_t* idx_b, uint8_t* empty_a,
                               uint8_t* empty_b, void* workspace, int64_t workspace_bytes, void* stream);
/* crb_ball_query2_stack for queries that come in spatially compact groups of `group` consecutive rows inside one frame
 * (every new_xyz_batch_cnt[b] a multiple of `group` for the fast path; a group that straddles two frames is still answered
 * correctly, by a per-query scan; the 216 grid points of one RoI in PVRCNNHead.roi_grid_pool,
 * pvrcnn_head.py:97-132, feeding pointnet2_utils.py:31-38): one workgroup per group prefilters the frame's points by the
 * group's bounding sphere, same index lists as crb_ball_query2_stack. */
int crb_ball_query2_grouped_stack(int B, int64_t M, int group, float radius_a, int nsample_a, float radius_b, int nsample_b,
                                  const float* new_xyz, const int32_t* new_xyz_batch_cnt, const float* xyz,
                                  const int32_t* xyz_batch_cnt, int32_t* idx_a, int32_t* idx_b, uint8_t* empty_a,
                                  uint8_t* empty_b, void* stream);
int crb_group_points_stack(int B, int64_t M, int C, int nsample, const float* features,
                           const int32_t* features_batch_cnt, const int32_t* idx,
                           const int32_t* idx_batch_cnt, float* out, void* stream);
int crb_group_points_grad_stack(int B, int64_t M, int C, int nsample, const float* grad_out,
                                const int32_t* idx, const int32_t* idx_batch_cnt,
                                const int32_t* features_batch_cnt, float* grad_features, void* stream);
/* fused QueryAndGroup (pointnet2_utils.py:107-155) in the layout the shared MLP consumes: out (3+C, M, nsample) =
 * [xyz[nbr]-new_xyz ; features[nbr]] per (query, sample), zero for empty balls (empty_mask (M) u8). idx as returned by
 * crb_ball_query_stack after the empty fix-up. grad: features only, atomics into a pre-zeroed (N,C) buffer. */
int crb_query_group_stack(int B, int64_t M, int C, int nsample, const float* xyz,
                          const int32_t* xyz_batch_cnt, const float* features, const float* new_xyz,
                          const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                          float* out, void* stream);
int crb_query_group_grad_stack(int B, int64_t M, int C, int nsample, const int32_t* xyz_batch_cnt,
                               const int32_t* new_xyz_batch_cnt, const int32_t* idx,
                               const uint8_t* empty_mask, const float* grad_out,
                               float* grad_features, void* stream);
/* the same grouping in row-major layout, out (M*nsample, 3+C): the training path runs the shared MLP as GEMMs + fused
 * BatchNorm/ReLU row kernels on it. The grad kernel pre-sums pairs that share a source row inside a workgroup (ball-query
 * padding repeats the first hit) before its atomics. */
int crb_query_group_rows_stack(int B, int64_t M, int C, int nsample, const float* xyz,
                               const int32_t* xyz_batch_cnt, const float* features, const float* new_xyz,
                               const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                               float* out, void* stream);
int crb_query_group_rows_grad_stack(int B, int64_t M, int C, int nsample, const int32_t* xyz_batch_cnt,
                                    const int32_t* new_xyz_batch_cnt, const int32_t* idx,
                                    const uint8_t* empty_mask, const float* grad_out, float* grad_features,
                                    void* stream);
/* training path, first shared-MLP layer without the grouped matrix: for a bias-free 1x1 conv on QueryAndGroup's output
 * (pointnet2_utils.py:107-155 feeding pointnet2_modules.py:94-97), y[p] = W1x (xyz_j - c_i) + P[j] with P = features @ W1f^T
 * (N,H) computed by the caller. out (M*nsample, H) row-major, rel (M*nsample, 3) = xyz_j - c_i (0 for empty balls, whose
 * rows of out are 0 like the reference's zeroed groups). The grad entry accumulates grad_P (N,H, pre-zeroed) and writes
 * part (crb_group_affine_rows_grad_blocks(M,nsample), 3, H): per-slab pieces of dW1x, summed by the caller. */
int crb_group_affine_rows_stack(int B, int64_t M, int H, int nsample, const float* xyz, const int32_t* xyz_batch_cnt,
                                const float* P, const float* new_xyz, const int32_t* new_xyz_batch_cnt,
                                const int32_t* idx, const uint8_t* empty_mask, const float* W1x, float* out, float* rel,
                                void* stream);
/* forward that also writes stat (crb_group_affine_rows_grad_blocks(M,nsample), 2, H): the column sums of out and out^2 of every
 * 64-row slab — the statistics pass of the BatchNorm that follows (crb_bn_relu_forward_partials) then reads those instead of
 * the (M*nsample, H) rows. H in {16, 32, 64, 128}. */
int crb_group_affine_rows_stats_stack(int B, int64_t M, int H, int nsample, const float* xyz, const int32_t* xyz_batch_cnt,
                                      const float* P, const float* new_xyz, const int32_t* new_xyz_batch_cnt,
                                      const int32_t* idx, const uint8_t* empty_mask, const float* W1x, float* out, float* rel,
                                      float* stat, void* stream);
int64_t crb_group_affine_rows_grad_blocks(int64_t M, int nsample);
/* the grad entry with the BatchNorm(+ReLU) backward of the layer's output folded into its slab loads (the BatchNorm2d + ReLU
 * that follow the first conv of a shared MLP, pointnet2_modules.py:94-99): grad_z = gradient w.r.t. relu(batchnorm(y)),
 * y = the forward's `out`, mean / invstd the batch statistics, dbeta / dgamma the reduced gradients (crb_bn_relu_backward with
 * dx = NULL): dy = gamma invstd (d - dbeta/n - xhat dgamma/n), d = grad_z [z > 0], n = M*nsample, is formed in registers — the
 * (M*nsample, H) gradient of y is neither written nor read. */
int crb_group_affine_rows_grad_bn_stack(int B, int64_t M, int H, int nsample, const int32_t* xyz_batch_cnt,
                                        const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                                        const float* rel, const float* grad_z, const float* y, const float* mean,
                                        const float* invstd, const float* gamma, const float* beta, const float* dbeta,
                                        const float* dgamma, float* grad_P, float* part, void* stream);
int crb_group_affine_rows_grad_stack(int B, int64_t M, int H, int nsample, const int32_t* xyz_batch_cnt,
                                     const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                                     const float* rel, const float* grad_out, float* grad_P, float* part, void* stream);
/* inference-only fused set abstraction: replaces the body of StackSAModuleMSG.forward
 * (pointnet2_modules.py:73-112: QueryAndGroup -> 2 x [Conv2d 1x1 + BatchNorm2d + ReLU] -> max_pool2d over nsample) for one
 * radius. BN is folded by the caller; layer 1 is split as W1 [dxyz ; f] = W1x dxyz + P[row], P = features @ W1f^T (N,h1).
 * W1x (3,h1), b1 (h1), W2 (h1,h2) [k][n], b2 (h2); idx / empty_mask as for crb_query_group_stack; writes
 * out[m*out_stride + n], n < h2 (out may point into a wider (M, sum h2) buffer). h1,h2 in {16,32,64}. */
int crb_sa_mlp2_max_supported(int h1, int h2);
int crb_sa_mlp2_max_stack(int B, int64_t M, int nsample, int h1, int h2, const float* xyz,
                          const int32_t* xyz_batch_cnt, const float* P, const float* new_xyz,
                          const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                          const float* W1x, const float* b1, const float* W2, const float* b2, float* out,
                          int out_stride, void* stream);
/* TRAINING-mode fused set abstraction of one radius (round 5): the body of StackSAModuleMSG.forward for a two-layer shared MLP
 * (pointnet2_modules.py:90-108: Conv2d 1x1 -> BatchNorm2d -> ReLU -> Conv2d 1x1 -> BatchNorm2d -> ReLU -> max_pool2d over nsample;
 * RoI-grid pooling: pvrcnn_head.py:102-113) without any (M*nsample, h) activation in memory. Train-mode BatchNorm needs the
 * full-tensor statistics of a layer before the next one can run, so the forward is three recompute passes over the ball-query
 * result:  (0) crb_group_affine_rows_stats_stack with out = rel = NULL -> slab sums of y1 -> crb_bn_relu_forward_partials(z = NULL);
 * (A) crb_sa_mlp2_train_stats -> wave_sums (crb_sa_mlp2_train_waves(M), 2, h2): column sums of y2, y2^2 per wave ->
 * crb_bn_relu_forward_partials(z = NULL);  (B) crb_sa_mlp2_train_max -> out[m*out_row_stride + c] = max over the samples of
 * relu(bn2(y2)), arg (M,h2) = the sample that attains it (lowest index on ties, as crb_bn_relu_max_forward), y_sel (M,h2) = y2 there.
 * W1x (3,h1), W2 (h2,h1) = the second conv's weight, P = features @ W1f^T (N,h1), mean / invstd = batch statistics,
 * gamma / beta = the BatchNorm parameters. h1, h2 in {16,32,64}, nsample a multiple of 16, M*nsample < 2^31. */
int crb_sa_mlp2_train_supported(int h1, int h2, int nsample);
int64_t crb_sa_mlp2_train_waves(int64_t M);
int crb_sa_mlp2_train_stats(int B, int64_t M, int nsample, int h1, int h2, const float* xyz,
                            const int32_t* xyz_batch_cnt, const float* P, const float* new_xyz,
                            const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                            const float* W1x, const float* mean1, const float* invstd1, const float* gamma1,
                            const float* beta1, const float* W2, float* wave_sums, void* stream);
int crb_sa_mlp2_train_max(int B, int64_t M, int nsample, int h1, int h2, const float* xyz,
                          const int32_t* xyz_batch_cnt, const float* P, const float* new_xyz,
                          const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                          const float* W1x, const float* mean1, const float* invstd1, const float* gamma1,
                          const float* beta1, const float* W2, const float* mean2, const float* invstd2,
                          const float* gamma2, const float* beta2, float* out, int64_t out_row_stride, int32_t* arg,
                          float* y_sel, void* stream);
/* backward of the above (autograd of the same module lines). Caller first reduces dbeta2 / dgamma2 from the selected entries
 * (crb_bn_relu_max_backward_sums on y_sel). This pass recomputes y1, z1, y2, forms dy2 (BatchNorm-2 backward of the max's scatter)
 * in registers, and produces: grad_z1_masked (M*nsample, h1) = (dy2 W2) [z1 > 0], dsums1 (2, h1) = its column sums and its column
 * sums times xhat1 (dbeta1, dgamma1), dW2 (h2, h1). The first layer's own backward then is
 * crb_group_affine_rows_grad_bn_recompute_stack. workspace: crb_sa_mlp2_train_backward_workspace_floats(M, h1, h2) floats. */
int64_t crb_sa_mlp2_train_backward_workspace_floats(int64_t M, int h1, int h2);
int crb_sa_mlp2_train_backward(int B, int64_t M, int nsample, int h1, int h2, const float* xyz,
                               const int32_t* xyz_batch_cnt, const float* P, const float* new_xyz,
                               const int32_t* new_xyz_batch_cnt, const int32_t* idx, const uint8_t* empty_mask,
                               const float* W1x, const float* mean1, const float* invstd1, const float* gamma1,
                               const float* beta1, const float* W2, const float* mean2, const float* invstd2,
                               const float* gamma2, const float* beta2, const float* grad_out,
                               int64_t grad_row_stride, const int32_t* arg, const float* dbeta2, const float* dgamma2,
                               float* grad_z1_masked, float* dsums1, float* dW2, float* workspace,
                               int64_t workspace_floats, void* stream);
/* crb_group_affine_rows_grad_bn_stack without the saved forward tensors: y (the first conv's output) and rel are recomputed from
 * xyz / new_xyz / P / W1x exactly as crb_group_affine_rows_stack forms them. */
int crb_group_affine_rows_grad_bn_recompute_stack(int B, int64_t M, int H, int nsample, const float* xyz,
                                                  const int32_t* xyz_batch_cnt, const float* P, const float* new_xyz,
                                                  const int32_t* new_xyz_batch_cnt, const int32_t* idx,
                                                  const uint8_t* empty_mask, const float* W1x, const float* grad_z,
                                                  const float* mean, const float* invstd, const float* gamma,
                                                  const float* beta, const float* dbeta, const float* dgamma,
                                                  const int32_t* sorted_pair, const int32_t* sorted_row, int64_t n_src,
                                                  float* grad_P, float* part, void* stream);
/* deterministic form of the call above (torch.use_deterministic_algorithms in the host mirror): what leaves a slab is added into
 * grad_P_fixed (n_src, H) int64, pre-zeroed, as round(value * scale) with 64-bit integer atomics - the sums do not depend on the
 * order in which the slabs arrive; the caller converts back (grad_P = grad_P_fixed / scale). scale: a finite f32 > 0, else CRB_ERR_ARG
 * (NaN, inf, 0 and negative values launch nothing). int64 wraps silently: scale * A * (M * nsample) < 2^63 must hold for a bound A on
 * the scattered values |gamma invstd (d - dbeta / n - xhat dgamma / n)| - every pair may hit one row. max |grad_z| * max |gamma invstd|
 * alone is no such bound; A = max |gamma invstd| * (max |grad_z| + max |dbeta| / n + max |dgamma| / sqrt(n)) is one for batch statistics
 * (|xhat| <= sqrt(n)), maxima over the rows of LIVE balls only (the others are never read and may hold anything). With scale = 2^(62 - e -
 * ceil(log2 n)), 2^e > A (sa_fixed_point_scale of the host mirror), 62 - ceil(log2 n) fractional bits remain below 2^e: 39 at the
 * RoI-grid size (7 M pairs). A NaN / Inf value converts to a finite integer: the caller checks grad_z, dbeta and dgamma first. */
int crb_group_affine_rows_grad_bn_recompute_stack_fixed(int B, int64_t M, int H, int nsample, const float* xyz,
                                                        const int32_t* xyz_batch_cnt, const float* P, const float* new_xyz,
                                                        const int32_t* new_xyz_batch_cnt, const int32_t* idx,
                                                        const uint8_t* empty_mask, const float* W1x, const float* grad_z,
                                                        const float* mean, const float* invstd, const float* gamma,
                                                        const float* beta, const float* dbeta, const float* dgamma,
                                                        const int32_t* sorted_pair, const int32_t* sorted_row, int64_t n_src,
                                                        int64_t* grad_P_fixed, float scale, float* part, void* stream);
/* optional operand of the calls above (sorted_pair / sorted_row, NULL = pair order): the (query, sample) pairs in SOURCE-ROW order,
 * stable (pairs of one row keep their order), pairs of empty balls last with sorted_row = n_src (the number of source rows). With it
 * the kernel adds the pairs of a row inside LDS and issues one row of atomics per run of a 64-pair slab instead of one per distinct
 * row of a 16-pair segment: for layers where many balls share a row (the RoI-grid scales of PV-RCNN: 7 M pairs onto 32 k keypoints,
 * 1.89 -> 0.81 ms + 0.19 ms for the sort; not for the voxel levels, where the sort costs more than it gains). Same sums, another
 * order of the float additions into grad_P. workspace: crb_pair_sort_workspace_bytes(M, nsample). */
int64_t crb_pair_sort_workspace_bytes(int64_t M, int nsample);
int crb_pair_sort_by_source(int B, int64_t M, int nsample, const int32_t* xyz_batch_cnt, const int32_t* new_xyz_batch_cnt,
                            const int32_t* idx, const uint8_t* empty_mask, int64_t n_src, int32_t* sorted_pair,
                            int32_t* sorted_row, void* workspace, int64_t workspace_bytes, void* stream);
/* rows per frame of a stacked tensor from its frame-index column (replaces the per-frame `(xyz_bs_idxs == bs_idx).sum()` of
 * voxel_set_abstraction.py:321-323, :365-367 and pvrcnn_head.py:96-98): key = the column (f32 if key_is_float else i32), `stride` elements
 * from row to row, n rows, NON-DECREASING (the stacked layout: rows of a frame together, frames in order) -> counts (B) i32.
 * Values outside [0, B) are not counted. One launch, no atomics. */
int crb_sorted_key_counts(const void* key, int key_is_float, int64_t stride, int64_t n, int B, int32_t* counts, void* stream);
/* voxel centres (common_utils.get_voxel_centers, pcdet/utils/common_utils.py:63-80): coords_zyx (n rows of 3 i32 [z,y,x], row_stride
 * elements apart: columns 1..3 of the (n,4) index tensor) -> out (n,3) xyz = (coord + 0.5) * scaled_voxel_size + range_min;
 * scaled_voxel_size[3] = voxel size x downsample factor (f32 product), range_min[3]: HOST arrays. */
int crb_voxel_centers(const int32_t* coords_zyx, int64_t row_stride, int64_t n, const float* scaled_voxel_size, const float* range_min,
                      float* out, void* stream);
/* xyz (B,n,3) -> out_idx (B,m); first pick is index 0; ties resolved like the reference kernel (see source).
 * temp: (B,n) f32 scratch for the running distances (the reference's `temp` argument); only needed for n > 40960
 * (below that the distances stay in registers) and may be NULL otherwise. */
int crb_farthest_point_sample(int B, int n, int m, const float* xyz, float* temp, int32_t* out_idx, void* stream);
int crb_three_nn_stack(int B, int64_t N, const float* unknown, const int32_t* unknown_batch_cnt,
                       const float* known, const int32_t* known_batch_cnt, float* dist2, int32_t* idx,
                       void* stream);
int crb_three_interpolate_stack(int64_t N, int C, const float* features, const int32_t* idx,
                                const float* weight, float* out, void* stream);
int crb_three_interpolate_grad_stack(int64_t N, int C, const float* grad_out, const int32_t* idx,
                                     const float* weight, float* grad_features, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a15  points-in-boxes and RoI-aware pooling
 * replaces: pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:172-177 (points_in_boxes_gpu :94-119, forward :46-70,
 *           backward :72-92).  boxes (B,T,7), pts (B,M,3) -> box_idx_of_points (B,M) i32, -1 = background.
 * pool: rois (N,7), pts (P,3), pts_feature (P,C); pts_idx_of_voxels (N,ox,oy,oz,max_pts) i32 and pooled_features
 * (N,ox,oy,oz,C) must be zero-filled by the caller; argmax (N,ox,oy,oz,C) i32. pool_method 0 = max, 1 = avg.
 * ---------------------------------------------------------------------------------------------- */
int crb_points_in_boxes(int B, int T, int M, const float* boxes, const float* pts, int32_t* box_idx_of_points,
                        void* stream);
/* GT point statistics of the CRB-patched post-processing, all frames and classes in two launches.
 * replaces: the per-frame / per-class loop of pcdet/models/detectors/detector3d_template.py:236-268 (points_in_boxes_gpu
 *           per class + `(idx == i).sum()` per unique index + torch.mean / median / var on the host side).
 * pts (N,stride) f32 rows [b,x,y,z,...] frame-sorted, frame_offsets (B+1) i32, gt_boxes (B,G,8) rows
 * [x,y,z,dx,dy,dz,heading,label] (label 0 = padding) -> stats (B,C,5) f32 {num_bbox, n_counted, mean, median, variance}
 * of the per-box point counts (boxes owning no point are not counted; when a frame has no background point for a class
 * the first counted box is dropped, as the reference's `[1:]` does). workspace: the first B*G i32 hold the per-box
 * counts afterwards (then B*C background counts). */
int64_t crb_gt_point_stats_workspace_bytes(int B, int G, int C);
int crb_gt_point_stats(int B, int G, int C, int64_t N, int stride, const float* pts, const int32_t* frame_offsets,
                       const float* gt_boxes, float* stats, void* workspace, int64_t workspace_bytes, void* stream);
int crb_roiaware_pool3d_forward(int N, int P, int C, int max_pts_each_voxel, int out_x, int out_y, int out_z,
                                const float* rois, const float* pts, const float* pts_feature,
                                int32_t* argmax, int32_t* pts_idx_of_voxels, float* pooled_features,
                                int pool_method, void* stream);
int crb_roiaware_pool3d_backward(int N, int C, int max_pts_each_voxel, int out_x, int out_y, int out_z,
                                 const int32_t* pts_idx_of_voxels, const int32_t* argmax,
                                 const float* grad_out, float* grad_in, int pool_method, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a15' RoI-aware pooling of all frames straight into the rows of the sparse RoI-grid tensor (csrc/roiaware_sparse.hip)
 * replaces: the per-frame loop of pcdet/models/roi_heads/partA2_head.py:71-89 (two RoIAwarePool3d calls per frame) and the
 *           dense -> sparse conversion at :105-117 (`pooled_part.sum(-1).nonzero()` + gather) and their backward.
 * rois (B*R,7), pts (N,3) stacked frame after frame with frame_offsets (B+1) i32, part (N,4) avg-pooled, feat (N,C)
 * max-pooled; all f32 device, 16-byte aligned rows of part. Cell membership, the first max_pts-1 points per cell in
 * ascending point index, avg and max are those of crb_roiaware_pool3d_forward. A cell becomes a ROW iff one of its kept
 * points has a non-zero part feature: for non-negative part features that is the dense rule "the f32 sum of the four
 * averages != 0" (DESIGN.md section 7 names the inputs on which the two could differ). *flag bit 0 is raised when a point
 * inside a RoI carries a negative part feature: the result then follows another rule than the dense route's and must be
 * discarded.
 *   count:  roi_counts (B*R,2) i32 = {rows, kept hits} of every RoI; zeroes and sets *flag. out_x*out_y*out_z must be
 *           <= crb_roiaware_sparse_max_cells() (per-wave LDS histogram), else CRB_ERR_UNSUPPORTED.
 *   fill:   roi_starts (B*R,2) i32 = the exclusive scan of roi_counts over the RoIs, T / H its two totals ->
 *           coords (T,4) i32 rows (b*R + r, x, y, z) in lexicographic order, row_ptr (T+1) i32, hit_pt (H) i32 point of
 *           every kept hit row after row in point order, hit_row (H) i32 its row. Every element is written.
 *   pool:   out_part (T,4), out_feat (T,C), argmax (T,C) i32 (index into the stacked points). Every element is written.
 *   backward: grad_part (N,4) / grad_feat (N,C), every element written (exact zero for a point that no row keeps); each is the
 *           sum over the point's rows in ascending row order - no float atomics, bit-identical between runs. No read-back.
 * ---------------------------------------------------------------------------------------------- */
int crb_roiaware_sparse_max_cells(void);
int crb_roiaware_sparse_count(int n_rois, int R, int B, int64_t N, int max_pts_each_voxel, int out_x, int out_y, int out_z,
                              const float* rois, const float* pts, const int32_t* frame_offsets, const float* part,
                              int32_t* roi_counts, int32_t* flag, void* stream);
int crb_roiaware_sparse_fill(int n_rois, int R, int B, int64_t N, int max_pts_each_voxel, int out_x, int out_y, int out_z,
                             const float* rois, const float* pts, const int32_t* frame_offsets, const float* part,
                             const int32_t* roi_starts, int64_t T, int64_t H, int32_t* coords, int32_t* row_ptr,
                             int32_t* hit_pt, int32_t* hit_row, void* stream);
int crb_roiaware_sparse_pool(int64_t T, int C, const int32_t* row_ptr, const int32_t* hit_pt, const float* part,
                             const float* feat, float* out_part, float* out_feat, int32_t* argmax, void* stream);
int64_t crb_roiaware_sparse_backward_workspace_bytes(int64_t N, int64_t H);
int crb_roiaware_sparse_backward(int64_t N, int64_t T, int64_t H, int C, const int32_t* row_ptr, const int32_t* hit_pt,
                                 const int32_t* hit_row, const int32_t* argmax, const float* g_part, const float* g_feat,
                                 float* grad_part, float* grad_feat, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a28  CRB stage 3: greedy point-cloud-density balancing
 * replaces: the sklearn KernelDensity / scipy.stats.entropy triple loop of
 *           pcdet/query_strategies/crb_sampling.py:276-331 (SELECT_NUMS x candidates x classes KDE fits on the CPU).
 * densities (n_candidates,dmax) f32 / labels (n_candidates,dmax) i32 (1..num_class, 0 = padding): predicted-box point
 * densities of the K2*N candidate frames in candidate order; xaxis/prior (num_class,400) f64 device: evaluation axis
 * and (un-normalised) uniform prior per class; order (select_nums) i32: picked candidate indices, first pick = 0,
 * -1 padded; best_scores (select_nums) f64 or NULL. f64 arithmetic. No synchronisation.
 * ---------------------------------------------------------------------------------------------- */
int64_t crb_density_greedy_workspace_bytes(int n_candidates, int num_class);
int crb_density_greedy(const float* densities, const int32_t* labels, int n_candidates, int dmax,
                       int num_class, const double* xaxis, const double* prior, double bandwidth,
                       int select_nums, int32_t* order, double* best_scores, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a5  fused BatchNorm1d (+ReLU) over sparse-tensor rows
 * replaces: nn.BatchNorm1d(eps=1e-3, momentum=0.01) + nn.ReLU after every sparse conv
 *           (pcdet/models/backbones_3d/spconv_backbone.py:21-25,73). x,z,dx,dz (n,C) f32, C % 4 == 0 and
 *           (C/4) divides 256 (C = 16,32,64,128,...). Training forward returns batch mean / biased var / invstd;
 *           running_mean / running_var (nullable) are updated in the same launch: r = (1-momentum) r + momentum batch,
 *           variance unbiased (n/(n-1)), as nn.BatchNorm does; num_batches_tracked (nullable, one int64) += 1 likewise.
 *           tickets (nullable): crb_bn_ticket_ints() int32 in device memory, ZERO before the first call and left zero by
 *           every call; with it the statistics launch also reduces its per-block partials ("last block done", same
 *           summation order: bit-identical results) and a call is two launches instead of three. One ticket area serves
 *           any number of calls on ONE stream (stream order keeps them apart); calls that may run concurrently on
 *           different streams need their own. NULL = the partials are reduced by a launch of their own.
 * ---------------------------------------------------------------------------------------------- */
int64_t crb_bn_workspace_bytes(int64_t n, int C);
int crb_bn_ticket_ints(void);
int crb_bn_relu_forward(const float* x, int64_t n, int C, const float* gamma, const float* beta, float eps,
                        int relu, float* z, int64_t z_row_stride, float* mean, float* var, float* invstd,
                        float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                        void* workspace, int64_t workspace_bytes, int32_t* tickets, void* stream);
/* training forward whose statistics come from slab sums the producer of x wrote (slab_sums (n_slabs, 2, C): column sums of x
 * and x^2 over consecutive row slabs covering all n rows): same outputs as crb_bn_relu_forward up to the rounding of another
 * summation order, without the statistics pass over x. */
int crb_bn_relu_forward_partials(const float* x, int64_t n, int C, const float* slab_sums, int64_t n_slabs, const float* gamma,
                                 const float* beta, float eps, int relu, float* z, int64_t z_row_stride, float* mean, float* var,
                                 float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                 float momentum, void* workspace, int64_t workspace_bytes, int32_t* tickets, void* stream);
/* z == NULL in crb_bn_relu_forward / crb_bn_relu_forward_partials: statistics only (mean / var / invstd, running statistics and the
 * batch counter as usual), no apply pass — for a consumer that applies the normalisation itself:
 * crb_bn_affine_table writes (scale, shift) = (gamma * invstd, beta - mean * gamma * invstd) per channel, interleaved (C, 2), the
 * table crb_conv3x3_winograd2_bnrelu_nhwc / crb_winograd2_wgrad_bnrelu take. */
int crb_bn_affine_table(const float* mean, const float* invstd, const float* gamma, const float* beta, int C, float* out_c2,
                        void* stream);
int crb_bn_relu_apply(const float* x, int64_t n, int C, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, int relu, float* z, int64_t z_row_stride, void* stream);
/* z_row_stride / dz_row_stride (floats, 0 = C): z may be a channel slice of a wider row-major buffer (the BEV backbone
 * writes its two up-sampled branches straight into the concatenated (N*H*W, 512) map, and their backward reads the matching
 * slices of its gradient: no torch.cat copy, no .contiguous() copies of the gradient slices). */
/* dx may be NULL: only dgamma / dbeta are computed (a consumer that applies the BatchNorm backward while it reads dz) */
int crb_bn_relu_backward(const float* x, const float* dz, int64_t dz_row_stride, int64_t n, int C, const float* mean,
                         const float* invstd, const float* gamma, const float* beta, int relu, float* dx,
                         float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes, int32_t* tickets,
                         void* stream);
/* training BatchNorm + ReLU over groups*ns rows followed by the max over every group of ns consecutive rows: the tail of
 * a StackSAModuleMSG scale (pointnet2_modules.py:96-103: BatchNorm2d, ReLU, F.max_pool2d over nsample) on the row-major
 * (M*nsample, C) layout. The normalised matrix is not materialised: zmax (groups, out_row_stride; 0 = C) and
 * arg (groups, C) = first row of the group attaining the max are the outputs; the backward takes the gradient of zmax
 * (groups, gz_row_stride) and writes the dense dx. workspace: crb_bn_workspace_bytes(groups*ns, C). */
int crb_bn_relu_max_forward(const float* x, int64_t groups, int ns, int C, const float* gamma, const float* beta, float eps,
                            float* zmax, int64_t out_row_stride, int32_t* arg, float* mean, float* var, float* invstd,
                            float* running_mean, float* running_var, int64_t* num_batches_tracked, float momentum,
                            void* workspace, int64_t workspace_bytes, int32_t* tickets, void* stream);
int crb_bn_relu_max_backward(const float* x, const float* gz, int64_t gz_row_stride, const int32_t* arg, int64_t groups,
                             int ns, int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                             float* dx, float* dgamma, float* dbeta, void* workspace, int64_t workspace_bytes,
                             int32_t* tickets, void* stream);
/* the reduction half of crb_bn_relu_max_backward alone, for a caller that kept only the selected entries: x_sel (groups, C) = the
 * BatchNorm input at each group's arg row (crb_sa_mlp2_train_max's y_sel), gz as above -> dbeta = sum gz [z > 0],
 * dgamma = sum gz [z > 0] xhat. workspace: crb_bn_workspace_bytes(groups, C). */
int crb_bn_relu_max_backward_sums(const float* x_sel, const float* gz, int64_t gz_row_stride, int64_t groups, int C,
                                  const float* mean, const float* invstd, const float* gamma, const float* beta, float* dgamma,
                                  float* dbeta, void* workspace, int64_t workspace_bytes, int32_t* tickets, void* stream);
/* Per-frame statistics (batched CRB stage 2: G frames per train-mode pass, every BatchNorm layer normalising each frame
 * with that frame's own batch statistics like G bs=1 passes, crb_sampling.py:174-212): four launches for all frames
 * (partial sums / finalize / running update / apply, a frame's rows cut into the blocks a single-frame call would use and
 * summed in the same order: bit-identical to n_frames calls of the forward above on the frames' row ranges). frame_row_offsets is a HOST int64[n_frames+1] array; the batch statistics are scratch, running
 * statistics are updated once per frame in frame order. Forward only (stage 2 differentiates the RoI-head FC stack only). */
int64_t crb_bn_frames_workspace_bytes(int n_frames, int64_t max_rows_per_frame, int C);
int crb_bn_relu_forward_frames(const float* x, int n_frames, const int64_t* frame_row_offsets, int C, const float* gamma,
                               const float* beta, float eps, int relu, float* z, int64_t z_row_stride,
                               float* running_mean, float* running_var, float momentum, void* workspace,
                               int64_t workspace_bytes, void* stream);
int crb_bn_relu_max_forward_frames(const float* x, int n_frames, int64_t groups_per_frame, int ns, int C,
                                   const float* gamma, const float* beta, float eps, float* zmax, int64_t out_row_stride,
                                   int32_t* arg, float* running_mean, float* running_var, float momentum, void* workspace,
                                   int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a10  anchor target assignment (nearest-BEV IoU + thresholds + residual box encoding)
 * replaces: AxisAlignedTargetAssigner.assign_targets (pcdet/models/dense_heads/target_assigner/
 *           axis_aligned_target_assigner.py:36-210), box_utils.boxes3d_nearest_bev_iou (pcdet/utils/box_utils.py:272-298),
 *           ResidualCoder.encode_torch (pcdet/utils/box_coder_utils.py:13-43); POS_FRACTION < 0 branch, single head.
 * anchors (A,7) in the head's flattened order with anchor_cls (A) i32 (1-based class); gt_boxes (B,G,8) zero padded,
 * gt_valid (B,G) u8; matched_thr / unmatched_thr: device f32 arrays of n_thr entries indexed by class id (entry 0 unused,
 * n_thr = largest class id + 1); a ground truth whose class id is outside 1 .. n_thr - 1 matches no anchor.
 * out: labels (B,A) i32 {-1,0,class}, reg_targets (B,A,7), reg_weights (B,A).
 * Limits: 1 <= G <= 1024 ground-truth rows per frame and n_thr <= 64 (class ids 1 .. 63), else CRB_ERR_UNSUPPORTED; G == 0 is
 * CRB_ERR_ARG (nothing to launch: every label, target and weight is 0, which the caller writes itself).
 * ---------------------------------------------------------------------------------------------- */
int64_t crb_assign_targets_workspace_bytes(int B, int A, int G);
int crb_assign_targets(const float* anchors, const int32_t* anchor_cls, int A, const float* gt_boxes,
                       const uint8_t* gt_valid, int B, int G, const float* matched_thr,
                       const float* unmatched_thr, int n_thr, int32_t* labels, float* reg_targets, float* reg_weights,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a11  RPN losses of the anchor head: sigmoid focal classification + weighted smooth-L1 regression (with the sine
 *      difference of the heading) + direction-bin cross entropy, forward and gradient
 * replaces: AnchorHeadTemplate.get_cls_layer_loss / add_sin_difference / get_direction_target / get_box_reg_layer_loss
 *           (pcdet/models/dense_heads/anchor_head_template.py:101-214), SigmoidFocalClassificationLoss,
 *           WeightedSmoothL1Loss, WeightedCrossEntropyLoss (pcdet/utils/loss_utils.py:9-188)
 * cls_preds (B,A,num_class) logits, box_preds (B,A,7), dir_preds (B,A,num_dir_bins) or NULL (no direction classifier),
 * labels (B,A) i32 {-1 ignored, 0 background, c > 0 class; num_class == 1: any c > 0 is the class}, reg_targets (B,A,7) as
 * written by crb_assign_targets (NaN entries = "no target": zero loss and gradient), anchors (A,7) (heading column only).
 * forward : loss (B,3) = per frame {cls, loc, dir} losses, each = weight * sum over anchors / max(npos,1); npos (B) f32 =
 *           positives of the frame. The reference's scalar losses are loss.sum(0) / B; its reduce=False variants are the rows.
 * backward: gradient of sum_b sum_k grad_loss[b,k] * loss[b,k] w.r.t. the three prediction tensors (every element written).
 * Sums are taken in a fixed order: bit-reproducible. Limits: num_class <= 8, num_dir_bins <= 8 (else CRB_ERR_ARG).
 * ---------------------------------------------------------------------------------------------- */
typedef struct CrbRpnLossCfg {
  float alpha, gamma;            /* focal loss (0.25, 2.0) */
  float beta;                    /* smooth-L1 knee (1/9) */
  float dir_offset;              /* MODEL.DENSE_HEAD.DIR_OFFSET */
  float code_weights[7];         /* LOSS_CONFIG.LOSS_WEIGHTS.code_weights */
  float cls_weight, loc_weight, dir_weight;
  int32_t num_class, num_dir_bins;
} CrbRpnLossCfg;
int64_t crb_rpn_loss_workspace_bytes(int B, int A);
int crb_rpn_loss_forward(const float* cls_preds, const float* box_preds, const float* dir_preds, const int32_t* labels,
                         const float* reg_targets, const float* anchors, int B, int A, const CrbRpnLossCfg* cfg,
                         float* loss, float* npos, void* workspace, int64_t workspace_bytes, void* stream);
int crb_rpn_loss_backward(const float* cls_preds, const float* box_preds, const float* dir_preds, const int32_t* labels,
                          const float* reg_targets, const float* anchors, int B, int A, const CrbRpnLossCfg* cfg,
                          const float* npos, const float* grad_loss, float* d_cls, float* d_box, float* d_dir, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a11m  RPN losses of AnchorHeadMulti over head slices (csrc/multihead_loss.hip)
 * replaces: AnchorHeadMulti.get_cls_layer_loss / get_box_reg_layer_loss (pcdet/models/dense_heads/anchor_head_multi.py:245-373)
 * heads: HOST array of num_heads <= CRB_MULTIHEAD_MAX_HEADS entries. Head h predicts the anchors [anchor_start, anchor_start +
 * anchor_count) of the multi-head anchor order (classes one after another, each (size, rot, z, y, x)) in its own tensors cls
 * (B,A_h,C_h), box (B,A_h,7), dir (B,A_h,num_dir_bins) or NULL (all heads or none). Its class columns are the classes class_start + 1 ..
 * class_start + class_count: column j's target is [label == class_start + j + 1], so a positive whose class lies outside the head's
 * columns has an all-zero target row (SEPARATE_MULTIHEAD; without it class_start = 0 and class_count = num_class for every head).
 * cfg->num_class is the head's total class count (== 1: any label > 0 is class 1). labels (B,A) i32, reg_targets (B,A,7), anchors (A,7)
 * over all heads, A = sum of anchor_count. Classification terms are weighted pos_cls_weight (label > 0), neg_cls_weight (label == 0),
 * 0 (ignored). The heading column goes through the sine difference only when the heads have a direction classifier, as in the reference.
 * forward : loss (B,3) = per frame {cls, loc, dir}, each = weight * sum over the anchors of ALL heads / max(npos,1); npos (B) f32.
 * backward: d_cls / d_box / d_dir of every entry are written whole (zeros where there is no term), in the head's own layout.
 * Sums are taken in a fixed order: bit-reproducible. Limits: class_count <= 8, num_dir_bins <= 8 (else CRB_ERR_ARG).
 * ---------------------------------------------------------------------------------------------- */
#define CRB_MULTIHEAD_MAX_HEADS 16
typedef struct CrbMultiHeadEntry {
  const float* cls;              /* (B, anchor_count, class_count) logits */
  const float* box;              /* (B, anchor_count, 7) */
  const float* dir;              /* (B, anchor_count, num_dir_bins) or NULL */
  float* d_cls;                  /* gradients, same shapes (backward only) */
  float* d_box;
  float* d_dir;
  int32_t anchor_start, anchor_count, class_start, class_count;
} CrbMultiHeadEntry;
int64_t crb_multihead_loss_workspace_bytes(int B, int A);
int crb_multihead_loss_forward(const CrbMultiHeadEntry* heads, int num_heads, const int32_t* labels, const float* reg_targets,
                               const float* anchors, int B, int A, const CrbRpnLossCfg* cfg, float pos_cls_weight,
                               float neg_cls_weight, float* loss, float* npos, void* workspace, int64_t workspace_bytes,
                               void* stream);
int crb_multihead_loss_backward(const CrbMultiHeadEntry* heads, int num_heads, const int32_t* labels, const float* reg_targets,
                                const float* anchors, int B, int A, const CrbRpnLossCfg* cfg, float pos_cls_weight,
                                float neg_cls_weight, const float* npos, const float* grad_loss, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a22  per-class selection of a whole batch: MULTI_CLASSES_NMS on a multi-head detector (csrc/multiclass_nms.hip)
 * replaces: the frames x heads x classes loop of Detector3DTemplate.post_processing (pcdet/models/detectors/detector3d_template.py:
 *           292-317) around model_nms_utils.multi_classes_nms (pcdet/models/model_utils/model_nms_utils.py:28-66)
 * A segment is one (frame, head, class) triple; with SEG = sum of class_count there are S = B * SEG of them, stored HEAD-major: segment
 * (b, h, c) has the row B * seg_start_h + b * C_h + c (seg_start_h = classes of the heads before h), so that head h's rows are one
 * contiguous (B, C_h * pre_max) block, the anchor_idx layout of crb_decode_selected_anchors.
 * crb_multiclass_candidates: heads as above (cls, anchor_count, class_count are read). For every segment the anchors with
 *   1 / (1 + exp(-logit)) >= score_thresh, of those the best min(pre_max, A_h) in descending order of that f32 score, equal scores by
 *   ascending anchor index -> top_idx (S,pre_max) i64 into the head's anchors, top_logit (S,pre_max), counts (S) i32; entries past
 *   counts[s] are 0. One workgroup per segment: count, radix select of the cut when more than the quota pass, compaction and a bitonic
 *   sort in LDS. Nothing of size (S, A_h) is written. pre_max <= 4096 (else CRB_ERR_UNSUPPORTED).
 * crb_multiclass_finish: keep (S,post) i32 / num_keep (S) of crb_nms_batched over those segments, top_boxes (S,pre_max,7) the decoded
 *   picks, label_map (SEG) i64 the class id of every (head, class) column -> per frame the survivors of its segments one after
 *   another (head order, class order inside a head, best first inside a class): pred_boxes (B,P,7), pred_logit (B,P), pred_labels (B,P)
 *   i64, pred_anchor (B,P) i64 (index into the head's anchors), seg_of (B,P) i32 (0 .. SEG-1), num (B) i32, P = SEG * post. Rows past num[b]
 *   are zero.
 * ---------------------------------------------------------------------------------------------- */
int crb_multiclass_candidates(const CrbMultiHeadEntry* heads, int num_heads, int B, float score_thresh, int pre_max, int64_t* top_idx,
                              float* top_logit, int32_t* counts, void* stream);
int crb_multiclass_finish(const CrbMultiHeadEntry* heads, int num_heads, int B, int pre_max, int post, const int32_t* keep,
                          const int32_t* num_keep, const int64_t* top_idx, const float* top_logit, const float* top_boxes,
                          const int64_t* label_map, float* pred_boxes, float* pred_logit, int64_t* pred_labels, int64_t* pred_anchor,
                          int32_t* seg_of, int32_t* num, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a21  proposal layer around its NMS (csrc/proposal_layer.hip)
 * crb_decode_selected_anchors replaces AnchorHeadTemplate.generate_predicted_boxes for the anchors the proposal layer keeps
 *   (pcdet/models/dense_heads/anchor_head_template.py:238-285 with ResidualCoder.decode_torch, pcdet/utils/box_coder_utils.py:45-73,
 *   and the direction-bin correction through common_utils.limit_period): box_preds (B,A,7), dir_preds (B,A,num_dir_bins) or NULL,
 *   anchors (A,7), anchor_idx (B,k) i64 -> out (B,k,7) = the rows the full decode holds at those indices, bit for bit.
 * crb_proposal_finish replaces the gathers of RoIHeadTemplate.proposal_layer behind the class-agnostic NMS
 *   (pcdet/models/roi_heads/roi_head_template.py:73-108): keep (B,post) i32 (-1 = padding, positions in the top-k order), top_idx (B,k)
 *   i64 anchor indices, top_boxes (B,k,box_row_stride), scores (B,A), labels (B,A) i64 (0-based argmax), cls_preds (B,A,num_class)
 *   -> rois (B,post,box_row_stride) zero padded, roi_scores (B,post), roi_labels (B,post) i64 (1-based; padding = 1 as in the
 *   reference), full_cls_scores (B,post,num_class).
 * ---------------------------------------------------------------------------------------------- */
int crb_decode_selected_anchors(const float* box_preds, const float* dir_preds, const float* anchors, const int64_t* anchor_idx, int B,
                                int64_t A, int k, int num_dir_bins, float dir_offset, float dir_limit_offset, float* out, void* stream);
int crb_proposal_finish(const int32_t* keep, const int64_t* top_idx, const float* top_boxes, const float* scores, const int64_t* labels,
                        const float* cls_preds, int B, int64_t A, int k, int post, int box_row_stride, int num_class, float* rois,
                        float* roi_scores, int64_t* roi_labels, float* full_cls_scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a20  point head in training (csrc/point_head.hip)
 * crb_point_labels replaces the label arithmetic of PointHeadTemplate.assign_stack_targets behind its two points_in_boxes_gpu calls
 *   (pcdet/models/dense_heads/point_head_template.py:49-129, set_ignore_flag mode of PointHeadSimple): inner / outer (B*M) i32 = first
 *   containing ground truth / enlarged ground truth of every point or -1, gt_boxes (B,G,gt_row_stride >= 8, class last)
 *   -> labels (B*M) i64: the box's class (1 when num_class == 1) inside a box, -1 in the enlarged shell only, 0 elsewhere.
 * crb_point_focal_loss replaces PointHeadTemplate.get_cls_layer_loss with SigmoidFocalClassificationLoss (:131-155,
 *   pcdet/utils/loss_utils.py:9-72) and its autograd: preds (n, num_class) logits, labels (n) i64 -> loss[3] = {point_loss_cls
 *   (x loss_weight, normalised by max(positives, 1)), positives, point_loss_cls again (the scalar a caller differentiates)},
 *   d_preds (n, num_class) = d loss / d preds. One workgroup, sums in a fixed order.
 * ---------------------------------------------------------------------------------------------- */
int crb_point_labels(const int32_t* inner, const int32_t* outer, const float* gt_boxes, int B, int64_t M, int G, int gt_row_stride,
                     int num_class, int64_t* labels, void* stream);
int crb_point_focal_loss(const float* preds, const int64_t* labels, int64_t n, int num_class, float alpha, float gamma,
                         float loss_weight, float* loss, float* d_preds, void* stream);
/* crb_point_focal_loss_per_frame replaces the reduce=False form of the same loss (point_head_template.py:131-155,
 *   src.view(-1, NUM_KEYPOINTS).sum(-1), ~25 torch launches forward and backward): n = B * points per frame -> loss (B + 1) =
 *   {per-frame point_loss_cls (x loss_weight, normalised by the WHOLE batch's max(positives, 1)), positives}; d_preds (n, num_class)
 *   = d loss[frame] / d preds for that frame's rows (a unit upstream value per frame; crb_scale_rows_per_frame applies the real one).
 *   One workgroup, frames in order, sums in a fixed order. */
int crb_point_focal_loss_per_frame(const float* preds, const int64_t* labels, int64_t n, int num_class, int B, float alpha, float gamma,
                                   float loss_weight, float* loss, float* d_preds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * point head of Part-A2 in training (csrc/part_head.hip)
 * crb_part_targets replaces PointHeadTemplate.assign_stack_targets in set_ignore_flag mode with ret_part_labels=True
 *   (pcdet/models/dense_heads/point_head_template.py:49-129: a loop over the frames with a host sync each) for all frames in one launch:
 *   points (N,4) f32 [b,x,y,z] frame-sorted, frame_offsets (B+1) i32 on the device (frames may differ in size or be empty), gt_boxes
 *   (B,G,8) zero padded, class last; extra_width: 3 HOST floats (TARGET_CONFIG.GT_EXTRA_WIDTH), added to the dims as
 *   box_utils.enlarge_box3d does -> labels (N) i64: the class of the first ground truth in index order that contains the point (1 when
 *   num_class == 1), -1 where only an enlarged ground truth does, 0 elsewhere; part_labels (N,3) f32 = rotate_z(p - c, -rz) / dims + 0.5
 *   of an owned point (formed in f64, rounded once), zeros elsewhere; owner (N) i32 = that ground truth's index or -1.
 *   Containment is the test of crb_points_in_boxes (csrc/pt_in_box.h): labels equal the crb_points_in_boxes + crb_point_labels route bit
 *   for bit. The ground truths are staged in LDS 64 at a time: any G.
 * crb_part_loss_forward replaces get_cls_layer_loss (:131-158) + get_part_layer_loss (:160-173) and their autograd: cls_preds (n,C)
 *   logits, part_preds (n,3) logits, labels (n) i64, part_labels (n,3) -> loss (3) f64 = {point_loss_cls = cls_weight * sum of the focal
 *   terms of the rows with label >= 0 / max(pos,1), point_loss_part = part_weight * sum of the binary cross entropies
 *   max(x,0) - x t + log1p(exp(-|x|)) of the rows with label > 0 / (3 max(pos,1)), pos}; d_cls (n,C), d_part (n,3) = the gradients of the
 *   two losses for unit upstream values. Two launches over cdiv(n,1024) workgroups: f32 terms, f64 sums inside a workgroup and across
 *   workgroups in a fixed order, no atomics - bit-identical from call to call. workspace: crb_part_loss_workspace_bytes(n), uninitialised.
 * crb_part_loss_backward: grad_losses (2) f32 on the device = upstream gradients of the two losses -> grad_cls = d_cls * grad_losses[0],
 *   grad_part = d_part * grad_losses[1]. One launch, no host read-back.
 * ---------------------------------------------------------------------------------------------- */
int crb_part_targets(const float* points, const int32_t* frame_offsets, const float* gt_boxes, int B, int64_t N, int G,
                     const float* extra_width, int num_class, int64_t* labels, float* part_labels, int32_t* owner, void* stream);
int64_t crb_part_loss_workspace_bytes(int64_t n);
int crb_part_loss_forward(const float* cls_preds, const float* part_preds, const int64_t* labels, const float* part_labels, int64_t n,
                          int C, float alpha, float gamma, float cls_weight, float part_weight, double* loss, float* d_cls, float* d_part,
                          void* workspace, int64_t workspace_bytes, void* stream);
int crb_part_loss_backward(const float* d_cls, const float* d_part, const float* grad_losses, int64_t n, int C, float* grad_cls,
                           float* grad_part, void* stream);

/* ------------------------------------------------------------------------------------------------
 * box branch of the point heads: PointIntraPartOffsetHead with TARGET_CONFIG.BOX_CODER (PartA2_free.yaml) and PointHeadBox
 * (csrc/point_box.hip)
 * crb_point_box_targets is crb_part_targets (same inputs, the same bits in labels, owner and part_labels) plus
 *   PointResidualCoder.encode_torch with use_mean_size (pcdet/utils/box_coder_utils.py:153-187) of every owned point, in one launch:
 *   mean_size (K,3) f32 on the device -> box_labels (N,8) f32 = {(xg - xa) / sqrt(dxa^2 + dya^2), (yg - ya) / the same, (zg - za) / dza,
 *   log(dxg / dxa), log(dyg / dya), log(dzg / dza), cos rz, sin rz} with the gt dims clamped at 1e-5 and (dxa, dya, dza) =
 *   mean_size[class - 1] of the ground truth's CLASS COLUMN (also when num_class == 1 labels the point 1), formed in f64 and rounded
 *   once; zeros on every row without an owner. A class column outside 1 .. K is clamped into it (the reference asserts; the class
 *   column lives on the device and reading it back would be the host sync this launch removes). part_labels may be NULL
 *   (PointHeadBox: no part branch), then it is not written.
 * crb_point_box_loss_forward is crb_part_loss_forward plus get_box_layer_loss (point_head_template.py:175-195) with
 *   WeightedSmoothL1Loss (pcdet/utils/loss_utils.py:75-134): box_preds, box_labels (n,8); code_weights: 8 HOST floats; beta: f64, as the reference's Python float; a NaN label is
 *   replaced by the prediction (a zero term, a zero gradient); diff * code_weight; 0.5 d^2 / beta below beta, |d| - beta / 2 above, |d|
 *   when beta < 1e-5; rows with label > 0 weigh 1 / max(pos,1), the others 0 -> loss (4) f64 = {point_loss_cls, point_loss_part,
 *   point_loss_box = box_weight * sum over rows and codes, pos}; d_cls (n,C), d_part (n,3), d_box (n,8) for unit upstream values.
 *   part_preds NULL switches the part term off (point_loss_part = 0, d_part untouched). Two launches over cdiv(n,1024) workgroups, the
 *   partials are four f64 sums per tile, every workgroup adds them in one fixed order, no atomics: bit-identical from call to call.
 *   workspace: crb_point_box_loss_workspace_bytes(n), uninitialised.
 * crb_point_box_loss_backward: grad_losses (3) f32 on the device = upstream gradients of the three losses -> grad_x = d_x *
 *   grad_losses[k]. d_part / grad_part NULL: no part branch. One launch, no host read-back.
 * crb_point_box_decode replaces generate_predicted_boxes (point_head_template.py:197-211) + PointResidualCoder.decode_torch
 *   (box_coder_utils.py:189-221) and the per-frame packing of RoIHeadTemplate.proposal_layer: cls_preds (N,C), box_preds (N,8), points
 *   (N,4) frame-sorted, frame_offsets (B+1) i32 -> batch_cls_preds (B,amax,C): the rows' logits, -inf past a frame's count;
 *   batch_box_preds (B,amax,7): decoded with mean_size[argmax class (first maximum)] (C <= K), rz = atan2(sin, cos), formed in f64
 *   and rounded once, zeros past the count; counts (B) i32 = rows of the frame. amax: the caller's bound on a frame's rows: rows beyond it
 *   are dropped, and counts[b] > amax is how the caller can tell. One launch.
 * ---------------------------------------------------------------------------------------------- */
int crb_point_box_targets(const float* points, const int32_t* frame_offsets, const float* gt_boxes, int B, int64_t N, int G,
                          const float* extra_width, int num_class, const float* mean_size, int K, int64_t* labels, int32_t* owner,
                          float* box_labels, float* part_labels, void* stream);
int64_t crb_point_box_loss_workspace_bytes(int64_t n);
int crb_point_box_loss_forward(const float* cls_preds, const float* part_preds, const float* box_preds, const int64_t* labels,
                               const float* part_labels, const float* box_labels, int64_t n, int C, float alpha, float gamma,
                               const float* code_weights, double beta, float cls_weight, float part_weight, float box_weight, double* loss,
                               float* d_cls, float* d_part, float* d_box, void* workspace, int64_t workspace_bytes, void* stream);
int crb_point_box_loss_backward(const float* d_cls, const float* d_part, const float* d_box, const float* grad_losses, int64_t n, int C,
                                float* grad_cls, float* grad_part, float* grad_box, void* stream);
int crb_point_box_decode(const float* points, const int32_t* frame_offsets, const float* cls_preds, const float* box_preds,
                         const float* mean_size, int B, int64_t N, int amax, int C, int K, float* batch_cls_preds, float* batch_box_preds,
                         int32_t* counts, void* stream);

/* ------------------------------------------------------------------------------------------------
 * a22 / a24  second-stage losses and the canonical transformation of the sampled ground truths (csrc/rcnn_loss.hip)
 * replaces: RoIHeadTemplate.get_box_cls_layer_loss (BinaryCrossEntropy; pcdet/models/roi_heads/roi_head_template.py:261-285),
 *           get_box_reg_layer_loss (smooth-l1 + CORNER_LOSS_REGULARIZATION, the branch without reg_sample_targets; :142-259) with
 *           ResidualCoder.encode_torch / decode_torch (pcdet/utils/box_coder_utils.py:13-73), get_corner_loss_lidar
 *           (pcdet/utils/loss_utils.py:209-232), boxes_to_corners_3d (pcdet/utils/box_utils.py:28-55); and the part of
 *           RoIHeadTemplate.assign_targets after the sampling (:118-138). ~270 torch launches of a PV-RCNN step as two.
 * crb_rcnn_loss: n sampled RoIs; rcnn_cls (n) logits, rcnn_reg (n,7), cls_labels (n) f32 or i64 (< 0 = ignored; soft labels in
 * [0,1] for CLS_SCORE_TYPE roi_iou), reg_valid_mask (n) i64, rois (n,7), gt_of_rois (n, gt_row_stride) in the RoI frame,
 * gt_of_rois_src the same boxes in LiDAR coordinates (corner loss; NULL when cfg->corner == 0)
 * -> loss[7] = {rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner, rcnn_loss (their sum), foreground RoIs, valid RoIs, rcnn_loss again
 *    (a second home for the scalar a caller differentiates)}, each loss already multiplied by its LOSS_WEIGHTS entry and divided by
 *    max(count, 1);
 *    d_cls (n), d_reg (n,7) = d rcnn_loss / d (rcnn_cls, rcnn_reg); reg_targets (n,7) (forward_ret_dict['rcnn_reg_gt']) or NULL.
 * One workgroup, sums in a fixed order: bit-reproducible. code size 7 only.
 * crb_roi_canonical_targets: rois (n, roi_row_stride >= 7), gt_of_rois (n, gt_row_stride >= 7) -> out (n, gt_row_stride).
 * ---------------------------------------------------------------------------------------------- */
typedef struct CrbRcnnLossCfg {
  float beta;                    /* smooth-L1 knee of the regression loss (1/9); the corner loss uses 1 */
  float code_weights[7];         /* LOSS_CONFIG.LOSS_WEIGHTS.code_weights */
  float cls_weight, reg_weight, corner_weight;   /* rcnn_cls_weight, rcnn_reg_weight, rcnn_corner_weight */
  int32_t corner;                /* CORNER_LOSS_REGULARIZATION */
} CrbRcnnLossCfg;
int crb_rcnn_loss(const float* rcnn_cls, const float* rcnn_reg, const void* cls_labels, int labels_are_int64,
                  const int64_t* reg_valid_mask, const float* rois, const float* gt_of_rois, const float* gt_of_rois_src,
                  int gt_row_stride, int64_t n, const CrbRcnnLossCfg* cfg, float* loss, float* d_cls, float* d_reg,
                  float* reg_targets, void* stream);
/* crb_rcnn_loss_per_frame replaces the reduce=False form of get_box_cls_layer_loss / get_box_reg_layer_loss (roi_head_template.py:
 *   142-285 with reduce=False, the LLAL loss-net phase; ~270 torch launches forward and backward): n = B * ROI_PER_IMAGE RoIs, same
 *   inputs as crb_rcnn_loss -> loss_frames (B, 4) = {rcnn_loss_cls, rcnn_loss_reg, rcnn_loss_corner, rcnn_loss} per frame, cls and
 *   reg divided by the WHOLE batch's valid / foreground counts, corner by the FRAME's foreground count (the reference's quirks);
 *   d_cls (n), d_reg (n,7) = d loss_frames[frame, 3] / d (rcnn_cls, rcnn_reg) for that frame's rows (unit upstream per frame).
 *   One workgroup, frames in order, sums in a fixed order. */
int crb_rcnn_loss_per_frame(const float* rcnn_cls, const float* rcnn_reg, const void* cls_labels, int labels_are_int64,
                            const int64_t* reg_valid_mask, const float* rois, const float* gt_of_rois, const float* gt_of_rois_src,
                            int gt_row_stride, int64_t n, int B, const CrbRcnnLossCfg* cfg, float* loss_frames, float* d_cls, float* d_reg,
                            float* reg_targets, void* stream);
/* crb_rcnn_iou_loss replaces SECONDHead.get_box_iou_layer_loss (pcdet/models/roi_heads/second_head.py:153-178; ~12 torch launches
 *   forward and as many backward): rcnn_iou (n) logits, labels (n) f32 soft IoU targets of CLS_SCORE_TYPE roi_iou (< 0 = ignored),
 *   kind = LOSS_CONFIG.IOU_LOSS (BinaryCrossEntropy with logits / L2 / smoothL1 with the knee 1/9 of loss_utils.py:75-131), weight =
 *   LOSS_WEIGHTS.rcnn_iou_weight -> loss[2] = {rcnn_loss_iou = sum over the valid rows / max(valid, 1) * weight, valid rows},
 *   d_iou (n) = d rcnn_loss_iou / d rcnn_iou (0 on ignored rows). One workgroup, sums in a fixed order: bit-reproducible. */
#define CRB_IOU_LOSS_BCE 0
#define CRB_IOU_LOSS_L2 1
#define CRB_IOU_LOSS_SMOOTH_L1 2
int crb_rcnn_iou_loss(const float* rcnn_iou, const float* labels, int64_t n, int kind, float weight, float* loss, float* d_iou,
                      void* stream);
/* backward of the per-frame losses above (replaces autograd's broadcast multiply of the per-row gradients by the (B,) upstream
 * gradient): src (rows, width) -> dst = src * g[row / (rows / frames)]. */
int crb_scale_rows_per_frame(const float* src, int64_t rows, int width, int frames, const float* g, float* dst, void* stream);
int crb_roi_canonical_targets(const float* rois, int roi_row_stride, const float* gt_of_rois, int gt_row_stride, int64_t n,
                              float* out, void* stream);
/* grid points of the RoI-grid pooling (PVRCNNHead.get_global_grid_points_of_roi + get_dense_grid_points, pvrcnn_head.py:116-141):
 * rois (n, roi_row_stride >= 7) -> out (n, grid_size^3, 3): ((i + 0.5) / G) * size - size / 2 per axis (x slowest, z fastest), turned by
 * the heading about z, moved to the centre. */
int crb_roi_grid_points(const float* rois, int roi_row_stride, int64_t n, int grid_size, float* out, void* stream);
/* second-stage box decode (RoIHeadTemplate.generate_predicted_boxes, roi_head_template.py:335-359): rois (n, roi_row_stride >= 7),
 * box_preds (n,7) residuals -> out (n,7) boxes in LiDAR coordinates (ResidualCoder.decode_torch against the RoI as anchor with centre
 * 0, the centre turned by the RoI's heading and moved to the RoI's centre). */
int crb_rcnn_decode_boxes(const float* rois, int roi_row_stride, const float* box_preds, int64_t n, float* out, void* stream);
/* CRB stage-1 records behind the final NMS (Detector3DTemplate.post_processing's per-frame selection, detector3d_template.py:186-234,
 * and the label entropy of crb_sampling.py:86-94), one workgroup per frame: sel (B,P) i64 indices into the N boxes of the frame, valid
 * (B,P) u8, box_preds (B,N,box_row_stride), cls_confs (B,N), label_preds (B,N) i64 (1-based), full_cls_scores (B,N,full_classes) or
 * NULL -> pred_boxes (B,P,box_row_stride), pred_scores (B,P), pred_labels (B,P) i64, pred_logits (B,P,full_classes), all zero where
 * not valid; entropy (B) = Shannon entropy of the label histogram of the valid boxes, absent classes counted as 1, 0 without boxes.
 * crb_box_point_density: first_box (B,M) i32 = first containing predicted box of every point (crb_points_in_boxes) -> density (B,P) =
 * points / max(volume, 1e-12) of the valid boxes, 0 elsewhere (P <= 2048). */
int crb_record_rows(const int64_t* sel, const uint8_t* valid, const float* box_preds, int box_row_stride, const float* cls_confs,
                    const int64_t* label_preds, const float* full_cls_scores, int full_classes, int B, int N, int P, int num_class,
                    float* pred_boxes, float* pred_scores, int64_t* pred_labels, float* pred_logits, float* entropy, void* stream);
int crb_box_point_density(const int32_t* first_box, const float* pred_boxes, int box_row_stride, const uint8_t* valid, int B, int M, int P,
                          float* density, void* stream);
/* RoI sampling for the second stage: one workgroup per frame (csrc/rcnn_loss.hip)
 * replaces: ProposalTargetLayer.forward / sample_rois_for_rcnn / subsample_rois / get_max_iou_with_same_class
 *           (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:15-228): per frame the (same-class) maximum IoU of every
 *           proposal, foreground / hard / easy background sets, FG_RATIO and HARD_BG_RATIO quotas, foreground without replacement in
 *           random order, background with replacement, the gathers, reg_valid_mask and rcnn_cls_labels. The random numbers are
 *           INPUTS: u_perm (B,R) orders the foreground, u_slot (B,P) draws with replacement (floor(u * n)) - the reference's
 *           np.random / torch.randint stream is not reproduced.
 * rois (B,R,roi_row_stride >= 7), roi_scores (B,R), roi_labels (B,R) i64, gt_boxes (B,G,gt_row_stride >= 8, class in the last column,
 * zero rows = padding), iou (B*R, B*G) = crb_boxes_iou3d of all proposals against all ground truths (frame b uses its diagonal block)
 * -> sampled (B,P) i64 proposal indices, out_rois (B,P,roi_row_stride), out_gt (B,P,gt_row_stride), out_iou / out_scores (B,P),
 *    out_labels (B,P) i64, reg_valid_mask (B,P) i64, cls_labels (B,P) f32 (score_type 0 = roi_iou) or i64 (1 = cls, -1 ignored).
 * R <= 1024, else CRB_ERR_UNSUPPORTED. */
typedef struct CrbRoiSamplerCfg {
  int32_t roi_per_image;         /* ROI_PER_IMAGE = P */
  int32_t fg_quota;              /* round(FG_RATIO * P) */
  int32_t by_class;              /* SAMPLE_ROI_BY_EACH_CLASS */
  int32_t score_type;            /* CLS_SCORE_TYPE: 0 roi_iou, 1 cls */
  float fg_thresh;               /* min(REG_FG_THRESH, CLS_FG_THRESH) */
  float reg_fg_thresh, cls_fg_thresh, cls_bg_thresh, cls_bg_thresh_lo, hard_bg_ratio;
  float soft_den;                /* CLS_FG_THRESH - CLS_BG_THRESH */
} CrbRoiSamplerCfg;
int crb_roi_sample_targets(const float* rois, int roi_row_stride, const float* roi_scores, const int64_t* roi_labels,
                           const float* gt_boxes, int gt_row_stride, const float* iou, const float* u_perm, const float* u_slot,
                           int B, int R, int G, const CrbRoiSamplerCfg* cfg, int64_t* sampled, float* out_rois, float* out_gt,
                           float* out_iou, float* out_scores, int64_t* out_labels, int64_t* reg_valid_mask, void* cls_labels,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * a7  3x3 stride-1 pad-1 convolution on channels_last maps as Winograd F(2x2,3x3) on the f32 MFMA (csrc/winograd_conv2.hip)
 * replaces: torch.nn.Conv2d(C, C, 3, padding=1) of the BEV backbone (pcdet/models/backbones_2d/base_bev_backbone.py:24-41;
 *           MIOpen's f32 implicit GEMM on this stack). 2.25x fewer multiplications than the direct convolution, results equal to
 *           it up to f32 rounding of the transforms (4e-7 of the output scale against an f64 convolution).
 * x (N,H,W,Cin) f32 NHWC, y (N,H,W,Cout); bias (Cout) or NULL, relu 0/1: epilogue on the output. The input gradient of the same
 * layer is the same call on dy with the flipped, transposed weights. Two waves per SIMD (128 accumulators each), the raw input
 * block and the weight block brought into LDS by LDS-DMA once per workgroup and chunk, the input transform read from LDS;
 * workgroup = 16 x 4 tiles of one spatial block x 64 output channels. Weight image: crb_winograd2_weights writes U in the order
 * the kernel's LDS-DMA copies it ([Cout/64][Cin/8][LDS image of a chunk]), crb_winograd2_weights_bytes floats*4.
 * crb_winograd2_supported: Cin % 8 == 0, Cout % 64 == 0, H >= 5. (The first design of round 3, crb_conv3x3_winograd_nhwc, lives in
 * the measurement library: include/crb_hip_measure.h.) */
int crb_winograd2_supported(int cin, int cout, int H, int W);
int64_t crb_winograd2_weights_bytes(int cin, int cout);
int crb_winograd2_weights(const float* g, float* U, int cin, int cout, void* stream);
/* the same image straight from an nn.Conv2d weight (Cout,Cin,3,3) with element strides (so, si, sky, skx) — contiguous or
 * channels_last, no permuted copy: mode 0 = forward (Cin -> Cout), mode 1 = input gradient (the convolution dy -> dx with the
 * flipped, transposed weights: Cout -> Cin) */
int crb_winograd2_weights_conv(const float* w, int64_t so, int64_t si, int64_t sky, int64_t skx, float* U, int conv_cin,
                               int conv_cout, int mode, void* stream);
/* the same for n <= 32 weight tensors in ONE launch (the 11 stride-1 layers of the BEV backbone need 22 images per training step, each
 * launch-bound at ~10 us): w[j] (Cout_j, Cin_j, 3, 3) with element strides strides[4 j .. 4 j + 3], U[j] its image for mode[j].
 * w, U, conv_cin, conv_cout, mode, strides are HOST arrays. */
int crb_winograd2_weights_conv_multi(int n, const float* const* w, const int64_t* strides, float* const* U, const int32_t* conv_cin,
                                     const int32_t* conv_cout, const int32_t* mode, void* stream);
int crb_conv3x3_winograd2_nhwc(const float* x, const float* U, float* y, int N, int H, int W, int cin, int cout,
                               const float* bias, int relu, void* stream);
/* training forward that also hands the following BatchNorm its statistics: stats (crb_winograd2_stats_slabs(N,H,W), 2, Cout) f32 =
 * column sums of y and y^2 per slab of outputs (a slab = half of the 64 tiles of one 16 x 4-tile spatial block; outputs outside
 * the map are not counted), every slab written exactly once, no atomics. Feed them to crb_bn_relu_forward_partials(y, N*H*W,
 * Cout, stats, slabs, ...): the BatchNorm's own statistics pass over y (pcdet/models/backbones_2d/base_bev_backbone.py:31-41,
 * nn.BatchNorm2d in training mode) is not launched. No bias, no ReLU (the Conv2d layers of the backbone have neither). */
int64_t crb_winograd2_stats_slabs(int N, int H, int W);
int crb_conv3x3_winograd2_stats_nhwc(const float* x, const float* U, float* y, float* stats, int N, int H, int W, int cin, int cout,
                                     void* stream);

/* a7, round 6: the same convolution with the 16 Winograd GEMMs on the bf16 matrix pipe through an EXACT three-way split of every
 * f32 operand (csrc/winograd_conv4.hip). replaces: the same torch.nn.Conv2d(C, C, 3, padding=1) of
 * pcdet/models/backbones_2d/base_bev_backbone.py:24-41 as crb_conv3x3_winograd2_nhwc. x = x1 + x2 + x3 with x1 = x & 0xffff0000,
 * x2 = (x - x1) & 0xffff0000, x3 = x - x1 - x2 (no rounding: an f32 significand is three bf16 significands); of the nine exact
 * partial products of x * w the six with i + j <= 4 are accumulated in f32 by v_mfma_f32_32x32x16_bf16 (the three dropped ones are
 * below 2^-23 |x w|, one f32 rounding of the product): f32 in, f32 out, errors against an f64 convolution at the level of the f32-MFMA
 * kernel's (tests/test_winograd_gpu.py holds both to the same bars), at 16 / 6 of the f32 MFMA rate. Inf / NaN inputs give NaN (inf -
 * inf in the split), values below 2^-110 lose their low pieces to flushing.
 * Same arguments as the *2 entry points; the weight image is bf16 pieces in LDS order ([Cout/64][Cin/16][xi row][xi][piece][k
 * group][64 rows][8]), crb_winograd4_weights_bytes bytes. crb_winograd4_supported: Cin % 16 == 0, Cout % 64 == 0, H >= 31 (a block of
 * 16 tile rows touches at most two images). One wave per SIMD with all 16 xi of a 32 x 32 block (256 accumulators), raw block shared
 * by the workgroup (halo rows fetched once), four xi-row phases per 16-channel chunk. Stats: crb_winograd4_stats_slabs slabs (one per
 * spatial block and tile half; tile rows per image NOT rounded up to even), same meaning as crb_winograd2_stats_slabs' otherwise. */
int crb_winograd4_supported(int cin, int cout, int H, int W);
int64_t crb_winograd4_weights_bytes(int cin, int cout);
int crb_winograd4_weights_conv(const float* w, int64_t so, int64_t si, int64_t sky, int64_t skx, void* U, int conv_cin, int conv_cout,
                               int mode, void* stream);
int crb_winograd4_weights_conv_multi(int n, const float* const* w, const int64_t* strides, void* const* U, const int32_t* conv_cin,
                                     const int32_t* conv_cout, const int32_t* mode, void* stream);
int crb_conv3x3_winograd4_nhwc(const float* x, const void* U, float* y, int N, int H, int W, int cin, int cout, const float* bias,
                               int relu, void* stream);
int64_t crb_winograd4_stats_slabs(int N, int H, int W);
int crb_conv3x3_winograd4_stats_nhwc(const float* x, const void* U, float* y, float* stats, int N, int H, int W, int cin, int cout,
                                     void* stream);
/* The same convolution with a workgroup tile of 32 tiles x 128 output channels (round 6, third form): V of a spatial block is formed once
 * per 128 output channels instead of once per 64. Cin % 16 == 0, Cout % 128 == 0; weight image: crb_winograd4_weights_conv(_multi) with
 * mode + 2 (same bytes, other order); statistics slabs: crb_winograd4c_stats_slabs (one per block of 8 tile rows x 4 tile columns).
 * Outputs bit-equal to crb_conv3x3_winograd4_nhwc. */
int crb_winograd4c_supported(int cin, int cout, int H, int W);
int crb_conv3x3_winograd4c_nhwc(const float* x, const void* U, float* y, int N, int H, int W, int cin, int cout,
                                const float* bias, int relu, void* stream);
int64_t crb_winograd4c_stats_slabs(int N, int H, int W);
int crb_conv3x3_winograd4c_stats_nhwc(const float* x, const void* U, float* y, float* stats, int N, int H, int W, int cin,
                                      int cout, void* stream);

/* Block lists of a sparse BEV map for the two kernels above and crb_winograd4_wgrad (csrc/bev_blocks.hip, csrc/winograd_blocks.h).
 * replaces: nothing in the reference, which runs cuDNN over the whole scattered map
 *           (pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-26 feeding base_bev_backbone.py:24-41); here the first
 *           3x3 layer skips the blocks of its 88 %-zero input that cannot change the result.
 * indices (n,4) int32 rows (b, z, y, x): the rows crb_sparse_to_dense_nhwc scatters; a pixel (b, y, x) named by a row is ACTIVE.
 * layout of out (int32, crb_bev_blocks_ints(N, H, W) entries, device memory; nothing is read back):
 *   [0..7]  counts: conv-in list, conv-out list, wgrad list, rest of conv-in, rest of conv-out, 0, 0, 0
 *   then five ascending lists: conv-in (nb), rest of conv-in (nb), conv-out (nb), rest of conv-out (nb), wgrad (nc); a list's entries
 *   behind its count are unspecified; behind the lists the builder's flag bytes.
 *   conv-in:  spatial blocks of crb_conv3x3_winograd4c_nhwc (8 tile rows over N * ceil(H / 2) x 4 tile columns, nb of them, numbered
 *             row-major) with an active pixel within one pixel of their outputs: every other block of y is +0 when x is zero outside
 *             the active pixels;  conv-out: blocks that hold an active pixel;  rest: the blocks not listed (what a fill has to clear);
 *   wgrad:    chunks of crb_winograd4_wgrad (4 x 4 tiles of one image, nc = N * ceil(th / 4) * ceil(tw / 4), numbered (n, row, column))
 *             with an active pixel within one pixel of their 8 x 8 pixels.
 * crb_bev_blocks_geometry: host array of 12: nb, nc, th, tw, block columns, chunk rows per image, chunk columns, tile size, block tile
 * rows / columns, chunk tile rows / columns. Marking: one thread per index, plain byte stores; compaction: an ordered scan. No atomics. */
int crb_bev_blocks_geometry(int N, int H, int W, int32_t* geom);
int64_t crb_bev_blocks_ints(int N, int H, int W);
int crb_bev_blocks(const int32_t* indices, int64_t n, int N, int H, int W, int32_t* out, int64_t out_ints, void* stream);
/* crb_conv3x3_winograd4c_nhwc without bias / ReLU (stats null) or crb_conv3x3_winograd4c_stats_nhwc over the blocks of `list` only
 * (*count of them); the blocks of `rest` (and their statistics slabs) are filled with +0 by a small launch in front. With the
 * conv-in list of a map that is zero outside its active pixels, y and stats are bit-equal to the dense launch; with the conv-out
 * list the listed blocks are (the input gradient of that map, which is read at the active pixels only). */
int crb_conv3x3_winograd4c_blocks_nhwc(const float* x, const void* U, float* y, float* stats, int N, int H, int W, int cin,
                                       int cout, const int32_t* list, const int32_t* count, const int32_t* rest,
                                       const int32_t* rest_count, void* stream);

/* a7 backward: weight gradient of the same convolution in the Winograd domain (csrc/winograd_wgrad.hip):
 * dU[xi][ci][co] = sum over tiles of (B^T d B)[xi][ci] * (A dY A^T)[xi][co] as 16 MFMA GEMMs whose two operands are both
 * produced by transforms inside the kernel, partial sums per range of tiles in the workspace, then dW = G^T dU G added up in
 * range order in double (bit-reproducible).
 * replaces: aten.convolution_backward(..., output_mask = [False, True, False]) = MIOpen's f32 implicit-GEMM wrw kernels for
 *           torch.nn.Conv2d(C, C, 3, padding=1) of pcdet/models/backbones_2d/base_bev_backbone.py:24-41.
 * x (N,H,W,Cin), dy (N,H,W,Cout) f32 NHWC; dw = gradient of the nn.Conv2d weight (Cout,Cin,3,3), written with that tensor's
 * element strides (so, si, sky, skx); Cin % 64 == 0, Cout % 64 == 0. */
int crb_winograd2_wgrad_supported(int cin, int cout, int H, int W);
int64_t crb_winograd2_wgrad_workspace_bytes(int cin, int cout);
int crb_winograd2_wgrad(const float* x, const float* dy, float* dw, int64_t so, int64_t si, int64_t sky, int64_t skx,
                        int N, int H, int W, int cin, int cout, void* workspace, int64_t workspace_bytes, void* stream);
/* The same weight gradient on the bf16 matrix pipe (csrc/winograd_wgrad4.hip): V = B^T d B and M = A dY A^T are formed in f32 with the
 * additions of crb_winograd2_wgrad, each is written as the exact sum of three bf16 values (the split of crb_conv3x3_winograd4_nhwc) and
 * every product runs as six bf16 MFMA passes with f32 accumulation; partials per range of tiles, summed in range order in double,
 * dW = G^T dU G in double: bit-reproducible, errors against f64 at the level of crb_winograd2_wgrad's. An Inf in x or dy turns the
 * entries it reaches into NaN (inf - inf in the split), values below 2^-110 lose their low pieces to flushing.
 * replaces: crb_winograd2_wgrad (v_mfma_f32_16x16x4_f32 runs at the f32 vector rate) where it has an instance, and through it
 *           aten.convolution_backward(..., output_mask = [False, True, False]) for torch.nn.Conv2d(C, C, 3, padding=1) of
 *           pcdet/models/backbones_2d/base_bev_backbone.py:24-41.
 * Same arguments as the crb_winograd2_wgrad trio. Instances: Cin % 128 == 0, Cout % 128 == 0, both <= 1024 (a workgroup owns one xi
 * row x 128 x 128 channels); everything else stays on crb_winograd2_wgrad. */
int crb_winograd4_wgrad_supported(int cin, int cout, int H, int W);
int64_t crb_winograd4_wgrad_workspace_bytes(int cin, int cout);
int crb_winograd4_wgrad(const float* x, const float* dy, float* dw, int64_t so, int64_t si, int64_t sky, int64_t skx,
                        int N, int H, int W, int cin, int cout, void* workspace, int64_t workspace_bytes, void* stream);
/* the same gradient over the chunks of `list` only (the wgrad list of crb_bev_blocks: x is zero in the patch of every other chunk).
 * The K ranges split the list instead of all chunks: equal to crb_winograd4_wgrad up to the order of the f32 sums, and bit-equal
 * from call to call. */
int crb_winograd4_wgrad_blocks(const float* x, const float* dy, float* dw, int64_t so, int64_t si, int64_t sky, int64_t skx,
                               int N, int H, int W, int cin, int cout, const int32_t* list, const int32_t* count,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* Transposed convolutions with kernel = stride as row GEMMs on the bf16 matrix pipe (csrc/rows_gemm4.hip): a channels_last map is
 * the row matrix (pixels x channels), so ConvTranspose2d(cin -> cout, k = s, stride = s, no padding, no bias, groups 1) is
 * X[N H W x cin] . W[cin x s s cout] with the s * s result blocks of a row scattered to the output pixels (s h + a, s w + b); the input
 * gradient gathers those pixels and contracts over (tap, cout); the weight gradient contracts over the rows. f32 in, f32 out:
 * operands are written as exact sums of three bf16 values (the split of crb_conv3x3_winograd4_nhwc) and every product runs as six
 * bf16 MFMA passes with f32 accumulation. No atomics: all three are bit-reproducible. An Inf operand turns the entries it reaches
 * into NaN (inf - inf in the split), values below 2^-110 lose their low pieces to flushing.
 * replaces: torch.nn.ConvTranspose2d(C, U, s, stride=s, bias=False) of the up-sampling branches of
 *           pcdet/models/backbones_2d/base_bev_backbone.py:52-58 (MIOpen / CK backward-data forward, MIOpen igemm input and weight
 *           gradients, hipBLASLt f32 GEMMs for s = 1).
 * w: the ConvTranspose2d weight (cin, cout, s, s) given by its element strides (s_ci, s_co, s_a, s_b) (a Conv2d 1x1 weight: swap the
 * first two). direction: 0 = forward, 1 = input gradient, 2 = weight gradient. stride in {1, 2}.
 * crb_rows_gemm4_supported: forward cin % 32 == 0 and cout % 128 == 0; input gradient cout % 32 == 0 and cin % 128 == 0; weight
 *   gradient cin % 256 == 0 and cout % 256 == 0; channel counts <= 4096.
 * crb_rows_gemm4_weights: image (crb_rows_gemm4_weights_bytes) of direction 0 or 1: [n / 32][k / 16][piece 3][lane 64][8 bf16] of
 *   Wm[k][n], forward k = ci, n = t cout + co; input gradient k = t cout + co, n = ci (t = a s + b); lane (r, h), element j of k step
 *   2 c + u holds k = 32 c + 16 h + 8 u + j, n = 32 (n / 32) + r.
 * crb_rows_gemm4_forward: x (N,H,W,cin) NHWC, image of direction 0 -> y (N,sH,sW,cout) NHWC.
 * crb_rows_gemm4_input_grad: dy (N,sH,sW,cout), image of direction 1 -> dx (N,H,W,cin).
 * crb_rows_gemm4_wgrad: x, dy as above -> dw written with the weight's element strides; partial sums per range of rows in the
 *   workspace (crb_rows_gemm4_wgrad_workspace_bytes), added in range order in double. */
int crb_rows_gemm4_supported(int cin, int cout, int stride, int direction);
int64_t crb_rows_gemm4_weights_bytes(int cin, int cout, int stride);
int crb_rows_gemm4_weights(const float* w, int64_t s_ci, int64_t s_co, int64_t s_a, int64_t s_b, void* image, int cin, int cout,
                           int stride, int direction, void* stream);
int crb_rows_gemm4_forward(const float* x, const void* image, float* y, int N, int H, int W, int cin, int cout, int stride,
                           void* stream);
int crb_rows_gemm4_input_grad(const float* dy, const void* image, float* dx, int N, int H, int W, int cin, int cout, int stride,
                              void* stream);
int64_t crb_rows_gemm4_wgrad_workspace_bytes(int cin, int cout, int stride);
int crb_rows_gemm4_wgrad(const float* x, const float* dy, float* dw, int64_t s_ci, int64_t s_co, int64_t s_a, int64_t s_b, int N,
                         int H, int W, int cin, int cout, int stride, void* workspace, int64_t workspace_bytes, void* stream);

/* Backward of BatchNorm(train) -> ReLU -> concat -> linear head (csrc/head_bn.hip): the head out = z W^T + b reads the concatenated
 * map z (n, Ct) = relu(gamma xhat + beta) of `nbranch` branch inputs x_i (n, width) (base_bev_backbone.py:100-104 followed by
 * anchor_head_single.py:57-72 as one convolution). With dOut (n, K) contiguous, W (K, Ct) contiguous, mask = [gamma xhat + beta > 0]:
 *   P2[k][c] = sum_r dOut[r][k] mask[r][c],  P3[k][c] = sum_r dOut[r][k] mask[r][c] xhat[r][c]
 *   dbeta = sum_k W P2, dgamma = sum_k W P3, dW = gamma P3 + beta P2, dx = gamma invstd (mask (dOut . W) - dbeta / n - xhat dgamma / n)
 * so the gradient of the map is never formed and the map is not read. Products on the bf16 matrix pipe through the exact three-way
 * split (Inf -> NaN); no atomics: bit-reproducible. Nothing is read past row n or past k = K.
 * par (4, Ct) f32: mean | invstd | gamma | beta of the concatenated channels.
 * crb_head_bn_supported: nbranch == 2, width in {128, 256}, K in {60, 72}; anything else CRB_ERR_UNSUPPORTED from every call.
 * crb_head_bn_sums: -> sums (crb_head_bn_sums_count f64) = P2 (K, Ct) | P3 (K, Ct) | column sums of dOut (K). Partials per range of
 *   rows in the workspace (crb_head_bn_workspace_bytes), added in range order in double. Two launches.
 * crb_head_bn_finalize: sums, W, par -> dgb (2, Ct) = dbeta | dgamma, dw (K, Ct), dbias (K) (NULL: not written), in double. One launch.
 * crb_head_bn_weights: image (crb_head_bn_weights_bytes) of W for crb_head_bn_apply: [Ct / 32][ceil(K / 16)][piece 3][lane 64][8 bf16],
 *   lane (r, h), element j of k step s holds W[16 s + 8 h + j][32 (c / 32) + r], zero past K.
 * crb_head_bn_apply: -> dx0, dx1 (n, width), bn_bwd_apply_kernel's expression on dz formed in accumulators. One launch. */
int crb_head_bn_supported(int nbranch, int width, int K);
int64_t crb_head_bn_workspace_bytes(int nbranch, int width, int K);
int64_t crb_head_bn_sums_count(int nbranch, int width, int K);
int crb_head_bn_sums(const float* x0, const float* x1, const float* par, const float* dout, int64_t n, int nbranch, int width, int K,
                     double* sums, void* workspace, int64_t workspace_bytes, void* stream);
int crb_head_bn_finalize(const double* sums, const float* w, const float* par, int nbranch, int width, int K, float* dgb, float* dw,
                         float* dbias, void* stream);
int64_t crb_head_bn_weights_bytes(int nbranch, int width, int K);
int crb_head_bn_weights(const float* w, void* image, int nbranch, int width, int K, void* stream);
int crb_head_bn_apply(const float* x0, const float* x1, const float* par, const float* dgb, const float* dout, const void* image,
                      int64_t n, int nbranch, int width, int K, float* dx0, float* dx1, void* stream);

/* Forward of the same region without the map (csrc/head_bn.hip): out (n, K) = relu(bn(x)) W^T + b from the branch inputs, with
 * relu(bn(.)) = bn_apply_kernel's expression formed in registers (a NaN stays a NaN), the product through the exact three-way split
 * (Inf -> NaN) with two accumulator sets. par as above (batch or running statistics). Same instances as crb_head_bn_supported.
 * crb_bn_head_forward_weights: image (crb_bn_head_forward_weights_bytes) of W (K, Ct):
 *   [ceil(K / 32)][Ct / 16][piece 3][lane 64][8 bf16], lane (r, h), element j of k step 2 c + u holds
 *   W[32 kb + r][32 c + 16 h + 8 u + j], zero past K.
 * crb_bn_head_forward: one launch of persistent workgroups; rows past n are not stored, nothing is read past row n - 1. */
int64_t crb_bn_head_forward_weights_bytes(int nbranch, int width, int K);
int crb_bn_head_forward_weights(const float* w, void* image, int nbranch, int width, int K, void* stream);
int crb_bn_head_forward(const float* x0, const float* x1, const float* par, const void* image, const float* bias, int64_t n,
                        int nbranch, int width, int K, float* out, void* stream);

/* Scheduling hint, no reference counterpart: PV-RCNN's keypoint sampling (crb_furthest_point_sampling_stack on a side stream under
 * the backbones) holds one CU per frame for ~5 ms while the persistent one-workgroup-per-CU Winograd launches of the BEV backbone
 * run on the main stream. crb_cu_reservation(cus, stream) right before such a kernel, crb_cu_reservation(0, stream) right after it
 * (same stream: two one-thread launches): the Winograd forward launches in between spread their units over (CUs - cus)
 * workgroups instead of leaving `cus` workgroups queued behind the taken CUs. Only launches that put a workgroup on every CU
 * look at it, and at most half of the CUs are ever announced as taken (a larger `cus` is clamped). Results do not depend on it. */
int crb_cu_reservation(int cus, void* stream);

/* a19: bilinear lookup of the BEV feature map at the keypoints.
 * replaces: VoxelSetAbstraction.interpolate_from_bev_features + bilinear_interpolate_torch
 *           (pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:176-207, :11-44): per frame four advanced-index gathers of
 *           the (H, W, C) map, four weights from the clamped corner coordinates, a weighted sum; autograd's backward = four
 *           index_put(accumulate) calls.
 * bev (B,H,W,C) f32 NHWC (= the channels_last (B,C,H,W) map), C % 4 == 0; keypoints (M,4) f32 [frame, x, y, z];
 * u = ((x - x_min) * (1 / voxel_x)) * (1 / bev_stride) in f32 (what torch's division of a tensor by a host scalar computes, twice,
 * as the reference writes it), corners floor(u), floor(u) + 1 clamped into the
 * map, weights from the CLAMPED corners, products added left to right: bit-identical to the torch expression. out (M,C).
 * backward: dbev (B,H,W,C) must be ZERO on entry; the four weighted copies of dout are added with float atomics (keypoints that
 * share a cell: sums in arrival order). */
int crb_bev_interpolate_forward(const float* bev, int B, int H, int W, int C, const float* keypoints, int64_t M, float x_min,
                                float y_min, float voxel_x, float voxel_y, float bev_stride, float* out, void* stream);
int crb_bev_interpolate_backward(const float* dout, int B, int H, int W, int C, const float* keypoints, int64_t M, float x_min,
                                 float y_min, float voxel_x, float voxel_y, float bev_stride, float* dbev, void* stream);

/* rotated grid pooling of the BEV map under the first-stage proposals (csrc/roi_bev_pool.hip)
 * replaces: SECONDHead.roi_grid_pool (pcdet/models/roi_heads/second_head.py:53-110): per frame theta from the RoI (:79-92),
 *           affine_grid (:95-98) and grid_sample (:100-103) over a (R, C, H, W) expand of the NCHW map, torch.cat over the frames.
 * bev (B,H,W,C) f32 NHWC (= the channels_last (B,C,H,W) map; never transposed), C % 4 == 0, H, W >= 2, 16-byte aligned;
 * rois (B * R, roi_row_stride >= 7) f32 [x, y, z, dx, dy, dz, rz, ...], R per frame, frame of row n = n / R; cell_x / cell_y =
 * VOXEL_SIZE[0 / 1] * DOWNSAMPLE_RATIO. Per RoI, with W1 = W - 1, H1 = H - 1:
 *   x1 = (x - dx/2 - x_min) / cell_x, x2 = (x + dx/2 - x_min) / cell_x, y1, y2 likewise, c = cos(rz), s = sin(rz),
 *   theta = [[(x2-x1)/W1 c, -(x2-x1)/W1 s, (x1+x2-W+1)/W1], [(y2-y1)/H1 s, (y2-y1)/H1 c, (y1+y2-H+1)/H1]];
 * per grid point (row j, column i): u = (2i+1)/G - 1, v = (2j+1)/G - 1, (gx, gy) = theta (u, v, 1), ix = ((gx+1) W - 1)/2,
 * iy = ((gy+1) H - 1)/2: affine_grid / grid_sample with align_corners=False, bilinear, zeros (what the reference executes; its
 * theta is written in the W - 1 convention and the quirk is kept). The position is formed in f64, the four weights come from the
 * unclamped coordinates, a corner outside [0,W) x [0,H) contributes nothing (zero padding, no clamping). Every row is pooled as it
 * stands: an all-zero padding row samples G*G times at one map point.
 * -> out (B * R, G*G, C) f32, 16-byte aligned: row (n, j * G + i) holds the C channels of that grid point; the reference's
 *    (B*R, C, G, G) tensor is out viewed (n, G, G, C) and permuted (0, 3, 1, 2). 16-byte gathers and stores along C, no atomics:
 *    bit-identical from call to call. No backward (the reference detaches the map and the RoIs). One launch, no synchronisation.
 * CRB_ERR_ARG: C % 4 != 0, grid_size < 1, a non-positive cell, H or W < 2, roi_row_stride < 7, H*W*C >= 2^31, NULL / misaligned
 * pointers; CRB_ERR_UNSUPPORTED: grid_size > 16. */
int crb_roi_bev_pool(const float* bev, int B, int H, int W, int C, const float* rois, int roi_row_stride, int R, int grid_size,
                     double x_min, double y_min, double cell_x, double cell_y, float* out, void* stream);

/* voxel-neighbourhood RoI grid pooling of Voxel R-CNN (csrc/voxel_pool.hip)
 * replaces: voxel_query_kernel_stack (pcdet/ops/pointnet2/pointnet2_stack/src/voxel_query_gpu.cu:10-89) with the dense
 *           (B, Z, Y, X) index of common_utils.generate_voxel2pinds, VoxelQueryAndGrouping (voxel_query_utils.py:51-100) and the
 *           body of one NeighborVoxelSAModuleMSG scale (voxel_pool_modules.py:96-120: grouping, mlps_pos Conv2d + BatchNorm2d, add,
 *           ReLU, max / avg pooling over nsample).
 * crb_voxel_query: xyz (N,3) f32 voxel centres of the level's feature rows, new_xyz (M,3) f32 grid points, new_coords (M,4) i32
 *   [b, z, y, x] of the grid point AT THE LEVEL (16-byte aligned), shape_dhw / ranges_zyx HOST int32[3], hkeys / hvals / capacity the
 *   site hash of crb_sparse_hash_build over the level's (N,4) coordinates (any row order; no dense index is ever built).
 *   Per grid point: scan dz in [-rz, rz], then dy, then dx, ascending; skip sites outside [0,D) x [0,H) x [0,W) and sites without
 *   a voxel; skip neighbours with dist2 = (px-nx)^2 + (py-ny)^2 + (pz-nz)^2 > radius^2 in f32 (equality is a hit); keep the first
 *   nsample hits in scan order. -> idx (M, nsample) i32 GLOBAL feature rows, slots behind the last hit filled with the first hit;
 *   cnt (M) i32 = number of hits kept (0 .. nsample; the scan stops at the nsample-th). cnt == 0: the ball is empty, its idx
 *   row is all 0 and consumers read row 0 with features and relative xyz zeroed. A frame index outside [0, B) gives an empty ball.
 *   CRB_ERR_UNSUPPORTED: nsample > 32 or a range > 4.
 * crb_voxel_pool_moments: sums (9) f64 = {sum dx, dy, dz, sum dx dx, dx dy, dx dz, dy dy, dy dz, dz dz} over ALL M * nsample
 *   slots, d = xyz[idx] - new_xyz in f32 (fill slots counted again, empty balls count nsample zeros), accumulated in f64 in a fixed
 *   order (bit-reproducible). mlps_pos is linear in d, so the batch statistics of its BatchNorm2d are w.mu and w^T Sigma w.
 * crb_voxel_pool_forward: out[m,c] = pool_s relu(features_in[idx[m,s], c] + A[c,0] dx + A[c,1] dy + A[c,2] dz + b[c]), pool = 0
 *   max / 1 avg over the nsample slots; A (C,3), b (C) = mlps_pos with its BatchNorm2d folded in. An empty ball yields relu(b)
 *   (the reference's quirk: features and d are zeroed, the bias of the folded BatchNorm is not). features_in (N,C) / out (M,C)
 *   f32, 16-byte aligned. Nothing of size (M, C, nsample) or (M, 3, nsample) is written in either direction.
 * crb_voxel_pool_backward: recomputes the values from idx. grad_out (M,C) -> d_Ab (C,4) f32 rows {dA x, dA y, dA z, db} (per-
 *   workgroup partials in the workspace, reduced in f64 in a fixed order: reproducible) and the gradient of features_in either
 *   - d_features (N,C) != NULL: ADDED with f32 atomics (the caller zero-fills; the summation order, hence the last bits, vary
 *     from call to call), or
 *   - d_features == NULL, max pooling: g_sel (M,C) f32 / a_row (M,C) i32 = the gradient and the feature row it belongs to (-1:
 *     none), for a deterministic scatter by the caller. Avg pooling: CRB_ERR_UNSUPPORTED.
 *   Max pooling passes the gradient to the first maximal slot; a maximum of 0 (ReLU inactive) and empty balls pass none.
 * Supported (crb_voxel_pool_supported, host): C in {32, 64}, 1 <= nsample <= 32; anything else CRB_ERR_UNSUPPORTED. */
int crb_voxel_pool_supported(int C, int nsample);
int crb_voxel_query(const float* xyz, int64_t N, const float* new_xyz, const int32_t* new_coords, int64_t M, int B,
                    const int32_t* shape_dhw, const int32_t* ranges_zyx, float radius, int nsample, const int64_t* hkeys,
                    const int32_t* hvals, int64_t capacity, int32_t* idx, int32_t* cnt, void* stream);
int64_t crb_voxel_pool_moments_workspace_bytes(int64_t M);
int crb_voxel_pool_moments(const float* xyz, const float* new_xyz, const int32_t* idx, const int32_t* cnt, int64_t M, int nsample,
                           double* sums, void* workspace, int64_t workspace_bytes, void* stream);
int crb_voxel_pool_forward(const float* features_in, int64_t N, int C, const float* xyz, const float* new_xyz, const int32_t* idx,
                           const int32_t* cnt, int64_t M, int nsample, int pool, const float* A, const float* b, float* out,
                           void* stream);
int64_t crb_voxel_pool_backward_workspace_bytes(int64_t M, int C);
int crb_voxel_pool_backward(const float* grad_out, const float* features_in, int64_t N, int C, const float* xyz,
                            const float* new_xyz, const int32_t* idx, const int32_t* cnt, int64_t M, int nsample, int pool,
                            const float* A, const float* b, float* d_features, float* g_sel, int32_t* a_row, float* d_Ab,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* Pillar feature net of PointPillars (csrc/pillar_vfe.hip)
 * replaces: PillarVFE.forward + PFNLayer.forward (pcdet/models/backbones_3d/vfe/pillar_vfe.py:29-49, 94-123) with one PFN layer:
 *           the (M, T, K) augmented points, Linear(K -> 64, bias=False), BatchNorm1d(64) on (M, 64, T), ReLU, max over T - three
 *           (M, T, 64) tensors each way in the reference, none here.
 * voxels (M, T, C) f32, num_points (M) i32, coords (M, 4) i32 [b, z, y, x] (16-byte aligned), voxel_size (3) / offsets (3) HOST f32
 * {x, y, z}, offsets = voxel / 2 + range_min. Only the slots t < num_points[m] (clamped to 0 .. T) are read.
 * Augmented point of a valid slot, K = C + 6: f = [point (C), xyz - mean_xyz, xyz - centre]; mean_xyz = sum over the valid slots
 * (in f64) / num_points, rounded to f32; centre = (float)coord * voxel + offset in f32, two roundings. Padded slots: f = 0.
 * crb_pillar_vfe_moments: sums (crb_pillar_vfe_num_moments(C) = (K+1)(K+2)/2 - 1) f64 = the upper triangle of sum g g^T over the valid
 *   slots, g = [f, 1], rows i = 0 .. K-1 one after the other, row i holding columns j = i .. K (column K: sum f_i). Products and sums
 *   in f64, per-workgroup partials reduced in a fixed order: bit-reproducible. Two launches.
 * crb_pillar_vfe_forward: A (Cout, K), b (Cout) -> out (M, Cout) = max over ALL T slots of relu(A f + b); a padded slot has the value
 *   relu(b) (the reference's quirk: its BatchNorm1d sees the zero rows). One launch, nothing of size (M, T, .) is written.
 * crb_pillar_vfe_backward: grad_out (M, Cout) -> d_sums (Cout, K + 1) f64: row c = {sum dy f^T (K), sum dy} over the selected slots,
 *   dy = grad_out where the slot is the first maximal one of its pillar and channel and the maximum is > 0 (a selected padded slot
 *   adds to sum dy only). f32 inside a workgroup, f64 across workgroups in a fixed order: bit-reproducible. Two launches. There is no
 *   gradient to the points.
 * Supported (crb_pillar_vfe_supported, host): C in {4, 5}, 1 <= T <= 32, Cout == 64; anything else CRB_ERR_UNSUPPORTED. */
int crb_pillar_vfe_supported(int C, int T, int Cout);
int crb_pillar_vfe_num_moments(int C);
int64_t crb_pillar_vfe_moments_workspace_bytes(int64_t M, int C);
int crb_pillar_vfe_moments(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M, int T, int C,
                           const float* voxel_size, const float* offsets, double* sums, void* workspace, int64_t workspace_bytes,
                           void* stream);
int crb_pillar_vfe_forward(const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M, int T, int C,
                           const float* voxel_size, const float* offsets, const float* A, const float* b, int Cout, float* out,
                           void* stream);
int64_t crb_pillar_vfe_backward_workspace_bytes(int64_t M, int C, int Cout);
int crb_pillar_vfe_backward(const float* grad_out, const float* voxels, const int32_t* num_points, const int32_t* coords, int64_t M,
                            int T, int C, const float* voxel_size, const float* offsets, const float* A, const float* b, int Cout,
                            double* d_sums, void* workspace, int64_t workspace_bytes, void* stream);

/* LLAL loss-prediction module (csrc/loss_net.hip)
 * replaces: LossNet.forward (pcdet/models/roi_heads/loss_net.py:54-70) and its autograd: per shared-FC layer k a Conv1d(C_k -> 1,
 *           k=1, bias=False) over the R = frames * rows_per_frame RoI rows, BatchNorm1d(1) (train mode: batch statistics over the R
 *           rows, running_mean / running_var updated with `momentum` and the unbiased variance, num_batches_tracked += 1; eval mode:
 *           the running statistics), ReLU, view(frames, rows_per_frame), cat over k, Linear(num_layer * rows_per_frame -> 1).
 *           ~12 torch launches each way per layer.
 * x[k] (R, channels[k]) f32 row-major: the post-ReLU output of shared FC layer k (pvrcnn_head.py:163-176); w[k] (channels[k]) the
 * conv weight; gamma / beta / running_mean / running_var (1) and num_batches_tracked (1) i64 of bn_k; lin_w (num_layer *
 * rows_per_frame), lin_b (1) -> out (frames) f32. Accumulation in f64, every sum in a fixed order, no atomics: bit-reproducible.
 * crb_lossnet_forward: two launches. ws (crb_lossnet_workspace_bytes) keeps what the backward reads; hand the same ws to it.
 * crb_lossnet_backward: two launches. d_out (frames) upstream gradient -> d_x[k] (R, channels[k]) (NULL: not formed), d_w[k]
 * (channels[k]), d_gamma_beta (2 * num_layer: gamma_k at 2k, beta_k at 2k + 1), d_lin_w, d_lin_b (1); all written, none added to.
 * ---------------------------------------------------------------------------------------------- */
#define CRB_LOSSNET_MAX_LAYERS 4
typedef struct CrbLossNetArgs {
  const float* x[CRB_LOSSNET_MAX_LAYERS];
  const float* w[CRB_LOSSNET_MAX_LAYERS];
  const float* gamma[CRB_LOSSNET_MAX_LAYERS];
  const float* beta[CRB_LOSSNET_MAX_LAYERS];
  float* running_mean[CRB_LOSSNET_MAX_LAYERS];
  float* running_var[CRB_LOSSNET_MAX_LAYERS];
  int64_t* num_batches_tracked[CRB_LOSSNET_MAX_LAYERS];
  int32_t channels[CRB_LOSSNET_MAX_LAYERS];
  int32_t num_layer;             /* 1 .. CRB_LOSSNET_MAX_LAYERS */
  int32_t rows_per_frame;        /* TARGET_CONFIG.ROI_PER_IMAGE */
  int32_t frames;                /* batch size */
  int32_t training;              /* 1: batch statistics + running-statistics update; 0: running statistics */
  float momentum, eps;           /* bn_k.momentum (not None), bn_k.eps */
} CrbLossNetArgs;
typedef struct CrbLossNetGrads {
  float* d_x[CRB_LOSSNET_MAX_LAYERS];
  float* d_w[CRB_LOSSNET_MAX_LAYERS];
  float* d_gamma_beta;
  float* d_lin_w;
  float* d_lin_b;
} CrbLossNetGrads;
int64_t crb_lossnet_workspace_bytes(int num_layer, int64_t rows);
int crb_lossnet_forward(const CrbLossNetArgs* args, const float* lin_w, const float* lin_b, float* out, void* ws, int64_t ws_bytes,
                        void* stream);
int crb_lossnet_backward(const CrbLossNetArgs* args, const float* lin_w, const float* d_out, void* ws, int64_t ws_bytes,
                         const CrbLossNetGrads* grads, void* stream);

/* Anchor-free centre head of CenterPoint (csrc/center_head.hip)
 * replaces: CenterHead.assign_targets + assign_target_of_single_head (pcdet/models/dense_heads/center_head.py:103-219) with
 *           centernet_utils.gaussian_radius / gaussian2D / draw_gaussian_to_heatmap (pcdet/models/model_utils/centernet_utils.py:9-69):
 *           three nested Python loops over heads, frames and boxes on the host, one .item() and one numpy window per box;
 *           CenterHead.get_loss (:225-251) with FocalLossCenterNet / RegLossCenterNet (pcdet/utils/loss_utils.py:264-386): ~25 launches
 *           per head and an .item() per term; decode_bbox_from_heatmap (centernet_utils.py:154-216) behind its top-K.
 * Maps are (B, C, H, W) f32 addressed as b * C*H*W + c * stride_c + (y * W + x) * stride_p: {H*W, 1} is NCHW memory, {1, C} is
 * channels_last memory; the maps are read (and their gradients written) where the convolutions left them.
 *
 * crb_center_assign_targets: gt_boxes (B, M, box_dim) f32, box_dim = 7 + E + 1, class (1 .. num_class, anything else: no object) in
 *   the last column. class_head / class_local (num_class) HOST i32: the head that names class c + 1 (-1: none) and its index there.
 *   head_channels (num_heads) HOST i32. Outputs, all zeroed inside the sequence: heatmaps = the heads' (B, C_h, H, W) NCHW blocks one
 *   after the other; target_boxes (num_heads, B, NMAX, 8 + E) f32; inds (num_heads, B, NMAX) i64 = y * W + x; masks (num_heads, B,
 *   NMAX) i64. The slot of a box is its rank among the frame's boxes of the same head in input order; ranks >= NMAX are dropped; a
 *   box with dx <= 0 or dy <= 0 keeps its slot, which stays zero. Centre, radius and the copied columns in f32 as the reference
 *   rounds them (gaussian_overlap is a double: its derived constants 1 - o, 1 + o, ... are formed in f64 and rounded to f32 once, as
 *   torch rounds a Python scalar); log / cos / sin and the Gaussian in f64, rounded once. Overlaps combine by an integer atomicMax on the bit pattern
 *   of the non-negative values: bit-reproducible. Two launches (slots, draw) and five memsets. Limits: num_class <= 16, num_heads <= 8,
 *   E <= 8 (else CRB_ERR_UNSUPPORTED).
 * crb_center_loss_forward (one head): hm logits + heatmap -> loss (2) f64 = {hm_loss * cls_weight, loc_loss * loc_weight},
 *   stats (2) f64 = {num_pos, sum of masks} for the backward. Sigmoid clamped to [1e-4, 1 - 1e-4]; num_pos over the whole batch;
 *   num_pos == 0: -neg_loss undivided. Regression: masked L1 of the maps of `reg` (HEAD_ORDER) gathered at inds against
 *   target_boxes, per-column sums / max(sum mask, 1), times code_weights. Terms and sums in f64, per-workgroup partials added in a
 *   fixed order: bit-reproducible. Two launches.
 * crb_center_loss_backward: grad_loss (2) f32 -> d_hm (layout of hm; zero outside the clamp range) and d_reg maps (layout of
 *   the reg maps: zero-filled, (+/-) code_weight * loc_weight / num at the inds cells, objects of one cell counted in integers
 *   before the product). One launch, no atomics on floats.
 *   NMAX <= 4096, else CRB_ERR_UNSUPPORTED from the forward AND the backward (the Python route takes the torch route there).
 * crb_center_decode (one head): top_val / top_idx (B, K) = logits and flat indices picked from the (C * H * W) logits of a frame
 *   (idx_channels_last = 0: c * H*W + cell, 1: cell * C + c) -> boxes (B, K, 7 + vel channels) = {x, y, z, exp(dim), atan2(sin, cos),
 *   vel}, scores (B, K) = sigmoid, labels (B, K) i64 (class in head), keep (B, K) u8 = inside limit_range (6, HOST) on x, y, z and
 *   score > score_thresh. `reg` holds center, center_z, dim, rot (+ vel) in this order. One launch.
 * ---------------------------------------------------------------------------------------------- */
#define CRB_CENTER_MAX_MAPS 8
#define CRB_CENTER_MAX_CODE 16
typedef struct CrbCenterMaps {
  const float* ptr[CRB_CENTER_MAX_MAPS];      /* (B, channels[i], H, W) */
  float* grad[CRB_CENTER_MAX_MAPS];           /* backward only: same layout as ptr[i] */
  int64_t stride_c[CRB_CENTER_MAX_MAPS];
  int64_t stride_p[CRB_CENTER_MAX_MAPS];
  int32_t channels[CRB_CENTER_MAX_MAPS];
  int32_t num_maps;
} CrbCenterMaps;
typedef struct CrbCenterLossCfg {
  float code_weights[CRB_CENTER_MAX_CODE];
  float cls_weight, loc_weight;
} CrbCenterLossCfg;
int64_t crb_center_assign_workspace_bytes(int num_heads, int B, int num_max_objs);
int crb_center_assign_targets(const float* gt_boxes, int B, int M, int box_dim, int num_class, const int32_t* class_head,
                              const int32_t* class_local, int num_heads, const int32_t* head_channels, int H, int W,
                              const float* pc_range_xy, const float* voxel_size_xy, int feature_map_stride, int num_max_objs,
                              double gaussian_overlap, int min_radius, float* heatmaps, float* target_boxes, int64_t* inds,
                              int64_t* masks, void* workspace, int64_t workspace_bytes, void* stream);
int64_t crb_center_loss_workspace_bytes(int B, int H, int W);
int crb_center_loss_forward(const float* hm, int64_t hm_stride_c, int64_t hm_stride_p, const float* heatmap, int B, int C, int H, int W,
                            const CrbCenterMaps* reg, const float* target_boxes, const int64_t* inds, const int64_t* masks,
                            int num_max_objs, const CrbCenterLossCfg* cfg, double* loss, double* stats, void* workspace,
                            int64_t workspace_bytes, void* stream);
int crb_center_loss_backward(const float* hm, int64_t hm_stride_c, int64_t hm_stride_p, const float* heatmap, int B, int C, int H, int W,
                             const CrbCenterMaps* reg, const float* target_boxes, const int64_t* inds, const int64_t* masks,
                             int num_max_objs, const CrbCenterLossCfg* cfg, const double* stats, const float* grad_loss, float* d_hm,
                             void* stream);
int crb_center_decode(const float* top_val, const int64_t* top_idx, int B, int K, int C, int H, int W, int idx_channels_last,
                      const CrbCenterMaps* reg, const float* pc_range_xy, const float* voxel_size_xy, int feature_map_stride,
                      const float* limit_range, float score_thresh, float* boxes, float* scores, int64_t* labels, uint8_t* keep,
                      void* stream);

/* Dynamic voxelization and the segmented mean (csrc/dyn_voxelize.hip)
 * replaces: the grouping of DynamicPillarVFE.forward (pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:93-103, 132-138) and
 *           DynamicMeanVFE.forward (dynamic_mean_vfe.py:53-72): floor / mask / merge_coords / torch.unique(return_inverse) /
 *           torch_scatter.scatter_mean. Every point in range belongs to its voxel: no cap on points per voxel, none on voxels.
 * points (n_points, row_stride) f32 rows [b, x, y, z, ...]; frames need not be contiguous. b = (int)column 0, truncated as .int()
 * does; rows with b outside 0 .. B - 1 are dropped. Cell c = floorf(__fdiv_rn(__fsub_rn(p, min), voxel)) per axis in f32 (torch's
 * arithmetic); a point is kept iff 0 <= c < grid on every masked axis. A NaN in b, x, y or z drops the point in both modes.
 *   CRB_DYN_PILLAR: x and y masked (z is NOT, as in the reference), key = (b * gx + cx) * gy + cy,            coords = [b, 0, cy, cx]
 *   CRB_DYN_VOXEL:  x, y and z masked,                              key = ((b * gx + cx) * gy + cy) * gz + cz, coords = [b, cz, cy, cx]
 * Keys are 64-bit. range_min_xyz / voxel_size_xyz (3) HOST f32, grid_xyz (3) HOST i32 (each < 2^24).
 * Outputs: counts (2) i32 = {M voxels, Nk kept points}; perm (n_points) i32: its first Nk entries are the kept point rows, voxel by
 * voxel in ascending key order (torch.unique's order), input order inside a voxel (a stable radix sort over the bits of the key
 * range only); seg_offsets (max_voxels + 1) i32: voxel v owns perm[seg_offsets[v] .. seg_offsets[v + 1]), seg_offsets[M] = Nk;
 * coords (max_voxels, 4) i32, rows 0 .. M - 1 written. max_voxels >= min(n_points, B * cells per frame), else CRB_ERR_ARG.
 * n_points == 0: counts and seg_offsets[0] are zeroed, nothing is launched. No atomics: bit-reproducible.
 * crb_dyn_mean_vfe: out (M, C) f32 = mean over the voxel's points of columns 1 .. C of `points`: an f64 sum in segment order,
 *   divided in f64, rounded once. M == 0: nothing is launched. One launch.
 * crb_dyn_canonical_order: perm_out (n_kept) i32 = perm with the points of every voxel re-ordered by content: ascending in the bit
 *   patterns (as unsigned) of feature columns 1 .. C, column 1 most significant; rows of equal content keep their order. A sum in
 *   segment order over perm_out depends on the multiset of input rows only, not on their order. perm_out != perm. C stable 32-bit
 *   radix sorts and one over the bits of M; workspace crb_dyn_canonical_order_workspace_bytes(n_kept). n_kept == 0: no launch. */
#define CRB_DYN_PILLAR 0
#define CRB_DYN_VOXEL 1
int64_t crb_dyn_voxelize_workspace_bytes(int64_t n_points);
int crb_dyn_voxelize(const float* points, int64_t n_points, int row_stride, int B, int mode, const float* range_min_xyz,
                     const float* voxel_size_xyz, const int32_t* grid_xyz, int64_t max_voxels, int32_t* perm, int32_t* seg_offsets,
                     int32_t* coords, int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int crb_dyn_mean_vfe(const float* points, int64_t n_points, int row_stride, int C, const int32_t* perm, const int32_t* seg_offsets,
                     int64_t M, float* out, void* stream);
int64_t crb_dyn_canonical_order_workspace_bytes(int64_t n_kept);
int crb_dyn_canonical_order(const float* points, int64_t n_points, int row_stride, int C, const int32_t* perm, int64_t n_kept,
                            const int32_t* seg_offsets, int64_t M, int32_t* perm_out, void* workspace, int64_t workspace_bytes,
                            void* stream);

/* Two-layer pillar feature net of DynamicPillarVFE over variable-length segments (csrc/dyn_pillar_vfe.hip)
 * replaces: PFNLayerV2.forward x 2 and the feature augmentation of DynamicPillarVFE.forward (pcdet/models/backbones_3d/vfe/
 *           dynamic_pillar_vfe.py:35-46, 105-124) with NUM_FILTERS [64, 64]: six or seven (N, 64) f32 tensors kept for the backward
 *           pass in the reference, nothing of size (N, .) here but the sorted point order.
 * Segments: perm / seg_offsets / coords of crb_dyn_voxelize in CRB_DYN_PILLAR mode, perm passed through crb_dyn_canonical_order
 * where the results must not depend on the order of the input rows (all sums run in segment order); pillar_mean (M, C) of crb_dyn_mean_vfe (columns
 * 0 .. 2 are read). Augmented point, K = C + 6: f = [point (C), xyz - pillar mean, x - ((float)cx * vx + ox), y - ((float)cy * vy +
 * oy), z - oz]; voxel_xy (2) / offsets (3) HOST f32, offsets = voxel / 2 + range_min.
 * Layer 1: x1 = relu(A1 f + b1), A1 (32, K), b1 (32) the folded affine; x_max (32) = its maximum over the pillar. Layer 2: y =
 * W2 [x1; x_max], W2 (64, 64) the raw weight; v = scale2 y + shift2; out = max over the pillar of relu(v).
 * crb_dyn_pillar_moments: sums (crb_dyn_pillar_num_moments(C)) f64, the layout of crb_pillar_vfe_moments, over all kept points.
 * crb_dyn_pillar_stats2: sums (128) f64 = {sum y (64), sum y^2 (64)} over all kept points.
 * crb_dyn_pillar_forward: out (M, 64). One launch; a pillar is walked twice.
 * crb_dyn_pillar_backward_a: arg2 (M, 64) i32 = position in its segment of the first maximal point of v per pillar and channel, -1
 *   where the maximum is <= 0; sums (128) f64 = {sum dy2, sum dy2 yhat2}, dy2 = grad_out at the selected points, yhat2 = (y - mean2)
 *   inv_sigma2.
 * crb_dyn_pillar_backward_b: d_sums (64 * 64 + 32 * 12) f64 = dW2 (64, 64) = sum dx2 [x1; x_max]^T with dx2 = scale2 (dy2 - k1 -
 *   yhat2 k2) over ALL points, then rows j = 0 .. 31 of 12: {G1[j] = sum dy1 f^T (K), G0[j] = sum dy1 at column K, zeros}, dy1 = the
 *   gradient at the layer-1 BatchNorm output (own W2^T dx2 half, plus the pillar sum of the x_max half at the first maximal point of
 *   the channel, ReLU mask applied). k1 = sum dy2 / n, k2 = dgamma2 / n in training, zeros in eval mode.
 * Sums: f32 inside a workgroup at most, f64 across workgroups in a fixed order, no atomics: bit-reproducible. workspace:
 * crb_dyn_pillar_workspace_bytes(M) for every call. Supported (crb_dyn_pillar_vfe_supported, host): C in {4, 5}, two layers of 64
 * filters; anything else CRB_ERR_UNSUPPORTED. M >= 1. There is no gradient to the points. */
typedef struct CrbDynPillarArgs {
  const float* points;          /* (n_points, row_stride) rows [b, x, y, z, ...] */
  const int32_t* perm;          /* (Nk) */
  const int32_t* seg_offsets;   /* (M + 1) */
  const int32_t* coords;        /* (M, 4) [b, 0, cy, cx] */
  const float* pillar_mean;     /* (M, C) */
  const float* A1;              /* (32, K) */
  const float* b1;              /* (32) */
  const float* W2;              /* (64, 64) */
  const float* scale2;          /* (64) */
  const float* shift2;          /* (64) */
  const float* mean2;           /* (64) backward */
  const float* inv_sigma2;      /* (64) backward */
  const float* k1;              /* (64) backward_b */
  const float* k2;              /* (64) backward_b */
  int64_t n_points;
  int64_t M;
  int32_t row_stride;
  int32_t C;
  float voxel_xy[2];
  float offsets[3];
} CrbDynPillarArgs;
int crb_dyn_pillar_vfe_supported(int C, int num_layers, int filters0, int filters1);
int crb_dyn_pillar_num_moments(int C);
int64_t crb_dyn_pillar_workspace_bytes(int64_t M);
int crb_dyn_pillar_moments(const CrbDynPillarArgs* args, double* sums, void* workspace, int64_t workspace_bytes, void* stream);
int crb_dyn_pillar_stats2(const CrbDynPillarArgs* args, double* sums, void* workspace, int64_t workspace_bytes, void* stream);
int crb_dyn_pillar_forward(const CrbDynPillarArgs* args, float* out, void* stream);
int crb_dyn_pillar_backward_a(const CrbDynPillarArgs* args, const float* grad_out, int32_t* arg2, double* sums, void* workspace,
                              int64_t workspace_bytes, void* stream);
int crb_dyn_pillar_backward_b(const CrbDynPillarArgs* args, const float* grad_out, const int32_t* arg2, double* d_sums, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* Sectorized proposal-centric keypoint sampling (csrc/spc_sampling.hip)
 * replaces: sample_points_with_roi and sector_fps (pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py:45-121) with the per-frame
 *           loop of get_sampled_points (:250-274), and stack_farthest_point_sampling_kernel (pointnet2_stack/src/sampling_gpu.cu).
 * All frames of a batch share every launch; nothing is read back between the three calls.
 * `points`: the address of the x column of row 0 of an f32 matrix with `row_stride` floats per row (x, y, z adjacent); rows are
 * stacked frame by frame, frame b = rows frame_offsets[b] .. frame_offsets[b + 1] (device i32, B + 1 ascending entries).
 * crb_roi_proximity_mask: rois (B, R, roi_stride >= 6) [x, y, z, dx, dy, dz, ...], zero rows included like any other. Per point
 *   mask = min_r |p - c_r| < |dims_nearest / 2| + radius (f32; nearest = the lowest r of the minimum), nearest (n) i32 or NULL.
 *   R == 0: nothing is kept.
 * crb_spc_plan: mask (n) u8 as above. sector (n) u8 = floor((atan2f(y, x) + pi) * inv_sector_size) clamped to [0, S] for EVERY point
 *   (inv_sector_size = 1.f / (float)(2 pi / S)); a frame with points but none kept keeps its first point; kept points of sector S
 *   belong to no segment unless all kept points of the frame do (then they are the frame's one segment, m = min(n, K)). Segments are
 *   ordered by (frame, sector); segment j = seg_table[8 j ..] = {first row of xyz_out, n, m, first output row, frame, 0, 0, 0} with
 *   m = min(n, ceil(((double)n / (double)kept_in_frame) * (double)K)); xyz_out (n, 3) / src_idx (n): the segments' points in input
 *   order and their rows in `points`; seg_table holds B * S rows; header (3 + B) i32 = {segments, rows of xyz_out, keypoints,
 *   keypoints of frame 0 .. B - 1}. B * (S + 1) <= 4096, S <= 254.
 * crb_fps_segments: one 1024-thread workgroup per table row (rows past *num_segments, a device i32 or NULL, do nothing; rows that
 *   point outside `rows` / `out_capacity` are skipped). First pick = the segment's first point, running distances start at 1e10,
 *   ties as the reference's 1024-thread scan + tree. out_idx (out_capacity) rows of xyz, out_keypoints (out_capacity, 4)
 *   [frame, x, y, z]; either may be NULL. temp (rows) f32 is needed when rows > 20480 (a segment may be that long:
 *   up to 20480 points a segment keeps coordinates and distances in registers, beyond that the distances live in temp). */
int crb_roi_proximity_mask(const float* points, int64_t n, int row_stride, const int32_t* frame_offsets, int B, const float* rois, int R,
                           int roi_stride, float radius, uint8_t* mask, int32_t* nearest, void* stream);
int64_t crb_spc_plan_workspace_bytes(int B, int S);
int crb_spc_plan(const float* points, int64_t n, int row_stride, const int32_t* frame_offsets, int B, const uint8_t* mask, int S, int K,
                 float inv_sector_size, uint8_t* sector, float* xyz_out, int32_t* src_idx, int32_t* seg_table, int32_t* header,
                 void* workspace, int64_t workspace_bytes, void* stream);
int crb_fps_segments(const float* xyz, int64_t rows, const int32_t* seg_table, const int32_t* num_segments, int max_segments,
                     int64_t out_capacity, float* temp, int32_t* out_idx, float* out_keypoints, void* stream);

/* KITTI object AP: image / BEV / 3D overlaps, ignore flags, true-positive scores, score thresholds, precision-recall counts
 * (csrc/kitti_eval.hip)
 * replaces: rotate_iou_gpu_eval (pcdet/datasets/kitti/kitti_object_eval_python/rotate_iou.py, numba.cuda) and image_box_overlap,
 *           d3_box_overlap_kernel, clean_data, compute_statistics_jit, get_thresholds, fused_compute_statistics of eval.py there
 *           (numba.jit), with the per-frame / per-part Python loops of calculate_iou_partly and eval_class around them.
 * Every call launches on `stream` and returns without waiting; nothing is read back between the calls.
 * Layout: the boxes of all frames are stacked. gt_off / dt_off / pair_off (num_frames + 1) i64 prefix sums of the ground-truth boxes,
 *   detections and (detection, ground truth) pairs of a frame; the pairs of frame f form a row-major [n_dt, n_gt] matrix at pair_off[f].
 *   bbox (n, 4) f64 [x1, y1, x2, y2]; cam (n, 7) f64 [x, y, z, l, h, w, ry] in rect camera coordinates, y the bottom centre.
 *   A combination q < num_combos is one (metric, class, difficulty, overlap row): combo_metric[q] in 0..2 (image, BEV, 3D),
 *   combo_flags[q] = class index * 3 + difficulty (the row of gt_flag / dt_flag), combo_min_overlap[q] f64, combo_aos[q] = the slot of
 *   its orientation-similarity sums in 0 .. num_aos - 1 or -1 for none.
 * crb_kitti_overlaps: overlaps (4, num_pairs) f64 = image-box IoU (f64), BEV IoU (f32 arithmetic on the pair translated to the
 *   ground-truth centre, positive ry clockwise), 3D IoU (BEV intersection x height overlap min(y1, y2) - max(y1 - h1, y2 - h2), zero
 *   when not positive, union = sum of l h w minus the intersection; rounded to f32), image intersection over the detection's area
 *   (the DontCare criterion).
 * crb_kitti_ignore_flags: cls i32 0..5 = car, pedestrian, cyclist, van, person_sitting, truck, anything else for other names;
 *   classes (num_classes) i32 device array of the evaluated classes; gt_flag (num_classes * 3, G) / dt_flag (num_classes * 3, D) i8:
 *   0 counts, 1 ignored, -1 another class; difficulty limits as clean_data (<= on the ground-truth height, < on |height| of a detection).
 * crb_kitti_match_scores: the compute_fp = False, thresh = 0 matching of every (frame, combination). tp_scores (num_combos, G) f64:
 *   the matched detection's score in the slot of its ground-truth box, -inf elsewhere. asg_off (num_frames + 1) i64 prefix sums of
 *   ceil(n_dt / 32); asg_workspace asg_off[num_frames] * num_combos u32.
 * crb_kitti_thresholds: sorted_scores (num_combos, G) f64 descending with num_scores[q] leading entries, num_valid_gt (num_combos)
 *   i32 -> thresholds (num_combos, 41) f64 and num_thresholds (num_combos) i32 by get_thresholds' skip rule.
 * crb_kitti_match_pr: the compute_fp = True matching of every (frame, combination, threshold). gt_dc (G) u8 marks DontCare boxes.
 *   Frames beyond crb_kitti_stage_limit (0: n_gt, 1: n_dt, 2: n_gt * n_dt) read global memory and keep their bits in asg_big:
 *   big_off (num_frames + 1) i64 prefix sums of ceil(n_dt / 32) for those frames and 0 for the others, asg_big big_off[num_frames] *
 *   num_combos * 64 u32. counts (num_combos, 41, 3) i32 and sim_part (num_frames, num_aos, 41) f64 are scratch.
 *   result (num_combos * 41 * 5 + num_combos) f64: rows [tp, fp, fn, similarity, threshold] per (combination, threshold), then the
 *   number of thresholds of every combination. Integer counts by integer atomics, the similarity summed over frames in frame order:
 *   the same bits on every run. */
int crb_kitti_stage_limit(int which);
int crb_kitti_overlaps(const int64_t* gt_off, const int64_t* dt_off, const int64_t* pair_off, int64_t num_frames, int64_t num_pairs,
                       const double* gt_bbox, const double* dt_bbox, const double* gt_cam, const double* dt_cam, double* overlaps,
                       void* stream);
int crb_kitti_ignore_flags(const int32_t* gt_cls, const double* gt_occ, const double* gt_trunc, const double* gt_bbox, int64_t G,
                           const int32_t* dt_cls, const double* dt_bbox, int64_t D, const int32_t* classes, int num_classes,
                           int8_t* gt_flag, int8_t* dt_flag, void* stream);
int crb_kitti_match_scores(const int64_t* gt_off, const int64_t* dt_off, const int64_t* pair_off, const int64_t* asg_off,
                           int64_t num_frames, int64_t G, int64_t D, int64_t num_pairs, const double* overlaps, const int8_t* gt_flag,
                           const int8_t* dt_flag, const double* dt_score, const int32_t* combo_metric, const int32_t* combo_flags,
                           const double* combo_min_overlap, int num_combos, uint32_t* asg_workspace, double* tp_scores, void* stream);
int crb_kitti_thresholds(const double* sorted_scores, const int32_t* num_scores, const int32_t* num_valid_gt, int num_combos, int64_t G,
                         double* thresholds, int32_t* num_thresholds, void* stream);
int crb_kitti_match_pr(const int64_t* gt_off, const int64_t* dt_off, const int64_t* pair_off, const int64_t* big_off, int64_t num_frames,
                       int64_t G, int64_t D, int64_t num_pairs, const double* overlaps, const int8_t* gt_flag, const int8_t* dt_flag,
                       const double* dt_score, const uint8_t* gt_dc, const double* gt_alpha, const double* dt_alpha,
                       const int32_t* combo_metric, const int32_t* combo_flags, const double* combo_min_overlap,
                       const int32_t* combo_aos, int num_combos, int num_aos, const double* thresholds, const int32_t* num_thresholds,
                       uint32_t* asg_big, int32_t* counts, double* sim_part, double* result, void* stream);

/* VectorPool aggregation of PV-RCNN++ (csrc/vector_pool.hip)
 * replaces: query_stacked_local_neighbor_idxs + query_three_nn_by_stacked_local_idxs, vector_pool_kernel_stack (pooling_type 1) and
 *           vector_pool_grad_kernel_stack (pointnet2_stack/src/vector_pool_gpu.cu) with the host loops around them
 *           (ThreeNNForVectorPoolByTwoStep, VectorPoolWithVoxelQuery of pointnet2_utils.py:302-448), and three_interpolate, the
 *           coordinate gather, the two cats, the mask write and the permute of VectorPoolLocalInterpolateModule.forward
 *           (pointnet2_modules.py:212-238).
 * No neighbour list, cursor, retry or read-back; no float atomics. Rows are stacked frame by frame: xyz_batch_cnt / new_xyz_batch_cnt
 * (B) device i32. Frame of new point m: the reference's walk over new_xyz_batch_cnt (a point past the sum belongs to the last frame);
 * the frame's support rows are clamped to [0, N). G = number of cells <= 64 (CRB_ERR_UNSUPPORTED above).
 * crb_vector_pool_three_nn: local = support - new (f32); cube: dropped when any |local| > query_dist, ball (neighbor_type 1): when
 *   lx^2 + ly^2 + lz^2 > query_dist^2. Candidates: the frame's kept points in ascending row order, at most nsample (when > 0) and at
 *   most 1000. Per cell d = (cx-x)^2 + (cy-y)^2 + (cz-z)^2 (f32, that association), strict < against best1, best2, best3 in turn;
 *   missing second / third slots repeat the first; none: idx -1, dist +inf. idx (M, G, 3) i32 global rows, dist (M, G, 3) = sqrtf(d).
 * crb_vector_pool_interp_forward: out (G, M, C + 9): C channels w0 f0 + w1 f1 + w2 f2 with w_j = r_j / max(r0 + r1 + r2, 1e-8),
 *   r_j = 1 / (dist_j + 1e-8), then centre - xyz[idx_j] for j = 0..2; cells with idx < 0 are zeros and read no row (N = 0 is legal).
 *   Row indices are clamped to [0, N).
 * crb_vector_pool_interp_backward: grad_out (G, M, C + 9) -> grad_features (N, C), every row written. sorted_rows (E = 3 M G) i32
 *   ascending = idx flattened and stably sorted, order (E) i64 = the flat (m, g, j) position of each; row n sums its contributions in
 *   that order: the same bits on every run.
 * crb_vector_pool_voxel_forward: voxel_random_choice. The range test above with R; cell = floorf((local_a + R) / grid_size_a) per
 *   axis, combined x ny nz + y nz + z and THEN clamped to [0, G - 1]; the first point to reach an empty cell fills it; the scan stops
 *   after min(nsample, G) filled cells (G when nsample <= 0). new_features (M, G C) the picked rows' features (zeros for empty cells),
 *   new_local_xyz (M, 3 G), point_cnt (M, G) i32 0 / 1, pick (M, G) i32 the picked global row or -1.
 * crb_vector_pool_voxel_backward: grad_new_features (M, G C) -> grad_features (N, C); sorted_rows / order (E = M G) from `pick` as
 *   above. */
int crb_vector_pool_three_nn(const float* support_xyz, int64_t N, const int32_t* xyz_batch_cnt, const float* new_xyz, int64_t M,
                             const int32_t* new_xyz_batch_cnt, int B, const float* grid_centers, int G, float query_dist, int nsample,
                             int neighbor_type, int32_t* idx, float* dist, void* stream);
int crb_vector_pool_interp_forward(const int32_t* idx, const float* dist, const float* grid_centers, const float* support_xyz,
                                   const float* features, int64_t N, int64_t M, int G, int C, float* out, void* stream);
int crb_vector_pool_interp_backward(const float* grad_out, const float* dist, const int32_t* sorted_rows, const int64_t* order,
                                    int64_t N, int64_t M, int G, int C, float* grad_features, void* stream);
int crb_vector_pool_voxel_forward(const float* support_xyz, const float* features, int64_t N, const int32_t* xyz_batch_cnt,
                                  const float* new_xyz, int64_t M, const int32_t* new_xyz_batch_cnt, int B, int num_grid_x,
                                  int num_grid_y, int num_grid_z, float max_distance, float grid_size_x, float grid_size_y,
                                  float grid_size_z, int C, int nsample, int neighbor_type, float* new_features, float* new_local_xyz,
                                  int32_t* point_cnt, int32_t* pick, void* stream);
int crb_vector_pool_voxel_backward(const float* grad_new_features, const int32_t* sorted_rows, const int64_t* order, int64_t N,
                                   int64_t M, int G, int C, float* grad_features, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CRB_HIP_H */
