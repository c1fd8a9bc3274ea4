"""Shared inputs, the numpy restatement of voxel_query + grouping and the f64 pooling definition for the Voxel R-CNN tests
(tests/test_voxel_rcnn_cpu.py, tests/test_voxel_rcnn_gpu.py) and their golden generator (tests/golden/make_goldens_voxel_rcnn.py).
No reference import here: this module travels with the tests.

Lengths of a level case are multiples of u = 0.05 * stride, the level's voxel edge in x / y (0.1 * stride in z): the level shape is
(Z, Y, X) = (5, 24, 20) for every stride and the pool radius 4 u is the configuration's (0.4 at stride 2, 1.6 at stride 8).
Margin safety is asserted, not measured: no grid coordinate lies within 1e-4 of a voxel face and no neighbour within `radius_margin`
(relative) of radius^2 in f64, so index comparisons are exact without excluding a point. radius_margin is 1e-4 where a seed can meet
it (case b). Case a (G = 6, ranges [4, 4, 4]) holds 97,451 (grid point, voxel) pairs inside the integer windows, about ten of which
fall within 1e-4 of the ball surface in ANY draw (forty seeds gave 1e-7 .. 5e-5): no seed meets 1e-4 there, and points are not
masked. Its margin is 1e-5: the f32 evaluation of dist2 (three differences, three products, two sums) is within 6 ulp = 4e-7
(relative) of the f64 value, with or without fused multiply-adds, 25 times below the margin."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_voxel_rcnn.npz')

VOXEL = [0.05, 0.05, 0.1]
SHAPE = (5, 24, 20)                                     # (Z, Y, X) at the level
B, R = 2, 3
N_VOX = (520, 470)                                      # unequal voxel counts
MARGIN = 1e-4

# name: stride, C_in, C (mlps_in / mlps_pos width), C_out, nsample, ranges (z, y, x), grid size, rows shuffled inside the frames
LEVEL_CASES = {
    'a': dict(stride=2, c_in=16, c=32, c_out=32, nsample=16, ranges=[4, 4, 4], grid=6, shuffled=False, seed=101, radius_margin=1e-5),
    'b': dict(stride=8, c_in=24, c=64, c_out=32, nsample=5, ranges=[1, 2, 4], grid=3, shuffled=True, seed=206, radius_margin=1e-4),
}
POOLS = ('max_pool', 'avg_pool')
MODULE_SEED = 57
ROWS = np.s_[::4]                                        # rows of the large per-row arrays the golden keeps
# RoI roles, row n = b * R + r of the case's RoI list
ROI_CLUSTER, ROI_BIG, ROI_PADDING, ROI_INSIDE, ROI_EMPTY, ROI_CORNER = 0, 1, 2, 3, 4, 5


def level_pcr(stride):
    """x / y / z minima chosen off the voxel lattice so that the all-zero padding RoI does not sit on a voxel face"""
    u = 0.05 * stride
    x0, y0, z0 = 0.43, -12 * u - 0.017, -3.03
    return [x0, y0, z0, x0 + SHAPE[2] * u, y0 + SHAPE[1] * u, z0 + SHAPE[0] * 2 * u]


def voxel_centers(coords_zyx, stride, pcr):
    """common_utils.get_voxel_centers in f32: (coords[z,y,x] flipped + 0.5) * (voxel_size * stride) + range minimum"""
    vs = (np.asarray(VOXEL, np.float32) * np.float32(stride)).astype(np.float32)
    return np.ascontiguousarray(((coords_zyx[:, ::-1].astype(np.float32) + np.float32(0.5)) * vs + np.asarray(pcr[:3], np.float32)).astype(np.float32))


def grid_points(rois, G):
    """get_global_grid_points_of_roi in f32 numpy: rois (n,7) -> (n, G^3, 3), grid index (ix, iy, iz) with iz fastest"""
    rois = np.asarray(rois, np.float32)
    g = np.arange(G)
    dense = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(1, -1, 3).astype(np.float32)
    size = rois[:, None, 3:6]
    local = (dense + np.float32(0.5)) / np.float32(G) * size - size / np.float32(2)
    c, s = np.cos(rois[:, 6]).astype(np.float32)[:, None], np.sin(rois[:, 6]).astype(np.float32)[:, None]
    x = local[..., 0] * c - local[..., 1] * s
    y = local[..., 0] * s + local[..., 1] * c
    return (np.stack([x, y, local[..., 2]], -1) + rois[:, None, 0:3]).astype(np.float32)


def level_case(name):
    """-> dict: coords (N,4) i32 [b,z,y,x], feats (N,c_in), rois (B,R,7), pcr, and the case's parameters"""
    p = dict(LEVEL_CASES[name])
    rng = np.random.default_rng(p['seed'])
    s = p['stride']
    u = 0.05 * s
    pcr = level_pcr(s)
    Z, Y, X = SHAPE
    x0, y0, z0 = pcr[:3]
    coords = []
    for b in range(B):
        occ = np.zeros(SHAPE, bool)
        occ.reshape(-1)[rng.choice(Z * Y * X, N_VOX[b], replace=False)] = True
        if b == 0:
            occ[:, 12:21, 10:19] = True                 # a fully occupied block under ROI_CLUSTER: more hits than nsample
        else:
            occ[:, :12, :11] = False                    # an emptied quarter around ROI_EMPTY
        zyx = np.argwhere(occ)                          # ascending (z, y, x)
        if p['shuffled']:
            zyx = zyx[rng.permutation(len(zyx))]
        coords.append(np.concatenate([np.full((len(zyx), 1), b), zyx], 1))
    coords = np.concatenate(coords, 0).astype(np.int32)
    feats = rng.normal(0, 1, (len(coords), p['c_in'])).astype(np.float32)
    zc = z0 + 5 * u                                      # mid height
    rois = np.zeros((B, R, 7), np.float32)
    rois[0, ROI_CLUSTER] = [x0 + 14.3 * u, y0 + 16.4 * u, zc + 0.2 * u, 5.1 * u, 3.3 * u, 4.2 * u, 0.4]
    rois[0, ROI_BIG] = [x0 + 10.2 * u, y0 + 12.3 * u, zc - 0.3 * u, 31.0 * u, 35.0 * u, 23.0 * u, -2.8]     # beyond every face, z < 0
    rois[1, ROI_INSIDE - R] = [x0 + 14.6 * u, y0 + 7.7 * u, zc + 0.6 * u, 6.2 * u, 4.4 * u, 5.3 * u, 1.9]
    rois[1, ROI_EMPTY - R] = [x0 + 5.1 * u, y0 + 5.6 * u, zc + 0.1 * u, 1.1 * u, 1.3 * u, 1.2 * u, 0.7]   # >= radius from any voxel
    rois[1, ROI_CORNER - R] = [x0 - 1.2 * u, y0 + 24.9 * u, z0 + 0.7 * u, 7.3 * u, 6.1 * u, 4.7 * u, -0.6]  # negative x / z coordinates, y beyond
    jitter = rng.uniform(-0.05 * u, 0.05 * u, (B, R, 6)).astype(np.float32)     # the seeded part of the boxes (see MARGIN)
    jitter[0, ROI_PADDING] = 0
    rois[:, :, :6] += jitter
    p.update(coords=coords, feats=feats, rois=rois, pcr=pcr, radius=float(np.float32(4 * u)), u=u)
    return p


def grid_voxel_coords(new_xyz, pcr, stride):
    """the reference's two float steps in f64-checked f32: ((xyz - min) // voxel_size) // stride -> (M,3) int [x,y,z]; asserts that
    no coordinate lies within MARGIN of a voxel face (then every float rule gives the same integers)"""
    q = (new_xyz.astype(np.float64) - np.asarray(pcr[:3], np.float32).astype(np.float64)) / np.asarray(VOXEL, np.float32).astype(np.float64)
    assert np.abs(q - np.round(q)).min() > MARGIN, 'a grid coordinate sits on a voxel face: change the seed / geometry'
    return np.floor(np.floor(q) / stride).astype(np.int64)


def case_query_inputs(p):
    """-> xyz (N,3) f32 voxel centres, new_xyz (M,3) f32, new_coords (M,4) int32 [b,z,y,x]"""
    G = p['grid']
    xyz = voxel_centers(p['coords'][:, 1:4], p['stride'], p['pcr'])
    new_xyz = grid_points(p['rois'].reshape(-1, 7), G).reshape(-1, 3)
    c = grid_voxel_coords(new_xyz, p['pcr'], p['stride'])
    b = np.repeat(np.arange(B), R * G ** 3)
    new_coords = np.stack([b, c[:, 2], c[:, 1], c[:, 0]], 1).astype(np.int32)
    return xyz, new_xyz, new_coords


def dense_index(coords, shape=SHAPE, batch=B):
    out = np.full((batch,) + tuple(shape), -1, np.int32)
    out[coords[:, 0], coords[:, 1], coords[:, 2], coords[:, 3]] = np.arange(len(coords), dtype=np.int32)
    return out


def _dist2_f32(p, n):
    d = (p - n).astype(np.float32)
    return ((d[..., 0] * d[..., 0]).astype(np.float32) + (d[..., 1] * d[..., 1]).astype(np.float32)).astype(np.float32) + \
        (d[..., 2] * d[..., 2]).astype(np.float32)


def voxel_query_np(ranges, radius, nsample, xyz, new_xyz, new_coords, point_indices):
    """restatement of voxel_query_kernel_stack + VoxelQuery.forward: the window is walked dz, dy, dx ascending for all grid points
    at once -> idx (M, nsample) int32 global rows, empty (M) bool"""
    Bn, Z, Y, X = point_indices.shape
    M = len(new_xyz)
    r2 = np.float32(radius) * np.float32(radius)
    idx = np.zeros((M, nsample), np.int32)
    cnt = np.zeros(M, np.int64)
    rows_m = np.arange(M)
    b = new_coords[:, 0].astype(np.int64)
    for dz in range(-ranges[0], ranges[0] + 1):
        z = new_coords[:, 1] + dz
        for dy in range(-ranges[1], ranges[1] + 1):
            y = new_coords[:, 2] + dy
            for dx in range(-ranges[2], ranges[2] + 1):
                x = new_coords[:, 3] + dx
                ok = (b >= 0) & (b < Bn) & (z >= 0) & (z < Z) & (y >= 0) & (y < Y) & (x >= 0) & (x < X)
                row = np.where(ok, point_indices[np.where(ok, b, 0), np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)], -1)
                hit = row >= 0
                d2 = _dist2_f32(xyz[np.maximum(row, 0)], new_xyz)
                hit &= ~(d2 > r2)
                first = hit & (cnt == 0)
                idx[first] = row[first, None]                              # the first hit fills every slot
                take = hit & (cnt < nsample)
                idx[rows_m[take], cnt[take]] = row[take]
                cnt[take] += 1
    return idx, cnt == 0


def voxel_query_brute(ranges, radius, nsample, xyz, new_xyz, new_coords, coords):
    """the same answer from an enumeration of ALL voxels of the grid point's frame (no window walk, no dense index): candidates are
    the voxels inside the integer window and the ball, ordered by (z, y, x); the first nsample are kept"""
    M = len(new_xyz)
    r2 = np.float32(radius) * np.float32(radius)
    idx = np.zeros((M, nsample), np.int32)
    empty = np.zeros(M, bool)
    key = (coords[:, 1].astype(np.int64) * 10 ** 6 + coords[:, 2]) * 10 ** 6 + coords[:, 3]
    for m in range(M):
        d = coords[:, 1:4].astype(np.int64) - new_coords[m, 1:4]
        cand = (coords[:, 0] == new_coords[m, 0]) & (np.abs(d[:, 0]) <= ranges[0]) & (np.abs(d[:, 1]) <= ranges[1]) & (np.abs(d[:, 2]) <= ranges[2])
        cand &= ~(_dist2_f32(xyz, new_xyz[m]) > r2)
        rows = np.nonzero(cand)[0]
        rows = rows[np.argsort(key[rows], kind='stable')][:nsample]
        if len(rows) == 0:
            empty[m] = True
            continue
        idx[m] = rows[0]
        idx[m, :len(rows)] = rows
    return idx, empty


def assert_radius_margin(ranges, radius, xyz, new_xyz, new_coords, coords, margin=MARGIN):
    """no voxel of the integer window lies within `margin` (relative) of radius^2 in f64"""
    r2 = float(np.float32(radius)) ** 2
    worst = np.inf
    for b in range(B):
        vm, gm = coords[:, 0] == b, new_coords[:, 0] == b
        d = coords[vm][None, :, 1:4].astype(np.int64) - new_coords[gm][:, None, 1:4]
        win = (np.abs(d[..., 0]) <= ranges[0]) & (np.abs(d[..., 1]) <= ranges[1]) & (np.abs(d[..., 2]) <= ranges[2])
        d2 = ((xyz[vm][None].astype(np.float64) - new_xyz[gm][:, None].astype(np.float64)) ** 2).sum(-1)
        if win.any():
            worst = min(worst, float(np.abs(d2[win] - r2).min() / r2))
    assert worst > margin, 'a neighbour sits on the ball surface (%.3g): change the seed' % worst
    return worst


def pool_f64(features_in, xyz, new_xyz, idx, empty, W, gamma, beta, eps, pool, mean=None, var=None):
    """the pooling definition in f64: out[m,c] = pool_s relu(f[idx[m,s],c] + BN(W d[m,s])_c), d = xyz[idx] - new_xyz
    (zero for an empty ball, whose features are zeroed too), BN with the batch statistics over all M * nsample slots (mean / var
    None: training) or the given running statistics. -> out (M,C), pre-activation values (M,nsample,C), batch mean, biased variance"""
    f = np.asarray(features_in, np.float64)[idx]                                       # (M, ns, C)
    d = xyz[idx].astype(np.float64) - new_xyz[:, None, :].astype(np.float64)
    f[empty] = 0
    d[empty] = 0
    pos = d @ np.asarray(W, np.float64).reshape(-1, 3).T                               # (M, ns, C)
    bm, bv = pos.reshape(-1, pos.shape[-1]).mean(0), pos.reshape(-1, pos.shape[-1]).var(0)
    m_, v_ = (bm, bv) if mean is None else (np.asarray(mean, np.float64), np.asarray(var, np.float64))
    v = f + (pos - m_) / np.sqrt(v_ + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    act = np.maximum(v, 0)
    return (act.max(1) if pool == 'max_pool' else act.mean(1)), v, bm, bv


# ---- head case: two levels of one geometry (stride 8 gives the (5, 24, 20) level; stride 2 the (20, 96, 80) one) ---------------
HEAD_PCR = level_pcr(8)
HEAD_STRIDES = {'x_conv2': 2, 'x_conv4': 8}
HEAD_CHANNELS = {'x_conv2': 16, 'x_conv4': 24}
HEAD_GRID, HEAD_FC, HEAD_SEED = 3, [32, 32], 91


def head_level_shape(stride):
    return tuple(int(v) * 8 // stride for v in SHAPE)


def head_cfg(dp_ratio=0.0):
    """ROI_HEAD of kitti_models/voxel_rcnn_car.yaml scaled down (plain dicts: each side wraps them in its own EasyDict): two levels
    with unequal ranges, both pool methods, both supported widths"""
    return {'NAME': 'VoxelRCNNHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': list(HEAD_FC), 'CLS_FC': list(HEAD_FC), 'REG_FC': list(HEAD_FC),
            'DP_RATIO': dp_ratio,
            'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                     'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                           'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'USE_FAST_NMS': False, 'SCORE_THRESH': 0.0,
                                    'NMS_PRE_MAXSIZE': 2048, 'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
            'ROI_GRID_POOL': {'FEATURES_SOURCE': ['x_conv2', 'x_conv4'], 'PRE_MLP': True, 'GRID_SIZE': HEAD_GRID,
                              'POOL_LAYERS': {
                                  'x_conv2': {'MLPS': [[32, 32]], 'QUERY_RANGES': [[4, 4, 4]], 'POOL_RADIUS': [0.4], 'NSAMPLE': [16],
                                              'POOL_METHOD': 'max_pool'},
                                  'x_conv4': {'MLPS': [[64, 32]], 'QUERY_RANGES': [[1, 2, 4]], 'POOL_RADIUS': [1.6], 'NSAMPLE': [5],
                                              'POOL_METHOD': 'avg_pool'}}},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': R, 'FG_RATIO': 0.5,
                              'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                              'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
            'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                            'GRID_3D_IOU_LOSS': False,
                            'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                             'rcnn_iou3d_weight': 1.0, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}


def head_inputs():
    """rois (B,R,7) car-sized boxes inside the stride-8 volume (one all-zero padding row), and per level coords (N,4) / feats (N,C):
    the level's voxels are drawn under the boxes so that balls of either radius find neighbours"""
    rng = np.random.default_rng(HEAD_SEED)
    x0, y0, z0, x1, y1, z1 = HEAD_PCR
    rois = np.zeros((B, R, 7), np.float32)
    for b in range(B):
        for r in range(R):
            if (b, r) == (1, 2):
                continue                                                     # padding row
            rois[b, r] = [rng.uniform(x0 + 2.2, x1 - 2.2), rng.uniform(y0 + 2.2, y1 - 2.2), rng.uniform(z0 + 1.2, z1 - 1.2),
                          rng.uniform(3.2, 4.4), rng.uniform(1.4, 1.9), rng.uniform(1.4, 1.8), rng.uniform(-np.pi, np.pi)]
    levels = {}
    for name, s in HEAD_STRIDES.items():
        Z, Y, X = head_level_shape(s)
        vs = np.array([VOXEL[0] * s, VOXEL[1] * s, VOXEL[2] * s])
        coords = []
        for b in range(B):
            occ = np.zeros((Z, Y, X), bool)
            for r in range(R):
                box = rois[b, r]
                if box[3] == 0:
                    continue
                half = 0.5 * np.hypot(box[3], box[4]) + 0.2
                lo = np.floor((np.array([box[0] - half, box[1] - half, box[2] - box[5] / 2 - 0.2]) - HEAD_PCR[:3]) / vs).astype(int)
                hi = np.ceil((np.array([box[0] + half, box[1] + half, box[2] + box[5] / 2 + 0.2]) - HEAD_PCR[:3]) / vs).astype(int)
                lo, hi = np.maximum(lo, 0), np.minimum(hi, [X, Y, Z])
                sub = rng.random((hi[2] - lo[2], hi[1] - lo[1], hi[0] - lo[0])) < (0.06 if s == 2 else 0.5)
                occ[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] |= sub
            zyx = np.argwhere(occ)
            coords.append(np.concatenate([np.full((len(zyx), 1), b), zyx], 1))
        coords = np.concatenate(coords, 0).astype(np.int32)
        levels[name] = (coords, rng.normal(0, 1, (len(coords), HEAD_CHANNELS[name])).astype(np.float32))
    return rois, levels


def head_sample():
    """the injected RoI sample of the head's training step: what ProposalTargetLayer.sample_rois_for_rcnn returns for the head case's
    RoIs (rois, gt_of_rois (B,R,8), max IoUs in [0, 1], roi scores, roi labels)"""
    rng = np.random.default_rng(HEAD_SEED + 2)
    rois, _ = head_inputs()
    gt = np.concatenate([rois + rng.normal(0, 0.1, rois.shape).astype(np.float32), np.ones(rois.shape[:2] + (1,), np.float32)], -1)
    ious = np.array([[0.9, 0.6, 0.1], [0.8, 0.4, 0.0]], np.float32)
    scores = rng.normal(0, 1, rois.shape[:2]).astype(np.float32)
    labels = np.ones(rois.shape[:2], np.int64)
    return rois, gt.astype(np.float32), ious, scores, labels
