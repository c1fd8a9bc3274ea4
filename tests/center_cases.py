"""Seeded cases of the centre head (CenterPoint) and its f64 numpy definition: target assignment, losses, box decoding.

Shared by tests/golden/make_goldens_centerpoint.py (which feeds the same inputs to the reference's CenterHead and centernet_utils
and records what they return), tests/test_centerpoint_cpu.py, tests/test_centerpoint_gpu.py and tools/center_head_host_check.py.

Geometry of every kernel case: B = 2, a 56 x 48 map (H x W, non-square on purpose: inds = y * W + x), stride 8, 0.05 m voxels, so a
cell is 0.4 m; classes Car / Pedestrian / Cyclist; M ragged with trailing all-zero rows.

Margins. A target is an integer decision on three f32 quantities (the two centre coordinates are truncated, so is the radius), so
boxes are redrawn until, in f64, the fractional parts of both centre coordinates and of the raw radius lie in [GAP, 1 - GAP],
GAP = 1e-3: about a hundred times the f32 rounding of a coordinate of 56 cells (56 * 2^-24 = 3e-6 times a few operations). Planted
logits of the loss cases stay 1e-3 away from +-ln 9999 (the clamp of the sigmoid), the 33 largest logits of a decode frame are
pairwise 1e-3 apart, decoded coordinates stay 1e-4 m away from the limit range and scores 1e-3 (in the logit) from the threshold."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ref_centerpoint.npz')

CLASSES = ['Car', 'Pedestrian', 'Cyclist']
B, H, W, STRIDE = 2, 56, 48, 8
VOXEL = [0.05, 0.05, 0.1]
PCR = [0.0, -11.2, -3.0, 19.2, 11.2, 1.0]                  # 48 x 56 cells of 0.4 m
OVERLAP, MIN_RADIUS = 0.1, 2
GAP = 1e-3
CELL = VOXEL[0] * STRIDE
SIZES = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}

ONE_HEAD = [['Car', 'Pedestrian', 'Cyclist']]
TWO_HEADS = [['Car'], ['Pedestrian', 'Cyclist']]
# name: (heads, NUM_MAX_OBJS, E extra columns, seed)
TARGET_CASES = {
    'one_head': (ONE_HEAD, 20, 0, 11),
    'two_heads': (TWO_HEADS, 20, 0, 12),
    'edges': (TWO_HEADS, 20, 0, 13),
    'overflow': (ONE_HEAD, 4, 0, 14),
    'empty_head': (TWO_HEADS, 20, 0, 15),
    'extras': (TWO_HEADS, 20, 2, 16),
}
HEAD_ORDER = ['center', 'center_z', 'dim', 'rot']
REG_CHANNELS = {'center': 2, 'center_z': 1, 'dim': 3, 'rot': 2, 'vel': 2}
LOSS_CASES = ['two_heads', 'edges', 'empty_head', 'extras']                  # target cases whose targets feed the loss
LOSS_WEIGHTS = {'cls_weight': 1.0, 'loc_weight': 2.0, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2]}
CLAMP_LOGIT = float(np.log(9999.0))
DECODE_CASES = {'plain': (0, 21), 'vel': (2, 22)}                             # name: (velocity channels, seed)
DECODE_K = 32
DECODE_LIMIT = [1.0, -10.0, -2.5, 18.0, 10.0, 0.5]
SCORE_THRESH = 0.1


def class_tables(heads):
    class_head, class_local = [-1] * len(CLASSES), [0] * len(CLASSES)
    for h, names in enumerate(heads):
        for k, n in enumerate(names):
            class_head[CLASSES.index(n)], class_local[CLASSES.index(n)] = h, k
    return class_head, class_local, [len(n) for n in heads]


# ---- the f64 definition of the targets --------------------------------------------------------------------------------------
def raw_radius(dx, dy, mo=OVERLAP):
    """gaussian_radius of the reference on (height, width) = (dx, dy) in cells, f64"""
    h, w = np.float64(dx), np.float64(dy)
    b1 = h + w
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * w * h * (1 - mo) / (1 + mo))) / 2
    b2 = 2 * (h + w)
    r2 = (b2 + np.sqrt(b2 ** 2 - 16 * (1 - mo) * w * h)) / 2
    b3 = -2 * mo * (h + w)
    r3 = (b3 + np.sqrt(b3 ** 2 - 16 * mo * (mo - 1) * w * h)) / 2
    return min(r1, r2, r3)


def box_geometry(box):
    """-> (cx, cy, raw radius) in f64 cells, centre clamped as the reference clamps it"""
    b = np.asarray(box, np.float64)
    cx = min(max((b[0] - PCR[0]) / VOXEL[0] / STRIDE, 0.0), W - 0.5)
    cy = min(max((b[1] - PCR[1]) / VOXEL[1] / STRIDE, 0.0), H - 0.5)
    r = raw_radius(b[3] / VOXEL[0] / STRIDE, b[4] / VOXEL[1] / STRIDE) if b[3] > 0 and b[4] > 0 else 0.5
    return cx, cy, r


def has_margin(box):
    frac = lambda v: v - np.floor(v)
    return all(GAP <= frac(v) <= 1 - GAP for v in box_geometry(box))


def targets_f64(gt, heads, nmax):
    """the definition: per head {'heatmap' (B,C,H,W) f32 = the f64 Gaussian rounded once, 'target_boxes' (B,nmax,8+E) f64, 'inds',
    'masks' (B,nmax) i64, 'radius' (B,nmax) i64 (0 where no object)}"""
    class_head, class_local, channels = class_tables(heads)
    E = gt.shape[2] - 8
    out = []
    for h, C in enumerate(channels):
        heat = np.zeros((B, C, H, W), np.float32)
        tb = np.zeros((B, nmax, 8 + E), np.float64)
        inds, masks, radius = (np.zeros((B, nmax), np.int64) for _ in range(3))
        for b in range(gt.shape[0]):
            k = -1
            for box in gt[b].astype(np.float64):
                c = int(box[-1]) if 1 <= box[-1] <= len(CLASSES) else 0
                if c == 0 or class_head[c - 1] != h:
                    continue
                k += 1
                if k >= nmax:
                    break
                if box[3] <= 0 or box[4] <= 0:
                    continue
                cx, cy, rr = box_geometry(box)
                x, y, r = int(cx), int(cy), max(int(rr), MIN_RADIUS)
                n = np.arange(-r, r + 1, dtype=np.float64)
                sigma = (2 * r + 1) / 6
                g = np.exp(-(n[None, :] ** 2 + n[:, None] ** 2) / (2 * sigma * sigma))
                left, right, top, bottom = min(x, r), min(W - x, r + 1), min(y, r), min(H - y, r + 1)
                view = heat[b, class_local[c - 1], y - top:y + bottom, x - left:x + right]
                np.maximum(view, g[r - top:r + bottom, r - left:r + right].astype(np.float32), out=view)
                inds[b, k], masks[b, k], radius[b, k] = y * W + x, 1, r
                tb[b, k, :8] = [cx - x, cy - y, box[2], np.log(box[3]), np.log(box[4]), np.log(box[5]), np.cos(box[6]), np.sin(box[6])]
                tb[b, k, 8:] = box[7:-1]
        out.append({'heatmap': heat, 'target_boxes': tb, 'inds': inds, 'masks': masks, 'radius': radius})
    return out


# ---- target cases -----------------------------------------------------------------------------------------------------------
def _box(rng, cls, E, xy=None):
    """a box of class `cls` with margins; xy: fixed centre in metres (redrawn in size and by a sub-cell jitter only)"""
    for _ in range(10000):
        s = np.array(SIZES[cls]) * rng.uniform(0.85, 1.15, 3)
        if xy is None:
            x, y = rng.uniform(PCR[0] + 0.1, PCR[3] - 0.1), rng.uniform(PCR[1] + 0.1, PCR[4] - 0.1)
        else:
            x, y = xy[0] + rng.uniform(-0.05, 0.05), xy[1] + rng.uniform(-0.05, 0.05)
        box = np.array([x, y, -1.0 + rng.uniform(-0.3, 0.3), *s, rng.uniform(-np.pi, np.pi), *rng.normal(0, 2, E), cls], np.float32)
        if has_margin(box):
            return box
    raise AssertionError('no box with margins')


def _pack(frames, E):
    M = max(len(f) for f in frames) + 2                            # trailing all-zero rows in every frame
    gt = np.zeros((B, M, 8 + E), np.float32)
    for b, f in enumerate(frames):
        for i, box in enumerate(f):
            gt[b, i] = box
    return gt


def make_targets_case(name):
    """-> {'gt_boxes' (B,M,8+E) f32, 'heads', 'nmax', 'E'}"""
    heads, nmax, E, seed = TARGET_CASES[name]
    rng = np.random.default_rng(seed)
    cell_xy = lambda cx, cy: (PCR[0] + cx * CELL, PCR[1] + cy * CELL)       # metres of a position in cells
    if name == 'edges':
        f0 = [_box(rng, 1, E, cell_xy(W - 0.5, H - 0.5)),                     # the last cell of both axes
              _box(rng, 2, E, (PCR[3] + 3.0, PCR[4] + 2.0)),                   # outside the range: clamped to size - 0.5
              _box(rng, 1, E, cell_xy(0.5, 20.5)),                            # clipped at the left border
              _box(rng, 1, E, cell_xy(25.5, 0.5)),                            # ... the top border
              _box(rng, 3, E, cell_xy(W - 1.5, 30.5)),                        # ... the right border
              _box(rng, 3, E, cell_xy(20.5, H - 1.5))]                        # ... the bottom border
        zero = _box(rng, 1, E, cell_xy(30.5, 30.5))
        zero[3] = 0.0                                                          # dx = 0: skipped, its slot stays zero
        f1 = [zero,
              _box(rng, 1, E, cell_xy(10.5, 10.5)), _box(rng, 1, E, cell_xy(12.5, 11.5)),      # same class, overlapping windows
              _box(rng, 2, E, cell_xy(30.4, 40.4)), _box(rng, 2, E, cell_xy(30.6, 40.6)),      # two boxes in one cell
              _box(rng, 3, E, cell_xy(31.5, 41.5)), _box(rng, 1, E, cell_xy(40.5, 5.5))]
        frames = [f0, f1]
    elif name == 'overflow':
        frames = [[_box(rng, int(rng.integers(1, 4)), E) for _ in range(7)], [_box(rng, int(rng.integers(1, 4)), E) for _ in range(3)]]
    elif name == 'empty_head':
        frames = [[_box(rng, int(rng.integers(2, 4)), E) for _ in range(n)] for n in (6, 4)]
    else:
        frames = []
        for n in (9, 6):
            f = [_box(rng, c, E) for c in (1, 2, 3)] + [_box(rng, int(rng.integers(1, 4)), E) for _ in range(n - 3)]
            frames.append([f[i] for i in rng.permutation(n)])
    gt = _pack(frames, E)
    for b in range(B):
        for box in gt[b]:
            assert box[-1] == 0 or box[3] <= 0 or has_margin(box), (name, box)
    return {'gt_boxes': gt, 'heads': heads, 'nmax': nmax, 'E': E}


def garbage_rows(gt):
    """the same case with garbage in the rows beyond every frame's boxes: class 0, NaN coordinates"""
    g = gt.copy()
    for b in range(g.shape[0]):
        for i in range(g.shape[1]):
            if not g[b, i].any():
                g[b, i, :-1] = np.nan
    return g


def permuted_overlaps(gt):
    """'edges' with the two overlapping same-class boxes of frame 1 (rows 1, 2) swapped and the two same-cell boxes (rows 3, 4) swapped:
    other slots, the same heatmap"""
    g = gt.copy()
    g[1, [1, 2]] = gt[1, [2, 1]]
    g[1, [3, 4]] = gt[1, [4, 3]]
    return g


# ---- loss cases -------------------------------------------------------------------------------------------------------------
def head_order(E):
    return HEAD_ORDER + (['vel'] if E else [])


def make_loss_case(name, h):
    """head h of target case `name`: the definition's targets (f32) + seeded logits and regression maps
    -> {'hm', 'heatmap' (B,C,H,W), 'reg': {branch: (B,c,H,W)}, 'target_boxes', 'inds', 'masks', 'planted': (idx arrays of hm), 'order', 'heads'}"""
    case = make_targets_case(name)
    t = targets_f64(case['gt_boxes'], case['heads'], case['nmax'])[h]
    C = t['heatmap'].shape[1]
    rng = np.random.default_rng(1000 + 10 * TARGET_CASES[name][3] + h)
    hm = rng.normal(-2.19, 2.0, (B, C, H, W)).astype(np.float32)
    near = np.abs(np.abs(hm) - CLAMP_LOGIT) < 2 * GAP
    hm[near] = -2.19
    n = 12
    planted = (rng.integers(0, B, n), rng.integers(0, C, n), rng.integers(0, H, n), rng.integers(0, W, n))
    hm[planted] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * rng.uniform(9.5, 14.0, n).astype(np.float32)
    peaks = np.argwhere(t['heatmap'] == 1)                      # one planted value on a positive cell of each sign, where there is one
    for i, p in enumerate(peaks[:2]):
        hm[tuple(p)] = (11.0, -12.5)[i]
        planted = tuple(np.append(planted[d], p[d]) for d in range(4))
    assert (np.abs(np.abs(hm) - CLAMP_LOGIT) >= GAP).all()
    order = head_order(case['E'])
    reg = {n_: rng.normal(0, 1, (B, REG_CHANNELS[n_], H, W)).astype(np.float32) for n_ in order}
    return {'hm': hm, 'heatmap': t['heatmap'], 'reg': reg, 'target_boxes': t['target_boxes'].astype(np.float32), 'inds': t['inds'],
            'masks': t['masks'], 'planted': planted, 'order': order, 'heads': case['heads']}


def loss_f64(case):
    """the definition: {hm_loss * cls_weight, loc_loss * loc_weight} in f64"""
    x = case['hm'].astype(np.float64)
    p = np.clip(1 / (1 + np.exp(-x)), 1e-4, 1 - 1e-4)
    gt = case['heatmap'].astype(np.float64)
    pos = gt == 1
    pos_loss = (np.log(p) * (1 - p) ** 2)[pos].sum()
    neg_loss = (np.log(1 - p) * p ** 2 * (1 - gt) ** 4)[~pos].sum()
    hm_loss = -neg_loss if pos.sum() == 0 else -(pos_loss + neg_loss) / pos.sum()
    maps = np.concatenate([case['reg'][n] for n in case['order']], 1).astype(np.float64).reshape(B, -1, H * W)
    rows = np.stack([maps[b][:, case['inds'][b]].T for b in range(B)])
    m = case['masks'][:, :, None].astype(np.float64)
    per_col = (np.abs(rows - case['target_boxes'].astype(np.float64)) * m).sum((0, 1)) / max(m.sum(), 1.0)
    loc = (per_col * np.array(LOSS_WEIGHTS['code_weights'][:len(per_col)])).sum()
    return np.array([hm_loss * LOSS_WEIGHTS['cls_weight'], loc * LOSS_WEIGHTS['loc_weight']])


# ---- decode cases -----------------------------------------------------------------------------------------------------------
def make_decode_case(name):
    """-> {'hm' (B,3,H,W) logits, 'reg': {branch: map}, 'order'}: 33 largest logits of a frame pairwise >= GAP apart, some picks below
    SCORE_THRESH, some outside DECODE_LIMIT, none within the margins of either"""
    vel, seed = DECODE_CASES[name]
    order = ['center', 'center_z', 'dim', 'rot'] + (['vel'] if vel else [])
    logit_thresh = float(np.log(SCORE_THRESH / (1 - SCORE_THRESH)))
    for attempt in range(200):
        rng = np.random.default_rng(seed * 1000 + attempt)
        hm = rng.normal(-6.0, 1.2, (B, 3, H, W)).astype(np.float32)
        reg = {n: rng.normal(0, 1, (B, REG_CHANNELS[n], H, W)).astype(np.float32) for n in order}
        reg['center'] = rng.uniform(0, 1, reg['center'].shape).astype(np.float32)
        reg['center_z'] = rng.normal(-1.0, 1.2, reg['center_z'].shape).astype(np.float32)
        reg['dim'] = (0.5 * reg['dim']).astype(np.float32)
        case = {'hm': hm, 'reg': reg, 'order': order}
        top = np.sort(hm.reshape(B, -1).astype(np.float64), 1)[:, ::-1][:, :DECODE_K + 1]
        d = decode_f64(case)
        lim = np.array(DECODE_LIMIT)
        near = min(np.abs(d['boxes'][..., :3] - lim[:3]).min(), np.abs(d['boxes'][..., :3] - lim[3:]).min())
        inside = ((d['boxes'][..., :3] >= lim[:3]) & (d['boxes'][..., :3] <= lim[3:])).all(2)
        if (-np.diff(top, axis=1)).min() >= GAP and near >= 1e-4 and np.abs(top[:, :DECODE_K] - logit_thresh).min() >= GAP and \
                (~inside).any() and inside.sum() > 8 and (d['scores'] <= SCORE_THRESH).any() and (d['scores'] > SCORE_THRESH).sum() > 8:
            return case
    raise AssertionError('no decode case with margins')


def decode_f64(case, K=DECODE_K):
    """the definition: the K largest logits of a frame over classes and cells, in descending order, decoded in f64"""
    hm = case['hm'].astype(np.float64).reshape(B, -1)
    idx = np.argsort(-hm, 1, kind='stable')[:, :K]
    cls, cell = idx // (H * W), idx % (H * W)
    maps = np.concatenate([case['reg'][n] for n in case['order']], 1).astype(np.float64).reshape(B, -1, H * W)
    rows = np.stack([maps[b][:, cell[b]].T for b in range(B)])
    x = ((cell % W) + rows[..., 0]) * STRIDE * VOXEL[0] + PCR[0]
    y = ((cell // W) + rows[..., 1]) * STRIDE * VOXEL[1] + PCR[1]
    boxes = np.concatenate([x[..., None], y[..., None], rows[..., 2:3], np.exp(rows[..., 3:6]), np.arctan2(rows[..., 7:8], rows[..., 6:7]),
                            rows[..., 8:]], -1)
    scores = 1 / (1 + np.exp(-np.take_along_axis(hm, idx, 1)))
    lim = np.array(DECODE_LIMIT)
    keep = ((boxes[..., :3] >= lim[:3]) & (boxes[..., :3] <= lim[3:])).all(2) & (scores > SCORE_THRESH)
    return {'boxes': boxes, 'scores': scores, 'labels': cls, 'keep': keep}


# ---- detector case ----------------------------------------------------------------------------------------------------------
DET_FIRST_FRAME, DET_POINTS, DET_SEED = 40, 8000, 71           # frames of pcdet.datasets.synthetic.kitti_batch; golden._constants.seeded_state
DET_PCR, DET_VOXEL, DET_MAX_VOXELS = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0], [0.05, 0.05, 0.1], 16000
DET_SCORE_GAP, DET_MAX_KEEP = 2e-6, 40                        # scores of the eval picks: pairwise this far apart (f32 error of a score: 4e-8)
DET_GRADS = {'dense_head.shared_conv.0.weight': np.s_[:8], 'dense_head.heads_list.0.hm.1.weight': np.s_[:],
             'dense_head.heads_list.0.dim.1.weight': np.s_[:]}


def det_state(sd):
    """golden._constants.seeded_state(model, DET_SEED) made sane for a centre head: the final convolutions of the regression branches scaled
    by 0.05 (sizes exp(dim) of order 1), that of hm by 0.5 (logits spread enough that no two picks tie) and the hm bias at the reference's -2.19, so scores straddle SCORE_THRESH"""
    out = {}
    for k, v in sd.items():
        if '.heads_list.' in k and k.endswith('.1.weight'):
            v = v * (0.5 if '.hm.' in k else 0.05)
        if k.endswith('.hm.1.bias'):
            v = v * 0 - 2.19
        out[k] = v
    return out


def ulp_f32(a):
    """spacing of f32 at |a| (elementwise)"""
    return np.spacing(np.abs(np.asarray(a, np.float32))).astype(np.float64)
