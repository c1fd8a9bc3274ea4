"""Seeded cases for the sparse RoI-aware pooling (csrc/roiaware_sparse.hip) and its definition in numpy f64.

A case is a dict: rois (B,R,7) f32, pts (N,3) f32 stacked frame after frame, off (B+1) i32, part (N,4) f32 >= 0 (avg-pooled),
feat (N,C) f32 (max-pooled), o (cells per edge), max_pts. Every generated point keeps >= MARGIN metres from every face of
every RoI of its frame and, inside a RoI, from every cell plane (rejection), so the f32 kernels and the f64 definition take the
same discrete decisions. Every case asserts its own premise.

pool_definition(case) -> rows in lexicographic (roi, x, y, z) order with the rule of the dense route:
  a point belongs to the RoI iff |lz| <= dz/2, |lx| < dx/2 + 1e-5, |ly| < dy/2 + 1e-5 in the RoI's frame; cell = floor of the
  offset from the lower face over the cell edge, clamped; a cell keeps its first max_pts - 1 points in ascending point index;
  avg = sum / n, max = first largest value (argmax = its point, index into the stacked points); a cell is a row iff the f32 sum
  of its four averages is != 0.
grad_definition(case, d, g_part, g_feat) -> the f64 gradients, the per-entry sum of |terms| and the per-entry term count."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden._constants import parta2_inputs  # noqa: E402

MARGIN = 1e-4
SIZES = [(3.9, 1.6, 1.56), (0.8, 0.6, 1.73), (1.76, 0.6, 1.73)]
# gradients stored in tests/golden/ref_parta2_net.npz (every module of the detector that has parameters) and the slice of each that is kept
PA2_GRADS = {'backbone_3d.conv_input.0.weight': np.s_[:], 'backbone_3d.inv_conv3.0.weight': np.s_[:8],
             'backbone_2d.blocks.0.1.weight': np.s_[:8], 'dense_head.conv_box.weight': np.s_[:],
             'point_head.cls_layers.0.weight': np.s_[:], 'point_head.part_reg_layers.0.weight': np.s_[:],
             'roi_head.conv_part.0.0.weight': np.s_[:], 'roi_head.conv_rpn.0.0.weight': np.s_[:],
             'roi_head.shared_fc_layer.0.weight': np.s_[:, :384]}
CASE_NAMES = ('golden', 'cap', 'ragged', 'wide', 'zeros', 'odd', 'few')


# ---------------------------------------------------------------------------------------------------------------- geometry
def locate(pts, roi, o):
    """pts (n,3), roi (7) -> inside (n) bool, cell (n) int code (x*o + y)*o + z (valid where inside), margin (n) f64: distance
    to the nearest face of the RoI and, inside, to the nearest cell plane"""
    p, r = pts.astype(np.float64), roi.astype(np.float64)
    ca, sa = np.cos(-r[6]), np.sin(-r[6])
    sx, sy = p[:, 0] - r[0], p[:, 1] - r[1]
    loc = np.stack([sx * ca - sy * sa, sx * sa + sy * ca, p[:, 2] - r[2]], 1)
    half = r[3:6] / 2
    inside = (np.abs(loc[:, 2]) <= half[2]) & (np.abs(loc[:, 0]) < half[0] + 1e-5) & (np.abs(loc[:, 1]) < half[1] + 1e-5)
    margin = np.abs(np.abs(loc) - half).min(1)
    cell = np.zeros(len(p), np.int64)
    if inside.any() and (r[3:6] > 0).all():
        t = (loc[inside] + half) / (r[3:6] / o)
        ci = np.clip(np.floor(t), 0, o - 1).astype(np.int64)
        cell[inside] = (ci[:, 0] * o + ci[:, 1]) * o + ci[:, 2]
        frac = np.abs(t - np.round(t)) * (r[3:6] / o)
        margin[inside] = np.minimum(margin[inside], frac.min(1))
    return inside, cell, margin


def reject(pts_frames, rois, o):
    """drop the points nearer than MARGIN to a face / cell plane of any RoI of their frame"""
    out = []
    for b, p in enumerate(pts_frames):
        keep = np.ones(len(p), bool)
        for roi in rois[b]:
            keep &= locate(p, roi, o)[2] >= MARGIN
        out.append(p[keep])
    return out


# ---------------------------------------------------------------------------------------------------------------- definition
def pool_definition(case):
    rois, pts, off, o, cap = case['rois'], case['pts'], case['off'], case['o'], case['max_pts'] - 1
    part, feat = case['part'].astype(np.float64), case['feat']
    B, R = rois.shape[:2]
    coords, avg, mx, am, kept_pts, n_hits_uncapped = [], [], [], [], [], []
    for b in range(B):
        idx = np.arange(off[b], off[b + 1])
        for r in range(R):
            inside, cell, _ = locate(pts[idx], rois[b, r], o)
            ii, cc = idx[inside], cell[inside]
            order = np.argsort(cc, kind='stable')
            ii, cc = ii[order], cc[order]
            uniq, start, cnt = np.unique(cc, return_index=True, return_counts=True)
            for u, s, n in zip(uniq, start, cnt):
                kept = ii[s:s + min(n, cap)]
                a = part[kept].sum(0) / len(kept)
                if np.float32(a.astype(np.float32).sum()) == 0:
                    continue
                coords.append([b * R + r, u // (o * o), (u // o) % o, u % o])
                avg.append(a)
                f = feat[kept]
                j = f.argmax(0)                                      # first largest value
                mx.append(f[j, np.arange(f.shape[1])])
                am.append(kept[j])
                kept_pts.append(kept)
                n_hits_uncapped.append(n)
    C = feat.shape[1]
    return {'coords': np.array(coords, np.int32).reshape(-1, 4), 'part': np.array(avg, np.float64).reshape(-1, 4),
            'feat': np.array(mx, np.float32).reshape(-1, C), 'argmax': np.array(am, np.int32).reshape(-1, C),
            'kept': kept_pts, 'hits': np.array(n_hits_uncapped, np.int64)}


def grad_definition(case, d, g_part, g_feat):
    """-> grad_part (N,4), grad_feat (N,C) f64, abs_part / abs_feat: sum of |terms| per entry, n_part / n_feat: terms per entry"""
    N, C = case['pts'].shape[0], case['feat'].shape[1]
    gp, gf = np.zeros((N, 4)), np.zeros((N, C))
    ap, af = np.zeros((N, 4)), np.zeros((N, C))
    npart, nfeat = np.zeros((N, 4), np.int64), np.zeros((N, C), np.int64)
    g_part, g_feat = g_part.astype(np.float64), g_feat.astype(np.float64)
    cols = np.arange(C)
    for row, kept in enumerate(d['kept']):
        t = g_part[row] / len(kept)
        gp[kept] += t
        ap[kept] += np.abs(t)
        npart[kept] += 1
        a = d['argmax'][row]
        gf[a, cols] += g_feat[row]
        af[a, cols] += np.abs(g_feat[row])
        nfeat[a, cols] += 1
    return {'grad_part': gp, 'grad_feat': gf, 'abs_part': ap, 'abs_feat': af, 'n_part': npart, 'n_feat': nfeat}


def scatter_dense(case, d):
    """the definition's rows as the dense route's two grids (B*R, o, o, o, 4 / C)"""
    o, n = case['o'], case['rois'].shape[0] * case['rois'].shape[1]
    part = np.zeros((n, o, o, o, 4), np.float64)
    feat = np.zeros((n, o, o, o, case['feat'].shape[1]), np.float32)
    c = d['coords']
    part[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = d['part']
    feat[c[:, 0], c[:, 1], c[:, 2], c[:, 3]] = d['feat']
    return part, feat


# ---------------------------------------------------------------------------------------------------------------- cases
def _object(rng, g):
    s = np.array(SIZES[g % 3]) * rng.uniform(0.9, 1.1, 3)
    return np.array([rng.uniform(5, 60), rng.uniform(-30, 30), rng.uniform(-1.2, -0.6), *s, rng.uniform(-np.pi, np.pi)])


def _points_in(rng, box, k, spread=0.55):
    loc = rng.uniform(-spread, spread, (k, 3)) * box[3:6]
    ca, sa = np.cos(box[6]), np.sin(box[6])
    return np.stack([loc[:, 0] * ca - loc[:, 1] * sa + box[0], loc[:, 0] * sa + loc[:, 1] * ca + box[1], loc[:, 2] + box[2]], 1)


def _jitter(rng, box):
    o = box.copy()
    o[:3] += rng.normal(0, 0.25, 3)
    o[3:6] *= rng.uniform(0.9, 1.2, 3)
    o[6] += rng.normal(0, 0.15)
    return o


def _finish(rng, frames, rois, o, max_pts, C, zero_fraction=0.0):
    rois = rois.astype(np.float32)
    frames = reject([f.astype(np.float32) for f in frames], rois, o)
    pts = np.concatenate(frames).astype(np.float32).reshape(-1, 3)
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int32)
    N = len(pts)
    score = rng.uniform(0.01, 1, (N, 1)).astype(np.float32)
    lead = rng.uniform(0.01, 1, (N, 3)).astype(np.float32)
    lead[score[:, 0] < 0.3] = 0                                       # the head's SEG_MASK_SCORE_THRESH
    part = np.concatenate([lead, score], 1)
    if zero_fraction:
        part[rng.uniform(0, 1, N) < zero_fraction] = 0
    feat = rng.normal(0, 1, (N, C)).astype(np.float32)
    return {'rois': rois, 'pts': pts, 'off': off, 'part': part, 'feat': feat, 'o': o, 'max_pts': max_pts}


def _scene(rng, B, R, n_obj, k_lo, k_hi, n_clutter):
    frames, rois = [], np.zeros((B, R, 7))
    for b in range(B):
        objs = [_object(rng, g) for g in range(n_obj)]
        p = [np.stack([rng.uniform(0, 70, n_clutter), rng.uniform(-40, 40, n_clutter), rng.uniform(-3, 1, n_clutter)], 1)]
        p += [_points_in(rng, ob, int(rng.integers(k_lo, k_hi))) for ob in objs]
        p = np.concatenate(p)
        frames.append(p[rng.permutation(len(p))])
        for r in range(R):
            rois[b, r] = _jitter(rng, objs[r % n_obj])
    return frames, rois


def case_golden():
    inp = parta2_inputs()
    pc, score = inp['point_coords'], inp['point_cls_scores'].reshape(-1, 1)
    lead = np.where(score < 0.3, np.float32(0), inp['point_part_offset'])
    B = inp['batch_size']
    off = np.searchsorted(pc[:, 0], np.arange(B + 1)).astype(np.int32)
    c = {'rois': inp['rois'], 'pts': np.ascontiguousarray(pc[:, 1:4]), 'off': off,
         'part': np.concatenate([lead, score], 1).astype(np.float32), 'feat': inp['point_features'], 'o': 4, 'max_pts': 32}
    return c


def case_cap():
    rng = np.random.default_rng(101)
    box = np.array([20.0, 3.0, -1.0, 4.0, 2.0, 1.6, 0.4])
    rois = np.stack([box, box])[None]
    c = _finish(rng, [_points_in(rng, box, 260, spread=0.49)], rois, 2, 4, 6)
    return c


def case_ragged():
    rng = np.random.default_rng(102)
    B, R = 3, 5
    frames, rois = _scene(rng, 1, R, 4, 150, 300, 900)
    rois = np.concatenate([rois, np.zeros((2, R, 7))])
    rois[0, 3] = 0                                                    # the padding proposal_layer leaves
    rois[0, 4] = [85, 55, 0, 2, 2, 2, 0.3]                            # far from every point
    lone = np.array([[30.0, 5.0, -1.0]])
    rois[1, 0] = [30.1, 5.1, -1.05, 3.9, 1.6, 1.5, 0.2]
    rois[1, 1] = [60, -20, -1, 3.9, 1.6, 1.5, 1.0]
    rois[2] = rois[0]                                                 # RoIs on the empty frame
    frames = [frames[0][:1400], lone, np.zeros((0, 3))]
    c = _finish(rng, frames, rois, 12, 128, 16)
    n0 = c['off'][1]
    keep = np.r_[np.arange(min(n0, 1337)), np.arange(n0, len(c['pts']))]   # frame 0 cut to exactly 1337 points
    for k in ('pts', 'part', 'feat'):
        c[k] = np.ascontiguousarray(c[k][keep])
    c['off'] = np.array([0, min(n0, 1337), min(n0, 1337) + 1, min(n0, 1337) + 1], np.int32)
    return c


def case_wide():
    rng = np.random.default_rng(103)
    frames, rois = _scene(rng, 2, 4, 3, 60, 120, 200)
    p = np.stack([rng.uniform(1, 69, 5200), rng.uniform(-39, 39, 5200), rng.uniform(-2.9, 0.9, 5200)], 1)
    frames[0] = p
    rois[0, 1] = [35, 0, -1, 72, 82, 4.2, 0.0]                       # holds every point of frame 0
    rois[0, 0] = [20, 5, -1, 3.9, 1.6, 1.56, 0.3]
    rois[0, 2] = [40, -10, -1, 0.8, 0.6, 1.73, 1.1]
    rois[0, 3] = [50, 20, -1, 1.76, 0.6, 1.73, -0.7]
    c = _finish(rng, frames, rois, 4, 64, 8)
    n0 = c['off'][1]
    assert n0 >= 5000
    keep = np.r_[np.arange(5000), np.arange(n0, len(c['pts']))]
    for k in ('pts', 'part', 'feat'):
        c[k] = np.ascontiguousarray(c[k][keep])
    c['off'] = (np.array([0, 5000, 5000 + c['off'][2] - n0])).astype(np.int32)
    return c


def case_zeros():
    rng = np.random.default_rng(104)
    frames, rois = _scene(rng, 2, 8, 4, 150, 300, 300)
    return _finish(rng, frames, rois, 6, 128, 16, zero_fraction=0.1)


def case_odd():
    rng = np.random.default_rng(105)
    frames, rois = _scene(rng, 2, 7, 3, 50, 130, 250)
    return _finish(rng, frames, rois, 5, 16, 5)


def case_few():
    rng = np.random.default_rng(106)
    box = np.array([20.0, 3.0, -1.0, 4.0, 2.0, 1.6, 0.4])
    rois = np.stack([box, [85, 55, 0, 2, 2, 2, 0.3], np.zeros(7)])[None]
    inside = _points_in(rng, box, 2, spread=0.45)
    away = np.stack([rng.uniform(40, 60, 50), rng.uniform(-30, 30, 50), rng.uniform(-3, 1, 50)], 1)
    return _finish(rng, [np.concatenate([inside[:1], away, inside[1:]])], rois, 6, 16, 32)


def check_premise(name, c, d):
    """the property the case exists for; raises AssertionError when the seeded data lost it"""
    off, o, cap = c['off'], c['o'], c['max_pts'] - 1
    B, R = c['rois'].shape[:2]
    assert (c['part'] >= 0).all() and len(off) == B + 1 and off[-1] == len(c['pts'])
    if name != 'golden':
        for b in range(B):
            for roi in c['rois'][b]:
                assert (locate(c['pts'][off[b]:off[b + 1]], roi, o)[2] >= MARGIN).all()
    T = len(d['coords'])
    if name == 'golden':
        assert (B, R, o, c['max_pts'], c['feat'].shape[1]) == (2, 16, 4, 32, 32) and T > 200
    elif name == 'cap':
        assert (o, c['max_pts']) == (2, 4) and T == 16 and (d['hits'] > cap).all() and len(c['pts']) >= 200
        assert all(len(k) == 3 for k in d['kept'])
        for k in d['kept']:                                           # the first three of the cell in point order
            _, cell, _ = locate(c['pts'], c['rois'][0, 0], o)
            assert (k == np.flatnonzero(cell == cell[k[0]])[:3]).all()
    elif name == 'ragged':
        assert (B, R, o, c['max_pts'], c['feat'].shape[1]) == (3, 5, 12, 128, 16)
        assert list(np.diff(off)) == [1337, 1, 0]
        assert not c['rois'][0, 3].any() and not (d['coords'][:, 0] == 3).any() and not (d['coords'][:, 0] == 4).any()
        assert (d['coords'][:, 0] == R).sum() == 1 and not (d['coords'][:, 0] > R).any()     # the lone point; the empty frame
        assert c['rois'][2].any() and T > 100
    elif name == 'wide':
        assert off[1] == 5000 and locate(c['pts'][:5000], c['rois'][0, 1], o)[0].all()
        assert d['hits'][d['coords'][:, 0] == 1].sum() == 5000 and (d['hits'] > cap).any() and (d['hits'] < cap).any()
        assert (d['coords'][:, 0] != 1).sum() > 20
    elif name == 'zeros':
        zero = ~c['part'].any(1)
        assert 0.05 < zero.mean() < 0.2
        absent = mixed = 0
        rows = {tuple(r) for r in d['coords'].tolist()}
        for b in range(B):
            idx = np.arange(off[b], off[b + 1])
            for r in range(R):
                inside, cell, _ = locate(c['pts'][idx], c['rois'][b, r], o)
                for u in np.unique(cell[inside]):
                    z = zero[idx[inside & (cell == u)][:cap]]
                    key = (b * R + r, u // (o * o), (u // o) % o, u % o)
                    if z.all():
                        absent += 1
                        assert key not in rows
                    elif z.any():
                        mixed += 1
                        assert key in rows
        assert absent >= 10 and mixed >= 10, (absent, mixed)
    elif name == 'odd':
        assert c['feat'].shape[1] == 5 and T > 50
    elif name == 'few':
        assert 0 < T < 3


_BUILD = {'golden': case_golden, 'cap': case_cap, 'ragged': case_ragged, 'wide': case_wide, 'zeros': case_zeros, 'odd': case_odd,
          'few': case_few}
_CACHE = {}


def get_case(name):
    """-> (case, definition), built once per process and shared; callers must not write into the arrays"""
    if name not in _CACHE:
        c = _BUILD[name]()
        d = pool_definition(c)
        check_premise(name, c, d)
        for v in list(c.values()) + [d['coords'], d['part'], d['feat'], d['argmax']]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[name] = (c, d)
    return _CACHE[name]
