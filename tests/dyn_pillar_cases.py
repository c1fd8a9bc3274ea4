"""Seeded cases, the f64 numpy definition of the two-layer dynamic pillar net and the margin checks for
tests/test_dyn_pillar_cpu.py, tests/test_dyn_pillar_gpu.py and their golden generator (tests/golden/make_goldens_dyn_pillar.py).
No reference import here: this module travels with the tests.

The points are those of tests/dyn_voxel_cases.py (pillar grid 32 x 24, range [-5.12, -3.84, -2, 5.12, 3.84, 4], voxel [0.32, 0.32, 6])
without the rows whose cell differs between f32 and f64 arithmetic (the points placed on cell faces): the yardstick is an f64 run of
the reference, which forms the cells in f64. Everything else of case a stays: B = 3 with an empty frame 1, C = 5, pillar sizes 1, 2,
63, 64, 65 and 300, the four corners, out-of-range and NaN rows, points outside the range in z only (kept), a global shuffle.

Margins, asserted on the f64 definition in train mode and in eval mode; the feature columns of the offending points are redrawn until
they hold (the grouping never changes):
  layer 1   every pre-activation of every kept point is farther from 0 than the bound
  both      per pillar and channel the maximum pre-activation lies more than the bound above the runner-up (ties at a common 0 are
            thereby excluded where the maximum is positive; a maximum below 0 passes nothing whichever point holds it)
  bound     max(GAP, MARGIN_FACTOR x the f32 evaluation-error bound of that pre-activation), GAP and MARGIN_FACTOR of pillar_cases.py
Two correct f32 evaluations, in any summation order, then select the same points and agree on every ReLU mask."""
import os

import numpy as np

import dyn_voxel_cases as vox
from pillar_cases import GAP, MARGIN_FACTOR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ref_dyn_pillar.npz')

PCR, VOXEL, GRID = vox.PCR, vox.VOXEL['pillar'], vox.GRID['pillar']
H1, COUT = 32, 64
EPS, MOMENTUM = 1e-3, 0.01
WEIGHT_SEED = 733
CASES = ('a', 'b', 'c')
KEYS = ['pfn_layers.%d.%s' % (i, k) for i in (0, 1) for k in ('linear.weight', 'norm.weight', 'norm.bias', 'norm.running_mean',
                                                               'norm.running_var', 'norm.num_batches_tracked')]
GRADS = ('dW1', 'dgamma1', 'dbeta1', 'dW2', 'dgamma2', 'dbeta2')
STATS = ('running_mean1', 'running_var1', 'running_mean2', 'running_var2')


def offsets():
    return [VOXEL[i] / 2 + PCR[i] for i in range(3)]


def vfe_cfg(num_filters=(64, 64), with_distance=False):
    return {'NAME': 'DynPillarVFE', 'WITH_DISTANCE': with_distance, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': list(num_filters)}


def weights(C):
    rng = np.random.default_rng(WEIGHT_SEED + C)
    K = C + 6
    w = {}
    for i, (cout, cin) in enumerate(((H1, K), (COUT, COUT))):
        p = 'pfn_layers.%d.' % i
        w[p + 'linear.weight'] = (rng.normal(0, 1, (cout, cin)) / np.sqrt(cin)).astype(np.float32)
        w[p + 'norm.weight'] = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        w[p + 'norm.bias'] = rng.normal(0, 0.2, cout).astype(np.float32)
        w[p + 'norm.running_mean'] = rng.normal(0, 0.5, cout).astype(np.float32)
        w[p + 'norm.running_var'] = rng.uniform(2.0, 6.0, cout).astype(np.float32)
        w[p + 'norm.num_batches_tracked'] = np.zeros((), np.int64)
    return w


def grad_out(name, M):
    return np.random.default_rng(vox.CASES[name]['seed'] + 7).normal(0, 1, (M, COUT)).astype(np.float32)


def _same_cell_in_f64(points):
    lo, vs = np.asarray(PCR[:2], np.float32), np.asarray(VOXEL[:2], np.float32)
    with np.errstate(invalid='ignore'):
        c32 = np.floor((points[:, 1:3] - lo) / vs)
        c64 = np.floor((points[:, 1:3].astype(np.float64) - lo.astype(np.float64)) / vs.astype(np.float64))
    return ((c32 == c64) | np.isnan(c32)).all(1)


def _segmax(x, seg):
    return np.stack([x[seg[v]:seg[v + 1]].max(0) for v in range(len(seg) - 1)])


def net_f64(points, B, w, training):
    """the definition in f64 numpy, rows in segment order -> dict out (M, 64), pre1 (Nk, 32), pre2 (Nk, 64), f, coords, seg_offsets,
    inv, the folded affines and (training) the running statistics after the step"""
    d = vox.definition(points, B, 'pillar')
    seg, M = d['seg_offsets'], len(d['coords'])
    inv = np.repeat(np.arange(M), np.diff(seg))
    P = points[d['perm']].astype(np.float64)
    xyz = P[:, 1:4]
    mean = np.stack([xyz[seg[v]:seg[v + 1]].sum(0) / (seg[v + 1] - seg[v]) for v in range(M)]).reshape(M, 3)
    off = offsets()
    ctr = np.stack([d['coords'][:, 3].astype(np.float64) * VOXEL[0] + off[0], d['coords'][:, 2].astype(np.float64) * VOXEL[1] + off[1],
                    np.full(M, off[2])], 1)
    f = np.concatenate([P[:, 1:], xyz - mean[inv], xyz - ctr[inv]], 1)
    n = len(f)
    r = {'f': f, 'coords': d['coords'], 'seg_offsets': seg, 'inv': inv, 'perm': d['perm']}
    x = f
    for i in (0, 1):
        p = 'pfn_layers.%d.' % i
        W = w[p + 'linear.weight'].astype(np.float64)
        lin = x @ W.T
        if training:
            mu, var = lin.mean(0), lin.var(0)
            r['running_mean%d' % (i + 1)] = (1 - MOMENTUM) * w[p + 'norm.running_mean'].astype(np.float64) + MOMENTUM * mu
            r['running_var%d' % (i + 1)] = (1 - MOMENTUM) * w[p + 'norm.running_var'].astype(np.float64) + MOMENTUM * var * n / max(n - 1, 1)
        else:
            mu, var = w[p + 'norm.running_mean'].astype(np.float64), w[p + 'norm.running_var'].astype(np.float64)
        scale = w[p + 'norm.weight'].astype(np.float64) / np.sqrt(var + EPS)
        A, b = scale[:, None] * W, w[p + 'norm.bias'].astype(np.float64) - mu * scale
        pre = x @ A.T + b
        r['A%d' % (i + 1)], r['b%d' % (i + 1)], r['pre%d' % (i + 1)], r['in%d' % (i + 1)] = A, b, pre, x
        mx = _segmax(np.maximum(pre, 0), seg)
        x = np.concatenate([np.maximum(pre, 0), mx[inv]], 1)
    r['out'] = mx
    return r


def margin_violations(r):
    """rows (in segment order) that break a margin: a layer-1 pre-activation too close to 0, or the two best points of a pillar and
    channel closer than the bound at a positive maximum"""
    u = 2.0 ** -24
    bound1 = (r['f'].shape[1] + 3) * u * (np.abs(r['b1'])[None, :] + np.abs(r['f']) @ np.abs(r['A1']).T)
    need1 = np.maximum(GAP, MARGIN_FACTOR * bound1)
    bad = (np.abs(r['pre1']) <= need1).any(1)
    seg = r['seg_offsets']
    bmax1 = _segmax(bound1, seg)[r['inv']]
    A2 = np.abs(r['A2'])
    bound2 = np.concatenate([bound1, bmax1], 1) @ A2.T + (COUT + 3) * u * (np.abs(r['b2'])[None, :] + np.abs(r['in2']) @ A2.T)
    for pre, need in ((r['pre1'], need1), (r['pre2'], np.maximum(GAP, MARGIN_FACTOR * bound2))):
        for v in range(len(seg) - 1):
            lo, hi = seg[v], seg[v + 1]
            cols = np.arange(pre.shape[1])
            order = np.argsort(pre[lo:hi], 0)
            top = order[-1]
            zero = np.abs(pre[lo + top, cols]) <= need[lo + top, cols]      # the sign of the maximum decides whether it passes a gradient
            bad[lo + top[zero]] = True
            if hi - lo < 2:
                continue
            second = order[-2]
            gap = pre[lo + top, cols] - pre[lo + second, cols]
            close = (pre[lo + top, cols] > -need[lo + top, cols]) & (gap <= np.maximum(need[lo + top, cols], need[lo + second, cols]))
            bad[lo + top[close]] = True
            bad[lo + second[close]] = True
    return np.nonzero(bad)[0]


MAX_ROUNDS = 400
_cache = {}


def make_case(name):
    """-> dict points (N, 1 + C) f32, B, C, rounds, redraws"""
    if name not in _cache:
        base = vox.make_case(name)
        pts = base['points'][_same_cell_in_f64(base['points'])].copy()
        w = weights(base['C'])
        redraws = 0
        for rounds in range(MAX_ROUNDS):
            bad = set()
            for training in (True, False):
                r = net_f64(pts, base['B'], w, training)
                bad.update(r['perm'][margin_violations(r)].tolist())
            if not bad:
                break
            for i in sorted(bad):                              # a stream of its own per (point, round): any point can be redrawn alone
                pts[i, 4:] = np.random.default_rng([vox.CASES[name]['seed'], i, rounds]).uniform(0, 1, base['C'] - 3)
            redraws += len(bad)
        else:
            raise AssertionError('case %s: margins not met after %d rounds' % (name, MAX_ROUNDS))
        _cache[name] = {'points': pts, 'B': base['B'], 'C': base['C'], 'name': name, 'rounds': rounds, 'redraws': redraws}
    c = _cache[name]
    return dict(c, points=c['points'].copy())


# ---- detector case: CenterPoint behind DynPillarVFE on a 64 x 64 grid, two synthetic Waymo-like frames ---------------------------
DET_PCR = [-10.24, -10.24, -2.0, 10.24, 10.24, 4.0]
DET_VOXEL = [0.32, 0.32, 6.0]
DET_GRID = [64, 64, 1]
DET_CLASSES = ['Vehicle', 'Pedestrian', 'Cyclist']
DET_FIRST_FRAME, DET_POINTS, DET_SEED = 40, 20000, 131
DET_SHIFT = [-25.0, 0.0, 0.0]                            # the synthetic boxes lie in x 5 .. 65: the crop sees a busy part of the frames
DET_GRADS = {'vfe.pfn_layers.0.linear.weight': np.s_[:], 'vfe.pfn_layers.1.linear.weight': np.s_[:16], 'backbone_2d.blocks.0.1.weight': np.s_[:8]}


def detector_inputs(kitti_batch):
    """kitti_batch: pcdet.datasets.synthetic.kitti_batch of THIS repository -> dict points (N, 6) [b, x, y, z, i, e], gt_boxes (B, G, 8),
    batch_size. The frames are shifted by DET_SHIFT; one seeded box per class joins the boxes that fall into the crop."""
    pts, off, gt = kitti_batch(DET_FIRST_FRAME, 2, DET_POINTS, waymo=True)
    B = len(off) - 1
    pts = pts.copy()
    pts[:, :3] += np.asarray(DET_SHIFT, np.float32)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))
    gts = []
    for b in range(B):
        g = gt[b].copy()
        g[:, :3] += np.asarray(DET_SHIFT, np.float32)
        inside = (g[:, 7] > 0) & (np.abs(g[:, 0]) < DET_PCR[3] - 1) & (np.abs(g[:, 1]) < DET_PCR[4] - 1)
        rng = np.random.default_rng(DET_SEED + b)
        extra = [[rng.uniform(-8, 8), rng.uniform(-8, 8), -1.0 + dz / 2 + rng.uniform(-0.1, 0.1), dx, dy, dz, rng.uniform(-np.pi, np.pi), cls]
                 for cls, (dx, dy, dz) in ((1, (4.7, 2.1, 1.7)), (2, (0.9, 0.86, 1.71)), (3, (1.78, 0.84, 1.78)))]
        gts.append(np.concatenate([g[inside], np.asarray(extra, np.float32)]))
    G = max(len(g) for g in gts)
    gt_out = np.zeros((B, G, 8), np.float32)
    for b, g in enumerate(gts):
        gt_out[b, :len(g)] = g
    return {'points': np.concatenate([bidx[:, None], pts], 1).astype(np.float32), 'gt_boxes': gt_out, 'batch_size': B}
