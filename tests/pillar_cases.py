"""Seeded cases, the f64 definition of the pillar feature net and the margin checks for the PointPillars tests
(tests/test_pointpillar_cpu.py, tests/test_pointpillar_gpu.py) and their golden generator (tests/golden/make_goldens_pointpillar.py).
No reference import here: this module travels with the tests.

Module cases live on a reduced grid: range [0, -10.24, -3, 20.48, 10.24, 1], voxel [0.16, 0.16, 4] -> 128 x 128 x 1.
  a        B = 2, M = 37, T = 32, C = 4: counts include 1, 2, 31 and 32, pillars at the grid corners (0, 0) and (ny - 1, nx - 1),
           frame 1 holds a single pillar, rows shuffled inside each frame
  b        C = 5, T = 20, M = 130: more than the 64 pillars a workgroup takes, more than two workgroups' worth, no multiple of 64
  c        M = 1
  a_big / a_nan   copies of `a` with 1e30 / NaN in every padded slot: results must equal a's bit for bit

Margins (asserted on the f64 pre-activations, train mode and eval mode): per pillar and channel the candidates are the valid slots
plus ONE padded slot when the pillar is not full (all padded slots hold the same value: ties among them are harmless). The maximum
must lie more than GAP = 1e-5 above the runner-up and more than GAP away from 0 - and, where that is more, MARGIN_FACTOR times the
bound on the f32 evaluation error of that very pillar's pre-activations (K products and sums on coordinates up to 20 m: a few 1e-6
here, so the two requirements are of the same order). A pillar that misses is redrawn alone, until every pillar holds. Two correct
f32 evaluations, in any summation order, with or without fused multiply-adds, then select the same slot and agree on the sign of
the maximum."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ref_pointpillar.npz')

PCR = [0.0, -10.24, -3.0, 20.48, 10.24, 1.0]
VOXEL = [0.16, 0.16, 4.0]
GRID = [128, 128, 1]                                     # nx, ny, nz
COUT = 64
EPS, MOMENTUM = 1e-3, 0.01
GAP = 1e-5
MARGIN_FACTOR = 4.0
WEIGHT_SEED = 311

CASES = {
    'a': dict(B=2, M=37, T=32, C=4, seed=1100),
    'b': dict(B=2, M=130, T=20, C=5, seed=2200),
    'c': dict(B=1, M=1, T=32, C=4, seed=3300),
}
GARBAGE = {'a_big': 1e30, 'a_nan': float('nan')}


def offsets():
    """voxel / 2 + range minimum, in Python floats as the reference's constructor forms them"""
    return [VOXEL[i] / 2 + PCR[i] for i in range(3)]


def vfe_cfg(num_filters=(64,), with_distance=False, use_absolute_xyz=True, use_norm=True):
    return {'NAME': 'PillarVFE', 'WITH_DISTANCE': with_distance, 'USE_ABSLOTE_XYZ': use_absolute_xyz, 'USE_NORM': use_norm,
            'NUM_FILTERS': list(num_filters)}


def weights(C):
    """seeded parameters and buffers of the single PFN layer, by state-dict key"""
    rng = np.random.default_rng(WEIGHT_SEED + C)
    K = C + 6
    return {'pfn_layers.0.linear.weight': (rng.normal(0, 1, (COUT, K)) / np.sqrt(K)).astype(np.float32),
            'pfn_layers.0.norm.weight': rng.uniform(0.5, 1.5, COUT).astype(np.float32),
            'pfn_layers.0.norm.bias': rng.normal(0, 0.2, COUT).astype(np.float32),
            'pfn_layers.0.norm.running_mean': rng.normal(0, 0.5, COUT).astype(np.float32),
            'pfn_layers.0.norm.running_var': rng.uniform(2.0, 6.0, COUT).astype(np.float32),
            'pfn_layers.0.norm.num_batches_tracked': np.zeros((), np.int64)}


def grad_out(name):
    p = CASES[name]
    return np.random.default_rng(p['seed'] + 7).normal(0, 1, (p['M'], COUT)).astype(np.float32)


def _pillar_points(name, m, attempt, coord, n, C):
    """the n points of pillar m (its own stream: a pillar can be redrawn alone), inside its cell"""
    rng = np.random.default_rng([CASES[name]['seed'], m, attempt])
    u = rng.uniform(0.02, 0.98, (n, 3))
    pts = np.empty((n, C), np.float32)
    pts[:, 0] = PCR[0] + (coord[3] + u[:, 0]) * VOXEL[0]
    pts[:, 1] = PCR[1] + (coord[2] + u[:, 1]) * VOXEL[1]
    pts[:, 2] = PCR[2] + u[:, 2] * VOXEL[2]
    pts[:, 3:] = rng.uniform(0, 1, (n, C - 3))
    return pts


def _draw(name):
    p = CASES[name]
    rng = np.random.default_rng(p['seed'])
    B, M, T, C = p['B'], p['M'], p['T'], p['C']
    nx, ny, _ = GRID
    per_frame = [M - (B - 1)] + [1] * (B - 1) if name == 'a' else [M // B + (1 if b < M % B else 0) for b in range(B)]
    coords, counts = [], []
    for b, n in enumerate(per_frame):
        cells = rng.choice(nx * ny, n, replace=False)
        cnt = rng.integers(1, T + 1, n)
        if name == 'a' and b == 0:
            cells = np.array([c for c in cells if c not in (0, nx * ny - 1)][:n - 2] + [0, nx * ny - 1])
            cnt[:4] = [1, 2, T - 1, T]
        order = rng.permutation(n)                       # rows shuffled inside the frame
        cells, cnt = cells[order], cnt[order]
        coords.append(np.stack([np.full(n, b), np.zeros(n, np.int64), cells // nx, cells % nx], 1))
        counts.append(cnt)
    coords = np.concatenate(coords).astype(np.int32)
    counts = np.concatenate(counts).astype(np.int32)
    voxels = np.zeros((M, T, C), np.float32)
    for m in range(M):
        voxels[m, :counts[m]] = _pillar_points(name, m, 0, coords[m], counts[m], C)
    return {'voxels': voxels, 'num_points': counts, 'coords': coords, 'B': B, 'name': name}


def augmented_f64(voxels, num_points, coords):
    """(M, T, K) f64 augmented points from the f32 inputs, everything in f64 - the centre too, as the reference's f64 run forms it
    (an f32 run forms coords * voxel + offset in f32, up to 1e-6 off at 20 m: part of every f32 route's error, the reference's
    own e_ref included)"""
    M, T, C = voxels.shape
    valid = np.arange(T)[None, :] < num_points[:, None]
    v = np.where(valid[..., None], voxels, 0).astype(np.float64)
    mean = v[:, :, :3].sum(1, keepdims=True) / num_points[:, None, None]
    off = offsets()
    ctr = np.stack([coords[:, 3].astype(np.float64) * VOXEL[0] + off[0], coords[:, 2].astype(np.float64) * VOXEL[1] + off[1],
                    coords[:, 1].astype(np.float64) * VOXEL[2] + off[2]], 1)
    f = np.concatenate([v, v[:, :, :3] - mean, v[:, :, :3] - ctr[:, None, :]], -1)
    return f * valid[..., None], valid


def vfe_f64(case, w, training):
    """the definition in f64 numpy -> dict(out (M,64), pre (M,T,64) BatchNorm outputs before the ReLU, A, b, mean, var (biased),
    running_mean / running_var after the step (training), f, valid)"""
    f, valid = augmented_f64(case['voxels'], case['num_points'], case['coords'])
    W = w['pfn_layers.0.linear.weight'].astype(np.float64)
    gamma, beta = w['pfn_layers.0.norm.weight'].astype(np.float64), w['pfn_layers.0.norm.bias'].astype(np.float64)
    x = f @ W.T                                          # (M, T, 64); padded rows are exact zeros
    n = x.shape[0] * x.shape[1]
    r = {'f': f, 'valid': valid}
    if training:
        mean, var = x.reshape(n, -1).mean(0), x.reshape(n, -1).var(0)
        r['running_mean'] = (1 - MOMENTUM) * w['pfn_layers.0.norm.running_mean'].astype(np.float64) + MOMENTUM * mean
        r['running_var'] = (1 - MOMENTUM) * w['pfn_layers.0.norm.running_var'].astype(np.float64) + MOMENTUM * var * n / max(n - 1, 1)
    else:
        mean, var = w['pfn_layers.0.norm.running_mean'].astype(np.float64), w['pfn_layers.0.norm.running_var'].astype(np.float64)
    scale = gamma / np.sqrt(var + EPS)
    r['A'], r['b'] = scale[:, None] * W, beta - mean * scale
    r['pre'] = (x - mean) * scale + beta
    r['out'] = np.maximum(r['pre'], 0).max(1)
    r['mean'], r['var'] = mean, var
    return r


def margins(r, num_points):
    """per pillar: (margin / required margin, margin), the worst over the channels; required = max(GAP, MARGIN_FACTOR * the f32
    evaluation bound of the pillar's pre-activations)"""
    pre, f, A, b = r['pre'], r['f'], r['A'], r['b']
    M, T, _ = pre.shape
    # f32 evaluation bound of one pre-activation: K products and K sums of partial results bounded by |b| + sum |A_k f_k|, each
    # rounded once (u = 2^-24; a fused multiply-add rounds less), plus the rounding of the mean / centre differences in f
    u = 2.0 ** -24
    bound = (f.shape[2] + 3) * u * (np.abs(b)[None, None, :] + np.abs(f) @ np.abs(A).T)
    ratio, gap = np.empty(M), np.empty(M)
    for m in range(M):
        n = int(num_points[m])
        k = n + 1 if n < T else n                        # valid slots + one padded slot
        cand = pre[m, :k]
        need = np.maximum(GAP, MARGIN_FACTOR * bound[m, :k].max(0))
        srt = np.sort(cand, 0)
        top = srt[-1]
        g = np.abs(top)
        if k > 1:                                        # a maximum below 0 passes nothing whichever slot holds it
            g = np.minimum(g, np.where(top > 0, top - srt[-2], np.inf))
        ratio[m], gap[m] = (g / need).min(), g.min()
    return ratio, gap


MAX_ROUNDS = 400
_cache = {}


def make_case(name):
    """-> dict voxels (M,T,C) f32 (padded slots zero), num_points (M) i32, coords (M,4) i32 [b,z,y,x], B, rounds, margin_ratio.
    Pillars whose margins do not hold (train mode or eval mode) get their points redrawn, the others stay, until all hold: the
    batch statistics move a little with every redraw, so all pillars are checked again each round."""
    if name in GARBAGE:
        base = make_case('a')
        v = base['voxels'].copy()
        v[np.arange(v.shape[1])[None, :] >= base['num_points'][:, None]] = GARBAGE[name]
        return dict(base, voxels=v, name=name)
    if name not in _cache:
        C = CASES[name]['C']
        w = weights(C)
        case = _draw(name)
        attempt = np.zeros(len(case['num_points']), np.int64)
        for rounds in range(MAX_ROUNDS):
            ratio = np.minimum(*[margins(vfe_f64(case, w, training), case['num_points'])[0] for training in (True, False)])
            bad = np.nonzero(ratio <= 1.0)[0]
            if len(bad) == 0:
                break
            for m in bad:
                attempt[m] += 1
                n = case['num_points'][m]
                case['voxels'][m, :n] = _pillar_points(name, m, attempt[m], case['coords'][m], n, C)
        else:
            raise AssertionError('case %s: margins not met after %d rounds' % (name, MAX_ROUNDS))
        case['rounds'], case['redraws'], case['margin_ratio'] = rounds, int(attempt.sum()), float(ratio.min())
        _cache[name] = case
    c = _cache[name]
    return dict(c, voxels=c['voxels'].copy())


# ---- detector case: two synthetic frames cropped to the reduced grid ---------------------------------------------------------
DET_FIRST_FRAME, DET_POINTS, DET_MAX_VOXELS, DET_T = 40, 20000, 16000, 32
DET_SEED = 97
# box centres of the synthetic frames lie in x 5 .. 65, y -30 .. 30: the frames are shifted by DET_SHIFT before the crop, so that
# the reduced range sees a busy part of them
DET_SHIFT = [-8.0, 0.0, 0.0]
# the gradients the golden keeps and the slice of each (the first-layer gradient whole would be 440 KB in f32 + f64)
DET_GRADS = {'vfe.pfn_layers.0.linear.weight': np.s_[:], 'backbone_2d.blocks.0.1.weight': np.s_[:8], 'dense_head.conv_cls.weight': np.s_[:]}


def pillarize(points, pcr=PCR, voxel=VOXEL, grid=GRID, max_points=DET_T, max_voxels=DET_MAX_VOXELS):
    """first-come pillar grouping of one frame in numpy: points (n, C) -> voxels (M, T, C), coords (M, 3) [z, y, x], counts (M)"""
    p = points.astype(np.float32)
    c = np.floor((p[:, :3] - np.asarray(pcr[:3], np.float32)) / np.asarray(voxel, np.float32)).astype(np.int64)
    ok = ((c >= 0) & (c < np.asarray(grid))).all(1)
    p, c = p[ok], c[ok]
    lin = c[:, 1] * grid[0] + c[:, 0]
    uniq, first, inv = np.unique(lin, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))                 # pillars in order of first appearance
    vid = rank[inv]
    keep = vid < max_voxels
    p, vid = p[keep], vid[keep]
    M = int(min(len(uniq), max_voxels))
    voxels = np.zeros((M, max_points, p.shape[1]), np.float32)
    counts = np.zeros(M, np.int32)
    for i in range(len(p)):
        v = vid[i]
        if counts[v] < max_points:
            voxels[v, counts[v]] = p[i]
            counts[v] += 1
    order = np.argsort(first)
    cells = uniq[order][:M]
    coords = np.stack([np.zeros(M, np.int64), cells // grid[0], cells % grid[0]], 1).astype(np.int32)
    return voxels, coords, counts


def detector_inputs(kitti_batch):
    """kitti_batch: the synthetic generator (pcdet.datasets.synthetic.kitti_batch of THIS repository) -> dict voxels, voxel_coords
    (M,4) [b,z,y,x], voxel_num_points, gt_boxes (B,G,8), batch_size"""
    pts, off, gt = kitti_batch(DET_FIRST_FRAME, 2, DET_POINTS)
    B = len(off) - 1
    vs, cs, ns, gts = [], [], [], []
    for b in range(B):
        p = pts[off[b]:off[b + 1]].copy()
        p[:, :3] += np.asarray(DET_SHIFT, np.float32)
        g = gt[b].copy()
        g[:, :3] += np.asarray(DET_SHIFT, np.float32)
        inside = (g[:, 0] > PCR[0] + 1) & (g[:, 0] < PCR[3] - 1) & (g[:, 1] > PCR[1] + 1) & (g[:, 1] < PCR[4] - 1)
        # few of a frame's boxes fall into the 20 m crop: one seeded box per class joins them (ground truth is an input)
        rng = np.random.default_rng(DET_SEED + b)
        extra = [[rng.uniform(3, 17), rng.uniform(-7, 7), -1.73 + dz / 2 + rng.uniform(-0.1, 0.1), dx, dy, dz, rng.uniform(-np.pi, np.pi), cls]
                 for cls, (dx, dy, dz) in ((1, (3.9, 1.6, 1.56)), (2, (0.8, 0.6, 1.73)), (3, (1.76, 0.6, 1.73)))]
        gts.append(np.concatenate([g[inside], np.asarray(extra, np.float32)]))
        v, c, n = pillarize(p)
        vs.append(v); ns.append(n)
        cs.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
    G = max(1, max(len(g) for g in gts))
    gt_out = np.zeros((B, G, 8), np.float32)
    for b, g in enumerate(gts):
        gt_out[b, :len(g)] = g
    return {'voxels': np.concatenate(vs), 'voxel_coords': np.concatenate(cs).astype(np.int32), 'voxel_num_points': np.concatenate(ns),
            'gt_boxes': gt_out, 'batch_size': B}


# Margin of the detector case around the ReLU kinks. Every BatchNorm output of the step (the pillar net's maximum over the slots, the
# 16 BatchNorm2d layers of the backbone's blocks, the 3 of its up-sampling branches) must lie farther than DET_KINK from 0 in the
# reference's f64 run. An element closer to 0 than the f32 error of the forward pass gets its ReLU mask from rounding, and with the
# gradient of 70,000 anchors concentrated on some 30 positives one flipped mask moves the first-layer gradients by a percent: fifteen
# flips (|pre-activation| <= 3e-5) between an f32 and the f64 run of the same network moved them by 1.6 %, and with the masks
# pinned the two agree to 8e-5. The golden generator therefore shifts the BatchNorm biases channel by channel, layer by layer in
# execution order, by the smallest amount that clears the margin (nudge_bias; typically 1e-4 ... 1e-3 on biases ~ N(0, 0.1)); the
# shifted biases are stored in the golden and loaded by detector_state(overrides=). 2e-4 is 8 x the largest forward error seen
# between f32 and f64 runs of this stack (2.5e-5 of the activation scale) and 50 x that of the convolution kernels (4e-6).
DET_KINK = 2e-4


def nudge_bias(values, margin=DET_KINK):
    """values (n) f64: the pre-activations of one channel -> the shift d of smallest size with min |values + d| > margin"""
    v = np.sort(np.asarray(values, np.float64))
    if len(v) == 0 or np.abs(v).min() > margin:
        return 0.0
    m = margin * 1.25                                    # (room for the f32 rounding of the shifted bias)
    lo = np.concatenate([[-np.inf], v])                  # zero may sit in any gap (lo + m, hi - m) of the sorted values
    hi = np.concatenate([v, [np.inf]])
    ok = hi - lo > 2 * m
    z = np.clip(0.0, lo[ok] + m, hi[ok] - m)             # the point of each wide gap that is nearest to 0
    return float(-z[np.abs(z).argmin()])


def detector_state(state_dict_items, seed=DET_SEED, overrides=None):
    """seeded values for every entry of a detector state dict, in name order from one numpy stream: (name, shape, is float) ->
    {name: array}; overrides: {name: array} replacing seeded entries (the kink-margin biases of the golden: golden_bias_overrides). Convolution / linear weights ~ N(0, 1 / fan_in), BatchNorm weight in [0.5, 1.5], biases and running means
    ~ N(0, 0.1), running variances in [0.5, 1.5]; integer buffers zero; the classification bias -log(99), the head's own initial value
    (with a random bias the focal loss of 70,000 anchors over some 30 positives is in the thousands)."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape, is_float in sorted(state_dict_items):
        if not is_float:
            a = np.zeros(shape, np.int64)
        elif name.endswith('conv_cls.bias'):
            a = np.full(shape, -np.log(99.0), np.float32)
        elif name.endswith('running_var') or (name.endswith('weight') and len(shape) == 1):
            a = rng.uniform(0.5, 1.5, shape).astype(np.float32)
        elif len(shape) == 1:
            a = rng.normal(0, 0.1, shape).astype(np.float32)
        else:
            fan_in = int(np.prod(shape)) // shape[0]
            a = (rng.normal(0, 1, shape) / np.sqrt(fan_in)).astype(np.float32)
        sd[name] = a
    for name, a in (overrides or {}).items():
        assert sd[name].shape == a.shape, name
        sd[name] = np.asarray(a, np.float32)
    return sd


def golden_bias_overrides(gold):
    """the BatchNorm biases the golden generator shifted away from the ReLU kinks, by state-dict key"""
    return {k[len('det_bias/'):]: gold[k] for k in gold.files if k.startswith('det_bias/')}
