"""Hand-built index patterns for the first-layer scatter of the set-abstraction modules (group_affine_rows_grad_kernel,
csrc/pointnet2_stack.hip) and its float64 reference. numpy and CPU torch only; no ball query: the patterns are the point.

A case (dict): B, xyz_batch_cnt (B), new_xyz_batch_cnt (B), idx (M, ns) int32 local to the frame, empty (M) bool, xyz (n_src, 3),
new_xyz (M, 3), P (n_src, H), W1x (3, H), grad_z (M * ns, H), mean / invstd / gamma / beta / dbeta / dgamma (H), all f32, plus
H, ns, M, n_src, n = M * ns and `row` (M, ns) int64, the source row of every pair (start of the frame + idx).

mean / invstd are the batch statistics of y over all n rows (rows of empty balls count as 0, as in the forward) and dbeta / dgamma the
sums that go with grad_z, so |xhat| <= sqrt(n) holds and the bound of sa_fixed_point_scale applies; `exact` sets them by hand.

reference(name) (float64, every f32 input taken as it is):
  y = P[row] + rel @ W1x, xhat = (y - mean) invstd, z = gamma xhat + beta, v = gamma invstd (grad_z [z > 0] - dbeta / n - xhat dgamma / n),
  grad_P = index_add(row, v) over the pairs of live balls, part_sum[d] = sum rel[:, d] v, mag = index_add(row, |v|).  reference(name, bn=False): v = grad_z (crb_group_affine_rows_grad_stack).
ReLU edge: grad_z is 0 wherever |z| <= 1e-4 (1 + |beta|), so an f32 and an f64 evaluation of the mask cannot disagree on an entry that
matters; at most EDGE_CAP of the live entries of a case may be touched (tests/test_sa_scatter_cpu.py)."""
import functools

import numpy as np
import torch

EDGE_CAP = 1e-3
EPS = 1e-5
NAMES = ('one_row', 'all_distinct', 'padded', 'padded_ns32', 'padded_ns48', 'alternating', 'borders', 'empties', 'outlier', 'exact',
         'tiny', 'huge', 'two_rows')
# width of every case: 16, 32, 64 and 128 at least twice each
WIDTH = {'one_row': 128, 'all_distinct': 16, 'padded': 64, 'padded_ns32': 32, 'padded_ns48': 16, 'alternating': 32, 'borders': 128,
         'empties': 64, 'outlier': 64, 'exact': 32, 'tiny': 16, 'huge': 128, 'two_rows': 64}
# run lengths of rows 0, 1, 2, ... of `borders` in source-row order (position = slab * 64 + pair, 0-based):
#   row 0: 0..14 (ends one before a segment border)       row 1: 15..16 (crosses it)        row 2: 17..62       row 3: 63 (last of slab 0)
#   row 4: 64..79 (one whole segment)                     row 5: 80..111 (2 whole segments)
#   row 6: 112..128 (the last segment of slab 1 and pair 0 of slab 2: one row in two slabs)
#   row 7: 129..143                                       row 8: 144..191 (3 whole segments, ends with slab 2)
#   row 9: 192..271 (5 whole segments: all of slab 3 and the first of slab 4)
#   row 10: 272..318 (ends at pair 62 of slab 4)          row 11: 319..320 (pair 63 of slab 4 and pair 0 of slab 5)
BORDER_RUNS = (15, 2, 46, 1, 16, 32, 17, 15, 48, 80, 47, 2)


def _padded_idx(rng, counts_src, counts_qry, ns):
    """the ball-query shape: j ~ U{1..ns} distinct hits (the first ns balls: j = 1, 2, .., ns, so that every count occurs), then
    repeats of the first hit"""
    out = []
    for ns_src, nq in zip(counts_src, counts_qry):
        for _ in range(nq):
            j = len(out) + 1 if len(out) < ns else int(rng.integers(1, ns + 1))
            hits = rng.choice(ns_src, j, replace=False)
            out.append(np.concatenate([hits, np.full(ns - j, hits[0])]))
    return np.stack(out).astype(np.int32)


def _layout(name, rng):
    """-> ns, xyz_batch_cnt, new_xyz_batch_cnt, idx (M, ns) local, empty (M)"""
    if name == 'one_row':
        M = 515                                                # 8240 pairs: not a multiple of 64
        return 16, [50], [M], np.full((M, 16), 7, np.int32), np.zeros(M, bool)
    if name == 'two_rows':                                     # one_row with two targets: the BatchNorm backward's values sum to 0 over
        M = 131                                                # all pairs, so the two rows get large sums of opposite sign
        return 16, [50], [M], np.where(rng.random((M, 16)) < 0.5, 7, 9).astype(np.int32), np.zeros(M, bool)
    if name == 'all_distinct':
        src, qry = [2600, 2600], [161, 160]                    # M = 321 = 4 * 80 + 1
        idx = np.concatenate([rng.permutation(s)[:q * 16].reshape(q, 16) for s, q in zip(src, qry)]).astype(np.int32)
        return 16, src, qry, idx, np.zeros(321, bool)
    if name in ('padded', 'tiny', 'huge'):
        src, qry = [400, 300], [300, 211]
        return 16, src, qry, _padded_idx(rng, src, qry, 16), np.zeros(511, bool)
    if name == 'padded_ns32':
        src, qry = [300, 200], [70, 31]
        return 32, src, qry, _padded_idx(rng, src, qry, 32), np.zeros(101, bool)
    if name == 'padded_ns48':
        src, qry = [300, 200], [33, 20]
        return 48, src, qry, _padded_idx(rng, src, qry, 48), np.zeros(53, bool)
    if name == 'alternating':
        M = 130
        idx = np.empty((M, 16), np.int32)
        for m in range(M):
            k = 2 if m % 2 == 0 else 3                         # A,B,A,B,...  /  A,B,C,A,B,C,...
            idx[m] = rng.choice(200, k, replace=False)[np.arange(16) % k]
        return 16, [200], [M], idx, np.zeros(M, bool)
    if name == 'borders':
        rows = np.repeat(np.arange(len(BORDER_RUNS)), BORDER_RUNS)
        fill = (-len(rows)) % 64 + 64 + 16                     # then single pairs of further rows: 464 pairs = 7.25 slabs, 29 balls
        rows = np.concatenate([rows, len(BORDER_RUNS) + np.arange(fill)])
        M = len(rows) // 16
        return 16, [int(rows.max()) + 5], [M], rng.permutation(rows).reshape(M, 16).astype(np.int32), np.zeros(M, bool)
    if name == 'empties':
        src, qry = [50, 200, 100, 150, 60], [0, 41, 12, 30, 0]
        idx = _padded_idx(rng, src, qry, 16)
        empty = np.zeros(83, bool)
        empty[2:41:3] = True                                   # interleaved
        empty[8:12] = True                                     # queries 8..11 = pairs 128..191: a whole empty slab
        empty[41:53] = True                                    # frame 2: queries, all empty
        empty[53::4] = True
        idx[empty] = 0                                         # what ball_query returns for an empty ball
        return 16, src, qry, idx, empty
    if name == 'outlier':
        src, qry = [1500, 1500], [1050, 1050]
        idx = np.concatenate([rng.integers(1, s, (q, 16)) for s, q in zip(src, qry)]).astype(np.int32)
        idx[3, 5] = 0                                          # row 0 of frame 0, the outlier, is hit by exactly one pair
        return 16, src, qry, idx, np.zeros(2100, bool)
    if name == 'exact':
        src, qry = [60, 40], [100, 63]
        idx = _padded_idx(rng, src, qry, 16)
        idx[:20] = 3                                           # and one row with a few hundred pairs
        return 16, src, qry, idx, np.zeros(163, bool)
    raise KeyError(name)


SEED = {n: 100 + i for i, n in enumerate(NAMES)}


@functools.lru_cache(maxsize=None)
def case(name):
    rng = np.random.default_rng(SEED[name])
    H = WIDTH[name]
    ns, src, qry, idx, empty = _layout(name, rng)
    B, M, n_src = len(src), int(sum(qry)), int(sum(src))
    n = M * ns
    assert idx.shape == (M, ns) and n_src <= 12000 and M <= 2100
    start = np.concatenate([[0], np.cumsum(src)[:-1]])
    qframe = np.repeat(np.arange(B), qry)
    assert all(int(idx[qframe == b].max(initial=0)) < src[b] for b in range(B)) and int(idx.min()) >= 0
    row = start[qframe][:, None] + idx.astype(np.int64)
    f32 = np.float32
    c = {'name': name, 'B': B, 'H': H, 'ns': ns, 'M': M, 'n': n, 'n_src': n_src, 'idx': idx, 'empty': empty, 'row': row,
         'xyz_batch_cnt': np.asarray(src, np.int32), 'new_xyz_batch_cnt': np.asarray(qry, np.int32)}
    live = np.repeat(~empty, ns)
    if name == 'exact':
        c['xyz'], c['new_xyz'] = np.zeros((n_src, 3), f32), np.zeros((M, 3), f32)
        c['P'] = rng.integers(-8, 9, (n_src, H)).astype(f32)
        c['W1x'] = rng.normal(size=(3, H)).astype(f32)
        c['grad_z'] = (rng.integers(-8, 9, (n, H)) * 2.0 ** -10).astype(f32)
        c['mean'], c['invstd'], c['gamma'] = np.zeros(H, f32), np.ones(H, f32), np.ones(H, f32)
        c['beta'], c['dbeta'], c['dgamma'] = np.full(H, 100, f32), np.zeros(H, f32), np.zeros(H, f32)
        c['edge_touched'] = 0.0
        return c
    c['xyz'], c['new_xyz'] = rng.normal(size=(n_src, 3)).astype(f32), rng.normal(size=(M, 3)).astype(f32)
    c['P'] = rng.normal(size=(n_src, H)).astype(f32)
    c['W1x'] = (rng.normal(size=(3, H)) * 0.3).astype(f32)
    c['gamma'] = (rng.normal(size=H) * 0.5 + 0.8).astype(f32)
    c['beta'] = (rng.normal(size=H) * 0.3).astype(f32)
    gz = rng.normal(size=(n, H))
    if name == 'outlier':
        c['P'][0] *= 1e3                                       # |xhat| of its one pair is close to sqrt(n)
        c['gamma'] = (np.abs(rng.normal(size=H)) * 0.5 + 2.5).astype(f32)
        c['beta'] = (rng.normal(size=H) * 0.02).astype(f32)    # the mask follows the sign of xhat: dgamma / n does not average out
        gz = rng.uniform(0.9, 1.0, size=(n, H))                # one sign: dbeta / n is about max |d|
    gz = gz * {'tiny': 1e-41, 'huge': 1e30}.get(name, 1.0)
    y = _y64(c)
    mean = y.mean(0)
    invstd = 1.0 / np.sqrt(y.var(0) + EPS)
    c['mean'], c['invstd'] = mean.astype(f32), invstd.astype(f32)
    xhat = (y - c['mean'].astype(np.float64)) * c['invstd'].astype(np.float64)
    z = c['gamma'].astype(np.float64) * xhat + c['beta'].astype(np.float64)
    edge = (np.abs(z) <= 1e-4 * (1.0 + np.abs(c['beta'].astype(np.float64)))) & live[:, None]
    c['edge_touched'] = float(edge.sum()) / max(int(live.sum()) * H, 1)
    gz = np.where(edge | ~live[:, None], 0.0, gz).astype(f32)  # rows of empty balls: 0 here, the tests overwrite them
    c['grad_z'] = gz
    d = gz.astype(np.float64) * (z > 0)
    c['dbeta'], c['dgamma'] = d.sum(0).astype(f32), (d * xhat).sum(0).astype(f32)
    return c


def _y64(c):
    """(n, H) float64 y = P[row] + rel @ W1x, 0 on the rows of empty balls; also used for the `y` operand of the _bn_stack form"""
    rel = rel64(c)
    y = c['P'].astype(np.float64)[c['row'].reshape(-1)] + rel @ c['W1x'].astype(np.float64)
    y[np.repeat(c['empty'], c['ns'])] = 0.0
    return y


def rel64(c):
    rel = c['xyz'].astype(np.float64)[c['row'].reshape(-1)] - np.repeat(c['new_xyz'].astype(np.float64), c['ns'], 0)
    rel[np.repeat(c['empty'], c['ns'])] = 0.0
    return rel


@functools.lru_cache(maxsize=None)
def reference(name, bn=True):
    """-> dict of float64 torch tensors: v (n, H), grad_P, mag (n_src, H), part_sum (3, H), y (n, H), xhat"""
    c = case(name)
    n, H = c['n'], c['H']
    live = torch.from_numpy(np.repeat(~c['empty'], c['ns']))
    rel = torch.from_numpy(rel64(c))
    y = torch.from_numpy(_y64(c))
    gz = torch.from_numpy(c['grad_z']).double()
    t = {k: torch.from_numpy(c[k]).double() for k in ('mean', 'invstd', 'gamma', 'beta', 'dbeta', 'dgamma')}
    xhat = (y - t['mean']) * t['invstd']
    if bn:
        z = t['gamma'] * xhat + t['beta']
        v = t['gamma'] * t['invstd'] * (gz * (z > 0) - t['dbeta'] / n - xhat * t['dgamma'] / n)
    else:
        v = gz.clone()
    v = v * live[:, None]
    rows = torch.from_numpy(c['row'].reshape(-1))[live]
    grad_P = torch.zeros((c['n_src'], H), dtype=torch.float64).index_add_(0, rows, v[live])
    mag = torch.zeros((c['n_src'], H), dtype=torch.float64).index_add_(0, rows, v[live].abs())
    part_sum = rel.t() @ v
    return {'v': v, 'grad_P': grad_P, 'mag': mag, 'part_sum': part_sum, 'y': y, 'xhat': xhat, 'live': live}


def sort_key(c):
    """key of crb_pair_sort_by_source: the source row of a pair, n_src for the pairs of empty balls"""
    return np.where(np.repeat(c['empty'], c['ns']), c['n_src'], c['row'].reshape(-1))


def maxima(c):
    """the scalar maxima sa_fixed_point_scale takes, from the case's f32 inputs (grad_z over the rows of live balls)"""
    live = np.repeat(~c['empty'], c['ns'])
    gz = np.abs(c['grad_z'].astype(np.float64))[live]
    return (float(gz.max()) if gz.size else 0.0,
            float(np.abs(c['gamma'].astype(np.float32) * c['invstd'].astype(np.float32)).max()),
            float(np.abs(c['dbeta']).max()), float(np.abs(c['dgamma']).max()))
