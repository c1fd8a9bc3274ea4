"""Small hand-built inputs and independent numpy references for the point-set ops of csrc/pointnet2_stack.hip (farthest point sampling,
the five ball-query kernels, grouping, three-NN, interpolation) at the places where such kernels go wrong: launch-variant boundaries,
exact ties, the radius itself, hit counts around nsample, the 64-candidate step, ragged and empty frames, hash collisions and the
fall-back thresholds of the grid and grouped kernels. numpy only, fixed seeds, no GPU, no oracle.

The references are written from the definitions (one loop over frames, numpy inside), not from oracle/pointnet2_oracle.c:

  ref_ball_query       d2 = (qx-x)*(qx-x) + (qy-y)*(qy-y) + (qz-z)*(qz-z) in f32, left to right; hit = d2 < f32(r)*f32(r); the first
                       nsample hits in index order, padded with the first hit; an empty ball is all zeros with its flag set; indices
                       are local to the frame
  ref_fps              start at 0; running distance min(old, f32 d2 to the last pick), initially 1e10; winner = largest distance, then
                       smallest bit-reversed (k mod bs) over log2 bs bits with bs = min(2^floor(log2 n), 1024), then smallest k
  ref_three_nn         the three smallest f32 d2 ordered by (distance, index); a missing neighbour is (inf, start row of the frame)
  ref_three_interpolate  (w0*f0 + w1*f1) + w2*f2 in f32
  ref_group_points     a gather; (M, C, nsample)
  *_grad64             f64 sums, with the number of addends and the sum of |addend| per output element (the rounding bound of a sum
                       in any order: (count + 1) 2^-24 sum |addend|)

Every reference takes `mutant=`: a named, deliberately wrong variant. tests/test_pointnet2_edges_cpu.py runs the mutants over the
cases and requires each of them to be told apart from the true reference somewhere - the cases, not the references, are on trial.

Ball-query cases (dict): name, xyz (N, 3), xyz_cnt (B), new_xyz (M, 3), new_cnt (B), pairs = ((ra, nsa, rb, nsb), ...) the queries to
run (ra < rb and ra == rb: the 8-queries-per-wave kernel or the grid; ra > rb: the one-query-per-wave pair kernel), `claims` = what the
case is built to be (checked on the CPU). Grouped cases add `group`.
"""
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24                                   # unit roundoff of f32

POINT_CNT = (0, 1, 63, 64, 65, 0, 130, 0)        # empty frames: first, in the middle (next to a one-point frame), last
QUERY_CNT = (3, 0, 4, 5, 31, 2, 33, 1)           # 79 queries; a frame without queries; queries into empty frames
M_TOTALS = (1, 3, 4, 5, 31, 32, 33, 79)          # B = 1: around the 4 waves of a workgroup and the 4 x 8 queries of the multi kernel
GENERIC_PAIRS = ((0.8, 16, 1.6, 32), (1.0, 1, 1.0, 65), (1.6, 24, 0.8, 7), (0.8, 128, 1.6, 2))
HIT_NSAMPLES = (1, 2, 16, 63, 64, 65, 128)
GROUPS = (1, 7, 216)
GQ_CAP = 2048
BQG_MAX_CAND, BQG_MAX_HITS = 4096, 1024

FPS_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 8192, 8193, 20480, 20481, 40960, 40961)
FPS_TIE_SIZES = (2400, 6000, 12000, 30000, 42000)         # one per launch variant, every point 8 times


def fps_variant(n):
    """the kernel crb_farthest_point_sample launches for n points per frame"""
    ppt = -(-n // 1024)
    return ('fps2_kernel<4>' if ppt <= 4 else 'fps2_kernel<8>' if ppt <= 8 else 'fps2_kernel<20>' if ppt <= 20 else
            'fps_kernel<40,false>' if ppt <= 40 else 'fps_large_kernel')


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _starts(cnt):
    cnt = np.asarray(cnt, np.int64)
    return np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)


def d2_f32(q, p):
    """(Q, 3), (N, 3) f32 -> (Q, N) f32 squared distances, the kernels' expression"""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    dx, dy, dz = (q[:, None, a] - p[None, :, a] for a in range(3))
    return dx * dx + dy * dy + dz * dz


# ------------------------------------------------------------------------------------------------------------------ references
BALL_MUTANTS = ('le', 'pad_last', 'candidate_order', 'wrong_start')
FPS_MUTANTS = ('tie_larger_k', 'tie_plain_k')
NN_MUTANTS = ('tie_higher_index', 'wrong_start')


def ref_ball_query(radius, nsample, xyz, xyz_cnt, new_xyz, new_cnt, mutant=None):
    """-> idx (M, nsample) int32 local to the frame, empty (M) bool"""
    xyz, new_xyz = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(new_xyz, F32).reshape(-1, 3)
    r2 = F32(radius) * F32(radius)
    M = len(new_xyz)
    idx, empty = np.zeros((M, nsample), np.int32), np.zeros((M,), bool)
    xs, qs = _starts(new_cnt if mutant == 'wrong_start' else xyz_cnt), _starts(new_cnt)
    for b in range(len(xyz_cnt)):
        p = xyz[xs[b]:xs[b] + int(xyz_cnt[b])]
        q0, q1 = int(qs[b]), int(qs[b]) + int(new_cnt[b])
        if q1 == q0:
            continue
        d2 = d2_f32(new_xyz[q0:q1], p)
        inside = d2 <= r2 if mutant == 'le' else d2 < r2
        order = None
        if mutant == 'candidate_order' and len(p):          # the order of a cell-sorted candidate list
            cell = np.floor(p / (F32(radius) * F32(1.001))).astype(np.int64)
            order = np.lexsort((np.arange(len(p)), cell[:, 0], cell[:, 1], cell[:, 2]))
        for q in range(q0, q1):
            row = inside[q - q0]
            hits = np.flatnonzero(row) if order is None else order[row[order]]
            hits = hits[:nsample]
            if len(hits) == 0:
                empty[q] = True
                continue
            idx[q, :len(hits)] = hits
            idx[q, len(hits):] = hits[-1] if mutant == 'pad_last' else hits[0]
    return idx, empty


def _bit_reverse(v, bits):
    out = np.zeros_like(v)
    for i in range(bits):
        out |= ((v >> i) & 1) << (bits - 1 - i)
    return out


def ref_fps(xyz, m, mutant=None):
    """xyz (B, n, 3) -> (B, m) int32"""
    xyz = np.asarray(xyz, F32)
    B, n, _ = xyz.shape
    log2bs = min(n.bit_length() - 1, 10)
    k = np.arange(n, dtype=np.int64)
    br = _bit_reverse(k % (1 << log2bs), log2bs)
    key = {None: (br << 32) + k, 'tie_larger_k': (br << 32) + (n - 1 - k), 'tie_plain_k': k}[mutant]
    out = np.zeros((B, m), np.int32)
    for b in range(B):
        dist = np.full((n,), 1e10, F32)
        last = 0
        for j in range(1, m):
            dist = np.minimum(dist, d2_f32(xyz[b, last:last + 1], xyz[b])[0])
            cand = np.flatnonzero(dist == dist.max())
            last = int(cand[np.argmin(key[cand])])
            out[b, j] = last
    return out


def fps_tie_sizes(xyz, m):
    """-> per frame, the number of candidates that share the largest running distance in every round (1 = no tie)"""
    xyz = np.asarray(xyz, F32)
    picks = ref_fps(xyz, m)
    sizes = np.ones(picks.shape, np.int64)
    for b in range(xyz.shape[0]):
        dist = np.full((xyz.shape[1],), 1e10, F32)
        for j in range(1, m):
            dist = np.minimum(dist, d2_f32(xyz[b, picks[b, j - 1]][None], xyz[b])[0])
            sizes[b, j] = int((dist == dist.max()).sum())
    return sizes


def ref_three_nn(unknown, ucnt, known, kcnt, mutant=None):
    """-> dist2 (N, 3) f32, idx (N, 3) int32 rows of `known`"""
    unknown, known = np.asarray(unknown, F32).reshape(-1, 3), np.asarray(known, F32).reshape(-1, 3)
    N = len(unknown)
    us, ks = _starts(ucnt), _starts(ucnt if mutant == 'wrong_start' else kcnt)
    dist2, idx = np.full((N, 3), np.inf, F32), np.zeros((N, 3), np.int32)
    for b in range(len(ucnt)):
        u0, u1 = int(us[b]), int(us[b]) + int(ucnt[b])
        kp = known[ks[b]:ks[b] + int(kcnt[b])]
        idx[u0:u1] = ks[b]
        K = len(kp)
        if u1 == u0 or K == 0:
            continue
        d = d2_f32(unknown[u0:u1], kp)
        if mutant == 'tie_higher_index':
            order = K - 1 - np.argsort(d[:, ::-1], axis=1, kind='stable')[:, :3]
        else:
            order = np.argsort(d, axis=1, kind='stable')[:, :3]            # stable: equal distances keep index order
        t = min(K, 3)
        dist2[u0:u1, :t] = np.take_along_axis(d, order, 1)[:, :t]
        idx[u0:u1, :t] = order[:, :t] + ks[b]
    return dist2, idx


def ref_three_interpolate(feat, idx, w):
    feat, w = np.asarray(feat, F32), np.asarray(w, F32)
    return (w[:, 0:1] * feat[idx[:, 0]] + w[:, 1:2] * feat[idx[:, 1]]) + w[:, 2:3] * feat[idx[:, 2]]


def _scatter64(rows, addends, n_rows):
    """rows (P), addends (P, C) f64 -> sum (n_rows, C), count, sum of |addend|"""
    C = addends.shape[1]
    acc, cnt, mag = np.zeros((n_rows, C)), np.zeros((n_rows, C), np.int64), np.zeros((n_rows, C))
    np.add.at(acc, rows, addends)
    np.add.at(cnt, rows, 1)
    np.add.at(mag, rows, np.abs(addends))
    return acc, cnt, mag


def ref_three_interpolate_grad64(grad_out, idx, w, M):
    """-> grad (M, C) f64, count, sum |addend|; an addend is grad_out[i, c] * w[i, t] (exact in f64)"""
    g, w = np.asarray(grad_out, np.float64), np.asarray(w, np.float64)
    add = (g[:, None, :] * w[:, :, None]).reshape(-1, g.shape[1])
    return _scatter64(np.asarray(idx, np.int64).reshape(-1), add, M)


def _group_rows(idx, idx_cnt, feat_cnt):
    start = np.repeat(_starts(feat_cnt), np.asarray(idx_cnt, np.int64))
    return np.asarray(idx, np.int64) + start[:, None]


def ref_group_points(feat, feat_cnt, idx, idx_cnt):
    """feat (N, C), idx (M, ns) local -> (M, C, ns)"""
    return np.ascontiguousarray(np.asarray(feat, F32)[_group_rows(idx, idx_cnt, feat_cnt)].transpose(0, 2, 1))


def ref_group_points_grad64(grad_out, idx, idx_cnt, feat_cnt, N):
    """grad_out (M, C, ns) -> grad (N, C) f64, count, sum |addend|"""
    g = np.asarray(grad_out, np.float64)
    rows = _group_rows(idx, idx_cnt, feat_cnt)
    return _scatter64(rows.reshape(-1), g.transpose(0, 2, 1).reshape(-1, g.shape[1]), N)


def grad_bound(count, mag):
    """worst-case rounding of a sum of `count` f32 addends in any order, product rounding included"""
    return (count + 1) * U * mag


# ------------------------------------------------------------------------------------------------------------------ grid model
def grid_cell(radius_b):
    """-> (cell edge, its inverse) as crb_ball_query2_grid_stack computes them in f32"""
    edge = F32(radius_b) * F32(1.001)
    return edge, F32(1.0) / edge


def grid_cells_of(xyz, radius_b):
    return np.floor(np.asarray(xyz, F32) * grid_cell(radius_b)[1]).astype(np.int64)


def grid_buckets(n_total):
    nb = 1024
    while nb < 2 * n_total and nb < (1 << 24):
        nb <<= 1
    return nb


def grid_bucket(b, cells, n_buckets):
    """bqg_bucket restated: cells (..., 3) int64 -> bucket"""
    m = 0xffffffff
    h = ((cells[..., 0] * 73856093) & m) ^ ((cells[..., 1] * 19349663) & m) ^ ((cells[..., 2] * 83492791) & m) ^ \
        ((np.asarray(b, np.int64) * 2654435761) & m)
    h ^= h >> 15
    return h & (n_buckets - 1)


NEIGHBOURS = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing='ij'), -1).reshape(27, 3)


def grid_candidates(case, q, radius_b):
    """T of query q: the points (of any frame) in the distinct buckets of its 27 neighbour cells"""
    b = int(np.searchsorted(np.cumsum(case['new_cnt']), q, side='right'))
    nb = grid_buckets(len(case['xyz']))
    mine = np.unique(grid_bucket(b, grid_cells_of(case['new_xyz'][q], radius_b)[None] + NEIGHBOURS, nb))
    frame = np.repeat(np.arange(len(case['xyz_cnt'])), case['xyz_cnt'])
    pts = grid_bucket(frame, grid_cells_of(case['xyz'], radius_b), nb)
    return int(np.isin(pts, mine).sum())


def hits_inside(case, q, radius):
    """number of points of q's frame inside the ball"""
    b = int(np.searchsorted(np.cumsum(case['new_cnt']), q, side='right'))
    s = int(_starts(case['xyz_cnt'])[b])
    p = case['xyz'][s:s + int(case['xyz_cnt'][b])]
    return int((d2_f32(case['new_xyz'][q:q + 1], p)[0] < F32(radius) * F32(radius)).sum())


# ------------------------------------------------------------------------------------------------------------------ ball-query cases
def _case(name, xyz, xyz_cnt, new_xyz, new_cnt, pairs, **claims):
    return _frozen(dict(name=name, xyz=np.ascontiguousarray(xyz, F32).reshape(-1, 3), xyz_cnt=np.asarray(xyz_cnt, np.int32),
                        new_xyz=np.ascontiguousarray(new_xyz, F32).reshape(-1, 3), new_cnt=np.asarray(new_cnt, np.int32),
                        pairs=tuple(pairs), claims=claims))


def _frames(name, pcnt, qcnt, seed, shift=0.0, compact_groups=None):
    """clouds in a 3 m box (130 points: about 10 hits at r = 0.8, most of the frame at 1.6); queries on points, between points, and
    one in six far away (empty balls). compact_groups = g: the queries come in runs of g around one centre"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 3, (int(sum(pcnt)), 3)).astype(F32)
    new = []
    for b, nq in enumerate(qcnt):
        if compact_groups:
            c = rng.uniform(0.5, 2.5, (nq // compact_groups, 1, 3)) + rng.uniform(-0.3, 0.3, (nq // compact_groups, compact_groups, 3))
            c[1::3] += 40.0                                  # whole groups far away
            c = c.reshape(-1, 3)
        else:
            c = rng.uniform(0, 3, (nq, 3))
            c[::6] += 40.0
        new.append(c)
    new = np.concatenate(new).astype(F32) if new else np.zeros((0, 3), F32)
    return _case(name, xyz + F32(shift), pcnt, new + F32(shift), qcnt, GENERIC_PAIRS)


def _exact_radius():
    """query at the origin, dyadic coordinates: every product and sum is exact in f32. r = 1.25, r^2 = 1.5625"""
    one_in, one_out = np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2))
    on = [(0.75, 1, 0), (-0.75, 1, 0), (1, 0, 0.75), (0, -1, -0.75), (1.25, 0, 0), (0, 0, -1.25)]        # d2 == r2: excluded
    inside = [(0.75, one_in, 0), (0, -0.75, -one_in), (0.5, 0.5, 0.5), (1, 0.5, 0.5)]
    outside = [(0.75, one_out, 0), (1, 1, 0), (1.25, 2.0 ** -10, 0)]
    pts = np.array(on[:2] + inside[:1] + outside[:1] + on[2:] + inside[1:] + outside[1:], F32)
    return _case('exact_radius', pts, [len(pts)], np.zeros((1, 3), F32), [1],
                 ((1.25, 16, 1.25, 3), (0.5, 4, 1.25, 16), (1.25, 16, 0.5, 4)),
                 on_sphere=np.array(on, F32), inside=np.array(inside, F32), outside=np.array(outside, F32), radius=1.25)


def _sparse_hits(name, n, hit_at, pairs, seed, **claims):
    """one frame of n points: those at `hit_at` within 0.4 of both query centres (inside both radii, 0.5 and 1.0), all others 50 m away.
    Queries: the centre, a second centre 0.1 away, a far one"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(50, 60, (n, 3))
    v = rng.normal(size=(len(hit_at), 3))
    xyz[np.asarray(hit_at, np.int64)] = 5.0 + 0.19 * v / np.maximum(np.abs(v).max(1, keepdims=True), 1e-9)
    new = np.array([[5, 5, 5], [5.1, 5, 5], [-30, 0, 0]], F32)
    return _case(name, xyz, [n], new, [3], pairs, hit_at=np.asarray(hit_at, np.int64), **claims)


def _hit_count(ns, delta):
    hits = ns + delta
    n = max(200, 2 * hits + 10)
    rng = np.random.default_rng(1000 + 10 * ns + delta)
    at = np.sort(rng.choice(n, hits, replace=False))
    return _sparse_hits('hits_ns%d%+d' % (ns, delta), n, at, ((0.5, ns, 1.0, ns), (1.0, ns, 0.5, ns)), 7, hits=hits, nsample=ns)


def _nth_hit_at(pos):
    rng = np.random.default_rng(pos)
    at = np.concatenate([np.sort(rng.choice(pos, 15, replace=False)), [pos, pos + 1, pos + 2, pos + 66]])
    return _sparse_hits('hit16_at_%d' % pos, 200, at, ((0.5, 16, 1.0, 16), (1.0, 16, 0.5, 16), (0.5, 17, 0.5, 15)), 8, nth=(16, pos))


def _first_hit_at(pos):
    return _sparse_hits('first_hit_at_%d' % pos, 260, [pos, pos + 3, pos + 70], ((0.5, 16, 1.0, 4), (1.0, 16, 0.5, 4), (0.5, 1, 0.5, 2)),
                        9, first=pos)


def _cell_edges():
    """points and queries on multiples of the grid's cell edge 1.001 r_b (r_b = 0.8), on both sides of 0"""
    edge = grid_cell(0.8)[0]
    k = np.arange(-3, 4)
    lat = np.stack(np.meshgrid(k, k, k, indexing='ij'), -1).reshape(-1, 3)
    pts = (lat.astype(F32) * edge).astype(F32)
    rng = np.random.default_rng(12)
    pts = pts[rng.permutation(len(pts))]
    new = np.concatenate([pts[rng.choice(len(pts), 30, replace=False)],
                          pts[rng.choice(len(pts), 20, replace=False)] + F32(0.5) * edge])
    return _case('cell_edges', pts, [len(pts)], new, [len(new)], ((0.4, 16, 0.8, 32), (0.8, 8, 0.8, 64), (0.8, 7, 1.7, 64)), edge=edge)


COLLISION_BLOCK = (-12, -5, 6)        # first cell of the block: 43 of its 64 cells have two of their 27 neighbour cells in one bucket


def _collisions():
    """300 points and 200 queries in a block of 4 x 4 x 4 cells (r_b = 0.5) placed where bqg_bucket folds neighbours together: 1,024
    buckets, the 27 buckets of a query collide among themselves and the kernel's duplicate drop has work to do"""
    rng = np.random.default_rng(13)
    edge = float(grid_cell(0.5)[0])
    lo = np.array(COLLISION_BLOCK) * edge
    pts = lo + rng.uniform(0.01, 3.99, (300, 3)) * edge
    new = lo + rng.uniform(0.01, 3.99, (200, 3)) * edge
    return _case('collisions', pts, [170, 130], new, [90, 110], ((0.25, 16, 0.5, 32), (0.5, 64, 0.5, 5)), radius_b=0.5)


def _threshold(name, n_in, n_out):
    """one frame, r_b = 1: n_in points inside the ball of the query at the centre of cell (0, 0, 0), n_out outside it but inside the
    query's 27 cells; storage order shuffled. Query 1 is far away"""
    rng = np.random.default_rng(14)
    edge = float(grid_cell(1.0)[0])
    c = np.full(3, 0.5 * edge)

    def sample(n, keep):
        out = np.zeros((0, 3))
        while len(out) < n:
            p = rng.uniform(-0.95 * edge, 1.95 * edge, (4 * n + 64, 3))
            out = np.concatenate([out, p[keep(np.linalg.norm(p - c, axis=1))]])
        return out[:n]
    pts = np.concatenate([sample(n_in, lambda r: r < 0.9), sample(n_out, lambda r: r > 1.1)])
    pts = pts[rng.permutation(len(pts))]
    new = np.stack([c, c + 500.0])
    return _case(name, pts, [len(pts)], new, [2], ((0.6, 16, 1.0, 64), (0.6, 64, 1.0, 16), (1.0, 64, 1.0, 16)),
                 T=n_in + n_out, H=n_in, radius_b=1.0)


def _all_empty():
    return _case('all_frames_empty', np.zeros((0, 3), F32), [0, 0], np.array([[0, 0, 0], [1, 2, 3], [-1, -2, -3], [4, 4, 4], [0.5, 0, 0]], F32),
                 [2, 3], ((0.8, 16, 1.6, 32), (1.0, 1, 1.0, 64)))


@functools.lru_cache(maxsize=None)
def ball_cases():
    cases = [_frames('frames', POINT_CNT, QUERY_CNT, 1)]
    cases += [_frames('one_frame_M%d' % m, (130,), (m,), 20 + m) for m in M_TOTALS]
    cases += [_frames('frames_negative', POINT_CNT, QUERY_CNT, 1, shift=-100.3), _exact_radius()]
    cases += [_hit_count(ns, d) for ns in HIT_NSAMPLES for d in (-1, 0, 1)]
    cases += [_nth_hit_at(63), _nth_hit_at(64), _first_hit_at(64), _first_hit_at(129), _cell_edges(), _collisions()]
    cases += [_threshold('grid_T4096_H1024', 1024, 3072), _threshold('grid_T4096_H1025', 1025, 3071),
              _threshold('grid_T4097_H1024', 1024, 3073), _all_empty()]
    return tuple(cases)


def _round_up(cnt, g):
    return tuple(-(-c // g) * g for c in cnt)


def _packed_group(n):
    """one frame of n points within 0.5 of a group of 7 queries (R about 0.05, r_b = 0.6): every point is a candidate of the group"""
    rng = np.random.default_rng(n)
    v = rng.normal(size=(n, 3))
    pts = 2.0 + v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0, 0.5, (n, 1))
    new = 2.0 + rng.uniform(-0.03, 0.03, (7, 3))
    c = _case('group_candidates_%d' % n, pts, [n], new, [7], ((0.3, 16, 0.6, 32), (0.6, 65, 0.3, 16)), candidates=n)
    return dict(c, group=7)


@functools.lru_cache(maxsize=None)
def grouped_cases():
    """ball-query cases whose queries come in compact runs of `group` rows, none across a frame boundary"""
    cases = [dict(_frames('frames_group%d' % g, POINT_CNT, _round_up(QUERY_CNT, g), 30 + g, compact_groups=g), group=g) for g in GROUPS]
    co = _frames('coincident_group7', (65, 0, 130), (7, 7, 14), 40, compact_groups=7)
    new = co['new_xyz'].copy()
    new[:] = new[::7].repeat(7, axis=0)                                 # R = 0
    cases.append(dict(co, new_xyz=new, group=7))
    cases += [_packed_group(GQ_CAP), _packed_group(GQ_CAP + 1)]
    return tuple(_frozen(c) for c in cases)


# ------------------------------------------------------------------------------------------------------------------ FPS cases
def _fps_case(name, xyz, ms, **claims):
    return _frozen(dict(name=name, xyz=np.ascontiguousarray(xyz, F32), ms=tuple(ms), claims=claims))


@functools.lru_cache(maxsize=None)
def fps_cases():
    cases = []
    for n in FPS_SIZES:
        rng = np.random.default_rng(n)
        cases.append(_fps_case('n%d' % n, rng.normal(size=(3, n, 3)) * np.array([20, 20, 2]), sorted({1, min(n, 48)}), variant=fps_variant(n)))
    for n in FPS_TIE_SIZES:
        rng = np.random.default_rng(n + 1)
        base = rng.normal(size=(3, n // 8, 3)).astype(F32)
        xyz = np.stack([np.concatenate([base[b]] * 8)[rng.permutation(n)] for b in range(3)])
        cases.append(_fps_case('ties_n%d' % n, xyz, (64,), variant=fps_variant(n), copies=8))
    rng = np.random.default_rng(99)
    base = rng.normal(size=(3, 65, 3)).astype(F32)
    xyz = np.stack([np.concatenate([base[b]] * 2)[rng.permutation(130)] for b in range(3)])
    cases.append(_fps_case('all_tie_n130', xyz, (130,), variant=fps_variant(130), copies=2))
    for n in (1, 2, 3):                                               # identical points, m == n: every round a full tie
        cases.append(_fps_case('identical_n%d' % n, np.ones((3, n, 3), F32), (n,), variant=fps_variant(n), copies=n))
    return tuple(cases)


# ------------------------------------------------------------------------------------------------------------------ three-NN cases
def _nn_case(name, kcnt, ucnt, seed, dup=1):
    rng = np.random.default_rng(seed)
    known = []
    for k in kcnt:
        base = rng.uniform(-5, 5, (-(-k // dup), 3))
        known.append(np.concatenate([base] * dup)[rng.permutation(len(base) * dup)[:k]] if k else np.zeros((0, 3)))
    known = np.concatenate(known).astype(F32)
    unknown = rng.uniform(-5, 5, (int(sum(ucnt)), 3)).astype(F32)
    if dup > 1 and len(known):                                         # some unknown points sit on a known one: distance 0, dup times
        us = _starts(ucnt)
        ks = _starts(kcnt)
        for b in range(len(kcnt)):
            if kcnt[b] and ucnt[b]:
                unknown[us[b]:us[b] + ucnt[b]:3] = known[ks[b] + rng.integers(0, kcnt[b], len(range(0, ucnt[b], 3)))]
    return _frozen(dict(name=name, known=known, kcnt=np.asarray(kcnt, np.int32), unknown=unknown, ucnt=np.asarray(ucnt, np.int32), dup=dup))


NN_KNOWN, NN_UNKNOWN = (0, 1, 2, 3, 4, 300), (2, 0, 255, 256, 257, 5)


@functools.lru_cache(maxsize=None)
def three_nn_cases():
    cases = [_nn_case('ragged', NN_KNOWN, NN_UNKNOWN, 50),
             _nn_case('ragged_empty_known_last', NN_KNOWN[1:] + NN_KNOWN[:1], NN_UNKNOWN[1:] + NN_UNKNOWN[:1], 51),
             _nn_case('duplicates', (30, 9, 2), (257, 40, 5), 52, dup=3)]
    cases += [_nn_case('one_frame_N%d' % n, (50,), (n,), 60 + n) for n in (255, 256, 257)]
    return tuple(cases)


def nn_usable(case):
    """rows of `unknown` whose frame has at least 3 known points (their indices may be fed to interpolation)"""
    return np.repeat(np.asarray(case['kcnt']) >= 3, case['ucnt'])


# ------------------------------------------------------------------------------------------------------------------ interpolation / grouping
IDX_MODES = ('one_row', 'last_row', 'random')
INTERP_SHAPES = ((1, 255), (1, 256), (1, 257), (3, 85), (3, 86), (33, 7), (33, 8), (33, 300))          # (C, N): N * C around 256
GROUP_C, GROUP_NS = (1, 3, 33), (1, 16, 65)
GROUP_FEAT_CNT, GROUP_IDX_CNT = (5, 3, 70), (100, 0, 157)                                               # M = 257, a frame without queries
LDS_FIT, LDS_OVER = (128, 127), ((128, 128), (129, 127))                                                 # (nsample, C): nsample (C + 1) floats <= 64 KB


@functools.lru_cache(maxsize=None)
def interp_cases():
    cases = []
    for i, (C, N) in enumerate(INTERP_SHAPES):
        for mode in IDX_MODES:
            rng = np.random.default_rng(200 + i)
            M = (255, 256, 257)[i % 3]
            idx = {'one_row': np.full((N, 3), 11), 'last_row': np.full((N, 3), M - 1), 'random': rng.integers(0, M, (N, 3))}[mode]
            cases.append(_frozen(dict(name='C%d_N%d_M%d_%s' % (C, N, M, mode), feat=rng.normal(size=(M, C)).astype(F32),
                                      idx=idx.astype(np.int32), w=rng.uniform(0, 1, (N, 3)).astype(F32),
                                      grad_out=rng.normal(size=(N, C)).astype(F32), M=M)))
    return tuple(cases)


def _group_case(name, C, ns, mode, fcnt, icnt, seed):
    rng = np.random.default_rng(seed)
    cnt_of_row = np.repeat(np.asarray(fcnt), np.asarray(icnt))
    M = int(sum(icnt))
    idx = {'one_row': np.full((M, ns), 2), 'last_row': np.repeat(cnt_of_row[:, None] - 1, ns, 1),
           'random': rng.integers(0, 1 << 30, (M, ns)) % cnt_of_row[:, None]}[mode]
    return _frozen(dict(name=name, feat=rng.normal(size=(int(sum(fcnt)), C)).astype(F32), feat_cnt=np.asarray(fcnt, np.int32),
                        idx=np.ascontiguousarray(idx, np.int32), idx_cnt=np.asarray(icnt, np.int32),
                        grad_out=rng.normal(size=(M, C, ns)).astype(F32)))


@functools.lru_cache(maxsize=None)
def group_cases():
    cases = [_group_case('C%d_ns%d_%s' % (C, ns, mode), C, ns, mode, GROUP_FEAT_CNT, GROUP_IDX_CNT, 300 + C + ns)
             for C in GROUP_C for ns in GROUP_NS for mode in IDX_MODES]
    cases.append(_group_case('lds_limit_ns%d_C%d' % LDS_FIT, LDS_FIT[1], LDS_FIT[0], 'random', (9, 4), (2, 1), 400))
    return tuple(cases)


def group_lds_over_cases():
    return tuple(_group_case('lds_over_ns%d_C%d' % (ns, C), C, ns, 'random', (9, 4), (2, 1), 401) for ns, C in LDS_OVER)
