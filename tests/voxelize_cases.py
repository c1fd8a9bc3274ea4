"""Seeded cases and the numpy definition of the capped voxel generator (crb_voxelize, csrc/voxelize.hip) for
tests/test_voxelize_cases_cpu.py and tests/test_voxelize_edges_gpu.py. No GPU and no crbhip import here.

Grid: reduced and non-cubic, range [-5.12, -3.84, -2, 5.12, 3.84, 3.4], voxel [0.32, 0.32, 0.45] -> 32 x 24 x 12. No voxel size is
exact in binary, so (p - min) / vs, (p - min) * (1 / vs) and the f64 quotient disagree on some cell faces of every axis; a swapped
cx / cy shows because nx != ny. (z = 0.45 and not 0.3: of the 13 z faces from -2 only one value changes cell under the reciprocal with
0.3, ten do with 0.45; a dyadic 0.5 tells nothing apart.) The `long` case uses the same voxel on 128 x 128 x 32.

The definition (the sequential semantics in the header of voxelize.hip, vectorised): per axis c = floor((p - min) / vs) in f32; a
point is dropped if that quotient is NaN or the floor lies outside [0, grid); a voxel is numbered the first time a point lands in it,
frame by frame, until max_voxels exist in the frame (later new voxels are dropped, points of existing voxels still join); a voxel
keeps its first max_points points in input order, zero padded. WRONG names deliberately wrong variants of it: the CPU test shows
that the cases tell every one of them from the right definition, so a kernel with that error cannot pass the GPU test.

  faces        B = 4, frames 0 and 3 empty. One point on every cell face of every axis, built as f32(min) + f32(k) * f32(vs) and as
               f32(min + k * vs), each also one ulp up and one ulp down: the range minimum (kept) and maximum (dropped) are among
               them. -0.0 coordinates; per axis +-inf, NaN, +-3e38 and a quotient just past +-2^31; NaN (two payloads), inf and -0.0
               in a feature column only (kept, copied bit for bit). Every face row stands twice in each live frame, shuffled.
  sizes        B = 3, C = 5, voxel populations 1, 2, 63, 64, 65, 300 and random small ones; shuffled inside the frames; N is no
               multiple of 256; 30 / 12 / 18 voxels per frame, so max_voxels = 20 binds in frame 0 only.
  frames256/7  B = 256 (the last size whose per-frame bases are formed inside vox_assign) and B = 257 (vox_frame_bases), 0 - 79
               points per frame, frames 0, 5, 6 and the last two empty, max_voxels = 20 binds in some frames only.
  feat3/feat7  C = 3 and C = 7.
  tiles_<n>    n in 1, 255, 256, 257, 2047, 2048, 2049, 4097: block (256) and scan tile (2048) edges, one or two frames.
  long         two frames, 256 * 2048 + 2048 + 77 points on 128 x 128 x 32, some outside: more than 256 scan tiles with a ragged last
               one (the carry loop of crb_scan_of_sums), more than 300 000 distinct voxels in the hash, a cap of 200 000 that binds
               in frame 0 only.
  n_below_cap  B * max_voxels > n: the outputs hold n rows."""
import numpy as np

PCR = [-5.12, -3.84, -2.0, 5.12, 3.84, 3.4]
VOXEL = [0.32, 0.32, 0.45]
GRID = [32, 24, 12]                                                       # nx, ny, nz
PCR_LONG = [-20.48, -20.48, -2.0, 20.48, 20.48, 12.4]
GRID_LONG = [128, 128, 32]
SCAN_TILE = 2048                                                         # CRB_SCAN_TILE of csrc/crb_common.h
LONG_N = 256 * SCAN_TILE + SCAN_TILE + 77
TILE_NS = (1, 255, 256, 257, 2047, 2048, 2049, 4097)

WRONG = ('trunc', 'reciprocal', 'f64', 'upper_inclusive', 'key_order', 'batch_cap', 'cap_stops_joining', 'last_k', 'swap_xy')


# ---------------------------------------------------------------------------------------------------------------- the definition
def cells(points, range_min, voxel_size, grid, variant=None):
    """-> kept (N) bool, c (N, 3) int64 [cx, cy, cz] (0 where dropped)"""
    if variant == 'f64':
        p, lo, vs = points[:, :3].astype(np.float64), np.asarray(range_min, np.float64), np.asarray(voxel_size, np.float64)
    else:
        p, lo, vs = points[:, :3].astype(np.float32), np.asarray(range_min, np.float32), np.asarray(voxel_size, np.float32)
    g = np.asarray(grid, np.float64)
    with np.errstate(all='ignore'):
        q = (p - lo) * (np.float32(1) / vs) if variant == 'reciprocal' else (p - lo) / vs
        f = np.trunc(q) if variant == 'trunc' else np.floor(q)
        kept = ~np.isnan(q) & (f >= 0) & ((f <= g) if variant == 'upper_inclusive' else (f < g))
    kept = kept.all(1)
    return kept, np.where(kept[:, None], f, 0).astype(np.int64)


def definition(points, frame_offsets, range_min, voxel_size, grid, max_voxels, max_points, variant=None):
    """-> dict voxels (M, K, C) f32, coords (M, 4) i32 [b, z, y, x], num_points (M) i32, counts (B) i32, mean (M, C) f32 summed slot
    by slot in f32 like MeanVFE, mean64 (M, C) the f64 mean of the kept points, abs_sum (M, C) f64 = sum |v_i| over them"""
    assert variant is None or variant in WRONG, variant
    points = np.ascontiguousarray(points, np.float32)
    off = np.asarray(frame_offsets, np.int64)
    N, C = points.shape
    B, K = len(off) - 1, int(max_points)
    gx, gy, gz = [int(v) + 1 for v in grid]                              # + 1: room for the cell `upper_inclusive` lets in
    kept, c = cells(points, range_min, voxel_size, grid, variant)
    idx = np.nonzero(kept)[0]
    b = np.searchsorted(off, idx, side='right') - 1                      # the last frame that starts at or before the point
    key = ((b * gz + c[idx, 2]) * gy + c[idx, 1]) * gx + c[idx, 0]
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    vorder = np.arange(len(uk)) if variant == 'key_order' else np.argsort(first, kind='stable')
    vframe = b[first[vorder]]                                            # ascending: frames are contiguous in the input
    starts = np.searchsorted(vframe, np.arange(B + 1))
    local = np.arange(len(uk)) - starts[vframe]
    vkeep = np.arange(len(uk)) < B * max_voxels if variant == 'batch_cap' else local < max_voxels
    counts = np.bincount(vframe[vkeep], minlength=B).astype(np.int32)
    rows_of_rank = np.where(vkeep, np.cumsum(vkeep) - 1, -1)
    row_of_voxel = np.empty(len(uk), np.int64)
    row_of_voxel[vorder] = rows_of_rank
    prow = row_of_voxel[inv]                                             # output row of every kept point, -1: its voxel was dropped
    if variant == 'cap_stops_joining':                                   # the first dropped voxel of a frame ends the frame
        stop = np.full(B, N, np.int64)
        over = np.nonzero(local == max_voxels)[0]
        stop[vframe[over]] = idx[first[vorder[over]]]
        prow = np.where(idx >= stop[b], -1, prow)
    M = int(vkeep.sum())
    sel = prow >= 0
    pi, pr = idx[sel], prow[sel]
    o = np.argsort(pr, kind='stable')                                    # voxel by voxel, input order inside
    pi, pr = pi[o], pr[o]
    cnt = np.bincount(pr, minlength=M)
    seg = np.concatenate([[0], np.cumsum(cnt)])
    pos = np.arange(len(pr)) - seg[pr]
    if variant == 'last_k':
        pos -= np.maximum(cnt[pr] - K, 0)
    take = (pos >= 0) & (pos < K)
    voxels = np.zeros((M, K, C), np.float32)
    voxels[pr[take], pos[take]] = points[pi[take]]
    num_points = np.minimum(cnt, K).astype(np.int32)
    v0 = vorder[vkeep]
    cc = c[idx[first[v0]]]
    coords = np.stack([vframe[vkeep], cc[:, 2], cc[:, 0] if variant == 'swap_xy' else cc[:, 1],
                       cc[:, 1] if variant == 'swap_xy' else cc[:, 0]], 1).astype(np.int32).reshape(-1, 4)
    k1 = np.maximum(num_points, 1)[:, None]
    with np.errstate(all='ignore'):
        s = np.zeros((M, C), np.float32)
        for t in range(K):
            s = s + voxels[:, t]                                         # f32, left to right over all K slots like MeanVFE's sum
        mean = s / k1.astype(np.float32)
        v64 = voxels.astype(np.float64)
        mean64, abs_sum = v64.sum(1) / k1, np.abs(v64).sum(1)
    return {'voxels': voxels, 'coords': coords, 'num_points': num_points, 'counts': counts, 'mean': mean, 'mean64': mean64,
            'abs_sum': abs_sum}


def bits(a):
    """f32 array as int32, so that -0.0 and NaN payloads count in a comparison"""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def mean_within_bound(mean, d, max_points):
    """the bar for the fused mean -> (ok, worst error / bound over the finite elements). Per element |mean - f64 mean| <=
    K * 2^-24 * sum|v_i| / k + 2^-150: at most K - 1 f32 additions and one correctly rounded division. The last term is the division's
    rounding error when the quotient is subnormal (half the spacing 2^-149 of the subnormals; the relative term does not cover it):
    `faces` holds the two f32 neighbours of 0.0, x = 0 being a cell face, and the correctly rounded mean of 1.4e-45, -1.4e-45, 1.4e-45
    is 0. Where the f64 mean is not finite the element must be non-finite as well"""
    fin = np.isfinite(d['mean64'])
    k = np.maximum(d['num_points'], 1)[:, None]
    bound = max_points * 2.0 ** -24 * d['abs_sum'] / k + 2.0 ** -150
    with np.errstate(all='ignore'):
        err = np.abs(mean.astype(np.float64) - d['mean64'])
        ok = bool((~np.isfinite(mean[~fin])).all() and (err[fin] <= bound[fin]).all())
        ratio = err[fin] / bound[fin]
    return ok, float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------------------------------- cases
def _inside(rng, n, C, lo_cell=(0, 0, 0), hi_cell=None, pcr=PCR):
    """n points uniform over the cells [lo_cell, hi_cell), 2 % of a cell away from the faces"""
    lo_cell = np.asarray(lo_cell)
    hi_cell = np.asarray(GRID if hi_cell is None else hi_cell)
    cell = rng.integers(lo_cell, hi_cell, (n, 3))
    p = np.empty((n, C), np.float32)
    p[:, :3] = np.asarray(pcr[:3]) + (cell + rng.uniform(0.02, 0.98, (n, 3))) * np.asarray(VOXEL)
    p[:, 3:] = rng.uniform(0, 1, (n, C - 3))
    return p


def _cell_points(rng, cell, n, C):
    return _inside(rng, n, C, cell, np.asarray(cell) + 1)


def face_values(axis):
    """every face of the axis, two constructions, each with both f32 neighbours -> f32 array"""
    lo, vs = PCR[axis], VOXEL[axis]
    out = []
    for k in range(GRID[axis] + 1):
        a = np.float32(lo) + np.float32(k) * np.float32(vs)              # f32 arithmetic
        b = np.float32(lo + k * vs)                                      # f64 arithmetic, rounded once
        for v in (a, b):
            out += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    return np.asarray(out, np.float32)


def _faces():
    rng = np.random.default_rng(5100)
    C = 4
    home = np.asarray([PCR[a] + (c + 0.37) * VOXEL[a] for a, c in enumerate((5, 3, 2))], np.float32)
    rows = []

    def row(axis, value):
        r = np.empty(C, np.float32)
        r[:3] = home
        r[axis] = value
        r[3] = rng.uniform(0, 1)
        rows.append(r)

    for a in range(3):
        for v in face_values(a):
            row(a, v)
    n_face = len(rows)
    for a in range(3):
        row(a, np.float32(-0.0))
        big = np.float32(2.0 ** 31 * 1.001 * VOXEL[a])
        for v in (np.inf, -np.inf, np.nan, 3e38, -3e38, np.float32(PCR[a]) + big, np.float32(PCR[a]) - big):
            row(a, np.float32(v))
    r = np.full(C, -0.0, np.float32)                                     # -0.0 on all three axes at once (a cell of its own)
    r[3] = 0.25
    rows.append(r)
    special = np.asarray([0x7fc00000, 0xffc01234, 0x7f800000, 0xff800000, 0x80000000], np.uint32).view(np.float32)
    for i, s in enumerate(special):                                      # feature-only specials: one per cell, next to a plain point
        two = _cell_points(rng, (20 + i, 15, 7), 2, C)
        two[0, 3] = s
        rows += [two[0], two[1]]
    rows = np.stack(rows)
    frames = []
    for b in (1, 2):
        again = rows[:n_face].copy()                                     # the face rows a second time, another feature value
        again[:, 3] = rng.uniform(0, 1, n_face)
        f = np.concatenate([rows, again])
        frames.append(f[rng.permutation(len(f))])
    n1, n2 = len(frames[0]), len(frames[1])
    return dict(points=np.concatenate(frames), frame_offsets=[0, 0, n1, n1 + n2, n1 + n2])


def _sizes():
    rng = np.random.default_rng(5200)
    C, per_frame = 5, (30, 12, 18)
    sizes = [1, 2, 63, 64, 65, 300] + [int(v) for v in rng.integers(1, 21, sum(per_frame) - 6)]
    frame_of_voxel = rng.permutation(np.repeat(np.arange(3), per_frame))
    cells_lin = rng.choice(GRID[0] * GRID[1] * GRID[2], len(sizes), replace=False)
    frames = [[], [], []]
    for lin, n, b in zip(cells_lin, sizes, frame_of_voxel):
        cell = (lin % GRID[0], (lin // GRID[0]) % GRID[1], lin // (GRID[0] * GRID[1]))
        frames[b].append(_cell_points(rng, cell, n, C))
    for b in range(3):                                                   # a few points outside the range in every frame
        out = _inside(rng, 4, C)
        out[:, b] += np.float32(20.0)
        frames[b].append(out)
    frames = [np.concatenate(f) for f in frames]
    if sum(len(f) for f in frames) % 256 == 0:
        frames[1] = frames[1][:-1]
    frames = [f[rng.permutation(len(f))] for f in frames]
    off = np.concatenate([[0], np.cumsum([len(f) for f in frames])])
    return dict(points=np.concatenate(frames), frame_offsets=off)


def _many_frames(B, seed):
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 80, B)
    n[[0, 5, 6, B - 2, B - 1]] = 0
    frames = []
    for b in range(B):
        lo = rng.integers(0, [GRID[0] - 8, GRID[1] - 6, GRID[2] - 2])
        f = _inside(rng, int(n[b]), 4, lo, lo + [8, 6, 2])              # 96 cells: several points share a voxel
        f[rng.uniform(size=len(f)) < 0.05, 1] = 9.0                      # some outside in y
        frames.append(f)
    return dict(points=np.concatenate(frames), frame_offsets=np.concatenate([[0], np.cumsum(n)]))


def _feat(C, seed):
    rng = np.random.default_rng(seed)
    f = [_inside(rng, n, C, (3, 2, 1), (9, 8, 4)) for n in (120, 90)]
    return dict(points=np.concatenate(f), frame_offsets=[0, 120, 210])


def _tiles(n):
    rng = np.random.default_rng(5400 + n)
    p = _inside(rng, n, 4)
    p[rng.uniform(size=n) < 0.03, 0] = -7.0
    off = [0, n] if n % 2 == 0 or n == 1 else [0, n // 3, n]
    return dict(points=p, frame_offsets=off)


def _long():
    rng = np.random.default_rng(5500)
    n0 = 300000
    lo, hi = np.asarray(PCR_LONG[:3]), np.asarray(PCR_LONG[3:])
    p = np.empty((LONG_N, 4), np.float32)
    p[:, :3] = rng.uniform(lo - 0.01 * (hi - lo), hi + 0.01 * (hi - lo), (LONG_N, 3))      # about 6 % outside
    p[:, 3] = rng.uniform(0, 1, LONG_N)
    return dict(points=p, frame_offsets=[0, n0, LONG_N], pcr=PCR_LONG, grid=GRID_LONG)


def _n_below_cap():
    rng = np.random.default_rng(5600)
    return dict(points=_inside(rng, 50, 4), frame_offsets=[0, 20, 50])


_BUILD = {'faces': _faces, 'sizes': _sizes, 'frames256': lambda: _many_frames(256, 5300), 'frames257': lambda: _many_frames(257, 5301),
          'feat3': lambda: _feat(3, 5310), 'feat7': lambda: _feat(7, 5311), 'long': _long, 'n_below_cap': _n_below_cap}
_BUILD.update({'tiles_%d' % n: (lambda n=n: _tiles(n)) for n in TILE_NS})
CASES = tuple(_BUILD)
_cache = {}


def make_case(name):
    """-> dict name, points (N, C) f32, frame_offsets (B + 1) i32, B, C, pcr, voxel, grid, runs [(max_voxels, max_points)].
    The arrays are shared and read-only"""
    if name not in _cache:
        c = _BUILD[name]()
        c['points'] = np.ascontiguousarray(c['points'], np.float32)
        c['frame_offsets'] = np.asarray(c['frame_offsets'], np.int32)
        c['points'].setflags(write=False)
        c['frame_offsets'].setflags(write=False)
        c.setdefault('pcr', PCR)
        c.setdefault('grid', GRID)
        c.update(name=name, voxel=VOXEL, runs=_RUNS[name], B=len(c['frame_offsets']) - 1, C=c['points'].shape[1])
        assert c['frame_offsets'][-1] == len(c['points'])
        _cache[name] = c
    return _cache[name]


_RUNS = {'faces': [(200, 3)], 'sizes': [(1000, 1), (1000, 5), (1000, 64), (20, 5)], 'frames256': [(20, 3)], 'frames257': [(20, 3)],
         'feat3': [(50, 4)], 'feat7': [(50, 4)], 'long': [(200000, 2)], 'n_below_cap': [(100, 3)]}
_RUNS.update({'tiles_%d' % n: [(1500, 3)] for n in TILE_NS})
RUNS = [(name, mv, K) for name in CASES for mv, K in _RUNS[name]]          # every (case, max_voxels, max_points) the tests use
_defs = {}


def defined(name, max_voxels, max_points, variant=None):
    """the definition on a case, computed once per process and shared (read-only)"""
    k = (name, max_voxels, max_points, variant)
    if k not in _defs:
        c = make_case(name)
        d = definition(c['points'], c['frame_offsets'], c['pcr'][:3], c['voxel'], c['grid'], max_voxels, max_points, variant)
        for a in d.values():
            a.setflags(write=False)
        _defs[k] = d
    return _defs[k]
