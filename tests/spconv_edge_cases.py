"""Hand-built neighbour tables and coordinate sets for the sparse convolution stack (csrc/sparse_conv.hip, csrc/rulebook.hip,
csrc/rulebook_plan.hip, crbhip/sparse.py) at the places where tiled kernels go wrong: row counts around the 16- and 64-row tiles,
the 128-row tile-order threshold and the 4,096-row sort chunk; pair counts per offset around every pair-block size of the weight
gradient; rows and offsets without pairs; sites on the borders of the grid and of a frame. numpy only, fixed seeds, no GPU.

Hand-built tables (dict): nbr (n_out, K) int32 = input row feeding output row i through offset o or -1, nbr_t (n_in, K) its exact
transpose, n_in, n_out, K = 27. Every column of nbr is injective (an input row at most once per offset), every index is in range,
n_in >= 1. The kernels see a table through sparse.Rulebook(nbr, nbr_t, n_in, n_out, ...).

  master     n_out 4,097, n_in 3,000. Entry (i, o) is present with a probability that depends on the column: PROB[o], 0.02 .. 0.9
             in an order that is not monotone in o. A column can hold at most n_in - (unreferenced rows) = 2,850 entries, so rows
             3,000 .. 4,089 use min(PROB[o], 0.2); the last 7 rows (the end of chunk 0 and the one-row chunk 1) use PROB[o]
             again. 205 rows are entirely empty by construction (a few more by chance), 150 input rows (row 0 among them: the
             row the kernels' clamped loads read) are never referenced. Row 0 and the last 3 rows are not empty.
  prefix(n)  the first n rows of master over the same 3,000 input rows
  window(n)  prefix(n) under the name the windowed weight-gradient tests use (its pair lists come from crb_tables_finish, ascending
             in output row inside an offset, as wgrad_window_bounds_kernel needs)
  ladder     n_in = n_out = 600, column o holds exactly LADDER[o] pairs on random rows (a full column is a permutation)

Geometry cases (dict): coords (n, 4) int32 [b, z, y, x] in random row order, shape [D, H, W], batch_size.

  borders(shape)    all 8 corners, sites on the 12 edges and 6 faces, interior sites, and the wrap traps (`traps`: a, b = two sites,
                    key_diff = linear key of b minus that of a, offset = the (dz, dy, dx) a wrapping linear index would give the
                    pair, or None for the same voxel in two frames)
  isolated          200 sites on the even lattice: Chebyshev distance >= 2 between any two, only the centre offset has pairs
  solid(extra)      a full 4 x 4 x 4 block (one 64-row tile; 8 sites have 27 neighbours), extra = 1 adds one far site (65 rows)
  line              130 consecutive sites along x in one (z, y) line
  uncovered         clustered cloud in a grid of depth 6 with 12 sites at z = 5, which no window of UNCOVERED_GEOMS reaches
  empty_frame       shape [41, 16, 16], 3 frames, sites in frames 0 and 2 only
"""
import functools

import numpy as np

K = 27
ROWS_SMALL = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193)
ROWS_CHUNK = (4095, 4096, 4097)
ROWS_WINDOW = (1, 31, 32, 33, 65)
N_OUT, N_IN = 4097, 3000
N_EMPTY, N_UNREF = 205, 150
LADDER = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 255, 256, 257, 600, 2, 3, 5, 7, 600, 1, 0, 0)
LADDER_N = 600
BORDER_SHAPES = ([5, 9, 7], [4, 8, 8])
BORDER_GEOM = ((3, 3, 3), (2, 2, 2), (1, 1, 1))
UNCOVERED_GEOMS = (((3, 1, 1), (2, 1, 1), (0, 0, 0)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)))
CHAIN_GEOMS = (((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)), ((3, 3, 3), (2, 2, 2), (0, 1, 1)),
               ((3, 1, 1), (2, 1, 1), (0, 0, 0)))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def transpose(nbr, n_in):
    """(n_in, K) table with nbr_t[nbr[i, o], o] = i"""
    nbr_t = np.full((n_in, nbr.shape[1]), -1, np.int32)
    i, o = np.nonzero(nbr >= 0)
    nbr_t[nbr[i, o], o] = i
    return nbr_t


def _table(nbr, n_in):
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    return _frozen(dict(nbr=nbr, nbr_t=transpose(nbr, n_in), n_in=int(n_in), n_out=int(nbr.shape[0]), K=int(nbr.shape[1])))


@functools.lru_cache(maxsize=None)
def column_prob():
    """PROB[o]: 27 values from 0.02 to 0.9, geometric, in a fixed shuffled order"""
    p = np.geomspace(0.02, 0.9, K)
    return p[np.random.default_rng(7).permutation(K)]


@functools.lru_cache(maxsize=None)
def master():
    rng = np.random.default_rng(20240)
    prob = column_prob()
    empty = 1 + rng.choice(N_OUT - 4, N_EMPTY, replace=False)            # rows 1 .. N_OUT - 4
    unref = np.concatenate([[0], 1 + rng.choice(N_IN - 1, N_UNREF - 1, replace=False)])
    usable = np.setdiff1d(np.arange(N_IN), unref)
    cap = np.ones(N_OUT)
    cap[3000:N_OUT - 7] = 0.2
    nbr = np.full((N_OUT, K), -1, np.int32)
    for o in range(K):
        has = rng.random(N_OUT) < np.minimum(prob[o], cap)
        has[empty] = False
        rows = np.flatnonzero(has)
        assert len(rows) <= len(usable)
        nbr[rows, o] = rng.choice(usable, len(rows), replace=False)
    for r in (0, N_OUT - 3, N_OUT - 2, N_OUT - 1):                       # never empty: a prefix always has a pair, both chunks too
        if (nbr[r] < 0).all():
            o = int(np.argmax(prob))
            free = np.setdiff1d(usable, nbr[:, o])
            nbr[r, o] = free[0]
    return _table(nbr, N_IN)


@functools.lru_cache(maxsize=None)
def prefix(n):
    assert 1 <= n <= N_OUT
    return _table(master()['nbr'][:n], N_IN)


def window(n):
    return prefix(n)


@functools.lru_cache(maxsize=None)
def ladder():
    rng = np.random.default_rng(20241)
    nbr = np.full((LADDER_N, K), -1, np.int32)
    for o, c in enumerate(LADDER):
        rows = np.sort(rng.choice(LADDER_N, c, replace=False))
        nbr[rows, o] = rng.choice(LADDER_N, c, replace=False)
    return _table(nbr, LADDER_N)


def table(name):
    """'master' | 'ladder' | 'prefix<n>' | 'window<n>'"""
    if name == 'master':
        return master()
    if name == 'ladder':
        return ladder()
    for kind in ('prefix', 'window'):
        if name.startswith(kind):
            return prefix(int(name[len(kind):]))
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------- geometry
def lin_key(site, shape):
    b, z, y, x = [int(v) for v in site]
    return ((b * shape[0] + z) * shape[1] + y) * shape[2] + x


def offset_index(dz, dy, dx):
    """column of a 3 x 3 x 3 table that holds the neighbour at (z + dz, y + dy, x + dx)"""
    return ((dz + 1) * 3 + (dy + 1)) * 3 + (dx + 1)


def _coords(sites, rng, shape, batch_size, **extra):
    c = np.array(sorted(set(tuple(int(v) for v in s) for s in sites)), np.int32).reshape(-1, 4)
    c = np.ascontiguousarray(c[rng.permutation(len(c))])
    assert (c >= 0).all() and (c[:, 0] < batch_size).all() and (c[:, 1:] < np.array(shape)).all()
    return _frozen(dict(coords=c, shape=[int(v) for v in shape], batch_size=int(batch_size), **extra))


def row_of(case, site):
    hit = np.flatnonzero((case['coords'] == np.array(site, np.int32)).all(1))
    assert len(hit) == 1, site
    return int(hit[0])


@functools.lru_cache(maxsize=None)
def borders(which):
    D, H, W = shape = BORDER_SHAPES[which]
    rng = np.random.default_rng(300 + which)
    B = 3
    sites = []
    ext = ((0, D - 1), (0, H - 1), (0, W - 1))
    for b in (0, 1):                                                      # corners
        sites += [(b, z, y, x) for z in ext[0] for y in ext[1] for x in ext[2]]
    for axis in range(3):                                                 # edges: the two other axes at an extreme
        others = [a for a in range(3) if a != axis]
        for e0 in ext[others[0]]:
            for e1 in ext[others[1]]:
                for t in rng.choice(np.arange(1, shape[axis] - 1), 2, replace=False):
                    s = [0, 0, 0]
                    s[axis], s[others[0]], s[others[1]] = int(t), e0, e1
                    sites.append((int(rng.integers(B)),) + tuple(s))
    for axis in range(3):                                                 # faces: one axis at an extreme
        others = [a for a in range(3) if a != axis]
        for e in ext[axis]:
            for _ in range(3):
                s = [0, 0, 0]
                s[axis] = e
                for a in others:
                    s[a] = int(rng.integers(1, shape[a] - 1))
                sites.append((int(rng.integers(B)),) + tuple(s))
    for _ in range(40):                                                   # interior
        sites.append((int(rng.integers(B)),) + tuple(int(rng.integers(1, shape[a] - 1)) for a in range(3)))
    traps = []

    def trap(a, b, offset):
        sites.extend([a, b])
        traps.append(dict(a=a, b=b, key_diff=lin_key(b, shape) - lin_key(a, shape), offset=offset))
    trap((0, 2, 3, W - 1), (0, 2, 4, 0), (0, 0, 1))                       # end of an x line / start of the next
    trap((2, 1, 5, W - 1), (2, 1, 6, 0), (0, 0, 1))
    trap((1, 1, H - 1, 3), (1, 2, 0, 3), (0, 1, 0))                       # last line of a slice / first line of the next
    trap((0, 0, H - 1, 2), (0, 1, 0, 2), (0, 1, 0))
    trap((0, D - 1, H - 1, W - 1), (1, 0, 0, 0), (0, 0, 1))               # last voxel of a frame / first voxel of the next
    trap((1, D - 1, H - 1, W - 1), (2, 0, 0, 0), (0, 0, 1))
    trap((0, 2, 4, 3), (2, 2, 4, 3), None)                                # one voxel in two frames
    return _coords(sites, rng, shape, B, traps=tuple(traps))


@functools.lru_cache(maxsize=None)
def isolated():
    rng = np.random.default_rng(310)
    shape, B = [12, 20, 20], 2
    lattice = np.stack(np.meshgrid(np.arange(0, 12, 2), np.arange(0, 20, 2), np.arange(0, 20, 2), indexing='ij'), -1).reshape(-1, 3)
    sites = []
    for b in range(B):
        sites += [(b,) + tuple(s) for s in lattice[rng.choice(len(lattice), 100, replace=False)]]
    return _coords(sites, rng, shape, B)


@functools.lru_cache(maxsize=None)
def solid(extra=0):
    rng = np.random.default_rng(320 + extra)
    shape = [8, 10, 9]
    sites = [(0, 2 + z, 3 + y, 1 + x) for z in range(4) for y in range(4) for x in range(4)]
    if extra:
        sites.append((0, 7, 0, 8))
    return _coords(sites, rng, shape, 1)


@functools.lru_cache(maxsize=None)
def line():
    rng = np.random.default_rng(330)
    return _coords([(0, 1, 2, 5 + x) for x in range(130)], rng, [3, 5, 140], 1)


@functools.lru_cache(maxsize=None)
def uncovered():
    rng = np.random.default_rng(340)
    shape, B = [6, 16, 16], 2
    sites = []
    for _ in range(14):                                                   # clusters
        b, c = int(rng.integers(B)), rng.uniform([0, 0, 0], shape)
        p = np.rint(c + rng.normal(size=(40, 3)) * [1.0, 1.8, 1.8]).astype(int)
        p = p[((p >= 0) & (p < np.array(shape))).all(1)]
        sites += [(b,) + tuple(s) for s in p]
    last = rng.choice(16 * 16, 12, replace=False)
    sites += [(int(k % B), 5, int(v // 16), int(v % 16)) for k, v in enumerate(last)]
    return _coords(sites, rng, shape, B)


@functools.lru_cache(maxsize=None)
def empty_frame():
    rng = np.random.default_rng(350)
    shape, B = [41, 16, 16], 3
    sites = []
    for b in (0, 2):
        for _ in range(8):
            c = rng.uniform([0, 0, 0], shape)
            p = np.rint(c + rng.normal(size=(40, 3)) * [3.0, 1.5, 1.5]).astype(int)
            p = p[((p >= 0) & (p < np.array(shape))).all(1)]
            sites += [(b,) + tuple(s) for s in p]
    return _coords(sites, rng, shape, B)


GEOMETRY = {'borders0': lambda: borders(0), 'borders1': lambda: borders(1), 'isolated': isolated, 'solid64': lambda: solid(0),
            'solid65': lambda: solid(1), 'line': line, 'uncovered': uncovered, 'empty_frame': empty_frame}


def geometry(name):
    return GEOMETRY[name]()


# ---------------------------------------------------------------------------------------------------------------- values
def feats(seed, n, c):
    """(n, c) f32 rows from rng.normal"""
    return np.random.default_rng([int(seed), int(n), int(c)]).normal(size=(n, c)).astype(np.float32)


def weights(seed, k, cin, cout):
    """(k, cin, cout) f32 from rng.normal / sqrt(cin)"""
    return (np.random.default_rng([int(seed), k, cin, cout]).normal(size=(k, cin, cout)) / np.sqrt(cin)).astype(np.float32)


def unreferenced(nbr, n_rows):
    """rows 0 .. n_rows - 1 that no entry of `nbr` names"""
    used = np.zeros(n_rows, bool)
    used[nbr[nbr >= 0]] = True
    return np.flatnonzero(~used)


def poison(a, nbr):
    """copy of `a` (n_rows, c) with NaN in every row that the table `nbr` does not reference"""
    out = np.array(a, dtype=np.float32, copy=True)
    out[unreferenced(nbr, len(out))] = np.nan
    return out
