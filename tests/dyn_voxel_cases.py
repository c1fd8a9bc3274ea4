"""Seeded cases and the numpy definition of dynamic voxelization for tests/test_dyn_voxel_cpu.py, tests/test_dyn_voxel_gpu.py and
their golden generator (tests/golden/make_goldens_dyn_voxel.py). No reference import here: this module travels with the tests.

Grid: reduced and deliberately non-square, range [-5.12, -3.84, -2, 5.12, 3.84, 4]:
  pillar mode  voxel [0.32, 0.32, 6]   -> 32 x 24 x 1   (x and y masked, z not)
  voxel mode   voxel [0.32, 0.32, 0.5] -> 32 x 24 x 12  (x, y and z masked)
A swapped cx / cy in the key or in the coords shows on it.

  a      B = 3, C = 5, about 90 pillars: sizes include 1, 2, 63, 64, 65 and one pillar of 300 points; frame 1 holds no point at all;
         pillars at all four grid corners; the points are globally shuffled, so pillars and frames interleave in the input; N is no
         multiple of 256. It also holds points outside the range in x and in y (dropped), points on every cell face of both axes and
         exactly at the range minimum (kept) and maximum (dropped), points outside the range in z only (kept in pillar mode, dropped
         in voxel mode) and two points with a NaN coordinate (dropped in both modes).
  b      B = 1, C = 4, about 20 pillars
  c      a single pillar of 2 points
  empty  every point out of range

The definition: cells in numpy f32 arithmetic, (p - min) / voxel and floor, which is IEEE and therefore torch's and the kernel's; keys
in int64; voxels in ascending key order; the points of a voxel in input order; means summed in f64 and rounded to f32 once."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'ref_dyn_voxel.npz')

PCR = [-5.12, -3.84, -2.0, 5.12, 3.84, 4.0]
VOXEL = {'pillar': [0.32, 0.32, 6.0], 'voxel': [0.32, 0.32, 0.5]}
GRID = {'pillar': [32, 24, 1], 'voxel': [32, 24, 12]}                    # nx, ny, nz
MODES = ('pillar', 'voxel')

CASES = {
    'a': dict(B=3, C=5, pillars=90, seed=4100),
    'b': dict(B=1, C=4, pillars=20, seed=4200),
    'c': dict(B=1, C=4, pillars=1, seed=4300),
    'empty': dict(B=2, C=4, pillars=0, seed=4400),
}


def _cell_points(rng, b, cx, cy, n, C):
    """n points of frame b inside pillar (cx, cy), 2 % of a cell away from its faces; z anywhere inside the range"""
    u = rng.uniform(0.02, 0.98, (n, 2))
    pts = np.empty((n, 1 + C), np.float32)
    pts[:, 0] = b
    pts[:, 1] = PCR[0] + (cx + u[:, 0]) * 0.32
    pts[:, 2] = PCR[1] + (cy + u[:, 1]) * 0.32
    pts[:, 3] = rng.uniform(PCR[2] + 0.05, PCR[5] - 0.05, n)
    pts[:, 4:] = rng.uniform(0, 1, (n, C - 3))
    return pts


def _row(b, x, y, z, C, rng):
    r = np.empty((1, 1 + C), np.float32)
    r[0, :4] = [b, x, y, z]
    r[0, 4:] = rng.uniform(0, 1, C - 3)
    return r


_cache = {}


def make_case(name):
    """-> dict points (N, 1 + C) f32 [b, x, y, z, ...], B, C, name"""
    if name in _cache:
        return dict(_cache[name], points=_cache[name]['points'].copy())
    p = CASES[name]
    rng = np.random.default_rng(p['seed'])
    B, C = p['B'], p['C']
    nx, ny, _ = GRID['pillar']
    rows = []
    if name == 'a':
        frames = [0, 2]                                                  # frame 1 stays empty
        corners = [(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]
        cells = [c for c in rng.choice(nx * ny, p['pillars'], replace=False) if (c % nx, c // nx) not in corners][:p['pillars'] - 4]
        cells = [(c % nx, c // nx) for c in cells] + corners
        sizes = [1, 2, 63, 64, 65, 300] + list(rng.integers(1, 21, len(cells) - 6))
        for i, ((cx, cy), n) in enumerate(zip(cells, sizes)):
            rows.append(_cell_points(rng, frames[i % 2], cx, cy, int(n), C))
        z_in = 0.3
        for b in frames:
            rows += [_row(b, 5.62, 0.1, z_in, C, rng), _row(b, -5.22, 0.1, z_in, C, rng),          # outside in x
                     _row(b, 0.1, 3.94, z_in, C, rng), _row(b, 0.1, -4.5, z_in, C, rng),            # outside in y
                     _row(b, 0.1, 0.1, 4.5, C, rng), _row(b, 0.1, 0.1, -2.5, C, rng)]               # outside in z only
        # every cell face of both axes, the range minimum (kept) and the range maximum (dropped): whichever side of the face the f32
        # value falls on, every route must put it on the same one
        for k in range(nx + 1):
            rows.append(_row(0, np.float32(PCR[0] + k * 0.32), 0.5, z_in, C, rng))
        for k in range(ny + 1):
            rows.append(_row(2, 0.5, np.float32(PCR[1] + k * 0.32), z_in, C, rng))
        for k in range(13):
            rows.append(_row(2, 0.7, 0.7, np.float32(PCR[2] + k * 0.5), C, rng))
        rows += [_row(0, np.nan, 0.2, z_in, C, rng), _row(2, 0.2, 0.2, np.nan, C, rng)]
    elif name == 'b':
        cells = rng.choice(nx * ny, p['pillars'], replace=False)
        for c in cells:
            rows.append(_cell_points(rng, 0, c % nx, c // nx, int(rng.integers(1, 40)), C))
    elif name == 'c':
        rows.append(_cell_points(rng, 0, 7, 3, 2, C))
        rows[0][:, 3] = [0.1, 0.3]                                       # one z cell too: a single voxel in both modes
    else:
        for b in range(B):
            rows += [_row(b, 6.0 + i, 0.0, 0.0, C, rng) for i in range(5)] + [_row(b, 0.0, -9.0 - i, 0.0, C, rng) for i in range(4)]
    pts = np.concatenate(rows)
    if name == 'a' and len(pts) % 256 == 0:
        pts = np.concatenate([pts, _cell_points(rng, 0, 5, 5, 1, C)])
    pts = pts[rng.permutation(len(pts))]                                 # global shuffle: pillars and frames interleave
    _cache[name] = {'points': pts, 'B': B, 'C': C, 'name': name}
    return make_case(name)


def cells_f32(points, mode):
    """-> kept (N) bool, cells (N, 3) int64 [cx, cy, cz] (cz = 0 in pillar mode), in f32 arithmetic as torch and the kernel form them"""
    lo, vs, grid = np.asarray(PCR[:3], np.float32), np.asarray(VOXEL[mode], np.float32), GRID[mode]
    with np.errstate(invalid='ignore'):
        c = np.floor((points[:, 1:4] - lo) / vs)                         # f32 throughout
        axes = (0, 1) if mode == 'pillar' else (0, 1, 2)
        kept = ~np.isnan(points[:, 1:4]).any(1)                          # a NaN coordinate drops the point in both modes
        for a in axes:
            kept &= (c[:, a] >= 0) & (c[:, a] < grid[a])
    c = np.where(kept[:, None], c, 0).astype(np.int64)
    if mode == 'pillar':
        c[:, 2] = 0
    return kept, c


def definition(points, B, mode):
    """-> dict coords (M, 4) i32 [b, z, y, x], seg_offsets (M + 1), perm (Nk): input rows voxel by voxel in ascending key order,
    input order inside a voxel, mean (M, C) f32 = f64 means rounded once, mean64 (M, C)"""
    nx, ny, nz = GRID[mode]
    kept, c = cells_f32(points, mode)
    b = points[:, 0].astype(np.int64)
    kept &= (b >= 0) & (b < B)
    key = ((b * nx + c[:, 0]) * ny + c[:, 1]) * nz + c[:, 2]
    idx = np.nonzero(kept)[0]
    order = idx[np.argsort(key[idx], kind='stable')]
    ks = key[order]
    heads = np.nonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))[0] if len(ks) else np.zeros(0, np.int64)
    seg = np.concatenate([heads, [len(ks)]]).astype(np.int32)
    uk = ks[heads] if len(ks) else np.zeros(0, np.int64)
    coords = np.stack([uk // (nx * ny * nz), uk % nz, (uk // nz) % ny, (uk // (nz * ny)) % nx], 1).astype(np.int32).reshape(-1, 4)
    C = points.shape[1] - 1
    mean64 = np.zeros((len(uk), C))
    for v in range(len(uk)):
        mean64[v] = points[order[seg[v]:seg[v + 1]], 1:].astype(np.float64).sum(0) / (seg[v + 1] - seg[v])
    return {'coords': coords, 'seg_offsets': seg, 'perm': order.astype(np.int32), 'mean': mean64.astype(np.float32), 'mean64': mean64}


def ulp_distance(a, b):
    """largest distance in units of the last place between two f32 arrays of finite values"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return int(np.abs(ia - ib).max()) if a.size else 0
