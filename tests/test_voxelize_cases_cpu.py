"""CPU: the cases of tests/voxelize_cases.py are what tests/test_voxelize_edges_gpu.py relies on. Their numpy definition equals the C
oracle (oracle.voxelize_batch + oracle.mean_vfe) bit for bit on every case; every deliberately wrong variant of the definition differs
from it on a named case, so the GPU test would see a kernel with that error; and the cases hold what their descriptions promise."""
import os
import re
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxelize_cases as cases

RUN_IDS = ['%s-mv%d-k%d' % r for r in cases.RUNS]
# wrong variant -> the run that tells it from the definition
SEEN_BY = {
    'trunc': ('faces', 200, 3),                 # one ulp below the range minimum: (int) of -1e-6 is 0, the floor is -1
    'reciprocal': ('faces', 200, 3),            # face points where (p - min) * (1 / vs) rounds to the other side
    'f64': ('faces', 200, 3),                   # face points where the f64 quotient lies on the other side
    'upper_inclusive': ('faces', 200, 3),       # the range maximum: quotient == grid exactly
    'key_order': ('sizes', 1000, 5),
    'batch_cap': ('sizes', 20, 5),              # frame 0 has 30 voxels, the batch 60 = 3 * 20
    'cap_stops_joining': ('sizes', 20, 5),
    'last_k': ('sizes', 1000, 5),
    'swap_xy': ('sizes', 1000, 5),
}
EXACT = ('voxels', 'coords', 'num_points', 'counts')


def same(a, b):
    if a.dtype == np.float32:
        a, b = cases.bits(a), cases.bits(b)
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize('name,max_voxels,max_points', cases.RUNS, ids=RUN_IDS)
def test_definition_equals_the_oracle(name, max_voxels, max_points):
    c = cases.make_case(name)
    d = cases.defined(name, max_voxels, max_points)
    v, co, n, counts = oracle.voxelize_batch(c['points'], c['frame_offsets'], c['pcr'][:3], c['voxel'], c['grid'], max_voxels, max_points)
    assert d['counts'].tolist() == counts.tolist()
    assert d['coords'].dtype == np.int32 and same(d['coords'], co)
    assert d['num_points'].dtype == np.int32 and same(d['num_points'], n)
    assert same(d['voxels'], v)                                             # as int32: -0.0 and NaN payloads count
    assert same(d['mean'], oracle.mean_vfe(v, n))
    ok, ratio = cases.mean_within_bound(d['mean'], d, max_points)           # the f32 mean itself meets the bar set for the kernel
    assert ok, ratio


@pytest.mark.parametrize('variant', cases.WRONG)
def test_every_wrong_variant_is_seen(variant):
    assert set(SEEN_BY) == set(cases.WRONG)
    name, max_voxels, max_points = SEEN_BY[variant]
    assert (name, max_voxels, max_points) in cases.RUNS
    right, wrong = cases.defined(name, max_voxels, max_points), cases.defined(name, max_voxels, max_points, variant)
    assert not all(same(right[k], wrong[k]) for k in EXACT), variant


def test_faces_holds_what_it_promises():
    c = cases.make_case('faces')
    pts, off = c['points'], c['frame_offsets']
    assert c['B'] == 4 and off[0] == off[1] and off[3] == off[4] and off[1] < off[2] < off[3]
    lo, vs = c['pcr'][:3], c['voxel']
    kept, cell = cases.cells(pts, lo, vs, c['grid'])
    for variant in ('reciprocal', 'f64'):
        k2, c2 = cases.cells(pts, lo, vs, c['grid'], variant)
        for a in range(3):
            moved = (kept != k2) | (kept & k2 & (cell[:, a] != c2[:, a]))
            only = np.ones(len(pts), bool)                                  # rows that are ordinary on the other two axes
            for o in range(3):
                if o != a:
                    only &= np.isfinite(pts[:, o]) & (np.abs(pts[:, o]) < 100) & (cell[:, o] == c2[:, o])
            n = len({pts[i, a].tobytes() for i in np.nonzero(moved & only)[0]})
            assert n >= 3, (variant, a, n)
    for a in range(3):
        col = pts[:, a]
        at_min, at_max = col == np.float32(lo[a]), col == np.float32(c['pcr'][3 + a])
        assert kept[at_min].all() and at_min.any() and at_max.any() and not kept[at_max].any()
        below = col == np.nextafter(np.float32(lo[a]), np.float32(-np.inf))
        assert below.any() and not kept[below].any()
        with np.errstate(all='ignore'):
            q = (col - np.float32(lo[a])) / np.float32(vs[a])
        for want in (np.isposinf(col), np.isneginf(col), np.isnan(col), col == np.float32(3e38), col == np.float32(-3e38),
                     np.isfinite(q) & (q > 2.0 ** 31) & (q < 2.0 ** 31 * 1.01), np.isfinite(q) & (q < -2.0 ** 31) & (q > -2.0 ** 31 * 1.01)):
            assert want.any() and not kept[want].any(), a
        neg0 = (col == 0) & np.signbit(col)
        assert neg0.any() and kept[neg0].all()
    f = pts[:, 3]
    for want in (np.isnan(f) & ~np.signbit(f), np.isnan(f) & np.signbit(f), np.isposinf(f), np.isneginf(f), (f == 0) & np.signbit(f)):
        assert want.any() and kept[want].all()                              # special in a feature column only: kept
    d = cases.defined('faces', 200, 3)
    assert (d['counts'] < 200)[[1, 2]].all() and (d['counts'][[0, 3]] == 0).all()      # no cap: every face cell is compared
    special = np.asarray([0x7fc00000, 0xffc01234, 0x7f800000, 0xff800000, 0x80000000], np.uint32).view(np.int32)
    assert set(special.tolist()) <= set(cases.bits(d['voxels'][..., 3]).ravel().tolist())         # the bit patterns reach the voxels
    assert not np.isfinite(d['mean64']).all() and np.isfinite(d['mean64'][:, :3]).all()


def test_long_holds_what_it_promises():
    c = cases.make_case('long')
    n = len(c['points'])
    assert n == cases.LONG_N > 256 * cases.SCAN_TILE and -(-n // cases.SCAN_TILE) > 256 and n % cases.SCAN_TILE not in (0, cases.SCAN_TILE)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'crb-active-3ddet_amd', 'csrc', 'crb_common.h')).read()
    assert int(re.search(r'#define CRB_SCAN_ITEMS (\d+)', src).group(1)) * 256 == cases.SCAN_TILE
    (max_voxels, max_points), = c['runs']
    natural = cases.defined('long', n, max_points)['counts']                # uncapped: the distinct voxels of each frame
    assert natural.sum() >= 300000 and natural[0] > max_voxels > natural[1] > 0
    capped = cases.defined('long', max_voxels, max_points)
    assert capped['counts'].tolist() == [max_voxels, natural[1]]
    kept, _ = cases.cells(c['points'], c['pcr'][:3], c['voxel'], c['grid'])
    assert 0.02 * n < (~kept).sum() < 0.2 * n                               # some points outside
    assert (capped['num_points'] == max_points).any() and (capped['num_points'] == 1).any()


def test_frame_cases_hold_what_they_promise():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'crb-active-3ddet_amd', 'csrc', 'voxelize.hip')).read()
    fused = int(re.search(r'constexpr int VOX_MAX_FUSED_FRAMES = (\d+);', src).group(1))
    assert 'B <= VOX_MAX_FUSED_FRAMES' in src                               # frames256 the last fused size, frames257 the first beyond
    for name, B in (('frames256', fused), ('frames257', fused + 1)):
        c = cases.make_case(name)
        (max_voxels, max_points), = c['runs']
        assert c['B'] == B
        n = np.diff(c['frame_offsets'])
        assert (n[[0, 5, 6, B - 2, B - 1]] == 0).all() and (n[[1, 4, 7, B - 3]] > 0).all() and n.max() < 80
        natural = cases.defined(name, 10 ** 6, max_points)['counts']
        got = cases.defined(name, max_voxels, max_points)['counts']
        assert (got == np.minimum(natural, max_voxels)).all()
        assert (natural > max_voxels).sum() >= 20 and ((natural > 0) & (natural < max_voxels)).sum() >= 20
        assert (cases.defined(name, max_voxels, max_points)['num_points'] == max_points).any()


def test_sizes_and_the_small_cases_hold_what_they_promise():
    c = cases.make_case('sizes')
    assert c['B'] == 3 and c['C'] == 5 and len(c['points']) % 256 != 0
    natural = cases.defined('sizes', 1000, 64)
    _, _, pop = np.unique(_voxel_of_point(c), return_index=True, return_counts=True)
    for s in (1, 2, 63, 64, 65, 300):
        assert (pop == s).any(), s
    assert natural['counts'].tolist() == [30, 12, 18]
    for max_voxels, max_points in c['runs']:
        assert pop.max() > max_points
        assert ((natural['counts'] > max_voxels).sum() == 1) == (max_voxels == 20)
    assert {k for _, k in c['runs']} == {1, 5, 64}
    assert cases.make_case('feat3')['C'] == 3 and cases.make_case('feat7')['C'] == 7
    assert [len(cases.make_case('tiles_%d' % n)['points']) for n in cases.TILE_NS] == list(cases.TILE_NS)
    assert {cases.make_case('tiles_%d' % n)['B'] for n in cases.TILE_NS} == {1, 2}
    c = cases.make_case('n_below_cap')
    (max_voxels, _), = c['runs']
    assert c['B'] * max_voxels > len(c['points'])


def _voxel_of_point(c):
    kept, cell = cases.cells(c['points'], c['pcr'][:3], c['voxel'], c['grid'])
    b = np.searchsorted(c['frame_offsets'], np.arange(len(c['points'])), side='right') - 1
    key = ((b * 64 + cell[:, 2]) * 64 + cell[:, 1]) * 64 + cell[:, 0]
    return key[kept]
