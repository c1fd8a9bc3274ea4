"""GPU: the capped voxel generator (crb_voxelize) against the numpy definition of tests/voxelize_cases.py, which
tests/test_voxelize_cases_cpu.py pins to the C oracle and shows to tell nine wrong variants apart: cell faces and non-finite
coordinates, B = 256 / 257 frames, block and scan-tile edges, more than 256 scan tiles, the hash at load, empty frames, caps that
bind in some frames, max_points 1 .. 64, 3 / 5 / 7 features; the wrapper's variants; determinism; a workspace of exactly the bytes
the library carves and guarded output rows; the return codes of the paths that launch nothing.

counts, coords, num_points and voxels are compared exactly (f32 as int32, so -0.0 and NaN payloads count); the fused mean against
the f64 mean of the kept points with the bound of voxelize_cases.mean_within_bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxelize_cases as cases

pytestmark = pytest.mark.gpu

RUN_IDS = ['%s-mv%d-k%d' % r for r in cases.RUNS]
CRB_OK, CRB_ERR_ARG, CRB_ERR_WORKSPACE = 0, -1, -2
SLACK = 4096                                  # crb_voxelize_workspace_bytes = the carves + this
GUARD_ROWS = 8


def on_dev(c, dev):
    return torch.tensor(c['points'], device=dev), torch.tensor(c['frame_offsets'], device=dev)      # (the case arrays are read-only)


def run(c, max_voxels, max_points, dev, points=None, offsets=None, **kw):
    from crbhip import voxel
    p, o = on_dev(c, dev)
    kw.setdefault('want_voxels', True)
    kw.setdefault('want_mean', True)
    r = voxel.voxelize(p if points is None else points, o if offsets is None else offsets, c['pcr'], c['voxel'], max_voxels,
                       max_points, grid_xyz=c['grid'], **kw)
    torch.cuda.synchronize()
    return r


def host(r):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in r.items()}


def same(a, b):
    if a.dtype == np.float32:
        a, b = cases.bits(a), cases.bits(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a == b).all())


def assert_equals_definition(r, d, max_points, what=''):
    assert r['counts'] == d['counts'].tolist(), what
    assert same(r['coords'], d['coords']), what
    assert same(r['num_points'], d['num_points']), what
    if r.get('voxels') is not None:
        assert same(r['voxels'], d['voxels']), what
    if r.get('mean') is not None:
        assert r['mean'].shape == d['mean64'].shape and r['mean'].dtype == np.float32
        ok, ratio = cases.mean_within_bound(r['mean'], d, max_points)
        print('%s mean: worst error / bound %.3g, equal to the slot-by-slot f32 mean: %s' % (what, ratio, same(r['mean'], d['mean'])))
        assert ok, (what, ratio)


@pytest.mark.parametrize('name,max_voxels,max_points', cases.RUNS, ids=RUN_IDS)
def test_kernel_equals_the_definition(dev, name, max_voxels, max_points):
    """frames256 runs vox_assign<true> (B <= VOX_MAX_FUSED_FRAMES), frames257 vox_frame_bases + vox_assign<false>:
    test_voxelize_cases_cpu.py holds the two sizes to the constant in voxelize.hip"""
    c = cases.make_case(name)
    r = host(run(c, max_voxels, max_points, dev))
    assert_equals_definition(r, cases.defined(name, max_voxels, max_points), max_points, name)
    if name == 'n_below_cap':
        assert c['B'] * max_voxels > len(c['points']) >= len(r['coords'])


@pytest.mark.parametrize('name,max_voxels,max_points', [('sizes', 20, 5), ('faces', 200, 3), ('frames257', 20, 3)])
def test_wrapper_variants(dev, name, max_voxels, max_points):
    c = cases.make_case(name)
    d = cases.defined(name, max_voxels, max_points)
    full = host(run(c, max_voxels, max_points, dev))
    # each optional output off: the others unchanged
    nv = host(run(c, max_voxels, max_points, dev, want_voxels=False))
    nm = host(run(c, max_voxels, max_points, dev, want_mean=False))
    assert nv['voxels'] is None and nm['mean'] is None
    assert_equals_definition(nv, d, max_points, 'want_voxels=False')
    assert_equals_definition(nm, d, max_points, 'want_mean=False')
    assert same(nv['mean'], full['mean']) and same(nm['voxels'], full['voxels'])
    # lazy: capacity-sized tensors and the counts on the device
    lz = run(c, max_voxels, max_points, dev, lazy=True)
    cap = min(c['B'] * max_voxels, len(c['points']))
    assert lz['pending'] and lz['counts'] is None and lz['counts_dev'].dtype == torch.int32 and lz['counts_dev'].is_cuda
    assert [lz[k].shape[0] for k in ('voxels', 'coords', 'num_points', 'mean')] == [cap] * 4
    cd = lz['counts_dev'].cpu().numpy()
    M = int(cd[-1])
    assert cd[:-1].tolist() == full['counts'] and M == len(d['coords']) == cd[:-1].sum()
    for k in ('voxels', 'coords', 'num_points', 'mean'):
        assert same(lz[k][:M].cpu().numpy(), full[k]), k
    # columns 1.. of an (N, 1 + C) tensor (what a caller gets from batch_points[:, 1:]) and int64 offsets
    p, o = on_dev(c, dev)
    wide = torch.cat([torch.full((len(p), 1), 7.0, device=dev), p], 1)
    view = wide[:, 1:]
    assert not view.is_contiguous()
    sv = host(run(c, max_voxels, max_points, dev, points=view, offsets=o.to(torch.int64)))
    for k in ('voxels', 'coords', 'num_points', 'mean'):
        assert same(sv[k], full[k]), k
    assert sv['counts'] == full['counts']
    assert same(wide.cpu().numpy()[:, 1:], c['points']) and (wide[:, 0] == 7.0).all()           # the input is left alone


@pytest.mark.parametrize('name,max_voxels,max_points', [('sizes', 20, 5), ('long', 200000, 2)])
def test_two_calls_give_the_same_bytes(dev, name, max_voxels, max_points):
    c = cases.make_case(name)
    a, b = run(c, max_voxels, max_points, dev), run(c, max_voxels, max_points, dev)
    assert a['counts'] == b['counts']
    for k in ('voxels', 'coords', 'num_points', 'mean'):
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def call_abi(dev, points, n, C, offsets, B, c, max_voxels, max_points, outs, ws, ws_bytes):
    from crbhip._lib import lib, ptr, cur_stream, host_f32x3, host_i32x3
    rc = lib.crb_voxelize(ptr(points), n, C, ptr(offsets), B, host_f32x3(c['pcr'][:3]), host_f32x3(c['voxel']), host_i32x3(c['grid']),
                          max_voxels, max_points, ptr(outs.get('voxels')), ptr(outs.get('coords')), ptr(outs.get('num_points')),
                          ptr(outs.get('mean')), ptr(outs.get('counts')), ptr(ws), ws_bytes, cur_stream(dev))
    torch.cuda.synchronize()
    return rc


def tight_bytes(n, B, max_voxels, max_points):
    from crbhip._lib import lib
    return int(lib.crb_voxelize_workspace_bytes(n, B, max_voxels, max_points)) - SLACK


@pytest.mark.parametrize('name,max_voxels,max_points', [('sizes', 20, 5), ('sizes', 1000, 64), ('frames257', 20, 3)])
def test_stays_inside_a_tight_workspace_and_its_rows(dev, name, max_voxels, max_points):
    """the workspace is exactly the sum of the carves, cut from the middle of a larger tensor with 4096 pattern bytes either side; every
    output has 8 pattern rows behind row cap. Everything the call may write lies in tensors of this test."""
    c = cases.make_case(name)
    d = cases.defined(name, max_voxels, max_points)
    p, o = on_dev(c, dev)
    n, C, B = len(p), c['C'], c['B']
    cap = min(B * max_voxels, n)
    M = len(d['coords'])
    assert M <= cap
    nbytes = tight_bytes(n, B, max_voxels, max_points)
    pad = 4096
    arena = torch.full((pad + nbytes + pad,), 0xA5, dtype=torch.uint8, device=dev)
    assert arena.data_ptr() % 256 == 0
    ws = arena[pad:pad + nbytes]
    PAT_F, PAT_I = -12345.5, -0x5A5A5A5B

    def guarded(shape, dtype, pat):
        t = torch.full((cap + GUARD_ROWS,) + shape, pat, dtype=dtype, device=dev)
        return t

    outs = {'voxels': guarded((max_points, C), torch.float32, PAT_F), 'coords': guarded((4,), torch.int32, PAT_I),
            'num_points': guarded((), torch.int32, PAT_I), 'mean': guarded((C,), torch.float32, PAT_F),
            'counts': torch.full((B + 1 + GUARD_ROWS,), PAT_I, dtype=torch.int32, device=dev)}
    rc = call_abi(dev, p, n, C, o, B, c, max_voxels, max_points, outs, ws, nbytes)
    assert rc == CRB_OK
    assert (arena[:pad] == 0xA5).all() and (arena[pad + nbytes:] == 0xA5).all()
    counts = outs['counts'].cpu().numpy()
    assert (counts[B + 1:] == PAT_I).all() and counts[B] == M
    r = {'counts': counts[:B].tolist()}
    for k in ('voxels', 'coords', 'num_points', 'mean'):
        a = outs[k].cpu().numpy()
        assert (a[cap:] == (PAT_F if a.dtype == np.float32 else PAT_I)).all(), k               # the guard rows
        assert (a[M:cap] == (PAT_F if a.dtype == np.float32 else PAT_I)).all(), k              # rows beyond the total: untouched
        r[k] = a[:M]
    assert_equals_definition(r, d, max_points, name)


def test_return_codes_of_the_paths_that_launch_nothing(dev):
    c = cases.make_case('feat3')
    p, o = on_dev(c, dev)
    n, C, B = len(p), c['C'], c['B']
    max_voxels, max_points = 50, 4
    none = {}
    for what, kw in (('n_points = -1', dict(n=-1)), ('B = 0', dict(B=0)), ('num_features = 2', dict(C=2)),
                     ('max_voxels = 0', dict(max_voxels=0)), ('max_points = 0', dict(max_points=0)),
                     ('n_points = 0x7f7f7f7f', dict(n=0x7f7f7f7f))):
        a = dict(n=n, C=C, B=B, max_voxels=max_voxels, max_points=max_points)
        a.update(kw)
        rc = call_abi(dev, None, a['n'], a['C'], None, a['B'], c, a['max_voxels'], a['max_points'], none, None, 0)
        assert rc == CRB_ERR_ARG, what
    # one byte less than the carves: refused before anything is launched, the outputs keep their pattern
    cap = min(B * max_voxels, n)
    nbytes = tight_bytes(n, B, max_voxels, max_points)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    outs = {'voxels': torch.full((cap, max_points, C), -1.0, device=dev), 'coords': torch.full((cap, 4), -7, dtype=torch.int32, device=dev),
            'num_points': torch.full((cap,), -7, dtype=torch.int32, device=dev), 'mean': torch.full((cap, C), -1.0, device=dev),
            'counts': torch.full((B + 1,), -7, dtype=torch.int32, device=dev)}
    assert call_abi(dev, p, n, C, o, B, c, max_voxels, max_points, outs, ws, nbytes - 1) == CRB_ERR_WORKSPACE
    assert all(bool((t == (-1.0 if t.dtype == torch.float32 else -7)).all()) for t in outs.values())
    assert call_abi(dev, p, n, C, o, B, c, max_voxels, max_points, outs, ws, nbytes) == CRB_OK
    assert outs['counts'].cpu().tolist() == cases.defined('feat3', max_voxels, max_points)['counts'].tolist() + \
        [len(cases.defined('feat3', max_voxels, max_points)['coords'])]
    # no points: the per-frame counts and the total are zeroed, nothing else is needed
    counts = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
    assert call_abi(dev, None, 0, C, o, B, c, max_voxels, max_points, {'counts': counts}, None, 0) == CRB_OK
    assert counts.cpu().tolist() == [0] * (B + 1)
