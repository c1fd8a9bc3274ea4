"""GPU: every case of tests/pointnet2_edge_cases.py through the public wrappers of pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils
against the independent numpy references. Ball-query indices and empty flags, sampling picks, three-NN indices, gathered and
interpolated values: exact. Gradients summed with float atomics: |got - f64| <= (count + 1) 2^-24 sum |addend| per element, the
worst-case rounding of a sum in any order. Which kernel a case reaches is stated (and checked without a GPU) in
tests/test_pointnet2_edges_cpu.py."""
import functools

import numpy as np
import pytest
import torch

import pointnet2_edge_cases as E

pytestmark = pytest.mark.gpu

BALL = {c['name']: c for c in E.ball_cases() + E.grouped_cases()}
FPS = {c['name']: c for c in E.fps_cases()}
NN = {c['name']: c for c in E.three_nn_cases()}
INTERP = {c['name']: c for c in E.interp_cases()}
GROUP = {c['name']: c for c in E.group_cases()}


def _t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)            # (a copy: the cases are read-only arrays)


@functools.lru_cache(maxsize=None)
def _ref(name, r, ns):
    c = BALL[name]
    idx, empty = E.ref_ball_query(r, ns, c['xyz'], c['xyz_cnt'], c['new_xyz'], c['new_cnt'])
    idx.setflags(write=False)
    empty.setflags(write=False)
    return idx, empty


def _ball_inputs(c, dev):
    return _t(c['xyz'], dev), _t(c['xyz_cnt'], dev), _t(c['new_xyz'], dev), _t(c['new_cnt'], dev)


def _same(got, name, r, ns):
    idx, empty = got
    ridx, rempty = _ref(name, r, ns)
    np.testing.assert_array_equal(empty.cpu().numpy().astype(bool), rempty, err_msg='%s r=%g ns=%d empty flags' % (name, r, ns))
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx, err_msg='%s r=%g ns=%d' % (name, r, ns))


# ------------------------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize('name', list(BALL))
def test_ball_query(dev, name):
    """ball_query_kernel: one radius, one query per wave"""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = BALL[name]
    args = _ball_inputs(c, dev)
    for r, ns in sorted({(r, n) for ra, na, rb, nb in c['pairs'] for r, n in ((ra, na), (rb, nb))}):
        _same(U.ball_query(r, ns, *args), name, r, ns)


@pytest.mark.parametrize('name', list(BALL))
def test_ball_query_pair(dev, name):
    """ra <= rb: ball_query2_multi_kernel<8> (4 x 8 queries per workgroup); ra > rb: ball_query2_kernel"""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = BALL[name]
    args = _ball_inputs(c, dev)
    for ra, na, rb, nb in c['pairs']:
        a, b = U.ball_query_pair(ra, na, rb, nb, *args)
        _same(a, name, ra, na)
        _same(b, name, rb, nb)


@pytest.mark.parametrize('name', list(BALL))
def test_ball_query_grouped(dev, monkeypatch, name):
    """ball_query2_grouped_kernel: the case's own group size (1 for the cases that name none)"""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = BALL[name]
    args = _ball_inputs(c, dev)
    calls = []
    real = U.lib.crb_ball_query2_grouped_stack
    monkeypatch.setattr(U.lib, 'crb_ball_query2_grouped_stack', lambda *a: calls.append(1) or real(*a))
    for ra, na, rb, nb in c['pairs']:
        a, b = U.ball_query_pair(ra, na, rb, nb, *args, group=c.get('group', 1))
        _same(a, name, ra, na)
        _same(b, name, rb, nb)
    assert len(calls) == len(c['pairs'])


@pytest.mark.parametrize('name', list(BALL))
def test_ball_query_grid(dev, monkeypatch, name):
    """ball_query2_grid_kernel through the wrapper with the grid switched on for every size; a pair the grid does not take
    (nsample above 64, ra > rb) must still be answered, by the scan kernels"""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    monkeypatch.setattr(U, 'BALL_QUERY_GRID', True)
    monkeypatch.setattr(U, 'BALL_QUERY_GRID_MIN_POINTS', 0)
    c = BALL[name]
    args = _ball_inputs(c, dev)
    calls = []
    real = U.lib.crb_ball_query2_grid_stack
    monkeypatch.setattr(U.lib, 'crb_ball_query2_grid_stack', lambda *a: calls.append(1) or real(*a))
    for ra, na, rb, nb in c['pairs']:
        del calls[:]
        a, b = U.ball_query_pair(ra, na, rb, nb, *args)
        assert len(calls) == int(ra <= rb and max(na, nb) <= 64), (ra, na, rb, nb)
        _same(a, name, ra, na)
        _same(b, name, rb, nb)


@pytest.mark.parametrize('n_total', [0, 1, 300, 4097])
def test_grid_call_stays_inside_the_workspace_it_asked_for(dev, n_total):
    """crb_ball_query2_grid_stack with exactly crb_ball_query2_grid_workspace_bytes(n_total) bytes, followed by 64 KB of sentinel that
    the test owns: the sentinel is untouched and the answer is the reference's"""
    from crbhip import lib, check, ptr, cur_stream
    rng = np.random.default_rng(n_total)
    xc = np.array([n_total // 3, n_total - n_total // 3], np.int32)
    xyz = rng.uniform(-2, 2, (n_total, 3)).astype(np.float32)
    new = rng.uniform(-2, 2, (5, 3)).astype(np.float32)
    nc = np.array([2, 3], np.int32)
    ra, na, rb, nb = 0.5, 16, 1.0, 64
    nbytes = int(lib.crb_ball_query2_grid_workspace_bytes(n_total))
    assert nbytes % 4 == 0
    guard, sentinel = 64 * 1024 // 4, 0x5a5a5a5a
    buf = torch.full((nbytes // 4 + guard,), sentinel, dtype=torch.int32, device=dev)
    ia = torch.empty((5, na), dtype=torch.int32, device=dev)
    ib = torch.empty((5, nb), dtype=torch.int32, device=dev)
    ea, eb = torch.empty((5,), dtype=torch.uint8, device=dev), torch.empty((5,), dtype=torch.uint8, device=dev)
    check(lib.crb_ball_query2_grid_stack(2, 5, ra, na, rb, nb, ptr(_t(new, dev)), ptr(_t(nc, dev)), ptr(_t(xyz, dev)), ptr(_t(xc, dev)),
                                         n_total, ptr(ia), ptr(ib), ptr(ea), ptr(eb), ptr(buf), nbytes, cur_stream(dev)),
          'crb_ball_query2_grid_stack')
    torch.cuda.synchronize(dev)
    touched = int((buf[nbytes // 4:] != sentinel).sum())
    assert touched == 0, '%d words written behind the %d bytes the size query reported' % (touched, nbytes)
    for (idx, empty), r, ns in (((ia, ea), ra, na), ((ib, eb), rb, nb)):
        ridx, rempty = E.ref_ball_query(r, ns, xyz, xc, new, nc)
        np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
        np.testing.assert_array_equal(empty.cpu().numpy().astype(bool), rempty)


# ------------------------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize('name', list(FPS))
def test_fps(dev, name):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = FPS[name]
    xyz = _t(c['xyz'], dev)
    for m in c['ms']:
        got = U.farthest_point_sample(xyz, m).cpu().numpy()
        np.testing.assert_array_equal(got, E.ref_fps(c['xyz'], m), err_msg='%s m=%d (%s)' % (name, m, c['claims']['variant']))


# ------------------------------------------------------------------------------------------------------------------ three-NN, interpolation
@pytest.mark.parametrize('name', list(NN))
def test_three_nn(dev, name):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = NN[name]
    dist, idx = U.three_nn(_t(c['unknown'], dev), _t(c['ucnt'], dev), _t(c['known'], dev), _t(c['kcnt'], dev))
    rd2, ridx = E.ref_three_nn(c['unknown'], c['ucnt'], c['known'], c['kcnt'])
    np.testing.assert_array_equal(idx.cpu().numpy(), ridx)
    dist = dist.cpu().numpy()
    missing = np.isinf(rd2)
    np.testing.assert_array_equal(np.isinf(dist), missing)
    # the wrapper's torch.sqrt of the kernel's dist2: IEEE sqrt is correctly rounded, so this is the reference's value; one ulp is what
    # a device library may take instead
    np.testing.assert_array_max_ulp(dist[~missing], np.sqrt(rd2[~missing]), maxulp=1)
    # and on to interpolation, from the rows whose frame has three known points (the others index past their frame, as in the reference)
    use = E.nn_usable(c)
    rng = np.random.default_rng(3)
    feat = rng.normal(size=(len(c['known']), 3)).astype(np.float32)
    w = rng.uniform(0, 1, (int(use.sum()), 3)).astype(np.float32)
    out = U.three_interpolate(_t(feat, dev), idx[_t(use, dev)].contiguous(), _t(w, dev))
    np.testing.assert_array_equal(out.cpu().numpy(), E.ref_three_interpolate(feat, ridx[use], w))


def _within(got, ref64, count, mag, what):
    err = np.abs(got.astype(np.float64) - ref64)
    bad = err > E.grad_bound(count, mag)
    assert not bad.any(), '%s: %d elements outside the bound, worst %.3e at count %d' % (
        what, int(bad.sum()), float(err[bad].max()), int(count[bad][np.argmax(err[bad])]))


@pytest.mark.parametrize('name', list(INTERP))
def test_three_interpolate(dev, name):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = INTERP[name]
    f = _t(c['feat'], dev).requires_grad_(True)
    out = U.three_interpolate(f, _t(c['idx'], dev), _t(c['w'], dev))
    np.testing.assert_array_equal(out.detach().cpu().numpy(), E.ref_three_interpolate(c['feat'], c['idx'], c['w']))
    out.backward(_t(c['grad_out'], dev))
    _within(f.grad.cpu().numpy(), *E.ref_three_interpolate_grad64(c['grad_out'], c['idx'], c['w'], c['M']), what=name)


# ------------------------------------------------------------------------------------------------------------------ grouping
@pytest.mark.parametrize('name', list(GROUP))
def test_grouping_operation(dev, name):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    c = GROUP[name]
    f = _t(c['feat'], dev).requires_grad_(True)
    out = U.grouping_operation(f, _t(c['feat_cnt'], dev), _t(c['idx'], dev), _t(c['idx_cnt'], dev))
    np.testing.assert_array_equal(out.detach().cpu().numpy(), E.ref_group_points(c['feat'], c['feat_cnt'], c['idx'], c['idx_cnt']))
    out.backward(_t(c['grad_out'], dev))
    _within(f.grad.cpu().numpy(), *E.ref_group_points_grad64(c['grad_out'], c['idx'], c['idx_cnt'], c['feat_cnt'], len(c['feat'])),
            what=name)


@pytest.mark.parametrize('case', E.group_lds_over_cases(), ids=lambda c: c['name'])
def test_grouping_past_the_lds_slab_is_an_error(dev, case):
    """nsample (C + 1) floats above 64 KB: no kernel for it, and no data"""
    from crbhip import CrbHipError
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as U
    with pytest.raises(CrbHipError):
        U.grouping_operation(_t(case['feat'], dev), _t(case['feat_cnt'], dev), _t(case['idx'], dev), _t(case['idx_cnt'], dev))
