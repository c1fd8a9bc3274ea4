"""GPU: the five entry points of group_affine_rows_grad_kernel (csrc/pointnet2_stack.hip), one launch at a time, on the hand-built
index patterns of tests/sa_scatter_cases.py against their float64 reference, and sa_first_layer_scatter_fixed / sa_fixed_point_scale
(pointnet2_utils.py), the host side of the deterministic mode's 64-bit fixed-point scatter.

Bar: |grad_P - ref| <= TOL * max(mag), mag = the same index_add of |v| (a row's sum cancels; its error does not), TOL = 2e-5 as in
tests/test_sa_train_gpu.py; the same bar for part.sum(0) (summed in float64) against part_sum.

`tiny` (grad_z of 1e-41) has a test of its own at the kernel level: every f32 operation on it rounds to the subnormal quantum
2^-149, 1e-4 of an addend, so the bar is TOL * max(mag) plus that quantum times the number of roundings that reach a sum, written
out in the test. The plain form (v = grad_z: sums of subnormals are exact) and the wrapper, which moves such a gradient into the
normal range first, are held to the bar itself."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sa_scatter_cases as S

pytestmark = pytest.mark.gpu
TOL = 2e-5
FORMS = ('grad', 'bn', 'recompute', 'recompute_sorted', 'fixed', 'fixed_sorted')
KERNEL_CASES = [n for n in S.NAMES if n != 'tiny']


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def Dev(name, dev):
    """the tensors of a case on the device, made once per (case, device)"""
    self = _Case()
    c = S.case(name)
    self.c = c
    for k in ('xyz', 'new_xyz', 'P', 'W1x', 'grad_z', 'mean', 'invstd', 'gamma', 'beta', 'dbeta', 'dgamma', 'idx',
              'xyz_batch_cnt', 'new_xyz_batch_cnt'):
        setattr(self, k, torch.from_numpy(np.ascontiguousarray(c[k])).to(dev))
    self.em = torch.from_numpy(c['empty'].astype(np.uint8)).to(dev)
    live = torch.from_numpy(np.repeat(~c['empty'], c['ns'])).to(dev)
    self.live = live
    row = torch.from_numpy(c['row'].reshape(-1)).to(dev)
    q = torch.arange(c['M'], device=dev).repeat_interleave(c['ns'])
    self.rel = ((self.xyz[row] - self.new_xyz[q]) * live[:, None]).contiguous()       # f32, as the forward writes it
    self.y = S.reference(name)['y'].float().to(dev).contiguous()
    self.gz_nan = torch.where(live[:, None], self.grad_z, torch.full_like(self.grad_z, float('nan'))).contiguous()
    self.d1 = torch.stack([self.dbeta, self.dgamma]).contiguous()
    self.nslab = -(-c['n'] // 64)
    self.sorted = None
    return self


def _sorted(t, dev):
    """crb_pair_sort_by_source, checked against a stable torch sort"""
    from crbhip import lib, check, ptr, cur_stream
    if t.sorted is None:
        c = t.c
        n = c['n']
        sp = torch.full((n,), -1, dtype=torch.int32, device=dev)
        sr = torch.full((n,), -1, dtype=torch.int32, device=dev)
        wsb = int(lib.crb_pair_sort_workspace_bytes(c['M'], c['ns']))
        wss = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        check(lib.crb_pair_sort_by_source(c['B'], c['M'], c['ns'], ptr(t.xyz_batch_cnt), ptr(t.new_xyz_batch_cnt), ptr(t.idx), ptr(t.em),
                                          c['n_src'], ptr(sp), ptr(sr), ptr(wss), wsb, cur_stream(dev)), 'sort')
        key = torch.from_numpy(S.sort_key(c)).to(dev)
        order = torch.sort(key, stable=True)[1]
        assert torch.equal(sp.long(), order) and torch.equal(sr.long(), key[order])
        t.sorted = (sp, sr)
    return t.sorted


def _scale(c):
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils import sa_fixed_point_scale
    return sa_fixed_point_scale(*S.maxima(c), c['n'])


def _launch(form, t, dev, scale=None, gz=None, d1=None):
    """-> grad_P (float64; the int64 sums for the fixed forms), part"""
    from crbhip import lib, check, ptr, cur_stream
    c = t.c
    B, M, H, ns, n_src = c['B'], c['M'], c['H'], c['ns'], c['n_src']
    st = cur_stream(dev)
    part = torch.full((t.nslab, 3, H), float('nan'), device=dev)
    gP = torch.zeros((n_src, H), dtype=torch.int64 if form.startswith('fixed') else torch.float32, device=dev)
    xc, nc = t.xyz_batch_cnt, t.new_xyz_batch_cnt
    if form == 'grad':
        check(lib.crb_group_affine_rows_grad_stack(B, M, H, ns, ptr(xc), ptr(nc), ptr(t.idx), ptr(t.em), ptr(t.rel), ptr(t.grad_z), ptr(gP),
                                                   ptr(part), st), form)
    elif form == 'bn':
        check(lib.crb_group_affine_rows_grad_bn_stack(B, M, H, ns, ptr(xc), ptr(nc), ptr(t.idx), ptr(t.em), ptr(t.rel), ptr(t.grad_z), ptr(t.y),
                                                      ptr(t.mean), ptr(t.invstd), ptr(t.gamma), ptr(t.beta), ptr(t.dbeta), ptr(t.dgamma),
                                                      ptr(gP), ptr(part), st), form)
    else:
        sp, sr = _sorted(t, dev) if form.endswith('sorted') else (None, None)
        gz = t.gz_nan if gz is None else gz
        d1 = t.d1 if d1 is None else d1
        head = (B, M, H, ns, ptr(t.xyz), ptr(xc), ptr(t.P), ptr(t.new_xyz), ptr(nc), ptr(t.idx), ptr(t.em), ptr(t.W1x), ptr(gz), ptr(t.mean),
                ptr(t.invstd), ptr(t.gamma), ptr(t.beta), ptr(d1[0]), ptr(d1[1]), ptr(sp), ptr(sr), n_src)
        if form.startswith('fixed'):
            check(lib.crb_group_affine_rows_grad_bn_recompute_stack_fixed(*head, ptr(gP), scale, ptr(part), st), form)
        else:
            check(lib.crb_group_affine_rows_grad_bn_recompute_stack(*head, ptr(gP), ptr(part), st), form)
    return gP, part


def _assert_close(name, what, gP, part, ref, extra=0.0, part_extra=0.0):
    """gP: float64 (n_src, H). extra / part_extra: what a case adds to the bar, derived where it is passed"""
    assert bool(torch.isfinite(part).all()), what
    bar = TOL * float(ref['mag'].max())
    err = float((gP.cpu() - ref['grad_P']).abs().max())
    perr = float((part.double().sum(0).cpu() - ref['part_sum']).abs().max())
    print('%s %s: grad_P err %.3g bar %.3g, part err %.3g bar %.3g' % (name, what, err, bar + extra, perr, bar + part_extra))
    assert err <= bar + extra, (name, what, err, bar + extra)
    assert perr <= bar + part_extra, (name, what, perr, bar + part_extra)


@pytest.mark.parametrize('name', KERNEL_CASES)
def test_entry_points_against_float64(dev, name):
    t = Dev(name, dev)
    c = t.c
    scale = _scale(c)[0]
    for form in FORMS:
        ref = S.reference(name, bn=form != 'grad')
        gP, part = _launch(form, t, dev, scale)
        if form.startswith('fixed'):
            # the 64-bit carries are exercised, both signs. (one_row: every pair on one row, and the BatchNorm backward's values
            # sum to 0 over all pairs - only the running sums pass 2^32 there; two_rows is the same pattern with both signs.)
            fx = ref['grad_P'] * scale
            assert float(ref['mag'].max()) * scale > 2.0 ** 32
            assert name == 'one_row' or (float(fx.max()) > 2.0 ** 32 and float(fx.min()) < -2.0 ** 32)
            for _ in range(2):
                again, part2 = _launch(form, t, dev, scale)
                assert torch.equal(again, gP) and torch.equal(part2, part)
            gP = gP.double() / scale
        _assert_close(name, form, gP.double(), part, ref)


def test_tiny_at_the_subnormal_quantum(dev):
    """grad_z of 1e-41: every value is a multiple of q = 2^-149 and every f32 operation on it rounds to q / 2 at the worst.
    plain form: grad_P is a sum of subnormals, exact in f32 - the bar itself (the LDS fold and the global float atomic must not flush
      them); part: one rounding per product rel * v, n products.
    BatchNorm forms: an addend gamma invstd (d - dbeta / n - xhat (dgamma / n)) takes three roundings inside the bracket (the two
      quotients and the product with xhat; the differences of subnormals are exact), each multiplied by |gamma invstd| <= gi, and one
      of the outer product: a = q (1.5 gi + 0.5) per addend, K addends on the fullest row; part: n products of |rel| <= R with an
      addend that is off by a, and their own rounding.
    bare fixed forms: the helper's scale stops at 2^127, the largest normal power of two, so every head that leaves a slab is
      rounded to 2^-127 - at most K heads on a row (the result is 0; the wrapper is what keeps the precision)."""
    t = Dev('tiny', dev)
    c = t.c
    q = 2.0 ** -149
    K = int(np.bincount(c['row'].reshape(-1)).max())
    gi = S.maxima(c)[1]
    R = float(t.rel.abs().max())
    a = q * (1.5 * gi + 0.5)
    scale = _scale(c)[0]
    assert scale == 2.0 ** 127
    for form in FORMS:
        ref = S.reference('tiny', bn=form != 'grad')
        gP, part = _launch(form, t, dev, scale)
        if form == 'grad':
            extra, part_extra = 0.0, c['n'] * q / 2
        else:
            extra, part_extra = K * a, c['n'] * (R * a + q / 2)
        if form.startswith('fixed'):
            again, part2 = _launch(form, t, dev, scale)
            assert torch.equal(again, gP) and torch.equal(part2, part)
            gP = gP.double() / scale
            extra += K * 0.5 / scale
        _assert_close('tiny', form, gP.double(), part, ref, extra, part_extra)


def test_exact_case_is_exact_in_every_form(dev):
    t = Dev('exact', dev)
    scale = _scale(t.c)[0]
    for form in FORMS:
        ref = S.reference('exact', bn=form != 'grad')
        gP, part = _launch(form, t, dev, scale)
        if form.startswith('fixed'):
            assert torch.equal(gP.cpu(), torch.round(ref['grad_P'] * scale).to(torch.int64)), form
            gP = gP.double() / scale
        assert torch.equal(gP.double().cpu(), ref['grad_P']), form
        assert float(part.abs().max()) == 0.0                                          # rel = 0


def _wrapper(t, dev, gz, sorted_, d1=None):
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils import sa_first_layer_scatter_fixed
    c = t.c
    sp, sr = _sorted(t, dev) if sorted_ else (None, None)
    part = torch.full((t.nslab, 3, c['H']), float('nan'), device=dev)
    gP = sa_first_layer_scatter_fixed(c['B'], c['M'], c['H'], c['ns'], t.xyz, t.xyz_batch_cnt, t.P, t.new_xyz, t.new_xyz_batch_cnt, t.idx,
                                      t.em, t.W1x, gz, t.mean, t.invstd, t.gamma, t.beta, t.d1 if d1 is None else d1, sp, sr, part)
    assert gP.dtype == torch.float32 and gP.shape == (c['n_src'], c['H'])
    return gP, part


@pytest.mark.parametrize('sorted_', [False, True])
def test_wrapper_ignores_the_rows_of_empty_balls(dev, sorted_):
    t = Dev('empties', dev)
    out = []
    for fill in (0.0, float('nan'), float('inf'), 3e38):
        gz = torch.where(t.live[:, None], t.grad_z, torch.full_like(t.grad_z, fill)).contiguous()
        out.append(_wrapper(t, dev, gz, sorted_))
    _assert_close('empties', 'wrapper', out[0][0].double(), out[0][1], S.reference('empties'))
    for gP, part in out[1:]:
        assert torch.equal(gP, out[0][0]) and torch.equal(part, out[0][1])              # not one bit


@pytest.mark.parametrize('name', ['outlier', 'tiny', 'huge'])
def test_wrapper_accuracy_and_bound(dev, name):
    t = Dev(name, dev)
    ref = S.reference(name)
    assert float(ref['v'].abs().max()) <= _scale(t.c)[1]
    for sorted_ in (False, True):
        gP, part = _wrapper(t, dev, t.gz_nan, sorted_)
        _assert_close(name, 'wrapper sorted' if sorted_ else 'wrapper', gP.double(), part, ref)
        gP2, part2 = _wrapper(t, dev, t.gz_nan, sorted_)
        assert torch.equal(gP, gP2) and torch.equal(part, part2)


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_wrapper_propagates_a_non_finite_gradient(dev, bad):
    """the float entry point on the same inputs says where grad_P is not finite; the wrapper's result is not finite there"""
    t = Dev('empties', dev)
    ref = S.reference('empties')
    z = torch.from_numpy(S.case('empties')['gamma']).double() * ref['xhat'] + torch.from_numpy(S.case('empties')['beta']).double()
    # a live entry with z > 0: the ReLU mask drops a gradient entry of z <= 0 whatever it holds, NaN included
    p, ch = [int(v) for v in torch.nonzero(ref['live'][:, None] & (z > 0.5))[7]]
    gz = t.gz_nan.clone()
    gz[p, ch] = bad
    cases = [(gz, None)]
    for k in (0, 1):                                           # dbeta, dgamma
        d1 = t.d1.clone()
        d1[k, 2] = bad
        cases.append((t.gz_nan, d1))
    for gz, d1 in cases:
        gPf, _ = _launch('recompute', t, dev, gz=gz, d1=d1)
        where = ~torch.isfinite(gPf)
        assert bool(where.any())
        gP, _ = _wrapper(t, dev, gz, False, d1=d1)
        assert bool((~torch.isfinite(gP))[where].all())


@pytest.mark.parametrize('scale', [float('inf'), float('nan'), 0.0, -1.0])
def test_fixed_entry_point_rejects_a_scale_that_is_not_finite_and_positive(dev, scale):
    from crbhip import lib, ptr, cur_stream
    t = Dev('exact', dev)
    c = t.c
    gP = torch.zeros((c['n_src'], c['H']), dtype=torch.int64, device=dev)
    part = torch.zeros((t.nslab, 3, c['H']), device=dev)
    rc = lib.crb_group_affine_rows_grad_bn_recompute_stack_fixed(
        c['B'], c['M'], c['H'], c['ns'], ptr(t.xyz), ptr(t.xyz_batch_cnt), ptr(t.P), ptr(t.new_xyz), ptr(t.new_xyz_batch_cnt), ptr(t.idx),
        ptr(t.em), ptr(t.W1x), ptr(t.grad_z), ptr(t.mean), ptr(t.invstd), ptr(t.gamma), ptr(t.beta), ptr(t.dbeta), ptr(t.dgamma), None, None,
        c['n_src'], ptr(gP), ctypes.c_float(scale), ptr(part), cur_stream(dev))
    assert rc == -1                                            # CRB_ERR_ARG
    torch.cuda.synchronize()
    assert int(gP.abs().sum()) == 0 and float(part.abs().sum()) == 0.0                 # nothing was launched
