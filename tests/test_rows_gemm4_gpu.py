"""The split-bf16 row GEMMs of the BEV up-sampling branches (csrc/rows_gemm4.hip, crbhip.rows_gemm) beside the vendor path they replace
(CRB_ROWS_GEMM_KERNEL=vendor: hipBLASLt f32 GEMMs for kernel 1, CK / MIOpen convolution kernels for kernel 2): forward, input gradient
and weight gradient of every case run through BaseBEVBackbone._up on BOTH paths, with every launch of the new path switched on, and are
compared with an f64 torch evaluation on the same inputs.

Bars. (1) The project's: |got - f64| <= 2e-5 of the largest entry, for both paths. (2) The new kernel's error is no worse than 1.5 x the
vendor path's on the same inputs, with the absolute floor tests/test_winograd_wgrad4_gpu.py set for the last kernel of this kind: 4 ulps of
the largest entry (4 * 2^-23 of it: the result is rounded to f32 once, and a case where the vendor kernel lands on the f64 value must not
fail the ratio). Observed on MI355X (new / vendor, of the largest entry): 16x256->256 k2s2 @100x88 forward 3.2e-7 / 6.9e-7, input gradient
2.0e-7 / 1.4e-6, weight gradient 5.4e-7 / 8.8e-7; 16x128->256 k1s1 @200x176 forward 2.3e-7 / 6.1e-7, input gradient 3.0e-7 / 8.5e-7; on
small maps both paths sit at 1e-7 .. 4e-7 and the floor is what holds (ratios up to 1.9 between two errors of one to three ulps). Every
case: profiles/rows_gemm4_errors_against_f64.txt."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BAR = 2e-5
RATIO = 1.5
FLOOR = 4 * 2.0 ** -23
ALL = {'1f', '1i', '1w', '2f', '2i', '2w'}

# (N, Cin, Cout, stride, H, W): the two layers of the bench (SECOND, batch 16)
BENCH = [(16, 128, 256, 1, 200, 176), (16, 256, 256, 2, 100, 88)]
# odd H and W, batches that do not fill a row tile (and one pixel), more ranges than chunks, 4 x 1 wave layout (128 columns), channel
# counts with an instance in one direction only (64 -> 128: forward), 512 columns at kernel 1
RAGGED = [(3, 128, 256, 1, 37, 29), (1, 256, 256, 2, 5, 3), (5, 256, 256, 2, 13, 9), (2, 64, 128, 2, 7, 11), (1, 256, 256, 1, 1, 1),
          (2, 128, 128, 2, 9, 7), (3, 256, 512, 1, 6, 5), (1, 256, 256, 2, 1, 1), (2, 256, 256, 1, 33, 17)]


def f64_all(x, w, dy, s):
    """(y, dx, dw) of conv_transpose2d(x, w, stride = kernel = s) in f64, as GEMMs on the row matrices"""
    N, cin, H, W = x.shape
    cout = w.shape[1]
    xr = x.permute(0, 2, 3, 1).reshape(-1, cin).double()
    wm = w.double().permute(0, 2, 3, 1).reshape(cin, s * s * cout)                       # [ci][(a, b, co)]
    y = (xr @ wm).view(N, H, W, s, s, cout).permute(0, 1, 3, 2, 4, 5).reshape(N, s * H, s * W, cout)
    dyr = dy.permute(0, 2, 3, 1).double().reshape(N, H, s, W, s, cout).permute(0, 1, 3, 2, 4, 5).reshape(-1, s * s * cout)
    dx = (dyr @ wm.t()).view(N, H, W, cin)
    dw = (xr.t() @ dyr).view(cin, s, s, cout).permute(0, 3, 1, 2)
    return y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2), dw


def test_f64_evaluation_is_the_transposed_convolution(dev):
    x, w, dy = maps(dev, 2, 8, 12, 2, 5, 3, 1)
    y, dx, dw = f64_all(x, w, dy, 2)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    yt = torch.nn.functional.conv_transpose2d(xd, wd, None, 2)
    yt.backward(dy.double())
    for a, b in ((y, yt.detach()), (dx, xd.grad), (dw, wd.grad)):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)


def maps(dev, N, cin, cout, s, H, W, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    cl = torch.channels_last
    x = torch.randn(N, cin, H, W, device=dev, generator=g).contiguous(memory_format=cl)
    w = torch.randn(cin, cout, s, s, device=dev, generator=g) / np.sqrt(cin)
    dy = torch.randn(N, cout, s * H, s * W, device=dev, generator=g).contiguous(memory_format=cl)
    return x, w, dy


def run(monkeypatch, kernel, x, w, dy, s):
    """(y, dx, dw) through the backbone's dispatch (BaseBEVBackbone._up) under CRB_ROWS_GEMM_KERNEL = kernel"""
    from crbhip import rows_gemm
    from pcdet.models.backbones_2d import BaseBEVBackbone
    monkeypatch.setattr(rows_gemm, 'KERNEL', kernel)
    monkeypatch.setattr(rows_gemm, 'LAUNCHES', set(ALL))
    conv = nn.ConvTranspose2d(w.shape[0], w.shape[1], s, stride=s, bias=False).to(x.device)
    with torch.no_grad():
        conv.weight.copy_(w)
    xi = x.detach().clone().requires_grad_(True)
    y = BaseBEVBackbone._up(conv, xi)
    y.backward(dy)
    return y.detach(), xi.grad, conv.weight.grad


def errors(got, want, keep=None):
    d = (got.double() - want).abs()
    w = want.abs()
    if keep is not None:
        d, w = d[keep], w[keep]
    return float(d.max()) / max(float(w.max()), 1e-300)


def check_both(monkeypatch, x, w, dy, s, label, keeps=(None, None, None)):
    want = f64_all(x, w, dy, s)
    new = run(monkeypatch, 'x6', x, w, dy, s)
    old = run(monkeypatch, 'vendor', x, w, dy, s)
    for name, n, o, t, keep in zip(('forward', 'input gradient', 'weight gradient'), new, old, want, keeps):
        e_new, e_old = errors(n, t, keep), errors(o, t, keep)
        print('%s %s: error / largest entry: rows_gemm4 path %.3e, vendor path %.3e (ratio %.2f)'
              % (label, name, e_new, e_old, e_new / max(e_old, 1e-300)), flush=True)
        assert e_old <= BAR, (label, name, e_old)
        assert e_new <= BAR, (label, name, e_new)
        assert e_new <= max(RATIO * e_old, FLOOR), (label, name, e_new, e_old)
    return new, old, want


class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


@pytest.mark.parametrize('N,cin,cout,s,H,W', BENCH + RAGGED)
def test_three_directions_match_f64_like_the_vendor_path(dev, monkeypatch, N, cin, cout, s, H, W):
    from crbhip import rows_gemm
    counted = {}
    for name in ('crb_rows_gemm4_forward', 'crb_rows_gemm4_input_grad', 'crb_rows_gemm4_wgrad'):
        counted[name] = _Counted(getattr(rows_gemm.lib, name))
        monkeypatch.setattr(rows_gemm.lib, name, counted[name])
    x, w, dy = maps(dev, N, cin, cout, s, H, W, 1000 * N + cin + cout + H + W)
    new, _, _ = check_both(monkeypatch, x, w, dy, s, '%dx%d->%d k%ds%d @%dx%d' % (N, cin, cout, s, s, H, W))
    # the new path ran each direction on the new kernel exactly where it has an instance (once), the vendor path never
    calls = tuple(counted[n].calls for n in ('crb_rows_gemm4_forward', 'crb_rows_gemm4_input_grad', 'crb_rows_gemm4_wgrad'))
    assert calls == tuple(int(rows_gemm.supported(cin, cout, s, d)) for d in range(3)), calls
    assert new[0].is_contiguous(memory_format=torch.channels_last) and new[0].shape == (N, cout, s * H, s * W)
    assert new[1].shape == x.shape and new[2].shape == w.shape
    # bit-equal rerun of every direction that ran on the new kernels (a direction without an instance ran on the vendor kernel, whose
    # weight gradient adds with float atomics)
    again = run(monkeypatch, 'x6', x, w, dy, s)
    for d, (a, b) in enumerate(zip(new, again)):
        if rows_gemm.supported(cin, cout, s, d):
            assert torch.equal(a, b), d


@pytest.mark.parametrize('cin,cout,s', [(128, 256, 1), (256, 256, 2), (64, 128, 2)])
def test_weight_image_equals_the_numpy_restatement(dev, cin, cout, s):
    from crbhip import rows_gemm
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    w = torch.randn(cin, cout, s, s, device=dev, generator=g) * 10.0 ** (6 * torch.rand(cin, cout, s, s, device=dev, generator=g) - 3)
    for direction in (rows_gemm.FORWARD, rows_gemm.INPUT_GRAD):
        if not rows_gemm.supported(cin, cout, s, direction):
            continue
        for wt in (w, w.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)):          # the weight's strides are honoured
            img = rows_gemm.weights(wt, cin, cout, s, direction)
            want = rows_gemm.weight_image_reference(w.cpu().numpy(), s, direction)
            got = img.cpu().numpy().view(np.uint16).reshape(want.shape)
            assert np.array_equal(got, want), (direction, tuple(wt.stride()))
    # cached per weight memory and version: the same image object until the weight changes
    a = rows_gemm.weights(w, cin, cout, s, rows_gemm.FORWARD)
    assert rows_gemm.weights(w, cin, cout, s, rows_gemm.FORWARD) is a
    w.mul_(2.0)
    b = rows_gemm.weights(w, cin, cout, s, rows_gemm.FORWARD)
    assert b is not a
    want = rows_gemm.weight_image_reference(w.cpu().numpy(), s, rows_gemm.FORWARD)
    assert np.array_equal(b.cpu().numpy().view(np.uint16).reshape(want.shape), want)


def _log_uniform(shape, dev, g, decades):
    mag = 10.0 ** ((torch.rand(shape, device=dev, generator=g) - 0.5) * decades)
    sign = torch.where(torch.rand(shape, device=dev, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('case', ['x', 'w', 'dy', 'all'])
def test_inputs_spanning_six_decades(dev, monkeypatch, case, s):
    N, cin, cout, H, W = 2, 256, 256, 19, 13
    x, w, dy = maps(dev, N, cin, cout, s, H, W, 70 + s)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    cl = torch.channels_last
    if case in ('x', 'all'):
        x = _log_uniform(x.shape, dev, g, 6).contiguous(memory_format=cl)
    if case in ('w', 'all'):
        w = _log_uniform(w.shape, dev, g, 6)
    if case in ('dy', 'all'):
        dy = _log_uniform(dy.shape, dev, g, 6).contiguous(memory_format=cl)
    new, old, _ = check_both(monkeypatch, x, w, dy, s, 'six decades in %s, k%d' % (case, s))
    for t in new + old:
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize('s', [1, 2])
@pytest.mark.parametrize('what', ['inf', 'nan'])
@pytest.mark.parametrize('where', ['x', 'dy'])
def test_one_non_finite_input(dev, monkeypatch, what, where, s):
    """one Inf / NaN in channel 5 of one pixel of x (of dy): what it reaches is non-finite on both paths and in f64 (the split turns Inf
    into NaN: inf - inf) - the output pixels of that input pixel and weight-gradient row 5 for x; the input-gradient pixel and
    weight-gradient column 5 for dy - and every other entry meets the bars"""
    N, cin, cout, H, W = 2, 256, 256, 12, 10
    x, w, dy = maps(dev, N, cin, cout, s, H, W, 80 + s)
    ky = torch.ones(N, cout, s * H, s * W, dtype=torch.bool, device=dev)
    kx = torch.ones(N, cin, H, W, dtype=torch.bool, device=dev)
    kw = torch.ones(cin, cout, s, s, dtype=torch.bool, device=dev)
    if where == 'x':
        x[1, 5, 7, 3] = float(what)
        ky[1, :, 7 * s:7 * s + s, 3 * s:3 * s + s] = False
        kw[5] = False
    else:
        dy[1, 5, 7 * s + s - 1, 3 * s] = float(what)
        kx[1, :, 7, 3] = False
        kw[:, 5, s - 1, 0] = False
    new, old, want = check_both(monkeypatch, x, w, dy, s, '%s in %s, k%d' % (what, where, s), keeps=(ky, kx, kw))
    for got in (new, old, want):
        for t, keep in zip(got, (ky, kx, kw)):
            assert bool(torch.isfinite(t[keep]).all())
            if not bool(keep.all()):
                assert not bool(torch.isfinite(t[~keep]).any())


@pytest.mark.parametrize('N,cin,cout,s,H,W', [(2, 256, 256, 2, 37, 29), (16, 256, 256, 2, 100, 88), (16, 128, 256, 1, 200, 176)])
def test_bit_equal_across_calls_and_streams(dev, monkeypatch, N, cin, cout, s, H, W):
    """no atomics and a fixed order of every sum: no dependence on the call or the stream"""
    x, w, dy = maps(dev, N, cin, cout, s, H, W, 5)
    ref = run(monkeypatch, 'x6', x, w, dy, s)
    for a, b in zip(ref, run(monkeypatch, 'x6', x, w, dy, s)):
        assert torch.equal(a, b)
    torch.cuda.synchronize()
    for _ in range(2):
        st = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(st):
            out = run(monkeypatch, 'x6', x, w, dy, s)
        st.synchronize()
        for a, b in zip(ref, out):
            assert torch.equal(a, b)


def test_conv2d_1x1_weight_and_switched_off_launches(dev, monkeypatch):
    """a Conv2d 1x1 weight (Cout,Cin,1,1) takes the same kernels with its strides swapped; a launch that is switched off runs on the vendor
    kernel of that direction inside the same autograd node"""
    from crbhip import rows_gemm
    from pcdet.models.backbones_2d import BaseBEVBackbone
    x, w, dy = maps(dev, 2, 256, 256, 1, 21, 10, 9)
    want = f64_all(x, w, dy, 1)
    monkeypatch.setattr(rows_gemm, 'KERNEL', 'x6')
    fwd = _Counted(rows_gemm.lib.crb_rows_gemm4_forward)
    wg = _Counted(rows_gemm.lib.crb_rows_gemm4_wgrad)
    monkeypatch.setattr(rows_gemm.lib, 'crb_rows_gemm4_forward', fwd)
    monkeypatch.setattr(rows_gemm.lib, 'crb_rows_gemm4_wgrad', wg)
    for launches, calls in ((set(ALL), (1, 1)), ({'1f'}, (2, 1)), ({'1i'}, (2, 1))):
        monkeypatch.setattr(rows_gemm, 'LAUNCHES', launches)
        conv = nn.Conv2d(256, 256, 1, bias=False).to(dev)
        with torch.no_grad():
            conv.weight.copy_(w[:, :, 0, 0].t()[:, :, None, None])
        xi = x.detach().clone().requires_grad_(True)
        y = BaseBEVBackbone._up(conv, xi)
        y.backward(dy)
        assert (fwd.calls, wg.calls) == calls, launches
        assert errors(y.detach(), want[0]) <= BAR and errors(xi.grad, want[1]) <= BAR
        assert errors(conv.weight.grad[:, :, 0, 0].t(), want[2][:, :, 0, 0]) <= BAR


def test_bev_backbone_training_step_new_against_vendor(dev, monkeypatch):
    """a BaseBEVBackbone training step (both up-sampling branches with an instance) on the new kernels against the vendor path, with the
    tolerances tests/test_second_gpu.py uses for the backbone's row path against its module path"""
    from crbhip import rows_gemm
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d import BaseBEVBackbone
    cfg = EasyDict({'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [128, 256], 'UPSAMPLE_STRIDES': [1, 2],
                    'NUM_UPSAMPLE_FILTERS': [256, 256]})
    torch.manual_seed(0)
    m = BaseBEVBackbone(cfg, input_channels=64).to(dev).train().to(memory_format=torch.channels_last)
    ref = copy.deepcopy(m)
    x1 = torch.randn(3, 64, 40, 48, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    x2 = x1.detach().clone().requires_grad_(True)
    go = torch.randn(3, 512, 40, 48, device=dev).contiguous(memory_format=torch.channels_last)
    counted = _Counted(rows_gemm.lib.crb_rows_gemm4_forward)
    monkeypatch.setattr(rows_gemm.lib, 'crb_rows_gemm4_forward', counted)
    monkeypatch.setattr(rows_gemm, 'LAUNCHES', set(ALL))
    monkeypatch.setattr(rows_gemm, 'KERNEL', 'x6')
    a = m({'spatial_features': x1})['spatial_features_2d']
    a.backward(go)
    assert counted.calls == 2
    monkeypatch.setattr(rows_gemm, 'KERNEL', 'vendor')
    b = ref({'spatial_features': x2})['spatial_features_2d']
    b.backward(go)
    assert counted.calls == 2
    torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4)

    def same_up_to_relu_flips(g1, g2, what):
        d, scale = (g1 - g2).abs(), max(1.0, float(g2.abs().max()))
        assert float(d.median()) < 1e-3 * scale, what
        assert float((d > 5e-3 * scale).float().mean()) < 0.05, what
        assert float(d.norm() / g2.norm()) < 3e-2, what
    same_up_to_relu_flips(x1.grad, x2.grad, 'input grad')
    for (n1, p1), (_, p2) in zip(m.named_parameters(), ref.named_parameters()):
        same_up_to_relu_flips(p1.grad, p2.grad, n1)
    for (n1, b1), (_, b2) in zip(m.named_buffers(), ref.named_buffers()):
        torch.testing.assert_close(b1.float(), b2.float(), rtol=1e-4, atol=1e-5, msg=lambda s, n1=n1: n1 + ': ' + s)
    # the scoring pass (eval, no grad) takes the forward kernel too, with the image made once per weight version
    m.eval()
    ref.eval()
    with torch.no_grad():
        monkeypatch.setattr(rows_gemm, 'KERNEL', 'x6')
        ya = m({'spatial_features': x1.detach()})['spatial_features_2d']
        assert counted.calls == 4
        monkeypatch.setattr(rows_gemm, 'KERNEL', 'vendor')
        yb = ref({'spatial_features': x1.detach()})['spatial_features_2d']
    torch.testing.assert_close(ya, yb, rtol=1e-4, atol=1e-4)


def test_deterministic_mode_keeps_the_default_modes_forward_and_input_gradient(dev, monkeypatch):
    """torch.use_deterministic_algorithms: the stride-2 branch's forward and input gradient are the default mode's bits (the mode promises
    the default mode's gradients up to summation order), its weight gradient is dense_strided's; with the forward switched off the caller
    keeps its dense_strided route whole"""
    from crbhip import rows_gemm, dense_strided
    x, w, dy = maps(dev, 2, 256, 256, 2, 20, 14, 21)
    ref = run(monkeypatch, 'x6', x, w, dy, 2)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        det = run(monkeypatch, 'x6', x, w, dy, 2)
        want_dw = dense_strided.weight_grad('deconv', x, dy, 2, 2, 2, 0)
        assert torch.equal(det[0], ref[0]) and torch.equal(det[1], ref[1])
        assert torch.equal(det[2], want_dw)
        assert errors(det[2], f64_all(x, w, dy, 2)[2]) <= BAR
        monkeypatch.setattr(rows_gemm, 'LAUNCHES', {'2i', '2w'})
        conv = nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False).to(dev)
        assert rows_gemm.up_conv(conv, x.detach().clone().requires_grad_(True)) is None
    finally:
        torch.use_deterministic_algorithms(was)
