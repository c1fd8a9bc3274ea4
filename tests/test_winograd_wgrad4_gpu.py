"""The split-bf16 Winograd weight gradient (csrc/winograd_wgrad4.hip, crb_winograd4_wgrad) beside the f32-MFMA kernel it replaces where
it has an instance (csrc/winograd_wgrad.hip, crb_winograd2_wgrad): every case runs on BOTH kernels (crbhip.winograd.WGRAD_KERNEL) and is
compared with the f64 weight gradient of the direct convolution (aten.convolution_backward in double = what F.conv2d's backward
computes).

Bars. (1) The project's: |got - f64| <= 2e-5 of the largest entry. (2) The split kernel's error is no worse than 1.5 x the f32 kernel's
on the same inputs (the bar of the forward kernel's split), with an absolute floor of 4 ulps of the largest entry (4 * 2^-23 of it: the
result is rounded to f32 once, 1/2 ulp, and a case where the f32 kernel lands on the f64 value must not fail the ratio).
Observed on MI355X (new / f32 kernel, of the largest entry): 16x128->128@200x176 1.8e-6 / 1.7e-6, 16x256->256@100x88 1.3e-6 / 1.7e-6,
16x256->128@200x176 2.3e-6 / 2.0e-6 (with one round of workgroups instead of two - accumulation chains of twice the length - the first
was 2.8e-6 / 1.7e-6, over the ratio bar: DESIGN.md section 6); small and wide-range maps 1.4e-7 .. 2.3e-7 / 0.4e-7 .. 2.4e-7, where the
floor (4.8e-7) is what holds: ratios up to 1.8 (3.8 on a 1 x 1 map) between two errors of one or two ulps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAR = 2e-5
RATIO = 1.5
FLOOR = 4 * 2.0 ** -23

BENCH = [(16, 128, 128, 200, 176), (16, 256, 256, 100, 88), (16, 256, 128, 200, 176)]
# half tiles and partial chunks (odd H, W), more ranges than chunks (5 x 3, 1 x 1), odd N, 128 -> 256, 384 -> 128, maps narrower than
# a chunk, chunk rows that end inside a chunk
RAGGED = [(3, 128, 128, 37, 29), (1, 128, 128, 5, 3), (1, 128, 128, 1, 1), (5, 128, 256, 12, 9), (2, 384, 128, 18, 23),
          (7, 256, 128, 9, 40), (1, 128, 128, 64, 2)]
# no split-bf16 instance (channel counts that are multiples of 64 but not of 128): the dispatcher falls back to the f32 kernel
FALLBACK = [(2, 64, 192, 9, 11), (2, 192, 128, 10, 10), (1, 64, 64, 21, 20)]


def f64_wgrad(x, dy, wshape):
    return torch.nn.grad.conv2d_weight(x.double(), wshape, dy.double(), padding=1)


def run(monkeypatch, kernel, x, dy, like):
    from crbhip import winograd
    monkeypatch.setattr(winograd, 'WGRAD_KERNEL', kernel)
    return winograd.conv3x3_wgrad(x, dy, like)


def errors(got, want, keep=None):
    """max |got - want| over the entries in `keep` (all), relative to the largest kept |want|"""
    d = (got.double() - want).abs()
    w = want.abs()
    if keep is not None:
        d, w = d[keep], w[keep]
    return float(d.max()) / max(float(w.max()), 1e-300)


def check_both(monkeypatch, x, dy, K, C, label, keep=None):
    want = f64_wgrad(x, dy, (K, C, 3, 3))
    like = torch.empty(K, C, 3, 3, device=x.device)
    new = run(monkeypatch, 'x6', x, dy, like)
    old = run(monkeypatch, 'f32', x, dy, like)
    e_new, e_old = errors(new, want, keep), errors(old, want, keep)
    print('%s: error / largest entry: split-bf16 path %.3e, f32-MFMA kernel %.3e (ratio %.2f)'
          % (label, e_new, e_old, e_new / max(e_old, 1e-300)), flush=True)
    assert e_old <= BAR, (label, e_old)
    assert e_new <= BAR, (label, e_new)
    assert e_new <= max(RATIO * e_old, FLOOR), (label, e_new, e_old)
    return new, old, want


def maps(dev, N, C, K, H, W, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.randn(N, C, H, W, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(N, K, H, W, device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    return x, dy, g


@pytest.mark.parametrize('N,C,K,H,W', BENCH + RAGGED + FALLBACK)
def test_both_kernels_match_the_f64_weight_gradient(dev, monkeypatch, N, C, K, H, W):
    from crbhip import winograd, lib
    assert winograd.wgrad_supported(C, K, H, W)
    assert bool(lib.crb_winograd4_wgrad_supported(C, K, H, W)) == (C % 128 == 0 and K % 128 == 0)
    x, dy, _ = maps(dev, N, C, K, H, W, 1000 * N + C + K + H + W)
    new, _, _ = check_both(monkeypatch, x, dy, K, C, '%dx%d->%d@%dx%d' % (N, C, K, H, W))
    # bit-equal rerun; the gradient lands in the weight's own memory layout
    assert torch.equal(new, run(monkeypatch, 'x6', x, dy, torch.empty(K, C, 3, 3, device=dev)))
    cl = run(monkeypatch, 'x6', x, dy, torch.empty(K, C, 3, 3, device=dev).contiguous(memory_format=torch.channels_last))
    assert cl.stride() == torch.empty(K, C, 3, 3).contiguous(memory_format=torch.channels_last).stride()
    assert torch.equal(cl, new)


def _log_uniform(shape, dev, g, decades):
    mag = 10.0 ** ((torch.rand(shape, device=dev, generator=g) - 0.5) * decades)
    sign = torch.where(torch.rand(shape, device=dev, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).float()


@pytest.mark.parametrize('case', ['log_uniform_x', 'log_uniform_dy', 'log_uniform_both', 'relu_outliers', 'tiny_dy', 'denormal_x',
                                  'denormal_dy'])
def test_wide_range_inputs(dev, monkeypatch, case):
    """magnitudes the forward kernel's split never saw: 12 decades log-uniform in x, in dy and in both; post-ReLU x (half zeros) with a
    few 1e4 outliers; dy at 1e-8 scale; half of the entries of x / of dy denormal (they contribute nothing to an f32 result of
    normal size, under either kernel, and must not turn into anything else)"""
    N, C, K, H, W = 2, 128, 128, 36, 28
    x, dy, g = maps(dev, N, C, K, H, W, 77)
    cl = torch.channels_last
    if case in ('log_uniform_x', 'log_uniform_both'):
        x = _log_uniform((N, C, H, W), dev, g, 12).contiguous(memory_format=cl)
    if case in ('log_uniform_dy', 'log_uniform_both'):
        dy = _log_uniform((N, K, H, W), dev, g, 12).contiguous(memory_format=cl)
    if case == 'relu_outliers':
        x = torch.relu(x)
        idx = torch.randint(0, x.numel(), (12,), device=dev, generator=g)
        x.permute(0, 2, 3, 1).view(-1)[idx] = 1e4          # (the NHWC view of channels_last memory: no copy)
    if case == 'tiny_dy':
        dy = dy * 1e-8
    if case == 'denormal_x':
        x = torch.where(torch.rand(x.shape, device=dev, generator=g) < 0.5, x * 1e-40, x).contiguous(memory_format=cl)
        assert float(x[x != 0].abs().min()) < 1.1754944e-38
    if case == 'denormal_dy':
        dy = torch.where(torch.rand(dy.shape, device=dev, generator=g) < 0.5, dy * 1e-40, dy).contiguous(memory_format=cl)
        assert float(dy[dy != 0].abs().min()) < 1.1754944e-38
    new, old, _ = check_both(monkeypatch, x, dy, K, C, case)
    assert bool(torch.isfinite(new).all()) and bool(torch.isfinite(old).all())


@pytest.mark.parametrize('what', ['inf', 'nan'])
@pytest.mark.parametrize('where', ['x', 'dy'])
def test_one_non_finite_input(dev, monkeypatch, what, where):
    """one Inf / NaN in channel 5 of x (of dy): the weight gradients of that input (output) channel are non-finite under both kernels
    (the split turns Inf into NaN: inf - inf), every other entry meets the bars"""
    N, C, K, H, W = 2, 128, 128, 36, 28
    x, dy, _ = maps(dev, N, C, K, H, W, 78)
    t = x if where == 'x' else dy
    t[1, 5, 17, 9] = float(what)
    keep = torch.ones(K, C, 3, 3, dtype=torch.bool, device=dev)
    if where == 'x':
        keep[:, 5] = False
    else:
        keep[5] = False
    new, old, want = check_both(monkeypatch, x, dy, K, C, '%s in %s' % (what, where), keep=keep)
    for got in (new, old, want):
        assert not bool(torch.isfinite(got[~keep]).any())
        assert bool(torch.isfinite(got[keep]).all())


@pytest.mark.parametrize('N,C,K,H,W', [(2, 128, 128, 37, 29), (16, 256, 256, 100, 88)])
def test_bit_equal_across_calls_streams_and_cu_reservations(dev, monkeypatch, N, C, K, H, W):
    """fixed reduction order (per-workgroup partials in f32, ranges added in range order in double): no dependence on the stream, on
    what else holds CUs (crb_cu_reservation), or on the call"""
    from crbhip import lib, check, cur_stream
    x, dy, _ = maps(dev, N, C, K, H, W, 5)
    like = torch.empty(K, C, 3, 3, device=dev)
    ref = run(monkeypatch, 'x6', x, dy, like)
    assert torch.equal(ref, run(monkeypatch, 'x6', x, dy, like))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(s):
            outs.append(run(monkeypatch, 'x6', x, dy, like))
        s.synchronize()
    assert torch.equal(outs[0], ref) and torch.equal(outs[1], ref)
    try:
        for n in (16, 100, 255, 4000):
            check(lib.crb_cu_reservation(n, cur_stream(dev)), 'crb_cu_reservation')
            assert torch.equal(run(monkeypatch, 'x6', x, dy, like), ref), n
    finally:
        check(lib.crb_cu_reservation(0, cur_stream(dev)), 'crb_cu_reservation')
    assert torch.equal(run(monkeypatch, 'x6', x, dy, like), ref)


class _Counted:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a):
        self.calls += 1
        return self.fn(*a)


def test_dispatcher_chooses_by_shape_and_the_knob_forces_the_f32_kernel(dev, monkeypatch):
    """conv3x3_wgrad takes crb_winograd4_wgrad where crb_winograd4_wgrad_supported says so and crb_winograd2_wgrad elsewhere;
    WGRAD_KERNEL = 'f32' (CRB_WINOGRAD_WGRAD_KERNEL=f32) runs the f32 kernel's entry point for every shape; the autograd node goes
    through the same choice"""
    from crbhip import winograd
    c4, c2 = _Counted(winograd.lib.crb_winograd4_wgrad), _Counted(winograd.lib.crb_winograd2_wgrad)
    monkeypatch.setattr(winograd.lib, 'crb_winograd4_wgrad', c4)
    monkeypatch.setattr(winograd.lib, 'crb_winograd2_wgrad', c2)
    x, dy, _ = maps(dev, 2, 128, 256, 20, 14, 3)
    like = torch.empty(256, 128, 3, 3, device=dev)
    a = run(monkeypatch, 'x6', x, dy, like)
    assert (c4.calls, c2.calls) == (1, 0)
    b = run(monkeypatch, 'f32', x, dy, like)
    assert (c4.calls, c2.calls) == (1, 1)
    want = f64_wgrad(x, dy, like.shape)
    assert errors(a, want) <= BAR and errors(b, want) <= BAR
    xs, dys, _ = maps(dev, 2, 64, 128, 20, 14, 4)               # no split-bf16 instance: the f32 kernel under either setting
    for kernel in ('x6', 'f32'):
        got = run(monkeypatch, kernel, xs, dys, torch.empty(128, 64, 3, 3, device=dev))
        assert errors(got, f64_wgrad(xs, dys, (128, 64, 3, 3))) <= BAR
    assert (c4.calls, c2.calls) == (1, 3)
    monkeypatch.setattr(winograd, 'WGRAD_KERNEL', 'x6')
    w = (torch.randn(256, 128, 3, 3, device=dev) / np.sqrt(9 * 128)).requires_grad_(True)
    winograd.conv3x3(x, w, None).backward(dy)
    assert (c4.calls, c2.calls) == (2, 3)
    assert torch.equal(w.grad, a)


def test_workspace_is_shared_by_both_kernels(dev, monkeypatch):
    """one workspace per (device, stream), sized by the larger of the two kernels' answers: switching kernels does not reallocate"""
    from crbhip import winograd
    x, dy, _ = maps(dev, 1, 128, 128, 12, 12, 9)
    like = torch.empty(128, 128, 3, 3, device=dev)
    run(monkeypatch, 'x6', x, dy, like)
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    p = winograd._WGRAD_WS[key].data_ptr()
    run(monkeypatch, 'f32', x, dy, like)
    run(monkeypatch, 'x6', x, dy, like)
    assert winograd._WGRAD_WS[key].data_ptr() == p
