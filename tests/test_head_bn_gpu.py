"""The anchor head's backward inside the concat BatchNorm backward (csrc/head_bn.hip, crbhip.head_bn) beside the path it replaces
(CRB_HEAD_BN=0: hipBLASLt GEMMs for the head's input and weight gradient, crb_bn_relu_backward per branch) and an f64 evaluation of
BatchNorm(train) -> ReLU -> concat -> linear backward on the same inputs. The f64 evaluation takes the ReLU mask from the f32 forward
output (z > 0), as both paths do: an entry within rounding of the kink would otherwise decide the comparison.

Bars (tests/test_rows_gemm4_gpu.py), for each of dx_i, dgamma_i, dbeta_i, dW and db: |got - f64| <= 2e-5 of the largest entry, and
<= max(1.5 x today's path's error, 4 * 2^-23 of the largest entry).

Inputs: gamma from 0.5 .. 1.5 with one channel at 0, beta from -0.5 .. 0.5 with one channel at -100 (every row masked); dOut and the
x_i are the leading rows of larger buffers whose remainder is NaN, so a read past row n or past k = K makes a result non-finite.
x is standard normal, except at 2 rows: there dx is (1 - xhat^2) of its terms and xhat^2 = 1 / (1 + eps / var), so with var = 1 and
eps = 1e-3 the result is 1e-3 of what is subtracted and NO f32 evaluation is good to 2e-5 of the largest entry; the 2-row case draws x
with a spread of 0.02 (var of the order of eps), where the expression is well conditioned. Every small case has more ranges (two
workgroups per CU) than 16-row chunks.

Observed on MI355X (fused / today, of the largest entry; every case: profiles/head_bn_errors_against_f64.txt): fused 0.2e-7 .. 2.3e-7,
today 0.3e-7 .. 1.7e-6 (the sliced weight-gradient GEMM); the worst ratio is 1.79 at 2 rows (dgamma 1.8e-7 / 1.0e-7: the floor holds).
The two-frame SECOND step: equal loss, worst parameter gradient 2.6e-6 of its largest entry from the switched-off path."""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BAR = 2e-5
RATIO = 1.5
FLOOR = 4 * 2.0 ** -23
EPS = 1e-3
NAMES = ('dx0', 'dx1', 'dgamma0', 'dgamma1', 'dbeta0', 'dbeta1', 'dW', 'db')

# (rows, width, K): 2 x 256 with K = 72 at 2, 31, 33, 65 rows and the two ragged maps; one of every other instance
CASES = [(2, 256, 72), (31, 256, 72), (33, 256, 72), (65, 256, 72), (3 * 37 * 29, 256, 72), (2 * 33 * 17, 256, 72),
         (2 * 33 * 17, 128, 72), (3 * 37 * 29, 256, 60), (333, 128, 60)]


class Case(object):
    def __init__(self, dev, n, width, K, seed=0):
        g = torch.Generator(device=dev)
        g.manual_seed(1000 * seed + n + width + K)
        self.n, self.width, self.K = n, width, K
        pad = 37
        spread = 0.02 if n < 8 else 1.0
        self.xbufs, self.xs = [], []
        for _ in range(2):
            buf = torch.full((n + pad, width), float('nan'), device=dev)
            buf[:n] = torch.randn(n, width, device=dev, generator=g) * spread
            self.xbufs.append(buf)
        dbuf = torch.full((n + pad, K), float('nan'), device=dev)
        dbuf[:n] = torch.randn(n, K, device=dev, generator=g)
        self.dbuf, self.dout = dbuf, dbuf[:n]
        self.gammas = [torch.rand(width, device=dev, generator=g) + 0.5 for _ in range(2)]
        self.betas = [torch.rand(width, device=dev, generator=g) - 0.5 for _ in range(2)]
        for i in range(2):
            self.gammas[i][3 + i] = 0.0
            self.betas[i][5 + i] = -100.0
        self.w = torch.randn(K, 2 * width, device=dev, generator=g) / np.sqrt(2 * width)
        self.b = torch.randn(K, device=dev, generator=g)
        self.gmap = torch.randn(n, 2 * width, device=dev, generator=g)          # gradient of a second consumer of the map


def run(monkeypatch, case, fused, second=False, only_w=False, launches=('sums', 'apply')):
    """forward + backward of bn_relu_concat -> head on one path -> (gradients in NAMES order, forward map, trace of launches)"""
    from crbhip import bnrelu, head_bn
    from pcdet.utils.linear_rows import LinearRows
    monkeypatch.setattr(head_bn, 'ENABLED', bool(fused))
    monkeypatch.setattr(head_bn, 'LAUNCHES', set(launches))
    trace = []
    monkeypatch.setattr(head_bn, 'TRACE', trace)
    dev = case.dout.device
    bns = []
    for i in range(2):
        bn = nn.BatchNorm1d(case.width, eps=EPS, momentum=0.01).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(case.gammas[i])
            bn.bias.copy_(case.betas[i])
        bn.weight.requires_grad_(not only_w)
        bn.bias.requires_grad_(not only_w)
        bns.append(bn)
    xs = [buf[:case.n].detach().requires_grad_(not only_w) for buf in case.xbufs]
    w = case.w.detach().clone().requires_grad_(True)
    b = case.b.detach().clone().requires_grad_(not only_w)
    rows = bnrelu.bn_relu_concat(xs, bns, relu=True)
    record = getattr(rows, '_crb_head_bn', None)
    path, why = head_bn.dispatch(rows, record, case.K)
    y = head_bn.linear(rows, w, b, record) if record is not None else None
    assert (y is not None) == (path == 'fused'), (path, why)
    if y is None:
        y = LinearRows.apply(rows, w, b)
    if second:
        torch.autograd.backward([y, rows], [case.dout, case.gmap])
    else:
        y.backward(case.dout)
    torch.cuda.synchronize()
    grads = [xs[0].grad, xs[1].grad, bns[0].weight.grad, bns[1].weight.grad, bns[0].bias.grad, bns[1].bias.grad, w.grad, b.grad]
    return grads, rows.detach(), trace, (path, why)


def f64_all(case, z, second=False):
    """the same gradients in f64, the ReLU mask taken from the f32 forward output z"""
    n, C = case.n, case.width
    dout, W = case.dout.double(), case.w.double()
    dz = dout @ W
    if second:
        dz = dz + case.gmap.double()
    out = {}
    for i in range(2):
        x, g, b = case.xs64[i], case.gammas[i].double(), case.betas[i].double()
        invstd = (x.var(0, unbiased=False) + EPS).rsqrt()
        xh = (x - x.mean(0)) * invstd
        mask = (z[:, i * C:(i + 1) * C] > 0).double()
        d = mask * dz[:, i * C:(i + 1) * C]
        dbeta, dgamma = d.sum(0), (d * xh).sum(0)
        out['dx%d' % i] = g * invstd * (d - dbeta / n - xh * dgamma / n)
        out['dgamma%d' % i], out['dbeta%d' % i] = dgamma, dbeta
        out['zi%d' % i] = mask * (g * xh + b)
    out['dW'] = dout.t() @ torch.cat([out['zi0'], out['zi1']], 1)
    out['db'] = dout.sum(0)
    return [out[k] for k in NAMES]


def err(got, want):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def check_both(monkeypatch, case, label, second=False):
    case.xs64 = [buf[:case.n].double() for buf in case.xbufs]
    new, z_new, trace, (path, _) = run(monkeypatch, case, True, second)
    old, z_old, trace_old, _ = run(monkeypatch, case, False, second)
    assert path == 'fused' and trace == ['sums', 'apply'] and trace_old == []
    assert torch.equal(z_new, z_old)
    want = f64_all(case, z_new, second)
    for name, a, o, t in zip(NAMES, new, old, want):
        assert a.shape == o.shape and bool(torch.isfinite(a).all()) and bool(torch.isfinite(o).all()), (label, name)
        e_new, e_old = err(a, t), err(o, t)
        print('%s %s: error / largest entry: fused %.3e, today %.3e (ratio %.2f)' % (label, name, e_new, e_old, e_new / max(e_old, 1e-300)),
              flush=True)
        assert e_old <= BAR, (label, name, e_old)
        assert e_new <= BAR, (label, name, e_new)
        assert e_new <= max(RATIO * e_old, FLOOR), (label, name, e_new, e_old)
    return new, old


@pytest.mark.parametrize('n,width,K', CASES)
def test_gradients_match_f64_like_todays_path(dev, monkeypatch, n, width, K):
    case = Case(dev, n, width, K)
    new, _ = check_both(monkeypatch, case, '%d rows 2x%d K=%d' % (n, width, K))
    # two calls give the same bytes
    again, _, _, _ = run(monkeypatch, case, True)
    for a, b in zip(new, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the NaN remainders of the buffers were not touched
    assert bool(torch.isnan(case.dbuf[n:]).all()) and all(bool(torch.isnan(buf[n:]).all()) for buf in case.xbufs)


def test_a_rejected_shape_takes_the_old_path_and_says_so(dev, monkeypatch):
    case = Case(dev, 65, 64, 72)
    case.xs64 = [buf[:case.n].double() for buf in case.xbufs]
    new, z, trace, (path, why) = run(monkeypatch, case, True)
    assert path == 'vendor' and 'no instance' in why and '[64, 64]' in why and trace == []
    old, _, _, _ = run(monkeypatch, case, False)
    want = f64_all(case, z)
    for name, a, o, t in zip(NAMES, new, old, want):
        assert err(a, t) <= BAR and err(o, t) <= BAR, name
    # K without an instance
    case = Case(dev, 65, 256, 40)
    _, _, trace, (path, why) = run(monkeypatch, case, True)
    assert path == 'vendor' and 'K = 40' in why and trace == []


def test_a_second_consumer_of_the_map(dev, monkeypatch):
    """BatchNorm backward is linear in the map's gradient: the concat backward handles the other consumer's gradient alone and autograd
    adds the two"""
    check_both(monkeypatch, Case(dev, 2 * 33 * 17, 256, 72, seed=2), 'second consumer', second=True)


def test_only_the_head_weight_requires_a_gradient(dev, monkeypatch):
    case = Case(dev, 3 * 37 * 29, 256, 72, seed=3)
    case.xs64 = [buf[:case.n].double() for buf in case.xbufs]
    new, z, trace, (path, _) = run(monkeypatch, case, True, only_w=True)
    old, _, _, _ = run(monkeypatch, case, False, only_w=True)
    assert path == 'fused' and trace == ['sums']                    # no apply launch: no dx is produced
    assert all(g is None for g in new[:6]) and new[7] is None
    want = f64_all(case, z)[6]
    e_new, e_old = err(new[6], want), err(old[6], want)
    print('only dW: fused %.3e, today %.3e' % (e_new, e_old), flush=True)
    assert e_new <= BAR and e_new <= max(RATIO * e_old, FLOOR)


@pytest.mark.parametrize('launches', [('sums',), ('apply',), ()])
def test_switched_off_launches_run_on_the_kernels_they_replace(dev, monkeypatch, launches):
    case = Case(dev, 2 * 33 * 17, 256, 72, seed=4)
    case.xs64 = [buf[:case.n].double() for buf in case.xbufs]
    new, z, trace, (path, _) = run(monkeypatch, case, True, launches=launches)
    assert path == 'fused'
    assert trace == ['sums' if 'sums' in launches else 'vendor_sums', 'apply' if 'apply' in launches else 'vendor_apply']
    for name, a, t in zip(NAMES, new, f64_all(case, z)):
        assert err(a, t) <= BAR, (launches, name)


def _second_step(dev, monkeypatch, fused):
    from crbhip import head_bn
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    monkeypatch.setattr(head_bn, 'ENABLED', fused)
    trace = []
    monkeypatch.setattr(head_bn, 'TRACE', trace)
    B = 2
    torch.manual_seed(0)
    model = build_network(second_cfg().MODEL, 3, SyntheticDataset(num_frames=2)).to(dev).train()
    pts, off, gt = kitti_batch(100, B, 20000)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))
    torch.manual_seed(7)
    b = {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
         'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': B, 'point_frame_counts_host': np.diff(off).tolist(),
         'frame_id': np.array(['%06d' % (100 + i) for i in range(B)])}
    ret, _, _ = model(b)
    ret['loss'].backward()
    torch.cuda.synchronize()
    return float(ret['loss'].detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, trace


def test_second_training_step_with_the_switch_on_and_off(dev, monkeypatch):
    """a two-frame SECOND step: equal loss, every parameter gradient within 2e-4 of its largest entry (tests/test_determinism.py's bar)"""
    loss_on, g_on, trace = _second_step(dev, monkeypatch, True)
    loss_off, g_off, trace_off = _second_step(dev, monkeypatch, False)
    assert trace == ['sums', 'apply'] and trace_off == []
    assert loss_on == loss_off
    assert set(g_on) == set(g_off) and len(g_on) >= 84
    worst = ('', 0.0)
    for n, g in g_on.items():
        e = float((g - g_off[n]).abs().max()) / max(float(g_off[n].abs().max()), 1e-30)
        worst = max(worst, (n, e), key=lambda t: t[1])
    print('worst parameter gradient: %s %.3e' % worst, flush=True)
    for n, g in g_on.items():
        e = float((g - g_off[n]).abs().max()) / max(float(g_off[n].abs().max()), 1e-30)
        assert e <= 2e-4, (n, e)
