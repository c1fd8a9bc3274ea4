"""CPU: the host-visible pieces of the anchor head's backward inside the concat BatchNorm backward (csrc/head_bn.hip, crbhip.head_bn):
prototypes and exports, which shapes have an instance, what the dispatcher answers (and why) without a device, and the formulas the
kernels evaluate, in f64 against autograd of BatchNorm(train) -> ReLU -> concat -> linear."""
import subprocess

import torch
import torch.nn as nn

NAMES = ('crb_head_bn_supported', 'crb_head_bn_workspace_bytes', 'crb_head_bn_sums_count', 'crb_head_bn_sums', 'crb_head_bn_finalize',
         'crb_head_bn_weights_bytes', 'crb_head_bn_weights', 'crb_head_bn_apply')


def test_prototypes_and_exports():
    import crbhip
    protos = crbhip.parse_header()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', crbhip.lib_path], text=True)
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in protos and name in names, name
    assert sorted(n for n in names if n.startswith('crb_head_bn')) == sorted(NAMES)
    # x0, x1, par, dout | n | nbranch, width, K | sums, workspace | bytes | stream
    assert len(protos['crb_head_bn_sums'][1]) == 12 and len(protos['crb_head_bn_apply'][1]) == 13


def test_supported_shapes():
    from crbhip import lib, head_bn
    ok = lib.crb_head_bn_supported
    assert ok(2, 256, 72) == 1 and ok(2, 256, 60) == 1 and ok(2, 128, 72) == 1 and ok(2, 128, 60) == 1
    for bad in ((1, 256, 72), (3, 256, 72), (2, 64, 72), (2, 512, 72), (2, 256, 64), (2, 256, 76), (2, 256, 0), (0, 256, 72),
                (2, 0, 72), (2, 192, 72)):
        assert ok(*bad) == 0, bad
        assert lib.crb_head_bn_workspace_bytes(*bad) == 0 and lib.crb_head_bn_weights_bytes(*bad) == 0
        assert lib.crb_head_bn_sums_count(*bad) == 0
    assert head_bn.supported([256, 256], 72) and head_bn.supported([128, 128], 60)
    assert not head_bn.supported([256, 128], 72) and not head_bn.supported([256], 72) and not head_bn.supported([], 72)
    assert lib.crb_head_bn_sums_count(2, 256, 72) == 2 * 72 * 512 + 72
    # image: [Ct / 32][ceil(K / 16)][3 pieces][64 lanes][8 bf16]
    assert lib.crb_head_bn_weights_bytes(2, 256, 72) == 16 * 5 * 3 * 1024
    assert lib.crb_head_bn_weights_bytes(2, 128, 60) == 8 * 4 * 3 * 1024
    # partials: whole ranges of (2, K, Ct) f32 plus (2, 96) f64 column sums, at least 8 ranges
    n = lib.crb_head_bn_workspace_bytes(2, 256, 72)
    per = 2 * 72 * 512 * 4 + 2 * 96 * 8
    assert n >= 8 * per and n < 4096 * per


def _record(xs, bns, rows):
    from crbhip import head_bn
    saved = [(x, x.mean(0), x.var(0, unbiased=False).add(bn.eps).rsqrt(), bn.weight.detach(), bn.bias.detach()) for x, bn in zip(xs, bns)]
    return head_bn.Record(rows, [(x, bn.weight, bn.bias) for x, bn in zip(xs, bns)], saved, True)


def test_dispatch_says_why(monkeypatch):
    from crbhip import head_bn
    assert head_bn.ENABLED == (__import__('os').environ.get('CRB_HEAD_BN', '1') == '1')
    assert set(head_bn.DEFAULT_LAUNCHES.split(',')) <= {'sums', 'apply'}
    xs = [torch.randn(5, 256), torch.randn(5, 256)]
    bns = [nn.BatchNorm1d(256), nn.BatchNorm1d(256)]
    rows = torch.zeros(5, 512)
    rec = _record(xs, bns, rows)
    w, b = torch.zeros(72, 512), torch.zeros(72)
    monkeypatch.setattr(head_bn, 'ENABLED', True)
    path, why = head_bn.dispatch(rows, None, 72)
    assert path == 'vendor' and 'no BatchNorm record' in why
    path, why = head_bn.dispatch(rows, rec, 72)
    assert path == 'vendor' and 'device' in why                   # a host tensor: no device, no kernel
    assert head_bn.linear(rows, w, b, rec) is None
    with torch.no_grad():
        path, why = head_bn.dispatch(rows, rec, 72)
    assert path == 'vendor' and 'grad mode' in why
    monkeypatch.setattr(head_bn, 'ENABLED', False)
    path, why = head_bn.dispatch(rows, rec, 72)
    assert path == 'vendor' and 'CRB_HEAD_BN=0' in why
    assert head_bn.linear(rows, w, b, rec) is None
    assert rec.widths == [256, 256]
    # the record holds no reference to the map it describes (the map carries the record: no cycle)
    assert not any(v is rows for v in vars(rec).values())


def test_formulas_in_f64_against_autograd():
    """P2 / P3 -> dbeta, dgamma, dW and the dx expression, evaluated in f64, equal autograd of BatchNorm(train) -> ReLU -> concat -> linear
    (3,219 rows, 2 x 256 channels, K = 72) to rounding"""
    torch.manual_seed(3)
    n, C, K, eps = 3 * 37 * 29, 256, 72, 1e-3
    xs = [torch.randn(n, C, dtype=torch.float64, requires_grad=True) for _ in range(2)]
    gs = [(torch.rand(C, dtype=torch.float64) + 0.5).requires_grad_(True) for _ in range(2)]
    bs = [(torch.rand(C, dtype=torch.float64) - 0.5).requires_grad_(True) for _ in range(2)]
    W = (torch.randn(K, 2 * C, dtype=torch.float64) / 16).requires_grad_(True)
    bias = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(n, K, dtype=torch.float64)
    z = torch.cat([torch.relu(torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.0, eps)) for x, g, b in zip(xs, gs, bs)], 1)
    (z @ W.t() + bias).backward(dout)
    with torch.no_grad():
        for i, (x, g, b) in enumerate(zip(xs, gs, bs)):
            Wi = W[:, i * C:(i + 1) * C]
            invstd = (x.var(0, unbiased=False) + eps).rsqrt()
            xh = (x - x.mean(0)) * invstd
            mask = (g * xh + b > 0).double()
            P2 = dout.t() @ mask
            P3 = dout.t() @ (mask * xh)
            dbeta, dgamma = (Wi * P2).sum(0), (Wi * P3).sum(0)
            dW = g * P3 + b * P2
            dx = g * invstd * (mask * (dout @ Wi) - dbeta / n - xh * dgamma / n)
            for got, want in ((dbeta, b.grad), (dgamma, g.grad), (dW, W.grad[:, i * C:(i + 1) * C]), (dx, x.grad)):
                assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
        assert float((dout.sum(0) - bias.grad).abs().max()) <= 1e-13 * float(bias.grad.abs().max())
