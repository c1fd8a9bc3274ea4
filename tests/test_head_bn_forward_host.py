"""CPU: the host-visible pieces of the anchor head's forward inside the concat BatchNorm apply (csrc/head_bn.hip: head_bn_forward_kernel,
crbhip.head_bn.linear_deferred): prototypes and sizes, what `dispatch_forward` answers without a device, the formula the kernel evaluates
against autograd in f64, and the backbone's deferral falling back for host tensors."""
import torch
import torch.nn as nn


def head_f64(xs, gammas, betas, W, bias, eps):
    """out = relu(gamma ((x - mean) invstd) + beta) W^T + b with the batch statistics of every branch, in the kernel's order"""
    z = []
    for x, g, b in zip(xs, gammas, betas):
        mean, invstd = x.mean(0), (x.var(0, unbiased=False) + eps).rsqrt()
        z.append(torch.relu(g * ((x - mean) * invstd) + b))
    return torch.cat(z, 1) @ W.t() + bias


def test_the_formula_in_f64_against_autograd():
    torch.manual_seed(5)
    n, C, K, eps = 2 * 33 * 17, 128, 60, 1e-3

    def leaves():
        torch.manual_seed(6)
        xs = [torch.randn(n, C, dtype=torch.float64, requires_grad=True) for _ in range(2)]
        gs = [(torch.rand(C, dtype=torch.float64) + 0.5).requires_grad_(True) for _ in range(2)]
        bs = [(torch.rand(C, dtype=torch.float64) - 0.5).requires_grad_(True) for _ in range(2)]
        W = (torch.randn(K, 2 * C, dtype=torch.float64) / 16).requires_grad_(True)
        bias = torch.randn(K, dtype=torch.float64).requires_grad_(True)
        return xs, gs, bs, W, bias
    dout = torch.randn(n, K, dtype=torch.float64)
    xs, gs, bs, W, bias = leaves()
    got = head_f64(xs, gs, bs, W, bias, eps)
    got.backward(dout)
    xr, gr, br, Wr, biasr = leaves()
    z = torch.cat([torch.relu(torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.0, eps)) for x, g, b in zip(xr, gr, br)], 1)
    want = z @ Wr.t() + biasr
    want.backward(dout)
    assert float((got - want).detach().abs().max()) <= 1e-13 * float(want.detach().abs().max())
    for a, o in zip(xs + gs + bs + [W, bias], xr + gr + br + [Wr, biasr]):
        assert float((a.grad - o.grad).abs().max()) <= 1e-12 * float(o.grad.abs().max())


def test_prototypes_and_image_size():
    import crbhip
    from crbhip import lib
    protos = crbhip.parse_header()
    # x0, x1, par, image, bias | n | nbranch, width, K | out | stream
    assert len(protos['crb_bn_head_forward'][1]) == 11 and len(protos['crb_bn_head_forward_weights'][1]) == 6
    # image: [ceil(K / 32)][Ct / 16][3 pieces][64 lanes][8 bf16]
    assert lib.crb_bn_head_forward_weights_bytes(2, 256, 72) == 3 * 32 * 3 * 1024
    assert lib.crb_bn_head_forward_weights_bytes(2, 128, 60) == 2 * 16 * 3 * 1024
    for bad in ((1, 256, 72), (2, 64, 72), (2, 256, 64), (2, 192, 72)):
        assert lib.crb_bn_head_forward_weights_bytes(*bad) == 0


def _pending_record(widths=(256, 256), n=5):
    from crbhip import head_bn
    xs = [torch.randn(n, c) for c in widths]
    bns = [nn.BatchNorm1d(c) for c in widths]
    saved = [(x, x.mean(0), x.var(0, unbiased=False).add(bn.eps).rsqrt(), bn.weight.detach(), bn.bias.detach()) for x, bn in zip(xs, bns)]
    return head_bn.Record(None, [(x, bn.weight, bn.bias) for x, bn in zip(xs, bns)], saved, True)


def test_dispatch_forward_says_why(monkeypatch):
    from crbhip import head_bn
    assert head_bn.FORWARD == (__import__('os').environ.get('CRB_HEAD_BN_FORWARD', '1') == '1')
    rec = _pending_record()
    assert rec.pending and rec.rows_shape == (5, 512) and rec.n == 5 and rec.widths == [256, 256]
    monkeypatch.setattr(head_bn, 'ENABLED', True)
    monkeypatch.setattr(head_bn, 'FORWARD', True)
    monkeypatch.setattr(head_bn, 'LAUNCHES', {'sums', 'apply'})
    assert head_bn.dispatch_forward(rec, 72) == ('fused', 'forward,apply,sums')
    assert head_bn.dispatch_forward(None, 72)[0] == 'vendor'
    path, why = head_bn.dispatch_forward(rec, 40)
    assert path == 'vendor' and 'K = 40' in why
    path, why = head_bn.dispatch_forward(_pending_record((64, 64)), 72)
    assert path == 'vendor' and '[64, 64]' in why
    with torch.no_grad():
        path, why = head_bn.dispatch_forward(rec, 72)
    assert path == 'vendor' and 'grad mode' in why
    monkeypatch.setattr(head_bn, 'FORWARD', False)
    assert head_bn.dispatch_forward(rec, 72) == ('vendor', 'CRB_HEAD_BN_FORWARD=0')
    assert head_bn.linear_deferred(rec, torch.zeros(72, 512), torch.zeros(72)) is None
    monkeypatch.setattr(head_bn, 'FORWARD', True)
    monkeypatch.setattr(head_bn, 'LAUNCHES', {'apply'})
    path, why = head_bn.dispatch_forward(rec, 72)
    assert path == 'vendor' and "'sums'" in why
    # CRB_HEAD_BN switches the backward alone
    monkeypatch.setattr(head_bn, 'ENABLED', False)
    assert head_bn.dispatch_forward(rec, 72) == ('fused', 'forward')
    # a written map's record is not pending
    rows = torch.zeros(5, 512)
    done = head_bn.Record(rows, rec.inputs, rec.saved, True)
    monkeypatch.setattr(head_bn, 'ENABLED', True)
    assert not done.pending and head_bn.dispatch_forward(done, 72)[0] == 'vendor'


def test_the_deferral_falls_back_for_host_tensors():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d import BaseBEVBackbone
    cfg = EasyDict({'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [8, 16], 'UPSAMPLE_STRIDES': [1, 2],
                    'NUM_UPSAMPLE_FILTERS': [8, 8]})
    torch.manual_seed(0)
    m = BaseBEVBackbone(cfg, input_channels=6).train()
    assert m.defer_concat is False
    x = torch.randn(2, 6, 8, 8).contiguous(memory_format=torch.channels_last)
    want = m({'spatial_features': x})['spatial_features_2d']
    m.defer_concat = True
    out = m({'spatial_features': x})
    assert 'spatial_features_2d_pending' not in out and out['spatial_features_2d'].shape == (2, 16, 8, 8)
    assert torch.equal(out['spatial_features_2d'], want)
