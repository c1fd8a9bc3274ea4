"""GPU: the first 3x3 BEV layer walking the block lists of its sparse input (csrc/bev_blocks.hip, crbhip.bev_blocks; the listed launches of
csrc/winograd_conv4.hip and csrc/winograd_wgrad4.hip; switch CRB_WINOGRAD_SPARSE).

* the device lists and counts are the numpy restatement's (tests/test_bev_blocks_host.py holds that one to a brute-force loop);
* forward: y and the BatchNorm slab sums with the conv-in list are bit-equal to the dense launch (an all-zero input patch gives +0);
* input gradient: with the conv-out list the listed blocks are bit-equal to the dense launch, every other block is exactly zero, and
  every active pixel lies in a listed block;
* weight gradient: inside the project's 2e-5 bar against the f64 gradient, no worse than 1.5 x the dense split-bf16 kernel's error (floor
  4 ulps of the largest entry, the floor of tests/test_winograd_wgrad4_gpu.py: skipped chunks add exact zeros, but the range boundaries
  move, so the f32 sums come in another order), and two calls are bit-equal;
* one SECOND training step at B = 2 with the lists against the same step with CRB_WINOGRAD_SPARSE=0: the loss and every parameter
  gradient are bit-equal except the first layer's weight gradient, which stays within 4e-5 of its largest entry (two kernels, each
  inside 2e-5 of the f64 gradient).
Shapes: 256 -> 128 at 3 x 37 x 29 (blocks that straddle images, half tiles, more workgroups than listed units) takes the lists; 128 -> 128
at 1 x 5 x 3 and 2 x 16 x 24 has no 32 x 128 instance (maps under 31 rows): forward and input gradient run dense there whatever the
tensor carries, the weight gradient takes its list at every size."""
import numpy as np
import pytest
import torch

from bev_blocks_cases import CASES, SHAPES, indices_of
from synth import kitti_batch

pytestmark = pytest.mark.gpu

BAR = 2e-5
RATIO = 1.5
FLOOR = 4 * 2.0 ** -23
CONV_SHAPES = [(3, 256, 128, 37, 29), (1, 128, 128, 5, 3), (2, 128, 128, 16, 24)]      # (N, Cin, Cout, H, W)
ACTIVE = ['random', 'empty', 'full']


@pytest.fixture(autouse=True)
def all_directions(monkeypatch):
    """every direction walks its list here, whatever the default set of CRB_WINOGRAD_SPARSE is"""
    from crbhip import winograd
    monkeypatch.setattr(winograd, 'SPARSE', {'f', 'i', 'w'})


def _count_calls(monkeypatch, name):
    from crbhip import winograd
    calls = []
    real = getattr(winograd.lib, name)
    monkeypatch.setattr(winograd.lib, name, lambda *a: (calls.append(1), real(*a))[1])
    return calls


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('case', CASES)
def test_device_lists_equal_the_numpy_restatement(dev, shape, case):
    from crbhip import bev_blocks
    N, H, W = shape
    idx = indices_of(case, N, H, W)
    want = bev_blocks.reference(idx, N, H, W)
    bl = bev_blocks.build(torch.from_numpy(idx).to(dev), N, H, W)
    counts = bl.counts.cpu().tolist()
    nb = bl.geom['nblocks']
    assert counts[:5] == [want['conv_in'].size, want['conv_out'].size, want['wgrad'].size, nb - want['conv_in'].size,
                          nb - want['conv_out'].size] and counts[5:] == [0, 0, 0]
    for k, c in (('conv_in', counts[0]), ('conv_out', counts[1]), ('wgrad', counts[2]), ('conv_in_rest', counts[3]),
                 ('conv_out_rest', counts[4])):
        assert np.array_equal(getattr(bl, k)[:c].cpu().numpy(), want[k]), k


def _sparse_map(dev, N, C, H, W, case, seed):
    """(x channels_last, zero outside the active pixels; its BlockLists)"""
    from crbhip import bev_blocks
    idx = torch.from_numpy(indices_of(case, N, H, W, seed)).to(dev)
    mask = torch.zeros((N, 1, H, W), device=dev)
    mask[idx[:, 0].long(), 0, idx[:, 2].long(), idx[:, 3].long()] = 1.0
    g = torch.Generator(device=dev).manual_seed(seed)
    x = (torch.randn((N, C, H, W), device=dev, generator=g) * mask).contiguous(memory_format=torch.channels_last)
    return x, bev_blocks.build(idx, N, H, W)


def _weight(dev, cout, cin, seed):
    g = torch.Generator(device=dev).manual_seed(100 + seed)
    return torch.randn((cout, cin, 3, 3), device=dev, generator=g) / np.sqrt(9.0 * cin)


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('case', ACTIVE)
def test_forward_with_the_list_is_bit_equal(dev, shape, case, monkeypatch):
    from crbhip import winograd
    N, cin, cout, H, W = shape
    calls = _count_calls(monkeypatch, 'crb_conv3x3_winograd4c_blocks_nhwc')
    x, bl = _sparse_map(dev, N, cin, H, W, case, 1)
    w = _weight(dev, cout, cin, 1)
    takes_list = bool(winograd._use_c(cin, cout)) and winograd.supported4(cin, cout, H, W)
    y0, s0 = winograd.conv3x3_stats(x, w)
    z0 = winograd.conv3x3(x, w)
    assert not calls
    xs = x.clone(memory_format=torch.preserve_format)
    xs._crb_bev_blocks = bl
    y1, s1 = winograd.conv3x3_stats(xs, w)
    z1 = winograd.conv3x3(xs, w)
    assert len(calls) == (2 if takes_list else 0)
    assert torch.equal(y1, y0) and torch.equal(s1, s0) and torch.equal(z1, z0) and torch.equal(z0, y0)
    if case == 'empty':
        assert not bool(y1.any()) and not bool(s1.any())
    else:
        assert bool(y1.any())


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('case', ACTIVE)
def test_input_gradient_with_the_list(dev, shape, case):
    """the layer is Cin -> Cout; its input gradient is the Cout -> Cin convolution of dy with the flipped weights"""
    from crbhip import winograd
    N, cin, cout, H, W = shape
    _, bl = _sparse_map(dev, N, 1, H, W, case, 2)
    w = _weight(dev, cout, cin, 2)
    g = torch.Generator(device=dev).manual_seed(3)
    dy = torch.randn((N, cout, H, W), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    U = winograd.weights_input_grad2(w)
    dense = winograd.conv3x3_U2(dy, U)
    dyv = dy.view_as(dy)
    dyv._crb_bev_blocks_out = bl
    got = winograd.conv3x3_U2(dyv, U)
    takes_list = bool(winograd._use_c(cout, cin)) and winograd.supported4(cout, cin, H, W)
    assert (getattr(got, '_crb_listed', None) is not None) == takes_list
    if not takes_list:
        assert torch.equal(got, dense)
        return
    mask = bl.pixel_mask('out')
    idx = bl.indices.long()
    assert bool(mask[idx[:, 0], idx[:, 2], idx[:, 3]].all())                   # every active pixel is covered
    a, b = got.permute(0, 2, 3, 1), dense.permute(0, 2, 3, 1)
    assert torch.equal(a[mask], b[mask])
    assert not bool(a[~mask].any())
    if case == 'empty':
        assert not bool(mask.any())
    elif case == 'full':
        assert bool(mask.all())
    else:
        assert bool(mask.any()) and not bool(mask.all())                       # (the case does skip blocks)


def _err(got, want):
    return float((got.double() - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('case', ACTIVE)
def test_weight_gradient_with_the_list(dev, shape, case, monkeypatch):
    from crbhip import winograd
    N, cin, cout, H, W = shape
    assert winograd._use_wgrad4(cin, cout, H, W)
    x, bl = _sparse_map(dev, N, cin, H, W, case, 4)
    g = torch.Generator(device=dev).manual_seed(5)
    dy = torch.randn((N, cout, H, W), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
    like = torch.empty((cout, cin, 3, 3), device=dev)
    want = torch.nn.grad.conv2d_weight(x.double(), like.shape, dy.double(), padding=1)
    dense = winograd.conv3x3_wgrad(x, dy, like)
    xs = x.clone(memory_format=torch.preserve_format)
    xs._crb_bev_blocks = bl
    calls = _count_calls(monkeypatch, 'crb_winograd4_wgrad_blocks')
    got = winograd.conv3x3_wgrad(xs, dy, like)
    again = winograd.conv3x3_wgrad(xs, dy, like)
    assert len(calls) == 2                                                     # the listed entry ran
    e_new, e_old = _err(got, want), _err(dense, want)
    print('%s %s: error / largest entry: listed %.3e, dense %.3e' % (shape, case, e_new, e_old), flush=True)
    assert torch.equal(got, again)
    assert e_old <= BAR and e_new <= BAR, (e_new, e_old)
    assert e_new <= max(RATIO * e_old, FLOOR), (e_new, e_old)
    if case == 'empty':
        assert not bool(got.any())


def _second_step(dev, B=2):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    torch.manual_seed(0)
    model = build_network(second_cfg('kitti').MODEL, 3, SyntheticDataset(num_frames=B)).to(dev).train()
    pts, off, gt = kitti_batch(0, B, 20000)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))[:, None]
    batch = {'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
             'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': B}
    torch.manual_seed(7)
    ret, _, _ = model(batch)
    ret['loss'].backward()
    torch.cuda.synchronize()
    return float(ret['loss'].detach()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def test_second_step_with_and_without_the_lists(dev, monkeypatch):
    """deterministic mode: without it the sparse backbone's own atomics move bits from run to run, whatever this layer does"""
    from crbhip import winograd
    first = 'backbone_2d.blocks.0.1.weight'
    seen = _count_calls(monkeypatch, 'crb_conv3x3_winograd4c_blocks_nhwc')
    seen_w = _count_calls(monkeypatch, 'crb_winograd4_wgrad_blocks')
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        loss1, g1 = _second_step(dev)
        assert len(seen) == 2 and len(seen_w) == 1                             # forward, input and weight gradient of the first layer only
        monkeypatch.setattr(winograd, 'SPARSE', set())
        loss0, g0 = _second_step(dev)
        assert len(seen) == 2 and len(seen_w) == 1
    finally:
        torch.use_deterministic_algorithms(was)
    assert first in g0 and len(g0) >= 84 and g0.keys() == g1.keys()
    assert loss1 == loss0
    differ = [n for n in g0 if n != first and not torch.equal(g0[n], g1[n])]
    assert not differ, differ
    err = float((g1[first] - g0[first]).abs().max()) / float(g0[first].abs().max())
    print('first-layer weight gradient, listed against dense: %.3e of the largest entry' % err, flush=True)
    assert err <= 4e-5, err
