"""GPU: the sparse RoI-aware pooling (csrc/roiaware_sparse.hip through crbhip/roiaware_sparse.py and RoIAwarePoolSparseFunction)
on the cases of tests/roiaware_cases.py.

Yardsticks. (1) The dense route on the same device - RoIAwarePool3d per frame, avg and max, `sum(-1).nonzero()` and the gather, as
PartA2FCHead.roiaware_pool / forward did before the sparse route existed: coords, part, feat and argmax torch.equal. (2) The numpy f64
definition: coords / max / argmax exact, avg rtol = atol = 1e-6 (the bar of tests/test_partA2_gpu.py). Gradients of a seeded upstream
gradient against the f64 definition, per entry |got - ref| <= (T + 2) * 2^-24 * sum|terms| with T the number of rows that contribute to
the entry: the bound for summing T f32 terms in any order (T - 1 additions), plus two roundings per term (1 / n and the product). The
dense route's atomics must meet the same bound in the same test. Entries without a term are exact zeros."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roiaware_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def _dev(c, dev):
    t = {k: torch.from_numpy(np.array(c[k])).to(dev) for k in ('rois', 'pts', 'off', 'part', 'feat')}
    return t


class _Ctx:
    pass


def _dense(c, t, grads=None):
    """the dense route: -> coords (T,4) i32, part rows, feat rows, argmax rows (stacked point index), and with grads = (g_part, g_feat)
    the gradients of the part / point features"""
    from pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils import RoIAwarePool3d, RoIAwarePool3dFunction
    B = c['rois'].shape[0]
    off = c['off']
    part, feat = t['part'], t['feat']
    if grads is not None:
        part, feat = part.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    layer = RoIAwarePool3d(c['o'], c['max_pts'])
    pp, pr, am = [], [], []
    for b in range(B):
        sl = slice(int(off[b]), int(off[b + 1]))
        xyz, roi = t['pts'][sl].contiguous(), t['rois'][b].contiguous()
        pp.append(layer(roi, xyz, part[sl].contiguous(), pool_method='avg'))
        pr.append(layer(roi, xyz, feat[sl].contiguous(), pool_method='max'))
        ctx = _Ctx()
        RoIAwarePool3dFunction.forward(ctx, roi, xyz, t['feat'][sl].contiguous(), c['o'], c['max_pts'], 'max')
        a = ctx.roiaware_pool3d_for_backward[1]
        am.append(torch.where(a >= 0, a + int(off[b]), a))
    pp, pr, am = torch.cat(pp), torch.cat(pr), torch.cat(am)
    idx = pp.sum(dim=-1).nonzero()
    r, x, y, z = idx.unbind(1)
    rows_p, rows_f = pp[r, x, y, z], pr[r, x, y, z]
    out = [idx.int(), rows_p.detach(), rows_f.detach(), am[r, x, y, z]]
    if grads is not None:
        torch.autograd.backward([rows_p, rows_f], list(grads))
        out += [part.grad, feat.grad]
    return out


def _sparse(c, t, buffers=None):
    from crbhip import roiaware_sparse
    return roiaware_sparse.forward(t['rois'], t['pts'], t['off'], t['part'], t['feat'], c['o'], c['max_pts'], buffers=buffers)


def _garbage(dev):
    def new(shape, dtype):
        if dtype == torch.float32:
            return torch.full(shape, float('nan'), dtype=dtype, device=dev)
        return torch.full(shape, 0x7f if dtype == torch.uint8 else 0x7f7f7f7f, dtype=dtype, device=dev)
    return new


@pytest.mark.parametrize('name', cases.CASE_NAMES)
def test_rows_equal_the_dense_route_and_the_definition(dev, name):
    c, d = cases.get_case(name)
    t = _dev(c, dev)
    sp = _sparse(c, t)
    assert sp is not None
    coords, part, feat, argmax = _dense(c, t)
    assert torch.equal(sp.coords, coords)
    assert torch.equal(sp.part, part)
    assert torch.equal(sp.feat, feat)
    assert torch.equal(sp.argmax, argmax)
    np.testing.assert_array_equal(sp.coords.cpu().numpy(), d['coords'])
    np.testing.assert_array_equal(sp.feat.cpu().numpy(), d['feat'])
    np.testing.assert_array_equal(sp.argmax.cpu().numpy(), d['argmax'])
    err = np.abs(sp.part.cpu().numpy().astype(np.float64) - d['part'])
    print('%s: rows %d, kept hits %d, avg max err %.3g' % (name, len(d['coords']), sp.hit_pt.numel(), err.max() if err.size else 0))
    np.testing.assert_allclose(sp.part.cpu().numpy(), d['part'], rtol=1e-6, atol=1e-6)
    # the CSR list is the definition's kept points, row after row
    np.testing.assert_array_equal(sp.hit_pt.cpu().numpy(), np.concatenate(d['kept']) if d['kept'] else np.zeros(0, np.int32))
    # outputs and workspaces pre-filled with garbage: the same bits
    sp2 = _sparse(c, t, buffers=_garbage(dev))
    for a, b in zip(sp, sp2):
        assert torch.equal(a, b)


@pytest.mark.parametrize('name', cases.CASE_NAMES)
def test_gradients_within_the_summation_bound_and_reproducible(dev, name):
    from crbhip import roiaware_sparse
    c, d = cases.get_case(name)
    t = _dev(c, dev)
    T, C, N = len(d['coords']), c['feat'].shape[1], len(c['pts'])
    rng = np.random.default_rng(7)
    g_part = rng.normal(0, 1, (T, 4)).astype(np.float32)
    g_feat = rng.normal(0, 1, (T, C)).astype(np.float32)
    ref = cases.grad_definition(c, d, g_part, g_feat)
    gp, gf = torch.from_numpy(g_part).to(dev), torch.from_numpy(g_feat).to(dev)
    sp = _sparse(c, t)
    got_p, got_f = roiaware_sparse.backward(sp, N, gp, gf)
    again_p, again_f = roiaware_sparse.backward(sp, N, gp, gf, buffers=_garbage(dev))
    assert torch.equal(got_p, again_p) and torch.equal(got_f, again_f)
    dense = _dense(c, t, grads=(gp, gf))
    for label, gpart, gfeat in (('sparse', got_p, got_f), ('dense', dense[4], dense[5])):
        for what, got, key in (('part', gpart, 'part'), ('feat', gfeat, 'feat')):
            got = got.cpu().numpy().astype(np.float64)
            bound = (ref['n_' + key] + 2) * EPS * ref['abs_' + key]
            err = np.abs(got - ref['grad_' + key])
            live = ref['n_' + key] > 0
            print('%s %s %s: max err / bound %.3f, entries with terms %d, most terms %d' % (
                name, label, what, (err[live] / bound[live]).max() if live.any() else 0, live.sum(), ref['n_' + key].max()))
            assert (err <= bound).all()
            assert (got[~live] == 0).all()                    # points in no RoI, cut by the cap or never an argmax
    assert (ref['n_part'] > 1).any() or name in ('few', 'ragged')     # some point sums over several rows (overlapping RoIs)
    # through autograd: the same numbers
    from pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils import roiaware_pool_sparse
    part, feat = t['part'].clone().requires_grad_(True), t['feat'].clone().requires_grad_(True)
    out = roiaware_pool_sparse(t['rois'], t['pts'], t['off'], part, feat, c['o'], c['max_pts'])
    torch.autograd.backward([out[1], out[2]], [gp, gf])
    assert torch.equal(part.grad, got_p) and torch.equal(feat.grad, got_f)


def _head_and_batch(c, dev, seed=43):
    from golden._constants import parta2_cfg, seeded_state
    from pcdet.models.roi_heads import PartA2FCHead
    cfg = parta2_cfg()
    cfg.ROI_AWARE_POOL.POOL_SIZE = c['o']
    cfg.ROI_AWARE_POOL.MAX_POINTS_PER_VOXEL = c['max_pts']
    head = PartA2FCHead(input_channels=c['feat'].shape[1], model_cfg=cfg, num_class=1)
    head.load_state_dict(seeded_state(head, seed))
    head.to(dev)
    B, R = c['rois'].shape[:2]
    frame = np.repeat(np.arange(B, dtype=np.float32), np.diff(c['off']))[:, None]

    def batch(part=None):
        part = c['part'] if part is None else part
        b = {'point_coords': np.concatenate([frame, c['pts']], 1), 'point_features': c['feat'],
             'point_part_offset': np.ascontiguousarray(part[:, :3]), 'point_cls_scores': np.ascontiguousarray(part[:, 3]),
             'rois': c['rois'], 'roi_labels': np.ones((B, R), np.int64)}
        b = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in b.items()}
        b['batch_size'] = B
        return b
    return head, batch


def _run_head(head, batch, enabled, monkeypatch, train):
    """-> rcnn_cls, rcnn_reg, number of dense roiaware_pool calls"""
    from crbhip import roiaware_sparse
    monkeypatch.setattr(roiaware_sparse, 'ENABLED', enabled)
    calls = []
    dense = type(head).roiaware_pool
    monkeypatch.setattr(head, 'roiaware_pool', lambda bd: (calls.append(1), dense(head, bd))[1], raising=False)
    head.train(train)
    if train:
        torch.manual_seed(0)
        head.assign_targets = lambda bd: {'rois': bd['rois'], 'roi_labels': bd['roi_labels'],
                                          'rcnn_cls_labels': torch.zeros(1), 'reg_valid_mask': torch.zeros(1)}
        head(batch)
        return head.forward_ret_dict['rcnn_cls'].detach(), head.forward_ret_dict['rcnn_reg'].detach(), len(calls)
    with torch.no_grad():
        bd = head(batch)
    return bd['batch_cls_preds'], bd['batch_box_preds'], len(calls)


@pytest.mark.parametrize('train', [False, True])
def test_head_gives_the_same_bits_with_the_switch_on_and_off(dev, monkeypatch, train):
    c, _ = cases.get_case('golden')
    head, batch = _head_and_batch(c, dev)
    cls_on, reg_on, dense_on = _run_head(head, batch(), True, monkeypatch, train)
    cls_off, reg_off, dense_off = _run_head(head, batch(), False, monkeypatch, train)
    assert (dense_on, dense_off) == (0, 1)
    assert torch.equal(cls_on, cls_off) and torch.equal(reg_on, reg_off)
    assert float(cls_on.abs().max()) > 0


def test_ungrouped_rows_are_sorted_by_frame_once(dev, monkeypatch):
    c, _ = cases.get_case('golden')
    head, batch = _head_and_batch(c, dev)
    b = batch()
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(c['pts']))).to(dev)
    for k in ('point_coords', 'point_features', 'point_part_offset', 'point_cls_scores'):
        b[k] = b[k][perm].contiguous()
    # a stable sort by frame keeps the shuffled order inside a frame, so the cells' first points differ from the grouped call: the
    # yardstick is the dense route on the same shuffled rows
    ref = _run_head(head, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}, False, monkeypatch, False)
    got = _run_head(head, b, True, monkeypatch, False)
    assert got[2] == 0 and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_few_rows_and_a_negative_part_feature_take_the_dense_route(dev, monkeypatch):
    from crbhip import roiaware_sparse
    c, d = cases.get_case('few')
    head, batch = _head_and_batch(c, dev)
    on = _run_head(head, batch(), True, monkeypatch, False)
    off = _run_head(head, batch(), False, monkeypatch, False)
    assert on[2] == 1 and torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])

    c, d = cases.get_case('golden')
    part = c['part'].copy()
    p = int(d['kept'][5][0])                                   # a kept point of some row
    part[p, 3] = max(float(part[p, 3]), 0.5)                   # above the score mask, so the head leaves its offsets alone
    part[p, 1] = -0.25
    t = _dev(dict(c, part=part), dev)
    assert roiaware_sparse.forward(t['rois'], t['pts'], t['off'], t['part'], t['feat'], c['o'], c['max_pts']) is None
    head, batch = _head_and_batch(c, dev)
    on = _run_head(head, batch(part), True, monkeypatch, False)
    off = _run_head(head, batch(part), False, monkeypatch, False)
    assert on[2] == 1 and torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    # and the unchanged input stays on the sparse route
    assert _run_head(head, batch(), True, monkeypatch, False)[2] == 0


def test_peak_memory_stays_far_below_one_dense_point_table(dev):
    """R 64, o 12, max_pts 128: one pts_idx_of_voxels table of the dense route is 64 * 12^3 * 128 * 4 B = 56.6 MB"""
    from crbhip import roiaware_sparse
    rng = np.random.default_rng(11)
    frames, rois = cases._scene(rng, 1, 64, 16, 150, 300, 12000)
    c = cases._finish(rng, frames, rois, 12, 128, 16)
    t = _dev(c, dev)
    N = len(c['pts'])
    table = 64 * 12 ** 3 * 128 * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sp = _sparse(c, t)
    g = roiaware_sparse.backward(sp, N, torch.ones_like(sp.part), torch.ones_like(sp.feat))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print('rows %d, kept hits %d, points %d: peak %.2f MB (dense table %.1f MB)' % (
        sp.coords.shape[0], sp.hit_pt.numel(), N, peak / 1e6, table / 1e6))
    assert sp.coords.shape[0] > 5000 and g[0].shape == (N, 4)
    assert peak < table / 4
