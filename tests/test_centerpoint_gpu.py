"""GPU: CenterPoint. csrc/center_head.hip (target assignment, losses forward and backward, box decoding) through crbhip.center_head
against the golden written by the reference's own CenterHead / centernet_utils / loss_utils, the f64 definition of
tests/center_cases.py and the torch route in f64 on the device; CenterHead in training without a host synchronisation; CenterPoint from
centerpoint_cfg('kitti') on synthetic frames and the entropy / random strategies on it.

Bars: tests/test_centerpoint_cpu.py (FACTOR = 4 times the reference's own f32 error e_ref; heatmaps within 1 f32 ulp; integer and
copied quantities equal). Every figure is printed before it is asserted. Reproducibility, garbage rows, permuted overlaps: bit-equal.
Detector: the golden step and eval pass of the reference's CenterPoint (three runs: f32 NCHW, f32 channels_last, f64) with the same
factor on its e_ref; the two routes of the head (CRB_CENTER_FUSED) within those bars of each other."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import center_cases as cases
import test_centerpoint_cpu as cpu

pytestmark = pytest.mark.gpu


class no_fallback(warnings.catch_warnings):
    """the HIP route must not announce the torch route"""
    def __enter__(self):
        r = super().__enter__()
        warnings.filterwarnings('error', message='.*torch route.*')
        return r


def _equal(a, b):
    return all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in x)


# ---- targets ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.TARGET_CASES))
def test_targets_against_the_reference(dev, name):
    case, _ = cpu.targets_case(name)
    with no_fallback():
        res = cpu.run_targets(case, dev)
    assert not cpu.check_targets(res, name)


def test_targets_are_reproducible_and_order_independent(dev):
    case, _ = cpu.targets_case('edges')
    with no_fallback():
        res, again = cpu.run_targets(case, dev), cpu.run_targets(case, dev)
        perm = cpu.run_targets(case, dev, gt=cases.permuted_overlaps(case['gt_boxes']))
    assert _equal(res, again)
    assert all(np.array_equal(a['heatmap'], b['heatmap']) for a, b in zip(res, perm))
    assert not np.array_equal(res[0]['target_boxes'], perm[0]['target_boxes'])          # (the slots did move)


@pytest.mark.parametrize('name', ['one_head', 'edges', 'extras'])
def test_rows_beyond_a_frames_boxes_are_never_used(dev, name):
    case, _ = cpu.targets_case(name)
    with no_fallback():
        clean = cpu.run_targets(case, dev)
        dirty = cpu.run_targets(case, dev, gt=cases.garbage_rows(case['gt_boxes']))
    assert _equal(clean, dirty)


# ---- losses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,h', cpu.LOSS_HEADS)
@pytest.mark.parametrize('channels_last', [False, True])
def test_loss_forward_and_backward(dev, name, h, channels_last):
    case = cpu.loss_case(name, h)
    with cpu.quiet():
        ref64 = cpu.run_loss(case, dev, torch.float64)
    with no_fallback():
        res = cpu.run_loss(case, dev, channels_last=channels_last)
        again = cpu.run_loss(case, dev, channels_last=channels_last)
    assert not cpu.check_loss(res, ref64, name, h)
    assert all(np.array_equal(res[k], again[k]) for k in res)                          # forward and backward bit-equal


def test_empty_head_gives_the_undivided_negative_loss(dev):
    case = cpu.loss_case('empty_head', 0)
    with no_fallback():
        res = cpu.run_loss(case, dev)
    x = case['hm'].astype(np.float64)
    p = np.clip(1 / (1 + np.exp(-x)), 1e-4, 1 - 1e-4)
    neg = (np.log(1 - p) * p ** 2 * (1 - case['heatmap'].astype(np.float64)) ** 4).sum()
    e_ref = cpu.gold()['loss_empty_head_0_e_ref'][0]
    print('empty head: loss %.9f, -neg_loss %.9f, e_ref %.3g' % (res['loss'][0], -neg, e_ref))
    assert abs(res['loss'][0] + neg) <= cpu.FACTOR * e_ref and res['loss'][1] == 0 and not res['g_reg'].any()


# ---- decoding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.DECODE_CASES))
@pytest.mark.parametrize('channels_last', [False, True])
def test_decode_against_the_reference(dev, name, channels_last):
    with no_fallback():
        res = cpu.run_decode(cpu.decode_case(name), dev, channels_last=channels_last)
    assert not cpu.check_decode(res, name)


# ---- the head ---------------------------------------------------------------------------------------------------------------
def test_head_training_step_raises_no_synchronisation(dev):
    """forward + get_loss + backward of CenterHead: the reference synchronises per frame, per head and per box (.cpu(), .item())"""
    head = cpu.make_head(cases.TWO_HEADS, channels=64, dev=dev).to(memory_format=torch.channels_last).train()
    bd = cpu._head_batch(dev, channels=64)
    bd['spatial_features_2d'] = bd['spatial_features_2d'].contiguous(memory_format=torch.channels_last)
    with no_fallback():
        head(dict(bd))
        head.get_loss()[0].backward()                                                  # (first launches load code objects)
        torch.cuda.synchronize()
        head.zero_grad(set_to_none=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            warnings.filterwarnings('error', message='.*torch route.*')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                head(dict(bd))
                loss, tb = head.get_loss()
                loss.backward()
            finally:
                torch.cuda.set_sync_debug_mode('default')
            # (the mode announces itself once as a prototype feature: that notice is no synchronisation)
            syncs = [str(w.message) for w in rec if 'synchroniz' in str(w.message).lower() and 'prototype feature' not in str(w.message)]
    print('synchronisation warnings:', syncs)
    assert not syncs
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    assert [int(m.sum()) for m in head.forward_ret_dict['target_dicts']['masks']] == [5, 10]


def test_head_on_the_device_equals_the_head_on_the_host(dev):
    """the same seeded head, NCHW on the host (torch route, plain modules) and channels_last on the device (kernels, fused first
    layers): targets as in the kernel tests; the loss within the f32 error of the convolutions in front of it (1e-4 relative: three
    3x3 convolutions and two train-mode BatchNorm layers at B = 2 in f32 on two different machines)"""
    host = cpu.make_head(cases.TWO_HEADS, channels=64).train()
    devh = cpu.make_head(cases.TWO_HEADS, channels=64, dev=dev).to(memory_format=torch.channels_last).train()
    devh.load_state_dict(host.state_dict())
    with cpu.quiet():
        host(cpu._head_batch(channels=64))
        l0, tb0 = host.get_loss()
    bd = cpu._head_batch(dev, channels=64)
    bd['spatial_features_2d'] = bd['spatial_features_2d'].contiguous(memory_format=torch.channels_last)
    with no_fallback():
        devh(bd)
        l1, tb1 = devh.get_loss()
    for k in tb0:
        a, b = float(tb0[k]), float(tb1[k])
        print('%-16s host %.7f device %.7f' % (k, a, b))
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), k
    for t0, t1 in zip(host.forward_ret_dict['target_dicts']['inds'], devh.forward_ret_dict['target_dicts']['inds']):
        assert torch.equal(t0, t1.cpu())


# ---- detector ---------------------------------------------------------------------------------------------------------------
POINTS = 8000


def _detector(dev):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import centerpoint_cfg
    from pcdet.models import build_network
    cfg = centerpoint_cfg('kitti')
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS))
    return cfg, model.to(dev)


def _batch(dev):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(40, 2, POINTS)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {'points': t(np.concatenate([bidx[:, None], pts], 1)), 'point_frame_offsets': t(off), 'batch_size': 2,
            'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': t(gt), 'frame_id': np.array(['000040', '000041'])}


def test_training_step_and_eval_pass(dev):
    """centerpoint_without_resnet.yaml on the KITTI geometry: a 200 x 176 map, one head of three classes"""
    cfg, model = _detector(dev)
    assert type(model).__name__ == 'CenterPoint' and type(model.dense_head).__name__ == 'CenterHead'
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    gt_before = None
    with no_fallback():
        batch = _batch(dev)
        gt_before = batch['gt_boxes'].clone()
        ret, tb, _ = model(batch)
    opt.zero_grad(set_to_none=True)
    ret['loss'].backward()
    opt.step()
    torch.cuda.synchronize()
    print('loss %.6f' % float(ret['loss'].detach()), {k: round(float(v), 6) for k, v in tb.items()})
    assert torch.isfinite(ret['loss']) and torch.equal(batch['gt_boxes'], gt_before)
    assert set(tb) == {'hm_loss_head_0', 'loc_loss_head_0', 'rpn_loss', 'loss_rpn'}
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values())
    missing = [n for n, t in model.named_parameters() if t.grad is None or not torch.isfinite(t.grad).all()]
    assert not missing, missing
    t = model.dense_head.forward_ret_dict['target_dicts']
    assert t['heatmaps'][0].shape == (2, 3, 200, 176) and int(t['masks'][0].sum()) == int((batch['gt_boxes'][:, :, 7] > 0).sum())
    assert all(torch.isfinite(p).all() for p in model.parameters())
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = 0.0              # (random weights: keep whatever the NMS keeps)
    model.eval()
    with torch.no_grad(), no_fallback():
        pred, recall = model(_batch(dev))
    assert len(pred) == 2 and any(len(p['pred_scores']) > 0 for p in pred) and 'gt' in recall
    for p in pred:
        assert set(p) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_logits'}
        n = len(p['pred_scores'])
        assert n <= 500 and p['pred_boxes'].shape == (n, 7) and p['pred_labels'].shape == (n,) and p['pred_logits'].shape == (n, 3)
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())
        assert bool((p['pred_scores'][:-1] >= p['pred_scores'][1:]).all())               # one head: descending scores
        # the score of a box is the sigmoid of its class's logit at its cell
        own = p['pred_logits'].gather(1, (p['pred_labels'] - 1)[:, None])[:, 0]
        assert torch.allclose(own.sigmoid(), p['pred_scores'], atol=1e-6)


def _golden_detector(dev):
    """CenterPoint from centerpoint_cfg('kitti') with the golden's seeded state and the golden's SCORE_THRESH (tests/center_cases.py)"""
    from golden._constants import seeded_state
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import centerpoint_cfg
    from pcdet.models import build_network
    g = cpu.gold()
    cfg = centerpoint_cfg('kitti')
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = float(g['det_ev_score_thresh'][0])
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=cases.DET_POINTS))
    assert list(model.state_dict().keys()) == g['det_keys'].tolist()
    model.load_state_dict(cases.det_state(seeded_state(model, cases.DET_SEED)))
    return model.to(dev)


def _golden_batch(dev):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(cases.DET_FIRST_FRAME, 2, cases.DET_POINTS)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {'points': t(np.concatenate([bidx[:, None], pts], 1)), 'point_frame_offsets': t(off), 'batch_size': 2,
            'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': t(gt),
            'frame_id': np.array(['%06d' % (cases.DET_FIRST_FRAME + i) for i in range(2)])}


def _golden_step(dev):
    model = _golden_detector(dev).train()
    with no_fallback():
        ret, tb, _ = model(_golden_batch(dev))
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    params = dict(model.named_parameters())
    res = {'loss': ret['loss'].detach().double().reshape(1).cpu().numpy(),
           'tb_vals': np.array([float(tb[k].double()) for k in sorted(tb)])}
    for n, sl in cases.DET_GRADS.items():
        res['grad/' + n] = params[n].grad.double().cpu().numpy()[sl]
    return res, tb, model


def test_detector_step_matches_the_reference(dev):
    """the golden step of the reference's CenterPoint (two synthetic frames, seeded weights): loss, every tb_dict entry and three
    gradients within FACTOR * e_ref of its f64 run, e_ref = the larger error of its two f32 runs (NCHW and channels_last memory)"""
    g = cpu.gold()
    res, tb, model = _golden_step(dev)
    assert sorted(tb) == g['det_tb_keys'].tolist()
    assert int(model.dense_head.forward_ret_dict['target_dicts']['masks'][0].sum()) == int(g['det_objects'][0])
    bad = []
    for k, v in res.items():
        err, e_ref = np.abs(v - g['det_f64_' + k]).max(), g['det_e_ref_' + k][0]
        print('detector %-48s err %.3g e_ref %.3g (%.2f x) on values up to %.3g' % (k, err, e_ref, err / e_ref, np.abs(g['det_f64_' + k]).max()))
        if v.shape != g['det_f64_' + k].shape or not err <= cpu.FACTOR * e_ref:
            bad.append(k)
    assert not bad, bad


def test_eval_pred_dict_matches_the_reference(dev):
    """the eval pass on the same frames and weights: the boxes the reference's post-processing keeps (SCORE_THRESH from the golden, set
    between two well-separated picks), frame 0 value by value, the counts of both frames"""
    g = cpu.gold()
    model = _golden_detector(dev).eval()
    with torch.no_grad(), no_fallback():
        pred, recall = model(_golden_batch(dev))
    counts = [len(p['pred_scores']) for p in pred]
    print('eval boxes per frame', counts, 'golden', g['det_ev_counts'].tolist())
    assert counts == g['det_ev_counts'].tolist()
    p = pred[0]
    assert np.array_equal(p['pred_labels'].cpu().numpy(), g['det_ev_pred_labels'])
    for k in ('pred_boxes', 'pred_scores'):
        err, e_ref = np.abs(p[k].double().cpu().numpy() - g['det_ev_f64_' + k]).max(), g['det_ev_e_ref_' + k][0]
        print('eval %-12s err %.3g e_ref %.3g (%.2f x)' % (k, err, e_ref, err / e_ref))
        assert err <= cpu.FACTOR * e_ref, k
    own = p['pred_logits'].gather(1, (p['pred_labels'] - 1)[:, None])[:, 0]
    assert p['pred_logits'].shape == (counts[0], 3) and torch.allclose(own.sigmoid(), p['pred_scores'], atol=1e-6)


def test_fused_and_torch_route_give_the_same_losses(dev):
    """CRB_CENTER_FUSED = 1 against = 0 (crbhip.center_head.FUSED) on the golden step: loss and every tb_dict entry within the bars
    of the detector step (FACTOR * e_ref) of each other"""
    from crbhip import center_head as ch
    g = cpu.gold()
    res = {}
    for fused in (True, False):
        ch.FUSED = fused
        try:
            res[fused] = _golden_step(dev)[0]
        finally:
            ch.FUSED = True
    for k in ('loss', 'tb_vals'):
        d, e_ref = np.abs(res[True][k] - res[False][k]).max(), g['det_e_ref_' + k][0]
        print('%-8s fused %s torch route %s, difference %.3g, e_ref %.3g' % (k, res[True][k], res[False][k], d, e_ref))
        assert d <= cpu.FACTOR * e_ref, k


@pytest.mark.parametrize('method', ['entropy', 'random'])
def test_strategies_select_from_a_pool(dev, tmp_path, method):
    import random
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.query_strategies import build_strategy
    cfg, model = _detector(dev)
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': method, 'AGGREGATION': 'mean', 'SELECT_NUMS': 2})
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = 0.0
    pool = SyntheticDataset(num_frames=4, first_frame=300, n_points=POINTS)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS)
    strat = build_strategy(method, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 2), 0, str(tmp_path), cfg)
    random.seed(5)
    with no_fallback():
        picked = strat.query(cur_epoch=0)
    assert len(picked) == 2 and len(set(picked)) == 2 and set(picked) <= set(pool.sample_id_list), picked
