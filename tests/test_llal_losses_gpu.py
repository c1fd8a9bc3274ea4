"""GPU: the LLAL loss-net phase — the per-frame (reduce=False) RoI-head and point-head loss kernels against the torch expressions
(CRB_*_FUSED=0 paths) with a random (B,) upstream gradient, and one step of the mirror's LLAL PV-RCNN against
tests/golden/ref_pvrcnn_llal.npz (tests/golden/make_goldens_llal.py: the reference's own PVRCNN with ROI_HEAD.LOSS_NET)."""
import copy
import os

import numpy as np
import pytest
import torch

from synth import kitti_batch
from test_rcnn_loss_gpu import _case, _head

pytestmark = pytest.mark.gpu


def _rel(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp(min=1e-30))


def _run_frames(head, case, fused, g):
    from pcdet.models.roi_heads import roi_head_template as T
    T.FUSED_LOSS, keep = fused, T.FUSED_LOSS
    try:
        head.proposal_target_layer.forward = lambda batch_dict, uniforms=None: {
            'rois': case['rois'], 'gt_of_rois': case['gt_raw'].clone(), 'reg_valid_mask': case['reg_valid_mask'],
            'rcnn_cls_labels': case['rcnn_cls_labels']}
        targets = head.assign_targets({'batch_size': case['rois'].shape[0]})
        cls = case['rcnn_cls'].clone().requires_grad_(True)
        reg = case['rcnn_reg'].clone().requires_grad_(True)
        head.forward_ret_dict = dict(targets, rcnn_cls=cls, rcnn_reg=reg)
        loss, tb = head.get_loss(reduce=False)
        (loss * g).sum().backward()
        return loss.detach(), {k: v.detach().clone() for k, v in tb.items()}, cls.grad, reg.grad
    finally:
        T.FUSED_LOSS = keep


FRAME_CASES = [dict(B=16, P=128, seed=11), dict(B=4, P=100, seed=12, labels='hard'), dict(B=2, P=128, seed=13, fg='none'),
               dict(B=2, P=64, seed=14, labels='none'), dict(B=4, P=128, seed=15, frame0='no_fg')]


@pytest.mark.parametrize('case', FRAME_CASES, ids=lambda c: 'B%d_P%d_%s' % (c['B'], c['P'], '_'.join(k for k in c if k not in ('B', 'P', 'seed'))))
def test_per_frame_rcnn_loss_kernel_equals_the_torch_expressions(dev, case):
    """crb_rcnn_loss_per_frame + crb_scale_rows_per_frame against get_box_cls_layer_loss + get_box_reg_layer_loss with reduce=False:
    per-frame losses and tb entries 2e-6 relative, gradients 2e-5 of the largest entry — the yardsticks of the reduce=True kernel,
    whose per-RoI arithmetic it shares; frames without a foreground RoI and all-ignored labels included; bit-equal re-run"""
    case = dict(case)
    frame0 = case.pop('frame0', None)
    head = _head(dev)
    c = _case(dev, **case)
    if frame0 == 'no_fg':
        c['reg_valid_mask'][0] = 0
    g = torch.from_numpy(np.random.default_rng(case['seed']).normal(0, 1, case['B']).astype(np.float32)).to(dev)
    loss_f, tb_f, gc_f, gr_f = _run_frames(head, c, True, g)
    loss_t, tb_t, gc_t, gr_t = _run_frames(head, c, False, g)
    assert loss_f.shape == loss_t.shape == (case['B'],)
    assert _rel(loss_f, loss_t) <= 2e-6, (loss_f, loss_t)
    assert set(tb_f) == set(tb_t)
    for k in tb_t:
        torch.testing.assert_close(tb_f[k], tb_t[k], rtol=2e-6, atol=1e-7, msg=lambda m, k=k: k + ': ' + m)
    for gf, gt, what in ((gc_f, gc_t, 'd rcnn_cls'), (gr_f, gr_t, 'd rcnn_reg')):
        assert gf.shape == gt.shape and torch.isfinite(gf).all()
        assert float((gf - gt).abs().max()) <= 2e-5 * max(float(gt.abs().max()), 1e-6), what
    loss_2, _, gc_2, gr_2 = _run_frames(head, c, True, g)
    assert torch.equal(loss_f, loss_2) and torch.equal(gc_f, gc_2) and torch.equal(gr_f, gr_2)


@pytest.mark.parametrize('num_class,B,M,mode', [(1, 16, 2048, 'mixed'), (1, 3, 333, 'mixed'), (1, 2, 2048, 'no_positive'),
                                                (1, 4, 256, 'ignored'), (3, 2, 333, 'mixed')])
def test_per_frame_point_focal_loss_kernel_equals_the_torch_expressions(dev, num_class, B, M, mode):
    """crb_point_focal_loss_per_frame against get_cls_layer_loss(reduce=False) (batch-wide positive normaliser, per-frame sums):
    losses 2e-6 relative, positives equal, gradient 2e-5 of its largest entry, random (B,) upstream, bit-equal re-run. With more than
    one class the reference's view(-1, NUM_KEYPOINTS) of the (n, classes) terms is not a per-frame sum (B * classes entries): that
    configuration keeps the torch expression, and both runs are the same"""
    from pcdet.model_cfgs import pv_rcnn_cfg
    from pcdet.models.dense_heads import point_head_template as PT
    from pcdet.models.dense_heads.point_head_simple import PointHeadSimple
    cfg = copy.deepcopy(pv_rcnn_cfg().MODEL.POINT_HEAD)
    cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_cls_weight'] = 0.7
    cfg.NUM_KEYPOINTS = M
    head = PointHeadSimple(num_class=num_class, input_channels=32, model_cfg=cfg).to(dev).train()
    rng = np.random.default_rng(B * 100 + M)
    n = B * M
    labels = rng.integers(0, num_class + 1, n)
    labels[rng.uniform(0, 1, n) < 0.3] = -1
    if mode == 'no_positive':
        labels[labels > 0] = 0
    if mode == 'ignored':
        labels[:M] = -1                                     # frame 0: every label ignored
    labels = torch.from_numpy(labels.astype(np.int64)).to(dev)
    preds = torch.from_numpy(rng.normal(0, 2, (n, num_class)).astype(np.float32)).to(dev)
    preds[::7] = 40.0
    g = torch.from_numpy(rng.normal(0, 1, B * num_class).astype(np.float32)).to(dev)
    out = []
    keep = PT.FUSED
    try:
        for fused in (True, False, True):
            PT.FUSED = fused
            p = preds.clone().requires_grad_(True)
            head.forward_ret_dict = {'point_cls_preds': p, 'point_cls_labels': labels}
            loss, tb = head.get_loss(reduce=False)
            (loss * g).sum().backward()
            out.append((loss.detach(), tb['point_pos_num'].detach().clone(), tb['point_loss_cls'].clone(), p.grad))
    finally:
        PT.FUSED = keep
    f, t, f2 = out
    assert f[0].shape == t[0].shape == (B * num_class,)
    assert _rel(f[0], t[0]) <= 2e-6
    assert float(f[1]) == float(t[1])
    torch.testing.assert_close(f[2], t[2], rtol=2e-6, atol=1e-7)
    assert float((f[3] - t[3]).abs().max()) <= 2e-5 * max(float(t[3].abs().max()), 1e-9)
    assert torch.equal(f[0], f2[0]) and torch.equal(f[3], f2[3])


def test_llal_step_matches_the_reference_detector(dev):
    """ONE loss-net-phase step (lal_flag on) and ONE frozen step of the mirror's LLAL PV-RCNN against ref_pvrcnn_llal.npz: the
    reference's PVRCNN with ROI_HEAD.LOSS_NET (pv_rcnn.py:29-43, pvrcnn_head.py:163-180, loss_net.py) on the two frames and seeded
    weights of ref_pvrcnn_detector.npz, its recorded RoI-sampler draws injected (256 keypoints, DP_RATIO 0, as there).
    Tolerances of test_train_step_matches_the_reference_detector: loss, per-frame losses and tb_dict 2e-4, detector gradients 2e-2
    of their largest entry; loss-net outputs (predictions, ranking loss, eval predictions, running statistics) and gradients 2e-4."""
    from golden._constants import PV_FIRST_FRAME, PV_KEYPOINTS, PV_KINDS, pv_grads, pv_seeded_state
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_llal_cfg
    from pcdet.models import build_network
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_pvrcnn_llal.npz'))
    cfg = pv_rcnn_llal_cfg().MODEL
    cfg.PFE.NUM_KEYPOINTS = PV_KEYPOINTS
    cfg.POINT_HEAD.NUM_KEYPOINTS = PV_KEYPOINTS
    cfg.ROI_HEAD.DP_RATIO = 0.0
    torch.manual_seed(0)
    n_points = PV_KINDS['kitti'][4]
    model = build_network(cfg, 3, SyntheticDataset(num_frames=2, kind='kitti', n_points=n_points))
    assert sorted(model.state_dict().keys()) == list(G['pv_keys'])
    seeded = pv_seeded_state(model)
    pts, off, _ = kitti_batch(PV_FIRST_FRAME, 2, n_points)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    ref_sampled = torch.from_numpy(np.take_along_axis(G['pv_proposals'], G['pv_sampled'][:, :, None], axis=1))

    def step(frozen):
        model.load_state_dict(seeded)
        model.to(dev).train()
        for p in model.roi_head.loss_net.parameters():
            p.requires_grad_(not frozen)
        model.roi_head.proposal_target_layer.injected_rois = ref_sampled
        b = {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
             'batch_size': 2, 'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': torch.from_numpy(G['pv_gt']).to(dev),
             'frame_id': np.array(['%06d' % (PV_FIRST_FRAME + i) for i in range(2)])}
        rec = {}
        heads = ((model.dense_head, 'rpn'), (model.point_head, 'point'), (model.roi_head, 'rcnn'))
        origs = [h.get_loss for h, _ in heads]
        ln = model.roi_head.loss_net

        def wrap(fn, key):
            def w(*a, **k):
                r = fn(*a, **k)
                rec[key] = r[0].detach().clone()
                return r
            return w
        for (h, key), fn in zip(heads, origs):
            h.get_loss = wrap(fn, key)
        orig_ln = ln.forward
        ln.forward = lambda features, batch_size=None: (rec.__setitem__('latents', [f.detach() for f in features]),
                                                        orig_ln(features, batch_size=batch_size))[1]
        try:
            ret, tb, _ = model(b)
            model.zero_grad(set_to_none=True)
            ret['loss'].backward()
        finally:
            for h, _ in heads:
                del h.get_loss
            del ln.forward
        torch.cuda.synchronize()
        return ret, tb, rec

    ret, tb, rec = step(False)
    head = model.roi_head
    np.testing.assert_allclose(float(ret['loss'].detach()), float(G['pv_loss'][0]), rtol=2e-4)
    assert sorted(tb.keys()) == list(G['pv_tb_keys'])
    for k, want in zip(G['pv_tb_keys'], G['pv_tb_vals']):
        np.testing.assert_allclose(float(tb[k]), want, rtol=2e-4, atol=2e-5, err_msg=str(k))
    for key in ('rpn', 'point', 'rcnn'):
        assert rec[key].shape == (2,), key
        np.testing.assert_allclose(rec[key].cpu().numpy(), G['llal/loss_' + key], rtol=2e-4, err_msg=key)
    assert _rel(head.forward_ret_dict['loss_predictions'], G['llal/pred']) <= 2e-4
    np.testing.assert_allclose(float(tb['loss_loss_net']), float(G['llal/loss_loss_net'][0]), rtol=2e-4)
    params = dict(model.named_parameters())
    for n, sl in pv_grads('kitti').items():
        got, want = params[n].grad.cpu().numpy()[sl], G['pv_grad/' + n]
        assert np.abs(got - want).max() <= 2e-2 * float(G['pv_gradmax/' + n][0]), n
    for n, p in head.loss_net.named_parameters():
        want = G['llal/grad/' + n]
        if np.abs(want).max() == 0:                       # the linear bias: the pair difference cancels it
            assert float(p.grad.abs().max()) == 0.0, n
        else:
            assert _rel(p.grad, want) <= 2e-4, (n, _rel(p.grad, want))
    for k in range(2):
        bn = getattr(head.loss_net, 'bn_%d' % k)
        assert _rel(bn.running_mean, G['llal/after/running_mean_%d' % k]) <= 2e-4
        assert _rel(bn.running_var, G['llal/after/running_var_%d' % k]) <= 2e-4
    head.loss_net.eval()
    with torch.no_grad():
        assert _rel(head.loss_net(rec['latents'], batch_size=2), G['llal/eval_pred']) <= 2e-4
    head.loss_net.train()

    ret, tb, rec = step(True)
    np.testing.assert_allclose(float(ret['loss'].detach()), float(G['frozen/loss'][0]), rtol=2e-4)
    assert sorted(tb.keys()) == list(G['frozen/tb_keys'])
    for k in range(2):
        bn = getattr(head.loss_net, 'bn_%d' % k)
        assert _rel(bn.running_mean, G['frozen/running_mean_%d' % k]) <= 2e-4
        assert _rel(bn.running_var, G['frozen/running_var_%d' % k]) <= 2e-4
