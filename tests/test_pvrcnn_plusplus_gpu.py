"""GPU: PVRCNNPlusPlus (proposals -> RoI sampling -> SPC keypoints -> point head -> RoI head) from pv_rcnn_plusplus_cfg.

The training step against tests/golden/ref_pvrcnn_plusplus.npz, written by the reference's own PVRCNNPlusPlus on the CPU
(tests/golden/make_goldens_spc.py): the golden's first-stage proposals and recorded RoI-sampler indices make the injected
roi_targets_dict, so the sampled rois are the reference's bit for bit and the SPC keypoints have to be too. Loss, tb_dict, second-stage
outputs, rois and gradients: the tolerances of tests/test_pvrcnn_gpu.py::test_train_step_matches_the_reference_detector for the same
quantities. Then: an eval pass on the full configuration with ragged frames, the random / entropy strategies, bit-reproducibility."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from synth import kitti_batch

pytestmark = pytest.mark.gpu

POINTS = 8000


def _golden_setup(dev):
    from golden._constants import PV_FIRST_FRAME, PV_KEYPOINTS, PV_KINDS, pv_seeded_state
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_pvrcnn_plusplus.npz'))
    n_points = PV_KINDS['kitti'][4]
    cfg = pv_rcnn_plusplus_cfg('kitti').MODEL
    cfg.PFE.NUM_KEYPOINTS = PV_KEYPOINTS
    cfg.POINT_HEAD.NUM_KEYPOINTS = PV_KEYPOINTS
    cfg.ROI_HEAD.DP_RATIO = 0.0
    torch.manual_seed(0)
    model = build_network(cfg, 3, SyntheticDataset(num_frames=2, n_points=n_points))
    assert type(model).__name__ == 'PVRCNNPlusPlus'
    assert sorted(model.state_dict().keys()) == list(G['pv_keys'])               # the reference's parameter / buffer names
    model.load_state_dict(pv_seeded_state(model))
    model.to(dev).train()
    pts, off, _ = kitti_batch(PV_FIRST_FRAME, 2, n_points)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))

    def batch():
        b = {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
             'batch_size': 2, 'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': torch.from_numpy(G['pv_gt']).to(dev),
             'frame_id': np.array(['%06d' % (PV_FIRST_FRAME + i) for i in range(2)])}
        # the reference's sampled RoIs: its proposals and its sampler's recorded draws through this head's assign_targets
        layer = model.roi_head.proposal_target_layer
        layer.injected_indices = torch.from_numpy(G['pv_sampled'])
        try:
            b['roi_targets_dict'] = model.roi_head.assign_targets({
                'batch_size': 2, 'gt_boxes': b['gt_boxes'], 'rois': torch.from_numpy(G['pv_proposals']).to(dev),
                'roi_scores': torch.from_numpy(G['pv_proposal_scores']).to(dev), 'roi_labels': torch.from_numpy(G['pv_proposal_labels']).to(dev)})
        finally:
            layer.injected_indices = None
        return b
    return G, model, batch


def test_train_step_matches_the_reference_detector(dev):
    from golden._constants import pv_grads
    G, model, batch = _golden_setup(dev)
    b = batch()
    np.testing.assert_array_equal(b['roi_targets_dict']['rois'].cpu().numpy(), G['pv_rois'])
    ret, tb, _ = model(b)
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    kp = b['point_coords'].cpu().numpy()
    print('keypoints per frame', np.bincount(kp[:, 0].astype(int)).tolist(), 'reference', np.bincount(G['pv_point_coords'][:, 0].astype(int)).tolist())
    np.testing.assert_array_equal(kp.view(np.int32), G['pv_point_coords'].view(np.int32))
    _rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    e_pf = _rel(b['point_features'].detach().cpu().numpy()[:, :32], G['pv_point_features'])
    e_ps = _rel(b['point_cls_scores'].detach().cpu().numpy(), G['pv_point_cls_scores'])
    print('point features %.2e, point scores %.2e, loss %.6f reference %.6f' % (e_pf, e_ps, float(ret['loss'].detach()), float(G['pv_loss'][0])))
    assert e_pf <= 1e-4 and e_ps <= 1e-5
    np.testing.assert_allclose(float(ret['loss'].detach()), float(G['pv_loss'][0]), rtol=2e-4)
    assert sorted(tb.keys()) == list(G['pv_tb_keys'])
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values())
    for k, want in zip(G['pv_tb_keys'], G['pv_tb_vals']):
        print('%-20s %.6f reference %.6f' % (k, float(tb[k]), want))
    for k, want in zip(G['pv_tb_keys'], G['pv_tb_vals']):
        np.testing.assert_allclose(float(tb[k]), want, rtol=2e-4, atol=2e-5, err_msg=str(k))
    for k, name in (('rcnn_cls', 'pv_rcnn_cls'), ('rcnn_reg', 'pv_rcnn_reg'), ('rcnn_cls_gt', 'pv_rcnn_cls_gt'), ('rcnn_reg_gt', 'pv_rcnn_reg_gt')):
        got, want = ret[k].detach().float().cpu().numpy().reshape(G[name].shape), G[name]
        assert np.abs(got - want).max() <= 2e-3 * max(1e-6, np.abs(want).max()), (k, np.abs(got - want).max(), np.abs(want).max())
    np.testing.assert_allclose(model.roi_head.forward_ret_dict['rois'].cpu().numpy(), G['pv_rois'], rtol=0, atol=2e-4)
    params = dict(model.named_parameters())
    worst = {}
    for n, sl in pv_grads('waymo').items():                                 # (two voxel-source SA layers, as the Waymo PV-RCNN)
        got, want = params[n].grad.cpu().numpy()[sl], G['pv_grad/' + n]
        worst[n] = float(np.abs(got - want).max()) / float(G['pv_gradmax/' + n][0])
        print('%-48s gradient error %.2e of its largest entry' % (n, worst[n]))
    assert all(e <= 2e-2 for e in worst.values()), worst


def test_training_step_is_bit_reproducible_under_deterministic_algorithms(dev):
    G, model, batch = _golden_setup(dev)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            model.load_state_dict(state)
            b = batch()
            ret, tb, _ = model(b)
            model.zero_grad(set_to_none=True)
            ret['loss'].backward()
            res.append((ret['loss'].detach().clone(), b['point_coords'].clone(), model.point_head.cls_layers[0].weight.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(False)
    for a, c in zip(*res):
        assert torch.equal(a, c)


def _ragged(dev, first, sizes):
    from pcdet.datasets.synthetic import kitti_frame
    frames = [kitti_frame(first + i, n) for i, n in enumerate(sizes)]
    pts = np.concatenate([f[0] for f in frames]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    gt = np.zeros((len(sizes), max(len(f[1]) for f in frames), 8), np.float32)
    for i, f in enumerate(frames):
        gt[i, :len(f[1])] = f[1]
    bidx = np.repeat(np.arange(len(sizes), dtype=np.float32), sizes)
    return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
            'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': len(sizes), 'point_frame_counts_host': list(sizes),
            'frame_id': np.array(['%06d' % (first + i) for i in range(len(sizes))])}


def test_eval_pass_on_the_full_configuration_with_ragged_frames(dev):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    from pcdet.models.detectors.post_processing import crb_frame_records
    from pcdet.query_strategies import scoring
    cfg = pv_rcnn_plusplus_cfg('kitti')
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS)).to(dev)
    # a training step with the model's own proposals and sampler first (train-mode statistics, every consumer counts the keypoints)
    model.train()
    b = _ragged(dev, 60, [6000, 9000])
    # (proposals on the ground truth, so that keypoints fall into boxes: a first stage with random weights proposes elsewhere)
    b.update(rois=b['gt_boxes'][:, :, :7].clone(), roi_scores=torch.ones_like(b['gt_boxes'][:, :, 0]), roi_labels=b['gt_boxes'][:, :, 7].long())
    ret, tb, _ = model(b)
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    assert torch.isfinite(ret['loss']) and b['rois'].shape == (2, 128, 7) and 'roi_targets_dict' in b
    # the frames have their own keypoint counts, and the point head labels every keypoint against ITS frame's boxes
    from pcdet.utils import box_utils
    kp, labels = b['point_coords'], model.point_head.forward_ret_dict['point_cls_labels']
    per_frame = torch.bincount(kp[:, 0].long(), minlength=2).tolist()
    assert per_frame[0] != per_frame[1] and per_frame == b['point_coords_counts_host'] and labels.shape == (kp.shape[0],)
    gt = b['gt_boxes']
    ext = box_utils.enlarge_box3d(gt.view(-1, 8), extra_width=cfg.MODEL.POINT_HEAD.TARGET_CONFIG.GT_EXTRA_WIDTH).view(2, -1, 8)
    for k in range(2):
        own = kp[kp[:, 0] == k].clone()
        own[:, 0] = 0
        want = model.point_head.assign_stack_targets(own, gt[k:k + 1], ext[k:k + 1])['point_cls_labels']
        assert torch.equal(labels[kp[:, 0] == k], want) and int((want != 0).sum()) > 0
    assert int((labels > 0).sum()) > 0
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    assert model.point_head.cls_layers[0].weight.grad.abs().sum() > 0
    assert any(p.grad is not None and p.grad.abs().sum() > 0 for p in model.pfe.parameters())
    model.eval()
    b = _ragged(dev, 60, [6000, 9000])
    model.pfe.prefetch_keypoints(b)                                          # SPC needs the rois: nothing starts early, nothing raises
    assert '_keypoints_prefetched' not in b and '_keypoints_prefetched' not in model.prefetch_sparse(dict(b))
    with torch.no_grad():
        pred, recall = model(dict(b))
        b = model.run_modules(b)
        rows = scoring.pack_records(crb_frame_records(model, b), scoring.RecordLayout.for_model(model))
    assert len(pred) == 2 and 'gt' in recall
    for p in pred:
        n = len(p['pred_scores'])
        assert p['pred_boxes'].shape == (n, 7) and p['pred_labels'].shape == (n,) and n <= 100
    kp = b['point_coords']
    per_frame = torch.bincount(kp[:, 0].long(), minlength=2).tolist()
    K, S = cfg.MODEL.PFE.NUM_KEYPOINTS, 6
    assert all(0 < m <= K + S for m in per_frame) and b['rois'].shape == (2, 100, 7)
    for k in range(2):                                                       # keypoints of frame k are points of frame k
        seg = b['points'][b['points'][:, 0] == k][:, 1:4]
        kk = kp[kp[:, 0] == k][:, 1:4]
        assert bool((kk[:64, None, :] == seg[None, :, :]).all(-1).any(1).all())
    assert rows.shape == (2, scoring.RecordLayout.for_model(model).stride) and torch.isfinite(rows).all()


@pytest.mark.parametrize('method', ['entropy', 'random'])
def test_strategies_select_from_a_pool(dev, tmp_path, method):
    import random
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    from pcdet.query_strategies import build_strategy
    cfg = pv_rcnn_plusplus_cfg('kitti')
    cfg.MODEL.PFE.NUM_KEYPOINTS = cfg.MODEL.POINT_HEAD.NUM_KEYPOINTS = 512
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS)).to(dev)
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': method, 'AGGREGATION': 'mean', 'SELECT_NUMS': 2})
    pool = SyntheticDataset(num_frames=4, first_frame=300, n_points=POINTS)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS)
    strat = build_strategy(method, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 2), 0, str(tmp_path), cfg)
    random.seed(5)
    picked = strat.query(cur_epoch=0)
    assert len(picked) == 2 and len(set(picked)) == 2 and set(picked) <= set(pool.sample_id_list), picked
