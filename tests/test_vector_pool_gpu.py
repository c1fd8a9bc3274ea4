"""GPU: VectorPool aggregation (csrc/vector_pool.hip).

Index outputs bit-equal to the numpy restatements of the reference kernels (tests/vector_pool_cases.py) on every cell of every case;
on the lattice cases the distances too. The interpolation against its f64 definition, bounded by the torch route's own error. The
module step against tests/golden/ref_vector_pool.npz and the detector step against tests/golden/ref_pvrcnn_plusplus_vp.npz (the
reference's own module and PVRCNNPlusPlus on the CPU, tests/golden/make_goldens_vector_pool.py) with the tolerances of
tests/test_pvrcnn_plusplus_gpu.py::test_train_step_matches_the_reference_detector for the same kinds of quantity. An eval pass with
ragged frames on the full configuration; bit-reproducibility."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_pool_cases as vc
from synth import kitti_batch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = 8000
_gold = {}
t = torch.from_numpy


def gold():
    if not _gold:
        _gold.update(np.load(os.path.join(HERE, 'golden', 'ref_vector_pool.npz')))
    return _gold


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _three_nn(c, dev):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    dist, idx, _ = pu.three_nn_for_vector_pool_by_two_step(
        t(c['support']).to(dev), t(c['xyz_cnt']).to(dev), t(c['new_xyz']).to(dev), t(c['centers']).to(dev), t(c['new_cnt']).to(dev), c['R'],
        c['nsample'], c['ntype'], 1000, c['centers'].shape[1], c['mult'])
    return idx, dist


@pytest.mark.parametrize('name', sorted(vc.three_nn_cases()))
def test_three_nn_is_bit_equal_to_the_restatement(dev, name):
    c = vc.three_nn_cases()[name]
    want_idx, want_dist, _ = vc.three_nn(c['support'], c['xyz_cnt'], c['new_xyz'], c['new_cnt'], c['centers'], c['R'] * c['mult'], c['nsample'],
                                         c['ntype'])
    idx, dist = _three_nn(c, dev)
    torch.cuda.synchronize()
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert idx.dtype == np.int32 and idx.shape == want_idx.shape == dist.shape
    differ = int((bits(dist) != bits(want_dist)).sum())
    print(name, 'cells', idx.shape[0] * idx.shape[1], 'index mismatches', int((idx != want_idx).sum()), 'distance bit mismatches', differ)
    assert np.array_equal(idx, want_idx)                                     # every cell of every case
    assert np.array_equal(np.isposinf(dist), want_idx < 0)
    if name.startswith('lattice'):
        assert differ == 0
    else:                                                                    # sqrtf of bit-equal squares: one ulp for the root
        fin = np.isfinite(want_dist)
        assert (np.abs(dist[fin] - want_dist[fin]) <= np.spacing(want_dist[fin])).all()


@pytest.mark.parametrize('name', sorted(vc.voxel_cases()))
def test_voxel_pool_is_bit_equal_to_the_restatement(dev, name):
    from crbhip import vector_pool
    c = vc.voxel_cases()[name]
    f, l, cnt, pick = vc.voxel_pool(c['support'], c['xyz_cnt'], c['feats'], c['new_xyz'], c['new_cnt'], c['grid'], c['R'], c['nsample'], c['ntype'])
    probe = gold()['voxel/%s/probe' % name]
    grads = []
    for _ in range(2):
        feats = t(c['feats']).to(dev).requires_grad_(True)
        f2, l2, cnt2, pick2 = vector_pool.voxel_pool(feats, t(c['support']).to(dev), t(c['xyz_cnt']).to(dev), t(c['new_xyz']).to(dev),
                                                     t(c['new_cnt']).to(dev), c['grid'], c['R'], c['nsample'], c['ntype'])
        (f2 * t(probe).to(dev)).sum().backward()
        grads.append(feats.grad.clone())
    torch.cuda.synchronize()
    assert np.array_equal(pick2.cpu().numpy(), pick) and np.array_equal(cnt2.cpu().numpy(), cnt)
    assert np.array_equal(bits(f2.detach().cpu().numpy()), bits(f)) and np.array_equal(bits(l2.cpu().numpy()), bits(l))
    assert np.array_equal(bits(grads[0].cpu().numpy()), bits(vc.voxel_pool_grad(probe, pick, len(c['support']))))
    assert torch.equal(grads[0], grads[1])
    # the op with the reference's argument list returns the same, and the value it was handed
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    f3, l3, mean, cnt3 = pu.vector_pool_with_voxel_query_op(t(c['support']).to(dev), t(c['xyz_cnt']).to(dev), t(c['feats']).to(dev),
                                                           t(c['new_xyz']).to(dev), t(c['new_cnt']).to(dev), *c['grid'], c['R'],
                                                           c['feats'].shape[1], 1, 20, c['nsample'], c['ntype'], 1)
    assert torch.equal(f3, f2.detach()) and torch.equal(l3, l2) and torch.equal(cnt3, cnt2) and mean.tolist() == [20]


INTERP_CASES = ('frames_333_a', 'frames_222_b', 'frames_123_b', 'count_2', 'lattice_cube', 'n_zero')


@pytest.mark.parametrize('name', INTERP_CASES)
def test_interpolation_against_f64(dev, name):
    """forward and backward of the fused kernel against the f64 definition. e_ref = the torch route's own error against f64 on the
    same inputs; the kernel may err by 4 e_ref (another association of the three-term sums), and never needs to be better than one
    f32 ulp of the largest entry."""
    from crbhip import vector_pool
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules import VectorPoolLocalInterpolateModule
    c = vc.three_nn_cases()[name]
    rng = np.random.default_rng(11)
    N, C = len(c['support']), 5
    M, G = c['centers'].shape[:2]
    feats = rng.normal(0, 1, (N, C)).astype(np.float32)
    probe = rng.normal(0, 1, (M, G, C + 9)).astype(np.float32)
    idx, dist = _three_nn(c, dev)
    sup, cen = t(c['support']).to(dev), t(c['centers']).to(dev)
    want = vc.interp_f64(idx.cpu().numpy(), dist.cpu().numpy(), c['centers'], c['support'], feats)
    want_grad = vc.interp_grad_f64(idx.cpu().numpy(), dist.cpu().numpy(), probe, N)
    runs = []
    for _ in range(2):
        f = t(feats).to(dev).requires_grad_(True)
        out = vector_pool.interpolate(f, idx, dist, cen, sup)                 # (G, M, C + 9)
        (out * t(probe).to(dev).permute(1, 0, 2)).sum().backward()
        runs.append((out.detach().permute(1, 0, 2).contiguous(), f.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    mod = VectorPoolLocalInterpolateModule(None, c['grid'], c['R'], c['nsample'], c['ntype'], neighbour_distance_multiplier=c['mult'])
    f = t(feats).to(dev).requires_grad_(True)
    ref = mod(sup, f, t(c['xyz_cnt']).to(dev), t(c['new_xyz']).to(dev), cen, t(c['new_cnt']).to(dev)).view(M, G, C + 9)
    if N:                                                                    # (no support rows: nothing to differentiate)
        (ref * t(probe).to(dev)).sum().backward()
    ref_grad = f.grad if N else torch.zeros_like(f)
    torch.cuda.synchronize()
    for what, got, torch_route, w in (('forward', runs[0][0], ref.detach(), want), ('backward', runs[0][1], ref_grad, want_grad)):
        e_k = float(np.abs(got.cpu().numpy() - w).max()) if w.size else 0.0
        e_ref = float(np.abs(torch_route.cpu().numpy() - w).max()) if w.size else 0.0
        floor = float(np.spacing(np.float32(np.abs(w).max()))) if w.size else 0.0
        print('%s %s: kernel error %.3e, torch route %.3e, ratio %.2f, one ulp of the largest entry %.3e' %
              (name, what, e_k, e_ref, e_k / e_ref if e_ref else float('nan'), floor))
        assert e_k <= max(4 * e_ref, floor)
    empty = idx[:, :, 0].cpu().numpy() < 0
    assert not runs[0][0].cpu().numpy()[empty].any()                         # empty cells are zeros (N = 0 included)


@pytest.mark.parametrize('name', sorted(vc.module_cfgs()))
def test_module_step_matches_the_reference_module(dev, name, monkeypatch):
    """train and eval against the golden: outputs and running statistics at 1e-4 of the largest entry (the detector test's bound for
    the keypoint features these layers produce), gradients at 2e-2 of their largest entry; both routes"""
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    assert pm.VECTOR_POOL_FUSED
    print('fused route')
    vc.check_module(name, gold(), vc.run_module(name, gold(), dev), 1e-4, 2e-2)
    monkeypatch.setattr(pm, 'VECTOR_POOL_FUSED', False)
    print('torch route')
    vc.check_module(name, gold(), vc.run_module(name, gold(), dev), 1e-4, 2e-2)


def _golden_setup(dev):
    from golden._constants import PV_FIRST_FRAME, PV_KEYPOINTS, PV_KINDS, pv_seeded_state
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    G = np.load(os.path.join(HERE, 'golden', 'ref_pvrcnn_plusplus_vp.npz'))
    n_points = PV_KINDS['kitti'][4]
    cfg = pv_rcnn_plusplus_cfg('kitti', aggregation='vector_pool').MODEL
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
        b = {'points': t(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': t(off).to(dev),
             'batch_size': 2, 'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': t(G['pv_gt']).to(dev),
             'frame_id': np.array(['%06d' % (PV_FIRST_FRAME + i) for i in range(2)])}
        layer = model.roi_head.proposal_target_layer                          # the reference's sampled RoIs, as in test_pvrcnn_plusplus_gpu.py
        layer.injected_indices = t(G['pv_sampled'])
        try:
            b['roi_targets_dict'] = model.roi_head.assign_targets({
                'batch_size': 2, 'gt_boxes': b['gt_boxes'], 'rois': t(G['pv_proposals']).to(dev),
                'roi_scores': t(G['pv_proposal_scores']).to(dev), 'roi_labels': t(G['pv_proposal_labels']).to(dev)})
        finally:
            layer.injected_indices = None
        return b
    return G, model, batch


def test_train_step_matches_the_reference_detector(dev):
    G, model, batch = _golden_setup(dev)
    b = batch()
    np.testing.assert_array_equal(b['roi_targets_dict']['rois'].cpu().numpy(), G['pv_rois'])
    ret, tb, _ = model(b)
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    kp = b['point_coords'].cpu().numpy()
    np.testing.assert_array_equal(kp.view(np.int32), G['pv_point_coords'].view(np.int32))
    _rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    e_pf = _rel(b['point_features'].detach().cpu().numpy()[:, :32], G['pv_point_features'])
    e_ps = _rel(b['point_cls_scores'].detach().cpu().numpy(), G['pv_point_cls_scores'])
    print('point features %.2e, point scores %.2e, loss %.6f reference %.6f' % (e_pf, e_ps, float(ret['loss'].detach()), float(G['pv_loss'][0])))
    assert e_pf <= 1e-4 and e_ps <= 1e-5
    np.testing.assert_allclose(float(ret['loss'].detach()), float(G['pv_loss'][0]), rtol=2e-4)
    assert sorted(tb.keys()) == list(G['pv_tb_keys'])
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
    for n, sl in vc.VP_GRADS.items():
        got, want = params[n].grad.cpu().numpy()[sl], G['pv_grad/' + n]
        worst[n] = float(np.abs(got - want).max()) / float(G['pv_gradmax/' + n][0])
        print('%-82s gradient error %.2e of its largest entry' % (n, worst[n]))
    assert sum('separate_local_aggregation_layer' in n for n in worst) == 2 and sum('msg_post_mlps' in n for n in worst) == 2
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
            res.append((ret['loss'].detach().clone(), b['point_features'].detach().clone(),
                        model.pfe.SA_layers[1].layer_0.separate_local_aggregation_layer[0].weight.grad.clone(),
                        model.roi_head.roi_grid_pool_layer.layer_1.post_mlps[0].weight.grad.clone(),
                        model.backbone_3d.conv_input[0].weight.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(False)
    for a, c in zip(*res):
        assert torch.equal(a, c)


def test_eval_pass_on_the_full_configuration_with_ragged_frames(dev):
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_frame
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    sizes = [6000, 9000]
    frames = [kitti_frame(60 + i, n) for i, n in enumerate(sizes)]
    pts = np.concatenate([f[0] for f in frames]).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    bidx = np.repeat(np.arange(2, dtype=np.float32), sizes)
    b = {'points': t(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': t(off).to(dev), 'batch_size': 2,
         'point_frame_counts_host': list(sizes), 'frame_id': np.array(['%06d' % (60 + i) for i in range(2)])}
    cfg = pv_rcnn_plusplus_cfg('kitti', aggregation='vector_pool')
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS)).to(dev)
    model.eval()
    with torch.no_grad():
        pred, _ = model(dict(b))
        b = model.run_modules(b)
    torch.cuda.synchronize()
    assert len(pred) == 2
    for p in pred:
        n = len(p['pred_scores'])
        assert p['pred_boxes'].shape == (n, 7) and p['pred_labels'].shape == (n,) and n <= 100
        assert torch.isfinite(p['pred_boxes']).all() and torch.isfinite(p['pred_scores']).all()
    per_frame = torch.bincount(b['point_coords'][:, 0].long(), minlength=2).tolist()
    assert all(m > 0 for m in per_frame) and b['rois'].shape == (2, 100, 7)
    assert torch.isfinite(b['point_features']).all() and torch.isfinite(b['batch_cls_preds']).all() and torch.isfinite(b['batch_box_preds']).all()
