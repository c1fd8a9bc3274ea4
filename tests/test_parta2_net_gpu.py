"""GPU: PartA2Net end to end on synthetic KITTI frames - a training step with the model's own proposals and sampler and an eval pass on
ragged frames (pred dicts and the CRB record), the random / entropy strategies and bit-reproducibility of the training step.

The training step against tests/golden/ref_parta2_net.npz, written by the reference's own PartA2Net on the CPU
(tests/golden/make_goldens_parta2_net.py): the golden's first-stage proposals and recorded RoI-sampler draws make the injected
roi_targets_dict. Bars: the project's for the same quantities in tests/test_pvrcnn_gpu.py::test_train_step_matches_the_reference_detector.

In the other tests the RoI head is the yaml's except for a 6^3 RoI grid (parta2_net_cfg's 12^3 grid gives a 57 M-parameter first FC layer;
every code path is the same): tests stay quick."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roiaware_cases  # noqa: E402
from synth import kitti_batch  # noqa: E402

pytestmark = pytest.mark.gpu
POINTS = 12000


def test_train_step_matches_the_reference_detector(dev):
    from golden._constants import PV_FIRST_FRAME, PV_KINDS, pv_seeded_state
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import parta2_net_cfg
    from pcdet.models import build_network
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_parta2_net.npz'))
    n_points = PV_KINDS['kitti'][4]
    cfg = parta2_net_cfg('kitti').MODEL
    cfg.ROI_HEAD.DP_RATIO = 0.0
    torch.manual_seed(0)
    model = build_network(cfg, 3, SyntheticDataset(num_frames=2, n_points=n_points))
    assert sorted(model.state_dict().keys()) == list(G['keys'])
    sd = pv_seeded_state(model)
    sd.update({k[len('bias/'):]: torch.from_numpy(G[k]) for k in G.files if k.startswith('bias/')})     # the generator's kink / mask margins
    model.load_state_dict(sd)
    model.to(dev).train()
    pts, off, _ = kitti_batch(PV_FIRST_FRAME, 2, n_points)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    b = {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
         'batch_size': 2, 'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': torch.from_numpy(G['gt']).to(dev),
         'frame_id': np.array(['%06d' % (PV_FIRST_FRAME + i) for i in range(2)])}
    layer = model.roi_head.proposal_target_layer
    layer.injected_indices = torch.from_numpy(G['sampled'])
    try:
        b['roi_targets_dict'] = model.roi_head.assign_targets({
            'batch_size': 2, 'gt_boxes': b['gt_boxes'], 'rois': torch.from_numpy(G['proposals']).to(dev),
            'roi_scores': torch.from_numpy(G['proposal_scores']).to(dev), 'roi_labels': torch.from_numpy(G['proposal_labels']).to(dev)})
    finally:
        layer.injected_indices = None
    np.testing.assert_array_equal(b['roi_targets_dict']['rois'].cpu().numpy(), G['rois'])                # sampled rois: exact
    ret, tb, _ = model(b)
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    # the voxel centres are the reference's; rows are matched by position (the voxel generators need not agree on the row order)
    pc = b['point_coords'].cpu().numpy()
    mine, ref = np.lexsort(pc.T[::-1]), np.lexsort(G['point_coords'].T[::-1])
    np.testing.assert_array_equal(pc[mine], G['point_coords'][ref])
    _rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    e_s = _rel(b['point_cls_scores'].detach().cpu().numpy().reshape(-1)[mine], G['point_cls_scores'].reshape(-1)[ref])
    e_o = _rel(b['point_part_offset'].detach().cpu().numpy()[mine], G['point_part_offset'][ref])
    print('point scores %.2e, part offsets %.2e, rows %d reference %d, loss %.6f reference %.6f' % (
        e_s, e_o, b['roi_grid_coords'].shape[0], len(G['coords']), float(ret['loss'].detach()), float(G['loss'][0])))
    np.testing.assert_array_equal(b['roi_grid_coords'].cpu().numpy(), G['coords'])                          # RoI-grid coords: exact
    assert e_s <= 1e-5 and e_o <= 1e-5
    for k, want in zip(G['tb_keys'], G['tb_vals']):
        print('%-20s %.6f reference %.6f' % (k, float(tb[k]), want))
    np.testing.assert_allclose(float(ret['loss'].detach()), float(G['loss'][0]), rtol=2e-4)
    assert sorted(tb.keys()) == list(G['tb_keys'])
    for k, want in zip(G['tb_keys'], G['tb_vals']):
        np.testing.assert_allclose(float(tb[k]), want, rtol=2e-4, atol=2e-5, err_msg=str(k))
    fr = model.roi_head.forward_ret_dict
    for k in ('rcnn_cls', 'rcnn_reg'):
        got, want = fr[k].detach().float().cpu().numpy().reshape(G[k].shape), G[k]
        print('%s error %.2e of its largest entry' % (k, np.abs(got - want).max() / np.abs(want).max()))
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max(), k
    params = dict(model.named_parameters())
    worst = {}
    for n, sl in roiaware_cases.PA2_GRADS.items():
        got, want = params[n].grad.cpu().numpy()[sl], G['grad/' + n]
        worst[n] = float(np.abs(got - want).max()) / float(G['gradmax/' + n][0])
        print('%-44s gradient error %.2e of its largest entry' % (n, worst[n]))
    assert all(e <= 2e-2 for e in worst.values()), worst


def _cfg():
    from pcdet.model_cfgs import parta2_net_cfg
    cfg = parta2_net_cfg('kitti')
    cfg.MODEL.ROI_HEAD.ROI_AWARE_POOL.POOL_SIZE = 6
    cfg.MODEL.ROI_HEAD.DP_RATIO = 0.0
    return cfg


def _model(dev, cfg):
    from pcdet.datasets import SyntheticDataset
    from pcdet.models import build_network
    torch.manual_seed(0)
    return build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS)).to(dev)


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


def _train_batch(dev):
    """proposals on the ground truth, so that the RoI grids hold points: a first stage with random weights proposes elsewhere"""
    b = _ragged(dev, 60, [6000, 9000])
    b.update(rois=b['gt_boxes'][:, :, :7].clone(), roi_scores=torch.ones_like(b['gt_boxes'][:, :, 0]), roi_labels=b['gt_boxes'][:, :, 7].long())
    return b


def _step(model, dev, seed=5):
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    b = _train_batch(dev)
    ret, tb, _ = model(b)
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    return ret, tb, b


def test_training_step_and_eval_pass_on_ragged_frames(dev):
    from pcdet.models.detectors.post_processing import crb_frame_records
    from pcdet.query_strategies import scoring
    model = _model(dev, _cfg())
    model.train()
    ret, tb, b = _step(model, dev)
    assert torch.isfinite(ret['loss']) and b['rois'].shape == (2, 128, 7)
    for k in ('rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'point_loss_cls', 'point_loss_part', 'point_pos_num',
              'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss'):
        assert k in tb and np.isfinite(float(tb[k])), k
    total = float(tb['rpn_loss']) + float(tb['point_loss_cls']) + float(tb['point_loss_part']) + float(tb['rcnn_loss'])
    assert abs(float(ret['loss'].detach()) - total) <= 1e-4 * max(1.0, abs(total))
    coords = b['roi_grid_coords']
    assert coords.shape[0] > 100 and int(coords[:, 0].max()) < 2 * 128 and int(coords[:, 1:].max()) < 6
    assert int(tb['point_pos_num']) > 0
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert all(torch.isfinite(g).all() for g in grads.values() if g is not None)
    for n in ('backbone_3d.conv_input.0.weight', 'point_head.cls_layers.0.weight', 'point_head.part_reg_layers.0.weight',
              'roi_head.conv_part.0.0.weight', 'roi_head.conv_rpn.0.0.weight', 'roi_head.shared_fc_layer.0.weight'):
        assert grads[n] is not None and float(grads[n].abs().sum()) > 0, n
    for prefix in ('backbone_2d.', 'dense_head.', 'roi_head.reg_layers.', 'roi_head.cls_layers.'):
        assert any(g is not None and float(g.abs().sum()) > 0 for n, g in grads.items() if n.startswith(prefix)), prefix
    # an injected RoI sample (as PVRCNNHead takes it) replaces the head's own target assignment: same RoIs, same RoI grids
    tgt = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in model.roi_head.forward_ret_dict.items()
           if k not in ('rcnn_cls', 'rcnn_reg')}
    b2 = _train_batch(dev)
    b2['roi_targets_dict'] = tgt
    model.roi_head.assign_targets = None                         # must not be reached
    try:
        ret2, _, _ = model(b2)
    finally:
        del model.roi_head.assign_targets
    assert torch.equal(b2['rois'], b['rois']) and torch.equal(b2['roi_grid_coords'], coords) and torch.isfinite(ret2['loss'])
    model.eval()
    b = _ragged(dev, 60, [6000, 9000])
    with torch.no_grad():
        pred, recall = model(dict(b))
        b = model.run_modules(b)
        rows = scoring.pack_records(crb_frame_records(model, b), scoring.RecordLayout.for_model(model))
    assert len(pred) == 2 and 'gt' in recall and b['rois'].shape == (2, 100, 7)
    for p in pred:
        n = len(p['pred_scores'])
        assert p['pred_boxes'].shape == (n, 7) and p['pred_labels'].shape == (n,) and n <= 100
    assert scoring.RecordLayout.for_model(model) == scoring.RecordLayout(100, 3)
    assert rows.shape == (2, scoring.RecordLayout(100, 3).stride) and torch.isfinite(rows).all()


@pytest.mark.parametrize('method', ['entropy', 'random'])
def test_strategies_select_from_a_pool(dev, tmp_path, method):
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.query_strategies import build_strategy
    cfg = _cfg()
    model = _model(dev, cfg)
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': method, 'AGGREGATION': 'mean', 'SELECT_NUMS': 2})
    pool = SyntheticDataset(num_frames=4, first_frame=300, n_points=POINTS)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS)
    strat = build_strategy(method, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 2), 0, str(tmp_path), cfg)
    random.seed(5)
    picked = strat.query(cur_epoch=0)
    assert len(picked) == 2 and len(set(picked)) == 2 and set(picked) <= set(pool.sample_id_list), picked


def test_training_step_is_bit_reproducible_under_deterministic_algorithms(dev):
    model = _model(dev, _cfg())
    model.train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            model.load_state_dict(state)
            ret, tb, b = _step(model, dev)
            res.append((ret['loss'].detach().clone(), b['roi_grid_coords'].clone(), model.point_head.cls_layers[0].weight.grad.clone(),
                        model.point_head.part_reg_layers[0].weight.grad.clone(), model.backbone_3d.conv_input[0].weight.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(False)
    assert float(res[0][4].abs().sum()) > 0
    for a, c in zip(*res):
        assert torch.equal(a, c)


def test_subm_16_to_64_is_the_sum_of_products_of_a_wider_instance(dev):
    """UNetV2 hands the RoI head 16 point features and the gather-GEMM has no (16, 64) instance: the layer runs as two (16, 32) output
    halves. Yardstick: the (32, 64) instance on the same rows padded with 16 zero channels - the same products, another kernel. Bound:
    432 products per output summed in f32 in two different orders, 432 * 2^-24 * sum|terms| <= 2.6e-5 * sum|terms|."""
    from pcdet.utils.spconv_utils import spconv
    rng = np.random.default_rng(2)
    cells = rng.permutation(2 * 6 * 6 * 6)[:300]
    coords = np.stack([cells // 216, (cells // 36) % 6, (cells // 6) % 6, cells % 6], 1).astype(np.int32)
    x = torch.from_numpy(rng.normal(0, 1, (300, 16)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.normal(0, 1, (300, 64)).astype(np.float32)).to(dev)
    narrow = spconv.SubMConv3d(16, 64, 3, bias=False, indice_key='n').to(dev)
    wide = spconv.SubMConv3d(32, 64, 3, bias=False, indice_key='w').to(dev)
    with torch.no_grad():
        wide.weight.zero_()
        wide.weight[..., :16] = narrow.weight
    c = torch.from_numpy(coords).to(dev)
    xn = x.clone().requires_grad_(True)
    xw = torch.cat([x, torch.zeros_like(x)], 1).requires_grad_(True)
    yn = narrow(spconv.SparseConvTensor(xn, c, [6, 6, 6], 2)).features
    yw = wide(spconv.SparseConvTensor(xw, c, [6, 6, 6], 2)).features
    yn.backward(g)
    yw.backward(g)
    assert yn.shape == (300, 64) and float(yn.detach().abs().max()) > 0
    scale = 432 * 2.0 ** -24
    for a, b, mag in ((yn, yw, x.abs().max() * narrow.weight.abs().max() * 432),
                      (xn.grad, xw.grad[:, :16], g.abs().max() * narrow.weight.abs().max() * 64 * 27),
                      (narrow.weight.grad, wide.weight.grad[..., :16], g.abs().max() * x.abs().max() * 300)):
        err = float((a - b).detach().abs().max())
        print('max err %.3g, bound %.3g' % (err, scale * float(mag)))
        assert err <= scale * float(mag)
