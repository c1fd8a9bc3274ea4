"""GPU: PointPillars. csrc/pillar_vfe.hip (moments, fused forward, fused backward) through PillarVFE against the f64 definition and the
torch route in f64 on the device; PointPillarScatter against the reference's scatter; PointPillar against the golden step written by
the reference's own detector; the full configuration on synthetic frames and the entropy / random strategies on it.

Bars. Forward (train and eval): max|fused - f64 definition| <= 4 * e_ref, e_ref = max|reference f32 - reference f64| of the output
(golden). Backward and running statistics: max|fused - torch route in f64 on this device| <= 4 * e_ref of the same quantity. Detector
step: loss, tb_dict entries and three gradients within 4 * e_ref of the reference's f64 values, e_ref = the larger error of the
reference's two f32 runs (NCHW and channels_last memory). Every figure is printed before it is
asserted. Garbage slots, reproducibility, raw points against voxels, scatter: bit-equal. Figures of the MI355X run: DESIGN.md section 6."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pillar_cases as cases
import test_pointpillar_cpu as cpu

pytestmark = pytest.mark.gpu
FACTOR = cpu.FACTOR
GRAD_KEYS = ('dW', 'dgamma', 'dbeta', 'running_mean', 'running_var')


class no_fallback(warnings.catch_warnings):
    """the HIP route must not announce the torch route"""
    def __enter__(self):
        r = super().__enter__()
        warnings.filterwarnings('error', message='.*torch route.*')
        return r


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def _fused(case, name, training, dev):
    with no_fallback():
        return cpu.run_vfe(cpu.make_vfe(case['voxels'].shape[2], dev=dev), case, name, training, dev=dev)


# ---- the fused pillar feature net -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.CASES))
@pytest.mark.parametrize('training', [True, False])
def test_fused_forward_against_the_f64_definition(dev, gold, name, training):
    case = cases.make_case(name)
    tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
    res = _fused(case, name, training, dev)
    assert res['out'].shape == (len(case['num_points']), cases.COUT) and res['out'].dtype == torch.float32
    d = cases.vfe_f64(case, cases.weights(case['voxels'].shape[2]), training)
    assert not cpu.check_against(res, {'out': d['out']}, lambda k: gold['%s_e_ref_%s' % (tag, k)][0], ('out',), tag)


@pytest.mark.parametrize('name', list(cases.CASES))
def test_fused_backward_and_running_statistics_against_the_torch_route_in_f64(dev, gold, name):
    case = cases.make_case(name)
    C = case['voxels'].shape[2]
    res = _fused(case, name, True, dev)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                                # (an f64 module on the device says that it takes the torch route)
        ref = cpu.run_vfe(cpu.make_vfe(C, torch.float64, dev), case, name, True, dev=dev, dtype=torch.float64)
    torch.cuda.synchronize()
    assert ref['dW'].dtype == torch.float64
    tag = 'vfe_%s_train' % name
    assert not cpu.check_against(res, ref, lambda k: gold['%s_e_ref_%s' % (tag, k)][0], GRAD_KEYS, tag)


def test_eval_mode_backward_against_the_torch_route_in_f64(dev):
    """the frozen-BatchNorm path: A, b folded from the running statistics, dW / dgamma / dbeta without the batch-statistics terms.
    The golden holds no eval-mode gradients, so the bar is the kernel's own rounding: G1[c, k] = sum_m dy f_k and G0[c] = sum_m dy are
    f32 products summed in f32 over the <= 64 pillars of a workgroup (65 roundings of a partial sum bounded by S_c F_k, S_c = sum_m
    |grad_out[m, c]|, F_k = max |f_k|), then in f64; dW = scale G1, dgamma = (w . G1 - mean G0) / sigma, dbeta = G0 in f64, rounded
    to f32 once. The margins of the case make both routes select the same slots."""
    case = cases.make_case('b')
    g = torch.from_numpy(cases.grad_out('b')).to(dev)
    got = {}
    for dtype in (torch.float32, torch.float64):
        vfe = cpu.make_vfe(5, dtype, dev).eval()
        with no_fallback() if dtype == torch.float32 else warnings.catch_warnings():
            if dtype == torch.float64:
                warnings.simplefilter('ignore')
            out = vfe(cpu.case_batch(case, dev, dtype))['pillar_features']
        (out * g.to(dtype)).sum().backward()
        p = vfe.pfn_layers[0]
        got[dtype] = {'dW': p.linear.weight.grad.double().cpu().numpy(), 'dgamma': p.norm.weight.grad.double().cpu().numpy(),
                      'dbeta': p.norm.bias.grad.double().cpu().numpy()}
    w = cases.weights(5)
    d = cases.vfe_f64(case, w, False)
    u = 2.0 ** -24
    S = np.abs(cases.grad_out('b').astype(np.float64)).sum(0)                     # (64)
    F = np.abs(d['f']).reshape(-1, d['f'].shape[-1]).max(0)                       # (K)
    W = np.abs(w['pfn_layers.0.linear.weight'].astype(np.float64))
    sigma = np.sqrt(d['var'] + cases.EPS)
    scale = np.abs(w['pfn_layers.0.norm.weight'].astype(np.float64)) / sigma
    eG1, eG0 = 66 * u * S[:, None] * F[None, :], 66 * u * S
    bound = {'dW': scale[:, None] * eG1 + u * np.abs(got[torch.float64]['dW']),
             'dgamma': ((W * eG1).sum(1) + np.abs(d['mean']) * eG0) / sigma + u * np.abs(got[torch.float64]['dgamma']),
             'dbeta': eG0 + u * np.abs(got[torch.float64]['dbeta'])}
    bad = []
    for k in ('dW', 'dgamma', 'dbeta'):
        err = np.abs(got[torch.float32][k] - got[torch.float64][k])
        print('vfe_b_eval %-7s err %.3g on values up to %.3g, largest err / bound %.3f' % (k, err.max(), np.abs(got[torch.float64][k]).max(), (err / bound[k]).max()))
        if not (err <= bound[k]).all():
            bad.append(k)
    assert not bad, bad


@pytest.mark.parametrize('garbage', list(cases.GARBAGE))
def test_padded_slots_are_never_read(dev, garbage):
    clean = _fused(cases.make_case('a'), 'a', True, dev)
    dirty = _fused(cases.make_case(garbage), 'a', True, dev)
    for k in cpu.TRAIN_KEYS:
        assert torch.equal(clean[k], dirty[k]), k
    clean, dirty = _fused(cases.make_case('a'), 'a', False, dev), _fused(cases.make_case(garbage), 'a', False, dev)
    assert torch.equal(clean['out'], dirty['out'])


@pytest.mark.parametrize('name', ['a', 'b'])
def test_forward_and_backward_are_reproducible(dev, name):
    case = cases.make_case(name)
    runs = [_fused(case, name, True, dev) for _ in range(2)]
    for k in cpu.TRAIN_KEYS:
        assert torch.equal(runs[0][k], runs[1][k]) and torch.isfinite(runs[0][k]).all(), k


def test_unsupported_config_says_torch_route_on_the_device(dev):
    case = cases.make_case('a')
    vfe = cpu.make_vfe(4, dev=dev, num_filters=(48,)).train()
    with pytest.warns(UserWarning, match='torch route'):
        out = vfe(cpu.case_batch(case, dev))['pillar_features']
    assert out.shape == (37, 48) and torch.isfinite(out).all()


def test_binding_answers_unsupported_shapes(dev):
    import crbhip
    from crbhip import pillar_vfe as pv
    w = {k: torch.from_numpy(np.asarray(v)).to(dev) for k, v in cases.weights(4).items()}
    v = torch.zeros((3, 33, 4), device=dev)
    with pytest.raises(crbhip.CrbHipError, match='UNSUPPORTED'):
        pv.pillar_vfe(v, torch.ones(3, dtype=torch.int32, device=dev), torch.zeros((3, 4), dtype=torch.int32, device=dev),
                      w['pfn_layers.0.linear.weight'], w['pfn_layers.0.norm.weight'], w['pfn_layers.0.norm.bias'],
                      w['pfn_layers.0.norm.running_mean'], w['pfn_layers.0.norm.running_var'], True, 0.01, 1e-3, cases.VOXEL, cases.offsets())


def test_raw_points_equal_loader_side_voxels(dev):
    """PillarVFE from raw points (voxelizes on the device first) == PillarVFE fed what crbhip.voxel.voxelize returns for the same points"""
    from crbhip import voxel
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, _ = kitti_batch(40, 2, 6000)
    pts = pts.copy()
    pts[:, 0] -= 8.0                                                  # a busy part of the frames inside the reduced range
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    points = torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev)
    offs = torch.from_numpy(off).to(dev)
    r = voxel.voxelize(points[:, 1:].contiguous(), offs, cases.PCR, cases.VOXEL, 16000, 32, want_voxels=True, want_mean=False, grid_xyz=cases.GRID)
    M = len(r['coords'])
    assert 100 < M < 12000 and int(r['num_points'].max()) > 1
    g = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (M, cases.COUT)).astype(np.float32)).to(dev)
    res = []
    for batch in ({'points': points, 'point_frame_offsets': offs, 'batch_size': 2},
                  {'voxels': r['voxels'], 'voxel_num_points': r['num_points'], 'voxel_coords': r['coords'], 'batch_size': 2}):
        vfe = cpu.make_vfe(4, dev=dev).train()
        with no_fallback():
            bd = vfe(batch)
        (bd['pillar_features'] * g).sum().backward()
        p = vfe.pfn_layers[0]
        res.append((bd['pillar_features'].detach(), bd['voxel_coords'], bd['voxel_num_points'], p.linear.weight.grad, p.norm.weight.grad,
                    p.norm.bias.grad, p.norm.running_mean.clone(), p.norm.running_var.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.isfinite(res[0][0]).all() and torch.isfinite(res[0][3]).all()


def test_no_pillars_give_an_empty_map(dev):
    vfe = cpu.make_vfe(4, dev=dev).train()
    with no_fallback():
        bd = vfe({'voxels': torch.zeros((0, 32, 4), device=dev), 'voxel_num_points': torch.zeros((0,), dtype=torch.int32, device=dev),
                  'voxel_coords': torch.zeros((0, 4), dtype=torch.int32, device=dev), 'batch_size': 2})
    assert bd['pillar_features'].shape == (0, cases.COUT) and bd['pillar_features'].is_cuda
    bev = cpu.make_scatter()(bd)['spatial_features']
    assert bev.shape == (2, cases.COUT, cases.GRID[1], cases.GRID[0]) and not bool(bev.any())


# ---- scatter ----------------------------------------------------------------------------------------------------------------
def test_scatter_equals_the_reference_and_its_backward_is_a_gather(dev, gold):
    case = cases.make_case('a')
    feats = torch.from_numpy(gold['vfe_a_train_out']).to(dev).requires_grad_(True)
    coords = torch.from_numpy(case['coords']).to(dev)
    bev = cpu.make_scatter()({'pillar_features': feats, 'voxel_coords': coords, 'batch_size': case['B']})['spatial_features']
    assert bev.shape == (2, cases.COUT, cases.GRID[1], cases.GRID[0]) and bev.is_contiguous(memory_format=torch.channels_last)
    assert np.array_equal(bev.detach().cpu().numpy(), gold['scatter_map'])
    g = torch.from_numpy(np.random.default_rng(3).normal(0, 1, tuple(bev.shape)).astype(np.float32)).to(dev)
    (bev * g).sum().backward()
    c = coords.long()
    assert torch.equal(feats.grad, g[c[:, 0], :, c[:, 2], c[:, 3]])


# ---- detector ---------------------------------------------------------------------------------------------------------------
def _reduced_detector(dev, gold):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pointpillar_cfg
    from pcdet.models import build_network
    ds = SyntheticDataset(num_frames=2, point_cloud_range=cases.PCR, voxel_size=cases.VOXEL, max_points_per_voxel=32)
    model = build_network(pointpillar_cfg().MODEL, 3, ds)
    sd = model.state_dict()
    seeded = cases.detector_state([(k, tuple(v.shape), v.dtype.is_floating_point) for k, v in sd.items()],
                                  overrides=cases.golden_bias_overrides(gold))       # (biases off the ReLU kinks: cases.DET_KINK)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(sd[k].shape) for k, v in seeded.items()})
    return model.to(dev)


def test_detector_step_matches_the_reference(dev, gold):
    """the golden step on the reduced grid: loss, every tb_dict entry and three gradients within 4 * e_ref of the reference's f64 run.

    Two properties of the case make that bar meaningful for a 20-BatchNorm stack at B = 2 (tests/pillar_cases.py):
    - the seeded state carries the golden's BatchNorm biases, which keep every pre-activation of the step farther than cases.DET_KINK
      from a ReLU kink. Without that margin about 15 of 5 M masks are decided by rounding and the two backbone-side gradients move by
      a percent (2720 x and 1096 x the NCHW e_ref on the MI355X);
    - e_ref of each quantity is the larger error of TWO f32 runs of the reference against its f64 run: in its own NCHW memory and in
      channels_last memory, the layout the device route runs the 2-D part in. The same torch modules differ by a factor of ten
      between the two (vfe.pfn_layers.0.linear.weight: 4.4e-5 and 4.3e-4 on values up to 8.45), so one of them alone is a sample,
      not a unit. With the NCHW sample alone the device route was 6.9 ... 9.8 x on that gradient and inside 4 x on everything else."""
    from pcdet.datasets.synthetic import kitti_batch
    inp = cases.detector_inputs(kitti_batch)
    model = _reduced_detector(dev, gold).train()
    batch = {'voxels': torch.from_numpy(inp['voxels']).to(dev), 'voxel_coords': torch.from_numpy(inp['voxel_coords']).to(dev),
             'voxel_num_points': torch.from_numpy(inp['voxel_num_points']).to(dev), 'gt_boxes': torch.from_numpy(inp['gt_boxes']).to(dev),
             'batch_size': inp['batch_size']}
    with no_fallback():
        ret, tb, _ = model(batch)
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    assert sorted(tb) == gold['det_tb_keys'].tolist()
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values())
    params = dict(model.named_parameters())
    res = {'loss': ret['loss'].detach().reshape(1), 'tb_vals': torch.stack([tb[k].double().reshape(()) for k in sorted(tb)])}
    for n, sl in cases.DET_GRADS.items():
        res['grad/' + n] = params[n].grad[sl]
    ref = {k: gold['det_f64_' + k] for k in res}
    assert not cpu.check_against(res, ref, lambda k: gold['det_e_ref_' + k][0], list(res), 'detector')


POINTS = 8000


def _full_detector(dev):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pointpillar_cfg, pointpillar_dataset_args
    from pcdet.models import build_network
    cfg = pointpillar_cfg()
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS, **pointpillar_dataset_args(cfg)))
    return cfg, model.to(dev)


def _full_batch(dev):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(40, 2, POINTS)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {'points': t(np.concatenate([bidx[:, None], pts], 1)), 'point_frame_offsets': t(off), 'batch_size': 2,
            'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': t(gt), 'frame_id': np.array(['000040', '000041'])}


def test_full_config_training_step_and_eval_pass(dev):
    """kitti_models/pointpillar.yaml as it stands: a 496 x 432 map, 321,408 anchors per frame"""
    from pcdet.query_strategies.scoring import RecordLayout
    cfg, model = _full_detector(dev)
    assert model.dense_head.anchors[0].shape[:3] == (1, 248, 216) and RecordLayout.for_model(model) == RecordLayout(500, 3)
    model.train()
    with no_fallback():
        ret, tb, _ = model(_full_batch(dev))
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(ret['loss'])
    assert set(tb) == {'loss_rpn', 'rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir'}
    missing = [n for n, t in model.named_parameters() if t.grad is None or not torch.isfinite(t.grad).all()]
    assert not missing, missing
    assert int(model.vfe.pfn_layers[0].norm.num_batches_tracked) == 1
    cfg.MODEL.POST_PROCESSING.SCORE_THRESH = 0.0                       # (random weights: keep whatever the NMS keeps)
    model.eval()
    with torch.no_grad(), no_fallback():
        pred, recall = model(_full_batch(dev))
    assert len(pred) == 2 and any(len(p['pred_scores']) > 0 for p in pred)
    ref_keys = {'confidence', 'rpn_preds', 'num_bbox', 'mean_points', 'median_points', 'variance_points', 'loss_predictions',
                'batch_rcnn_cls', 'batch_rcnn_reg', 'embeddings', 'pred_logits', 'pred_boxes', 'pred_scores', 'pred_labels',
                'pred_box_unique_density'}
    for p in pred:
        assert ref_keys <= set(p.keys())
        n = len(p['pred_scores'])
        assert n <= 500 and p['pred_boxes'].shape == (n, 7) and p['pred_labels'].shape == (n,)
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())


@pytest.mark.parametrize('method', ['entropy', 'random'])
def test_strategies_select_from_a_pool(dev, tmp_path, method):
    import random
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.model_cfgs import pointpillar_dataset_args
    from pcdet.query_strategies import build_strategy
    cfg, model = _full_detector(dev)
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': method, 'AGGREGATION': 'mean', 'SELECT_NUMS': 2})
    cfg.MODEL.POST_PROCESSING.SCORE_THRESH = 0.0
    args = pointpillar_dataset_args(cfg)
    pool = SyntheticDataset(num_frames=4, first_frame=300, n_points=POINTS, **args)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS, **args)
    strat = build_strategy(method, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 2), 0, str(tmp_path), cfg)
    random.seed(5)
    with no_fallback():
        picked = strat.query(cur_epoch=0)
    assert len(picked) == 2 and len(set(picked)) == 2 and set(picked) <= set(pool.sample_id_list), picked
