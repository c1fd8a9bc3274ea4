"""GPU: DynamicPillarVFE on the fused route (csrc/dyn_pillar_vfe.hip through crbhip.dyn_vfe.dyn_pillar_net) against the golden written
by the reference's own DynamicPillarVFE.

Bars. Forward, train and eval: max|fused - reference f64| <= 4 * e_ref of the output. All six parameter gradients and both layers'
running statistics: <= 4 * e_ref of the same quantity; e_ref = max|reference f32 - reference f64| (golden). voxel_coords: exactly the
reference's. Two calls, and a call on permuted input points: every output, gradient and running statistic bit-equal. Every figure is
printed before it is asserted."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_pillar_cases as cases
import test_dyn_pillar_cpu as cpu

pytestmark = pytest.mark.gpu


class no_fallback(warnings.catch_warnings):
    """the fused route must not announce the torch route"""
    def __enter__(self):
        r = super().__enter__()
        warnings.filterwarnings('error', message='.*torch route.*')
        return r


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def _fused(case, training, dev):
    with no_fallback():
        return cpu.run_vfe(cpu.make_vfe(case['C'], dev=dev), case, training, dev=dev)


@pytest.mark.parametrize('name', cases.CASES)
@pytest.mark.parametrize('training', [True, False])
def test_fused_route_equals_the_reference(dev, gold, name, training):
    case = cases.make_case(name)
    tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
    cpu.compare(_fused(case, training, dev), gold, tag, lambda k: cpu.FACTOR * float(gold['%s_e_ref_%s' % (tag, k)][0]), 'fused')


@pytest.mark.parametrize('name', ['a', 'b'])
def test_two_calls_are_bit_equal(dev, name):
    case = cases.make_case(name)
    first, again = _fused(case, True, dev), _fused(case, True, dev)
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize('name', ['a', 'b'])
def test_permuted_input(dev, name):
    """A permutation of the input points changes nothing: the binding orders the points of a pillar by content before any sum is
    taken (crb_dyn_canonical_order), and the margins of the cases exclude argmax ties. voxel_coords, the outputs, all six gradients
    and both layers' running statistics are bit-equal, train and eval."""
    case = cases.make_case(name)
    p = np.random.default_rng(11).permutation(len(case['points']))
    pcase = dict(case, points=case['points'][p])
    for training in (True, False):
        first, perm = _fused(case, training, dev), _fused(pcase, training, dev)
        assert set(first) == set(perm) and len(first) == (2 + len(cases.GRADS) + len(cases.STATS) if training else 2)
        for k in first:
            print('%s %s %-14s max difference under a permutation %.3g' % (name, 'train' if training else 'eval', k,
                                                                          np.abs(first[k].astype(np.float64) - perm[k]).max()))
        for k in first:
            assert first[k].tobytes() == perm[k].tobytes(), k


def test_canonical_order_is_a_function_of_the_rows_alone(dev):
    """crb_dyn_canonical_order: the same segments, every pillar's rows ascending in the bit patterns of columns 1 .. C (column 1 most
    significant); the ordered rows of a permuted input are bit-equal"""
    from crbhip import dyn_vfe
    case = cases.make_case('a')
    rows = []
    for pts in (case['points'], case['points'][np.random.default_rng(3).permutation(len(case['points']))]):
        t = torch.from_numpy(pts).to(dev)
        seg = dyn_vfe.dyn_voxelize(t, case['B'], cases.PCR, cases.VOXEL, cases.GRID, dyn_vfe.PILLAR)
        can = dyn_vfe.dyn_canonical_order(t, seg)
        assert can['seg_offsets'] is seg['seg_offsets'] and can['coords'] is seg['coords']
        so, a, b = seg['seg_offsets'].cpu().numpy(), seg['perm'].cpu().numpy(), can['perm'].cpu().numpy()
        for v in range(seg['M']):
            assert sorted(a[so[v]:so[v + 1]].tolist()) == sorted(b[so[v]:so[v + 1]].tolist()), v
            bits = pts[b[so[v]:so[v + 1]], 1:].view(np.uint32)
            assert [tuple(r) for r in bits.tolist()] == sorted(tuple(r) for r in bits.tolist()), v
        rows.append(pts[b, 1:])
    assert rows[0].tobytes() == rows[1].tobytes()


@pytest.mark.parametrize('training', [True, False])
def test_forward_on_the_face_points(dev, gold, training):
    """dyn_pillar_cases drops the points placed on cell faces, because the reference's f64 run forms their cells in f64. The f64
    definition of dyn_pillar_cases takes the f32 cells, so the forward pass of the fused route is held to it on the whole case a of
    dyn_voxel_cases, face points included: 4 * e_ref of the output of case a (the same weights and sizes, four pillars more). Forward only:
    the margins that the gradients need are not enforced on these points."""
    import dyn_voxel_cases as vox
    base = vox.make_case('a')
    assert len(base['points']) > len(cases.make_case('a')['points'])
    d = cases.net_f64(base['points'], base['B'], cases.weights(base['C']), training)
    vfe = cpu.make_vfe(base['C'], dev=dev).train(training)
    with torch.no_grad(), no_fallback():
        bd = vfe({'points': torch.from_numpy(base['points']).to(dev), 'batch_size': base['B']})
    assert (bd['voxel_coords'].cpu().numpy() == d['coords']).all()
    err = np.abs(bd['pillar_features'].double().cpu().numpy() - d['out']).max()
    bar = cpu.FACTOR * float(gold['vfe_a_%s_e_ref_out' % ('train' if training else 'eval')][0])
    print('face points, %s: err %.3g bar %.3g' % ('train' if training else 'eval', err, bar))
    assert err <= bar


def test_eval_calls_are_bit_equal(dev):
    case = cases.make_case('a')
    a, b = _fused(case, False, dev), _fused(case, False, dev)
    assert a['out'].tobytes() == b['out'].tobytes()


def test_unsupported_configs_take_the_torch_route_and_say_so(dev):
    from crbhip import CrbHipError, dyn_vfe
    case = cases.make_case('b')
    for cfg in (cases.vfe_cfg(num_filters=(64,)), cases.vfe_cfg(with_distance=True)):
        vfe = cpu.make_vfe(case['C'], dev=dev, cfg=cfg).eval()
        with pytest.warns(UserWarning, match='torch route'):
            bd = vfe({'points': torch.from_numpy(case['points']).to(dev), 'batch_size': case['B']})
        assert bd['pillar_features'].shape[1] == 64 and torch.isfinite(bd['pillar_features']).all()
    assert not dyn_vfe.pillar_supported(4, [64]) and not dyn_vfe.pillar_supported(3, [64, 64]) and dyn_vfe.pillar_supported(5, [64, 64])
    pts = torch.from_numpy(case['points']).to(dev)
    seg = dyn_vfe.dyn_voxelize(pts, case['B'], cases.PCR, cases.VOXEL, cases.GRID, dyn_vfe.PILLAR)
    z = lambda *s: torch.zeros(s, device=dev)
    with pytest.raises(CrbHipError, match='CRB_ERR_UNSUPPORTED'):
        dyn_vfe.dyn_pillar_net(pts, seg, z(64, 10), z(64), z(64), z(64, 64), z(64), z(64), (z(64), z(64)), (z(64), z(64)), False, 0.01, 1e-3,
                               cases.VOXEL, cases.offsets())
    # the C entry points themselves: three point features are refused before anything is read or launched (CRB_ERR_UNSUPPORTED = -4)
    import ctypes
    from crbhip._lib import lib
    a = dyn_vfe._Args()
    a.n_points, a.M, a.row_stride, a.C = 2, 1, 4, 3
    assert lib.crb_dyn_pillar_forward(ctypes.byref(a), None, None) == -4
    assert lib.crb_dyn_pillar_moments(ctypes.byref(a), None, None, 0, None) == -4
    assert lib.crb_dyn_pillar_backward_b(ctypes.byref(a), None, None, None, None, 0, None) == -4


def test_training_on_a_single_point_raises_as_batch_norm_does(dev):
    vfe = cpu.make_vfe(4, dev=dev).train()
    pts = torch.tensor([[0, 0.1, 0.1, 0.1, 0.5]], device=dev)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        vfe({'points': pts, 'batch_size': 1})
    bd = vfe.eval()({'points': pts, 'batch_size': 1})
    assert bd['pillar_features'].shape == (1, 64)


def test_no_point_in_range_gives_an_empty_result(dev):
    pts = torch.tensor([[0, 9.0, 0.0, 0.0, 0.5], [1, 0.0, 9.0, 0.0, 0.5]], device=dev)
    for training in (True, False):
        bd = cpu.make_vfe(4, dev=dev).train(training)({'points': pts, 'batch_size': 2})
        assert bd['pillar_features'].shape == (0, 64) and bd['voxel_coords'].shape == (0, 4)


# ---- the detector: CenterPoint behind DynPillarVFE (waymo_models/centerpoint_dyn_pillar_1x.yaml) -------------------------------
POINTS = 5000


def _detector(dev):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import centerpoint_dyn_pillar_cfg, centerpoint_dyn_pillar_dataset_args
    from pcdet.models import build_network
    cfg = centerpoint_dyn_pillar_cfg()
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS, **centerpoint_dyn_pillar_dataset_args(cfg)))
    return cfg, model.to(dev)


def _batch(dev):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(40, 2, POINTS, waymo=True)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {'points': t(np.concatenate([bidx[:, None], pts], 1)), 'point_frame_offsets': t(off), 'batch_size': 2,
            'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': t(gt), 'frame_id': np.array(['000040', '000041'])}


def test_full_config_training_step_and_eval_pass(dev):
    """the yaml as it stands: a 468 x 468 map at stride 1 under the centre head"""
    cfg, model = _detector(dev)
    assert type(model.vfe).__name__ == 'DynamicPillarVFE' and model.dense_head.feature_map_stride == 1
    model.train()
    with no_fallback():
        ret, tb, _ = model(_batch(dev))
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(ret['loss'])
    missing = [n for n, t in model.named_parameters() if t.grad is None or not torch.isfinite(t.grad).all()]
    assert not missing, missing
    assert [int(p.norm.num_batches_tracked) for p in model.vfe.pfn_layers] == [1, 1]
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = 0.0             # (random weights: keep whatever the NMS keeps)
    model.eval()
    with torch.no_grad(), no_fallback():
        pred, recall = model(_batch(dev))
    assert len(pred) == 2 and any(len(p['pred_scores']) > 0 for p in pred)
    for p in pred:
        n = len(p['pred_scores'])
        assert n <= 500 and p['pred_boxes'].shape == (n, 7) and torch.isfinite(p['pred_boxes']).all()
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())


@pytest.mark.parametrize('method', ['entropy', 'random'])
def test_strategies_select_from_a_pool(dev, tmp_path, method):
    import random
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.model_cfgs import centerpoint_dyn_pillar_dataset_args
    from pcdet.query_strategies import build_strategy
    cfg, model = _detector(dev)
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': method, 'AGGREGATION': 'mean', 'SELECT_NUMS': 2})
    cfg.MODEL.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = 0.0
    args = centerpoint_dyn_pillar_dataset_args(cfg)
    pool = SyntheticDataset(num_frames=4, first_frame=300, n_points=POINTS, **args)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS, **args)
    strat = build_strategy(method, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 2), 0, str(tmp_path), cfg)
    random.seed(5)
    with no_fallback():
        picked = strat.query(cur_epoch=0)
    assert len(picked) == 2 and len(set(picked)) == 2 and set(picked) <= set(pool.sample_id_list), picked


def _golden_detector(dev, gold):
    import pillar_cases
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import centerpoint_dyn_pillar_cfg
    from pcdet.models import build_network
    cfg = centerpoint_dyn_pillar_cfg()
    ds = SyntheticDataset(num_frames=2, kind='waymo', point_cloud_range=cases.DET_PCR, voxel_size=cases.DET_VOXEL)
    assert ds.grid_size.tolist() == cases.DET_GRID
    model = build_network(cfg.MODEL, 3, ds)
    sd = model.state_dict()
    assert list(sd.keys()) == gold['det_keys'].tolist()
    seeded = pillar_cases.detector_state([(k, tuple(v.shape), v.dtype.is_floating_point) for k, v in sd.items()], seed=cases.DET_SEED,
                                         overrides=pillar_cases.golden_bias_overrides(gold))
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(sd[k].shape) for k, v in seeded.items()})
    return model.to(dev).train()


def test_detector_step_matches_the_reference(dev, gold):
    """the golden step of the reference's CenterPoint with DynPillarVFE (64 x 64 grid, two synthetic frames, seeded weights, BatchNorm
    biases off the ReLU kinks): loss, every tb_dict entry and three gradients within FACTOR * e_ref of its f64 run, e_ref = the larger
    error of its two f32 runs (NCHW and channels_last memory)"""
    from pcdet.datasets.synthetic import kitti_batch
    model = _golden_detector(dev, gold)
    inp = cases.detector_inputs(kitti_batch)
    with no_fallback():
        ret, tb, _ = model({'points': torch.from_numpy(inp['points']).to(dev), 'gt_boxes': torch.from_numpy(inp['gt_boxes']).to(dev),
                            'batch_size': inp['batch_size']})
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    assert sorted(tb) == gold['det_tb_keys'].tolist()
    assert int(model.dense_head.forward_ret_dict['target_dicts']['masks'][0].sum()) == int(gold['det_objects'][0])
    params = dict(model.named_parameters())
    res = {'loss': ret['loss'].detach().double().reshape(1).cpu().numpy(), 'tb_vals': np.array([float(tb[k].double()) for k in sorted(tb)])}
    for n, sl in cases.DET_GRADS.items():
        res['grad/' + n] = params[n].grad.double().cpu().numpy()[sl]
    bad = []
    for k, v in res.items():
        err, e_ref = np.abs(v - gold['det_f64_' + k]).max(), gold['det_e_ref_' + k][0]
        print('detector %-48s err %.3g e_ref %.3g (%.2f x) on values up to %.3g' % (k, err, e_ref, err / e_ref, np.abs(gold['det_f64_' + k]).max()))
        if v.shape != gold['det_f64_' + k].shape or not err <= cpu.FACTOR * e_ref:
            bad.append(k)
    assert not bad, bad
