"""CPU: DynamicPillarVFE. The registry builds it; state-dict keys; its torch route (the definition of the fused route) against the
golden written by the reference's own DynamicPillarVFE and against the f64 numpy definition of tests/dyn_pillar_cases.py; the
closed-form layer-1 gradients of crbhip.dyn_vfe against autograd in f64; the margins of the cases.

Bars. voxel_coords and the row order: exactly the reference's. f64: max|torch route - golden f64| <= 1e-10 on every quantity (outputs,
the six gradients, the running statistics). f32: <= 4 * e_ref, e_ref = max|reference f32 - reference f64| of the same quantity."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_pillar_cases as cases

FACTOR = 4.0


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def make_vfe(C, dtype=torch.float32, dev=None, cfg=None):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d import vfe
    m = vfe.__all__['DynPillarVFE'](model_cfg=EasyDict(cfg or cases.vfe_cfg()), num_point_features=C, voxel_size=cases.VOXEL,
                                    grid_size=cases.GRID, point_cloud_range=cases.PCR)
    if cfg is None:
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.weights(C).items()})
    m = m.to(dtype)
    return m if dev is None else m.to(dev)


def run_vfe(vfe, case, training, dev=None, dtype=torch.float32):
    """-> dict out, coords (+ the six gradients and the running statistics in training), numpy"""
    vfe.train(training)
    vfe.zero_grad(set_to_none=True)
    pts = torch.from_numpy(case['points']).to(dtype)
    bd = vfe({'points': pts if dev is None else pts.to(dev), 'batch_size': case['B']})
    out = bd['pillar_features']
    res = {'out': out.detach(), 'coords': bd['voxel_coords']}
    if training:
        g = torch.from_numpy(cases.grad_out(case['name'], out.shape[0])).to(out.dtype).to(out.device)
        (out * g).sum().backward()
        for i, p in enumerate(vfe.pfn_layers):
            res.update({'dW%d' % (i + 1): p.linear.weight.grad, 'dgamma%d' % (i + 1): p.norm.weight.grad, 'dbeta%d' % (i + 1): p.norm.bias.grad,
                        'running_mean%d' % (i + 1): p.norm.running_mean.detach().clone(),
                        'running_var%d' % (i + 1): p.norm.running_var.detach().clone()})
    return {k: v.detach().cpu().numpy() for k, v in res.items()}


def compare(res, gold, tag, bar_of, label):
    """every float quantity of res against the golden f64 values; bar_of(key) -> the bound. Prints each figure, then asserts all."""
    bad = []
    for key, v in res.items():
        if key == 'coords':
            assert v.dtype == np.int32 and (v == gold['%s_coords' % tag]).all()
            continue
        err, bar = np.abs(v.astype(np.float64) - gold['%s_f64_%s' % (tag, key)]).max(), bar_of(key)
        print('%s %s %-14s err %.3g bar %.3g' % (label, tag, key, err, bar))
        if not err <= bar:
            bad.append((key, err, bar))
    assert not bad, bad


def test_registry_builds_the_module_and_keys_equal_the_reference(gold):
    from pcdet.models.backbones_3d import vfe
    from pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import DynamicPillarVFE, PFNLayerV2
    assert vfe.__all__['DynPillarVFE'] is DynamicPillarVFE
    m = make_vfe(4)
    assert list(m.state_dict().keys()) == list(gold['vfe_keys']) == cases.KEYS
    assert isinstance(m.pfn_layers[0], PFNLayerV2) and m.get_output_feature_dim() == 64
    assert tuple(m.pfn_layers[0].linear.weight.shape) == (32, 10) and tuple(m.pfn_layers[1].linear.weight.shape) == (64, 64)


@pytest.mark.parametrize('name', cases.CASES)
@pytest.mark.parametrize('training', [True, False])
def test_torch_route_equals_the_reference(gold, name, training):
    case = cases.make_case(name)
    tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
    compare(run_vfe(make_vfe(case['C'], torch.float64), case, training, dtype=torch.float64), gold, tag, lambda k: 1e-10, 'f64')
    compare(run_vfe(make_vfe(case['C']), case, training), gold, tag, lambda k: FACTOR * float(gold['%s_e_ref_%s' % (tag, k)][0]), 'f32')


@pytest.mark.parametrize('name', cases.CASES)
@pytest.mark.parametrize('training', [True, False])
def test_numpy_definition_equals_the_reference(gold, name, training):
    case = cases.make_case(name)
    tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
    d = cases.net_f64(case['points'], case['B'], cases.weights(case['C']), training)
    assert (d['coords'] == gold['%s_coords' % tag]).all()
    assert np.abs(d['out'] - gold['%s_f64_out' % tag]).max() <= 1e-10
    for k in cases.STATS if training else ():
        assert np.abs(d[k] - gold['%s_f64_%s' % (tag, k)]).max() <= 1e-10, k
    assert len(cases.margin_violations(d)) == 0
    print('case %s: %d point redraws in %d rounds' % (name, case['redraws'], case['rounds']))


def test_closed_form_layer_1_gradients_equal_autograd():
    """dW1, dgamma1, dbeta1 from G1 = sum dy f^T, G0 = sum dy and the moments (crbhip.pillar_vfe.param_grads, n = Nk, no padded rows)"""
    from crbhip.pillar_vfe import batch_stats, param_grads
    rng = np.random.default_rng(3)
    n, K = 57, 11
    f = torch.from_numpy(rng.normal(0, 1, (n, K)))
    W = torch.from_numpy(rng.normal(0, 0.3, (32, K))).requires_grad_()
    gamma, beta = torch.from_numpy(rng.uniform(0.5, 1.5, 32)).requires_grad_(), torch.from_numpy(rng.normal(0, 0.2, 32)).requires_grad_()
    dy = torch.from_numpy(rng.normal(0, 1, (n, 32)))
    y = torch.nn.functional.batch_norm(f @ W.t(), None, None, gamma, beta, True, 0.01, cases.EPS)
    (y * dy).sum().backward()
    with torch.no_grad():
        mean, var, WS2 = batch_stats(W, f.sum(0), f.t() @ f, float(n))
        sigma = torch.sqrt(var + cases.EPS)
        dW, dgamma, dbeta = param_grads(W, mean, sigma, gamma / sigma, dy.t() @ f, dy.sum(0), float(n), f.sum(0), WS2)
    assert (dW - W.grad).abs().max() < 1e-10 and (dgamma - gamma.grad).abs().max() < 1e-10 and (dbeta - beta.grad).abs().max() < 1e-10


def test_dropped_point_rules():
    C, B = 4, 2
    rows = {'inside': [0, 0.1, 0.1, 0.1], 'inside too': [0, 0.15, 0.12, 1.1], 'x high': [0, 5.62, 0.1, 0.1], 'y low': [0, 0.1, -3.94, 0.1],
            'z high, kept': [1, 0.1, 0.1, 4.5], 'z low, kept': [1, 0.12, 0.13, -2.5], 'NaN x': [1, np.nan, 0.1, 0.1],
            'NaN z': [1, 0.1, 0.1, np.nan], 'frame B': [B, 0.1, 0.1, 0.1]}
    pts = np.asarray([r + [0.5] for r in rows.values()], np.float32)
    out = run_vfe(make_vfe(C), {'points': pts, 'B': B, 'name': 'b'}, False)
    assert out['coords'].tolist() == [[0, 0, 12, 16], [1, 0, 12, 16]] and out['out'].shape == (2, 64) and np.isfinite(out['out']).all()


def test_no_point_in_range_gives_an_empty_result():
    pts = np.asarray([[0, 9.0, 0.0, 0.0, 0.5], [1, 0.0, 9.0, 0.0, 0.5]], np.float32)
    for training in (True, False):
        vfe = make_vfe(4).train(training)
        bd = vfe({'points': torch.from_numpy(pts), 'batch_size': 2})
        assert bd['pillar_features'].shape == (0, 64) and bd['voxel_coords'].shape == (0, 4)


def test_config_builds_centerpoint_on_the_pillar_grid():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import centerpoint_dyn_pillar_cfg, centerpoint_dyn_pillar_dataset_args
    from pcdet.models import build_network
    cfg = centerpoint_dyn_pillar_cfg()
    ds = SyntheticDataset(num_frames=2, n_points=2000, **centerpoint_dyn_pillar_dataset_args(cfg))
    assert ds.grid_size.tolist() == [468, 468, 1] and cfg.CLASS_NAMES == ['Vehicle', 'Pedestrian', 'Cyclist']
    model = build_network(cfg.MODEL, 3, ds)
    assert [type(m).__name__ for m in model.module_list] == ['DynamicPillarVFE', 'PointPillarScatter', 'BaseBEVBackbone', 'CenterHead']
    assert model.dense_head.feature_map_stride == 1 and cfg.MODEL.BACKBONE_2D.LAYER_STRIDES == [1, 2, 2]
    assert cfg.MODEL.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE == [-80, -80, -10.0, 80, 80, 10.0]
    assert [tuple(p.linear.weight.shape) for p in model.vfe.pfn_layers] == [(32, 11), (64, 64)]
    from pcdet.query_strategies.scoring import RecordLayout
    assert RecordLayout.for_model(model) == RecordLayout(500, 3)


def test_config_carries_the_values_of_the_reference_yaml(gold):
    import json
    from pcdet.model_cfgs import centerpoint_dyn_pillar_cfg, centerpoint_dyn_pillar_dataset_args
    y = json.loads(str(gold['cfg_json']))
    cfg = centerpoint_dyn_pillar_cfg()
    plain = json.loads(json.dumps(cfg.MODEL))
    assert cfg.CLASS_NAMES == y['CLASS_NAMES'] and plain == y['MODEL']
    args = centerpoint_dyn_pillar_dataset_args(cfg)
    assert args['point_cloud_range'] == y['POINT_CLOUD_RANGE'] and args['voxel_size'] == y['VOXEL_SIZE']
