"""CPU: PointPillars. The case builder of tests/pillar_cases.py and its margins; the mirror's host (torch) route of PillarVFE and
PointPillarScatter against the golden written by the reference's own modules (tests/golden/make_goldens_pointpillar.py); the closed
form of the fused route's parameter gradients against autograd in f64; config, dataset arguments, registries and the binding's
refusals.

Bars. The host route is the reference's formulation, so max|mirror f32 - reference f64| <= FACTOR * e_ref with e_ref = max|reference
f32 - reference f64| of the same quantity (golden) and FACTOR = 4, the convention of tests/test_voxel_rcnn_gpu.py. Scatter: exact."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pillar_cases as cases

FACTOR = 4.0
TRAIN_KEYS = ('out', 'dW', 'dgamma', 'dbeta', 'running_mean', 'running_var')


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def _cfg(**kw):
    from pcdet.config import EasyDict
    return EasyDict(cases.vfe_cfg(**kw))


def make_vfe(C, dtype=torch.float32, dev='cpu', **kw):
    from pcdet.models.backbones_3d.vfe import PillarVFE
    vfe = PillarVFE(model_cfg=_cfg(**kw), num_point_features=C, voxel_size=cases.VOXEL, point_cloud_range=cases.PCR, grid_size=cases.GRID)
    if not kw:
        vfe.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.weights(C).items()})
    return vfe.to(dtype).to(dev)


def case_batch(case, dev='cpu', dtype=torch.float32):
    return {'voxels': torch.from_numpy(case['voxels']).to(dtype).to(dev), 'voxel_num_points': torch.from_numpy(case['num_points']).to(dev),
            'voxel_coords': torch.from_numpy(case['coords']).to(dev), 'batch_size': case['B']}


def run_vfe(vfe, case, name, training, dev='cpu', dtype=torch.float32):
    """one forward (+ backward in train mode) of a PillarVFE on a case -> dict of tensors keyed like the golden"""
    vfe.train(training)
    vfe.zero_grad(set_to_none=True)
    out = vfe(case_batch(case, dev, dtype))['pillar_features']
    res = {'out': out.detach()}
    if training:
        (out * torch.from_numpy(cases.grad_out(name)).to(dtype).to(dev)).sum().backward()
        p = vfe.pfn_layers[0]
        res.update({'dW': p.linear.weight.grad.clone(), 'dgamma': p.norm.weight.grad.clone(), 'dbeta': p.norm.bias.grad.clone(),
                    'running_mean': p.norm.running_mean.detach().clone(), 'running_var': p.norm.running_var.detach().clone()})
    return res


def check_against(res, ref, e_ref_of, keys, label, factors=None):
    """every key: max|res - ref| <= FACTOR * e_ref (factors: {key: another factor}, for a quantity whose bar is stated where it is
    used), figures printed first -> list of failures"""
    bad = []
    for key in keys:
        err = float((res[key].double().cpu() - torch.as_tensor(ref[key]).double().cpu()).abs().max())
        e_ref = float(e_ref_of(key))
        print('%s %-13s err %.3g, e_ref %.3g, ratio %s' % (label, key, err, e_ref, ('%.2f' % (err / e_ref)) if e_ref > 0 else ('0/0' if err == 0 else 'inf')))
        if not err <= (factors or {}).get(key, FACTOR) * e_ref:
            bad.append((key, err, e_ref))
    return bad


# ---- the case builder -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.CASES))
def test_case_builder_terminates_inside_the_margins(name):
    case = cases.make_case(name)
    p = cases.CASES[name]
    assert case['voxels'].shape == (p['M'], p['T'], p['C']) and case['rounds'] < cases.MAX_ROUNDS
    w = cases.weights(p['C'])
    for training in (True, False):
        ratio, gap = cases.margins(cases.vfe_f64(case, w, training), case['num_points'])
        assert ratio.min() > 1.0 and gap.min() > cases.GAP, (training, ratio.min(), gap.min())
    n, T = case['num_points'], p['T']
    assert n.min() >= 1 and n.max() <= T
    assert (case['voxels'][np.arange(T)[None, :] >= n[:, None]] == 0).all()
    again = cases.make_case(name)
    assert np.array_equal(again['voxels'], case['voxels']) and np.array_equal(again['coords'], case['coords'])


def test_case_a_holds_the_edge_cases():
    case = cases.make_case('a')
    n, c = case['num_points'], case['coords']
    assert {1, 2, 31, 32} <= set(n.tolist())
    assert np.bincount(c[:, 0]).tolist() == [36, 1]
    cells = {(int(y), int(x)) for b, _, y, x in c if b == 0}
    assert (0, 0) in cells and (cases.GRID[1] - 1, cases.GRID[0] - 1) in cells
    lin = c[c[:, 0] == 0][:, 2] * cases.GRID[0] + c[c[:, 0] == 0][:, 3]
    assert (np.diff(lin) < 0).any()                                   # shuffled, not in scan order
    for g in cases.GARBAGE:
        v = cases.make_case(g)['voxels']
        pad = np.arange(32)[None, :] >= n[:, None]
        assert np.array_equal(v[~pad], case['voxels'][~pad]) and not (v[pad] == 0).any()


# ---- the host route against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.CASES))
def test_host_route_matches_the_reference(gold, name):
    case = cases.make_case(name)
    C = case['voxels'].shape[2]
    for training in (True, False):
        tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
        res = run_vfe(make_vfe(C), case, name, training)
        assert res['out'].shape == (len(case['num_points']), cases.COUT)                 # (1, 64) for one pillar, not (64,)
        keys = TRAIN_KEYS if training else ('out',)
        ref = {k: gold['%s_f64_%s' % (tag, k)] for k in keys}
        assert not check_against(res, ref, lambda k: gold['%s_e_ref_%s' % (tag, k)][0], keys, tag)
    d = cases.vfe_f64(case, cases.weights(C), True)
    assert np.abs(d['out'] - gold['vfe_%s_train_f64_out' % name]).max() < 1e-10      # the numpy definition is the reference's f64 run


def test_num_batches_tracked_and_state_dict_keys(gold):
    vfe = make_vfe(4)
    assert list(vfe.state_dict().keys()) == gold['vfe_keys'].tolist()
    run_vfe(vfe, cases.make_case('a'), 'a', True)
    assert int(vfe.pfn_layers[0].norm.num_batches_tracked) == 1


@pytest.mark.parametrize('garbage', list(cases.GARBAGE))
def test_host_route_ignores_the_padded_slots(garbage):
    clean = run_vfe(make_vfe(4), cases.make_case('a'), 'a', True)
    dirty = run_vfe(make_vfe(4), cases.make_case(garbage), 'a', True)
    for k in TRAIN_KEYS:
        assert torch.equal(clean[k], dirty[k]), k


def test_closed_form_gradients_equal_autograd_in_f64():
    """the sums the backward kernel forms (G1 = sum dy f^T, G0 = sum dy over the selected slots) and the moments, taken from the f64
    definition, through crbhip.pillar_vfe.batch_stats / param_grads against autograd of the host route in f64: train and eval"""
    from crbhip import pillar_vfe as pv
    for name in cases.CASES:
        case = cases.make_case(name)
        C = case['voxels'].shape[2]
        w = cases.weights(C)
        g = cases.grad_out(name).astype(np.float64)
        for training in (True, False):
            d = cases.vfe_f64(case, w, training)
            M, T, _ = d['pre'].shape
            f = torch.from_numpy(d['f'])
            sel = d['pre'].argmax(1)                                               # first maximal slot (padded ones hold f = 0)
            live = np.take_along_axis(d['pre'], sel[:, None, :], 1)[:, 0, :] > 0
            dy = torch.from_numpy(np.where(live, g, 0.0))
            fsel = f[torch.arange(M)[:, None], torch.from_numpy(sel)]              # (M, 64, K)
            G1, G0 = (dy[:, :, None] * fsel).sum(0), dy.sum(0)
            W = torch.from_numpy(w['pfn_layers.0.linear.weight']).double()
            n = float(M * T)
            if training:
                S1, S2 = f.reshape(-1, f.shape[-1]).sum(0), torch.einsum('mti,mtj->ij', f, f)
                mean, var, WS2 = pv.batch_stats(W, S1, S2, n)
                assert float((mean - torch.from_numpy(d['mean'])).abs().max()) < 1e-12
                assert float((var - torch.from_numpy(d['var'])).abs().max()) < 1e-10
            else:
                S1 = WS2 = None
                mean, var = torch.from_numpy(d['mean']), torch.from_numpy(d['var'])
            sigma = torch.sqrt(var + cases.EPS)
            scale = torch.from_numpy(w['pfn_layers.0.norm.weight']).double() / sigma
            dW, dgamma, dbeta = pv.param_grads(W, mean, sigma, scale, G1, G0, n, S1, WS2)
            ref = run_vfe(make_vfe(C, torch.float64), case, name, True, dtype=torch.float64) if training else None
            if not training:                                                       # eval-mode autograd: the frozen-BatchNorm path
                vfe = make_vfe(C, torch.float64).eval()
                out = vfe(case_batch(case, dtype=torch.float64))['pillar_features']
                (out * torch.from_numpy(g)).sum().backward()
                p = vfe.pfn_layers[0]
                ref = {'dW': p.linear.weight.grad, 'dgamma': p.norm.weight.grad, 'dbeta': p.norm.bias.grad}
            for key, val in (('dW', dW), ('dgamma', dgamma), ('dbeta', dbeta)):
                err, top = float((val - ref[key]).abs().max()), float(ref[key].abs().max())
                assert err <= 1e-10 * max(top, 1.0), (name, training, key, err, top)


# ---- scatter ----------------------------------------------------------------------------------------------------------------
def make_scatter():
    from pcdet.config import EasyDict
    from pcdet.models.backbones_2d.map_to_bev import PointPillarScatter
    return PointPillarScatter(model_cfg=EasyDict({'NUM_BEV_FEATURES': cases.COUT}), grid_size=cases.GRID)


def test_host_scatter_is_exact(gold):
    case = cases.make_case('a')
    bd = make_scatter()({'pillar_features': torch.from_numpy(gold['vfe_a_train_out']), 'voxel_coords': torch.from_numpy(case['coords']),
                         'batch_size': case['B']})
    assert np.array_equal(bd['spatial_features'].numpy(), gold['scatter_map'])


# ---- config, dataset, registries --------------------------------------------------------------------------------------------
def test_cfg_carries_the_yaml(gold):
    from pcdet.model_cfgs import pointpillar_cfg, pointpillar_dataset_args
    ref = json.loads(str(gold['cfg_json']))
    c = pointpillar_cfg()

    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        return [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
    assert plain(c.MODEL) == ref['MODEL']
    assert list(c.CLASS_NAMES) == ref['CLASS_NAMES']
    a = pointpillar_dataset_args(c)
    assert a['point_cloud_range'] == ref['POINT_CLOUD_RANGE'] and a['voxel_size'] == ref['VOXEL_SIZE']
    assert a['max_points_per_voxel'] == ref['MAX_POINTS_PER_VOXEL'] and a['max_num_voxels'] == ref['MAX_NUMBER_OF_VOXELS']
    assert [s.NAME for s in c.DATA_CONFIG.DATA_AUGMENTOR.AUG_CONFIG_LIST] == ref['AUG_NAMES']
    n = c.MODEL.POST_PROCESSING.NMS_CONFIG
    assert (n.NMS_THRESH, n.NMS_PRE_MAXSIZE, n.NMS_POST_MAXSIZE) == (0.01, 4096, 500)


def test_synthetic_dataset_arguments():
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets import synthetic as syn
    from pcdet.model_cfgs import pointpillar_dataset_args
    for ds in (SyntheticDataset(), SyntheticDataset(4, 1000, 'kitti'), SyntheticDataset(num_frames=2, kind='kitti')):
        assert ds.voxel_size == list(syn.KITTI_VOXEL) and ds.grid_size.tolist() == [1408, 1600, 40]
        assert np.array_equal(ds.point_cloud_range, np.array(syn.KITTI_RANGE, np.float32)) and ds.point_cloud_range.dtype == np.float32
        assert ds.max_points_per_voxel == 5 and ds.max_num_voxels == {'train': 16000, 'test': 40000}
    w = SyntheticDataset(num_frames=2, kind='waymo')
    assert w.voxel_size == list(syn.WAYMO_VOXEL) and w.max_num_voxels == {'train': 150000, 'test': 150000} and w.max_points_per_voxel == 5
    ds = SyntheticDataset(num_frames=2, **pointpillar_dataset_args())
    assert ds.grid_size.tolist() == [432, 496, 1] and ds.grid_size.dtype == np.int64
    assert ds.max_points_per_voxel == 32 and ds.max_num_voxels == {'train': 16000, 'test': 40000} and ds.voxel_size == [0.16, 0.16, 4.0]


def test_registries_and_detector_state_dict(gold):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pointpillar_cfg
    from pcdet.models import build_network
    from pcdet.models.backbones_2d import map_to_bev
    from pcdet.models.backbones_3d import vfe
    from pcdet.models import detectors
    assert 'PillarVFE' in vfe.__all__ and 'PointPillarScatter' in map_to_bev.__all__ and 'PointPillar' in detectors.__all__
    c = pointpillar_cfg()
    ds = SyntheticDataset(num_frames=2, point_cloud_range=cases.PCR, voxel_size=cases.VOXEL, max_points_per_voxel=32)
    model = build_network(c.MODEL, 3, ds)
    assert list(model.state_dict().keys()) == gold['det_keys'].tolist()
    assert type(model).__name__ == 'PointPillar' and getattr(model, 'backbone_3d', None) is None
    over = cases.golden_bias_overrides(gold)                         # one shifted bias per BatchNorm of the step, all small shifts
    sd = model.state_dict()
    assert len(over) == 20 and all(k in sd and k.endswith('.bias') for k in over)
    seeded = cases.detector_state([(k, tuple(v.shape), v.dtype.is_floating_point) for k, v in sd.items()])
    assert max(float(np.abs(over[k] - seeded[k]).max()) for k in over) < 0.01


def test_nudge_bias_clears_the_margin():
    rng = np.random.default_rng(0)
    for n in (1, 5, 512, 8192):
        v = rng.normal(0, 1, n)
        v[0] = 1e-7
        d = cases.nudge_bias(v)
        assert np.abs(v + d).min() > cases.DET_KINK and abs(d) < 0.05
    assert cases.nudge_bias(np.array([0.5, -0.3])) == 0.0


# ---- unsupported configurations, refusals -------------------------------------------------------------------------------
def test_unsupported_config_builds_and_takes_the_torch_route():
    case = cases.make_case('a')
    for kw in (dict(num_filters=(32, 64)), dict(with_distance=True), dict(use_absolute_xyz=False), dict(num_filters=(48,))):
        vfe = make_vfe(4, **kw).train()
        assert vfe.unsupported_reason(4, 32) is not None, kw
        with warnings.catch_warnings():
            warnings.simplefilter('error')                       # host tensors: the torch route is the route, nothing to announce
            out = vfe(case_batch(case))['pillar_features']
        assert out.shape == (37, vfe.get_output_feature_dim()) and torch.isfinite(out).all()
    assert make_vfe(4).unsupported_reason(4, 32) is None
    assert make_vfe(4).unsupported_reason(4, 33) is not None and make_vfe(4).unsupported_reason(6, 32) is not None


def test_no_pillars_give_an_empty_feature_tensor():
    vfe = make_vfe(4).train()
    bd = vfe({'voxels': torch.zeros((0, 32, 4)), 'voxel_num_points': torch.zeros((0,), dtype=torch.int32),
              'voxel_coords': torch.zeros((0, 4), dtype=torch.int32), 'batch_size': 2})
    assert bd['pillar_features'].shape == (0, 64)
    bev = make_scatter()(bd)['spatial_features']
    assert bev.shape == (2, 64, cases.GRID[1], cases.GRID[0]) and not bev.any()
    assert int(vfe.pfn_layers[0].norm.num_batches_tracked) == 0


def test_supported_predicate():
    import crbhip
    from crbhip import pillar_vfe as pv
    for C, T, Cout, ok in ((4, 32, 64, 1), (5, 20, 64, 1), (4, 1, 64, 1), (5, 32, 64, 1), (3, 32, 64, 0), (6, 32, 64, 0), (4, 0, 64, 0),
                           (4, 33, 64, 0), (4, 32, 32, 0), (4, 32, 128, 0)):
        assert crbhip.lib.crb_pillar_vfe_supported(C, T, Cout) == ok, (C, T, Cout)
        assert pv.supported(C, T, Cout) == bool(ok)
    assert crbhip.lib.crb_pillar_vfe_num_moments(4) == 65 and crbhip.lib.crb_pillar_vfe_num_moments(5) == 77


def test_binding_refuses_host_tensors():
    import crbhip
    from crbhip import pillar_vfe as pv
    case = cases.make_case('c')
    w = {k: torch.from_numpy(np.asarray(v)) for k, v in cases.weights(4).items()}
    v, n, c = torch.from_numpy(case['voxels']), torch.from_numpy(case['num_points']), torch.from_numpy(case['coords'])
    with pytest.raises(crbhip.CrbHipError):
        pv.pillar_vfe(v, n, c, w['pfn_layers.0.linear.weight'], w['pfn_layers.0.norm.weight'], w['pfn_layers.0.norm.bias'],
                      w['pfn_layers.0.norm.running_mean'], w['pfn_layers.0.norm.running_var'], True, 0.01, 1e-3, cases.VOXEL, cases.offsets())
    with pytest.raises(crbhip.CrbHipError):
        pv.moments(v, n, c, cases.VOXEL, cases.offsets())
