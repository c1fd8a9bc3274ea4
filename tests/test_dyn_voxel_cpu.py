"""CPU: dynamic voxelization. The registry builds DynMeanVFE; its torch route (the definition of the device route) against the golden
written by the reference's own DynamicMeanVFE and against the numpy definition of tests/dyn_voxel_cases.py; the dropped-point rules.

Bars. voxel_coords and the row order: exactly the reference's. voxel_features in f32: max|torch route - f64 means| <= 4 * e_ref,
e_ref = max|reference f32 - f64 means of the same voxels| (golden), the project's bar for an f32 route. The torch route on f64
points (cases without face points): the f64 means to 1e-12 (sums of at most 40 values below 10)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_voxel_cases as cases

FACTOR = 4.0
GOLD_CASES = [n for n in cases.CASES if n != 'empty']


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def make_vfe(C, mode='voxel', dev=None):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d import vfe
    m = vfe.__all__['DynMeanVFE'](model_cfg=EasyDict({'NAME': 'DynMeanVFE'}), num_point_features=C, voxel_size=cases.VOXEL[mode],
                                  grid_size=cases.GRID[mode], point_cloud_range=cases.PCR)
    return m if dev is None else m.to(dev)


def run_vfe(points, B, dev=None, dtype=torch.float32):
    t = torch.from_numpy(points).to(dtype)
    bd = make_vfe(points.shape[1] - 1, dev=dev)({'points': t if dev is None else t.to(dev), 'batch_size': B})
    return bd['voxel_features'].cpu().numpy(), bd['voxel_coords'].cpu().numpy()


def test_registry_builds_the_module():
    from pcdet.models.backbones_3d import vfe
    from pcdet.models.backbones_3d.vfe.dynamic_mean_vfe import DynamicMeanVFE
    assert vfe.__all__['DynMeanVFE'] is DynamicMeanVFE
    m = make_vfe(5)
    assert m.get_output_feature_dim() == 5 and list(m.state_dict().keys()) == []


def test_second_builds_with_the_dynamic_vfe():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    cfg = second_cfg()
    cfg.MODEL.VFE.NAME = 'DynMeanVFE'
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2))
    assert type(model.vfe).__name__ == 'DynamicMeanVFE' and model.backbone_3d is not None


@pytest.mark.parametrize('name', GOLD_CASES)
def test_torch_route_equals_the_reference(gold, name):
    case = cases.make_case(name)
    feats, coords = run_vfe(case['points'], case['B'])
    assert coords.dtype == np.int32 and coords.shape == gold['mean_%s_coords' % name].shape
    assert (coords == gold['mean_%s_coords' % name]).all()                  # the NaN rows the reference never saw change nothing
    d = cases.definition(case['points'], case['B'], 'voxel')
    e_ref = float(gold['mean_%s_e_ref' % name][0])
    err = np.abs(feats.astype(np.float64) - d['mean64']).max()
    print('case %s: torch route f32 against the f64 means %.3g, e_ref %.3g' % (name, err, e_ref))
    assert err <= FACTOR * e_ref
    assert np.abs(gold['mean_%s_features' % name].astype(np.float64) - d['mean64']).max() == e_ref
    if name != 'a':                       # (an f64 run forms the cells in f64: the face points of case a land in other voxels)
        f64, c64 = run_vfe(case['points'], case['B'], dtype=torch.float64)
        assert (c64 == coords).all() and np.abs(f64 - d['mean64']).max() <= 1e-12


@pytest.mark.parametrize('name', list(cases.CASES))
@pytest.mark.parametrize('mode', cases.MODES)
def test_definition_equals_the_reference_grouping(gold, name, mode):
    case = cases.make_case(name)
    d = cases.definition(case['points'], case['B'], mode)
    if name == 'empty':
        assert d['coords'].shape == (0, 4) and list(d['seg_offsets']) == [0] and len(d['perm']) == 0
        return
    ref = gold['%s_%s_coords' % ('mean' if mode == 'voxel' else 'pillar', name)]
    assert d['coords'].shape == ref.shape and (d['coords'] == ref).all()
    assert (d['coords'][:, 1] == 0).all() or mode == 'voxel'
    # every kept row once, rows of a voxel in input order, voxels in ascending key order
    assert len(set(d['perm'].tolist())) == len(d['perm']) == d['seg_offsets'][-1]
    for v in range(len(d['coords'])):
        seg = d['perm'][d['seg_offsets'][v]:d['seg_offsets'][v + 1]]
        assert len(seg) >= 1 and (np.diff(seg) > 0).all()


def test_case_a_holds_what_it_promises():
    case = cases.make_case('a')
    pts = case['points']
    assert len(pts) % 256 != 0 and not (pts[:, 0] == 1).any()
    d = cases.definition(pts, case['B'], 'pillar')
    sizes = np.diff(d['seg_offsets'])
    nx, ny, _ = cases.GRID['pillar']
    for s in (1, 2, 63, 64, 65):
        assert (sizes == s).any(), s
    assert sizes.max() >= 300
    have = {(int(c[3]), int(c[2])) for c in d['coords']}
    assert {(0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)} <= have
    assert np.abs(np.diff(pts[:, 0])).sum() > 100                           # frames interleave in the input


def test_dropped_point_rules():
    C, B = 4, 2
    f = [0.5]
    rows = {
        'inside': [0, 0.1, 0.1, 0.1] + f, 'x high': [0, 5.62, 0.1, 0.1] + f, 'x low': [0, -5.22, 0.1, 0.1] + f,
        'y high': [0, 0.1, 3.94, 0.1] + f, 'y low': [0, 0.1, -3.94, 0.1] + f, 'z high': [0, 0.1, 0.1, 4.5] + f,
        'z low': [0, 0.1, 0.1, -2.5] + f, 'x at the maximum': [0, 5.12, 0.1, 0.1] + f, 'x at the minimum': [0, -5.12, 0.1, 0.1] + f,
        'y at the maximum': [1, 0.1, 3.84, 0.1] + f, 'z at the maximum': [1, 0.1, 0.1, 4.0] + f, 'NaN x': [1, np.nan, 0.1, 0.1] + f,
        'NaN z': [1, 0.1, 0.1, np.nan] + f, 'frame -1': [-1, 0.1, 0.1, 0.1] + f, 'frame B': [B, 0.1, 0.1, 0.1] + f,
    }
    kept = {'pillar': {'inside', 'z high', 'z low', 'x at the minimum', 'z at the maximum'}, 'voxel': {'inside', 'x at the minimum'}}
    names = list(rows)
    pts = np.asarray([rows[n] for n in names], np.float32)
    for mode in cases.MODES:
        d = cases.definition(pts, B, mode)
        assert {names[i] for i in d['perm']} == kept[mode], mode
    _, coords = run_vfe(pts, B)
    assert (coords == cases.definition(pts, B, 'voxel')['coords']).all() and len(coords) == 2


def test_empty_input_and_empty_result():
    case = cases.make_case('empty')
    for pts in (case['points'], case['points'][:0]):
        feats, coords = run_vfe(pts, case['B'])
        assert feats.shape == (0, case['C']) and coords.shape == (0, 4) and coords.dtype == np.int32
