"""GPU: dynamic voxelization. csrc/dyn_voxelize.hip (crb_dyn_voxelize in both modes, crb_dyn_mean_vfe) through crbhip.dyn_vfe and
DynMeanVFE against the numpy definition of tests/dyn_voxel_cases.py and the golden of the reference's own modules; SECOND with
VFE.NAME = 'DynMeanVFE' on device points.

Bars. coords, seg_offsets and the per-voxel point lists: bit-equal to the definition (and coords to the reference's) on every case,
the empty frame, the face points, the NaN points and the empty input included. Means: within 1 ulp of the f64 means rounded to f32
(the kernel sums in f64 in segment order and rounds once; the division is one more f64 rounding before it) and bit-equal across two
calls. A permutation of the input changes the order of the f64 sums only: same voxels, means within the same 1 ulp."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_voxel_cases as cases
import test_dyn_voxel_cpu as cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def _voxelize(points, B, mode, dev):
    from crbhip import dyn_vfe
    t = torch.from_numpy(points).to(dev)
    r = dyn_vfe.dyn_voxelize(t, B, cases.PCR, cases.VOXEL[mode], cases.GRID[mode], dyn_vfe.PILLAR if mode == 'pillar' else dyn_vfe.VOXEL)
    mean = dyn_vfe.dyn_mean(t, r['perm'], r['seg_offsets'])
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in dict(r, mean=mean).items()}


def _assert_equals_definition(r, d):
    assert r['M'] == len(d['coords']) and r['Nk'] == len(d['perm'])
    assert r['coords'].shape == d['coords'].shape and (r['coords'] == d['coords']).all()
    assert (r['seg_offsets'] == d['seg_offsets']).all() and (r['perm'] == d['perm']).all()
    assert r['mean'].shape == d['mean'].shape
    ulp = cases.ulp_distance(r['mean'], d['mean'])
    print('means: %d ulp from the f64 means rounded to f32' % ulp)
    assert ulp <= 1


@pytest.mark.parametrize('name', list(cases.CASES))
@pytest.mark.parametrize('mode', cases.MODES)
def test_voxelization_and_mean_equal_the_definition(dev, gold, name, mode):
    case = cases.make_case(name)
    r = _voxelize(case['points'], case['B'], mode, dev)
    _assert_equals_definition(r, cases.definition(case['points'], case['B'], mode))
    if name != 'empty':
        assert (r['coords'] == gold['%s_%s_coords' % ('mean' if mode == 'voxel' else 'pillar', name)]).all()
    again = _voxelize(case['points'], case['B'], mode, dev)
    for k in ('coords', 'seg_offsets', 'perm', 'mean'):
        assert r[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize('mode', cases.MODES)
def test_no_points_at_all(dev, mode):
    r = _voxelize(np.zeros((0, 5), np.float32), 2, mode, dev)
    assert r['M'] == 0 and r['Nk'] == 0 and r['coords'].shape == (0, 4) and list(r['seg_offsets']) == [0] and r['mean'].shape == (0, 4)


@pytest.mark.parametrize('mode', cases.MODES)
def test_permuted_input_gives_the_same_voxels(dev, mode):
    case = cases.make_case('a')
    p = np.random.default_rng(5).permutation(len(case['points']))
    a, b = _voxelize(case['points'], case['B'], mode, dev), _voxelize(case['points'][p], case['B'], mode, dev)
    assert (a['coords'] == b['coords']).all() and (a['seg_offsets'] == b['seg_offsets']).all()
    for v in range(a['M']):                                                  # the same rows per voxel, each list in its input's order
        sa, sb = a['perm'][a['seg_offsets'][v]:a['seg_offsets'][v + 1]], b['perm'][b['seg_offsets'][v]:b['seg_offsets'][v + 1]]
        assert (np.diff(sb) > 0).all() and sorted(p[sb].tolist()) == sa.tolist()
    _assert_equals_definition(b, cases.definition(case['points'][p], case['B'], mode))


def test_keys_beyond_31_bits(dev):
    """2 frames x 2048 x 2048 x 1024 cells = 2^33 keys: the reference's int32 key would wrap, the 64-bit one orders the voxels"""
    from crbhip import dyn_vfe
    rng = np.random.default_rng(9)
    grid, voxel, pcr = [2048, 2048, 1024], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0, 1024.0, 1024.0, 512.0]
    n = 300
    cells = np.stack([rng.integers(0, 2, n), rng.integers(0, 2048, n), rng.integers(0, 2048, n), rng.integers(0, 1024, n)], 1)
    cells[:4] = [[1, 2047, 2047, 1023], [0, 0, 0, 0], [1, 0, 0, 0], [0, 2047, 2047, 1023]]
    cells = np.concatenate([cells, cells[:50]])                              # some voxels hold two points
    pts = np.concatenate([cells[:, :1], (cells[:, 1:] + 0.5) * 0.5, rng.uniform(0, 1, (len(cells), 1))], 1).astype(np.float32)
    t = torch.from_numpy(pts).to(dev)
    r = dyn_vfe.dyn_voxelize(t, 2, pcr, voxel, grid, dyn_vfe.VOXEL)
    key = ((cells[:, 0] * 2048 + cells[:, 1]) * 2048 + cells[:, 2]) * 1024 + cells[:, 3]
    assert key.max() >= 2 ** 32
    uk, first = np.unique(key, return_index=True)
    want = cells[first][:, [0, 3, 2, 1]]
    assert r['M'] == len(uk) and r['Nk'] == len(pts) and (r['coords'].cpu().numpy() == want).all()
    order = np.argsort(key, kind='stable')
    assert (r['perm'].cpu().numpy() == order).all()


def test_module_on_the_device_equals_its_torch_route(dev, gold):
    case = cases.make_case('a')
    f_dev, c_dev = cpu.run_vfe(case['points'], case['B'], dev=dev)
    f_cpu, c_cpu = cpu.run_vfe(case['points'], case['B'])
    assert c_dev.dtype == np.int32 and (c_dev == c_cpu).all()
    d = cases.definition(case['points'], case['B'], 'voxel')
    err, e_ref = np.abs(f_dev.astype(np.float64) - d['mean64']).max(), float(gold['mean_a_e_ref'][0])
    print('device route against the f64 means %.3g, torch route %.3g, e_ref %.3g' % (
        err, np.abs(f_cpu.astype(np.float64) - d['mean64']).max(), e_ref))
    assert err <= cpu.FACTOR * e_ref and cases.ulp_distance(f_dev, d['mean']) <= 1


def test_binding_answers_bad_arguments(dev):
    from crbhip import CrbHipError, dyn_vfe, lib, ptr, host_f32x3, host_i32x3, cur_stream
    pts = torch.from_numpy(cases.make_case('c')['points']).to(dev)
    with pytest.raises(CrbHipError):
        dyn_vfe.dyn_voxelize(pts, 1, cases.PCR, cases.VOXEL['voxel'], cases.GRID['voxel'], 2)
    with pytest.raises(CrbHipError):
        dyn_vfe.dyn_voxelize(pts.cpu(), 1, cases.PCR, cases.VOXEL['voxel'], cases.GRID['voxel'], dyn_vfe.VOXEL)
    with pytest.raises(CrbHipError):
        dyn_vfe.dyn_voxelize(pts.double(), 1, cases.PCR, cases.VOXEL['voxel'], cases.GRID['voxel'], dyn_vfe.VOXEL)
    # output buffers smaller than the input can fill are refused before anything is launched (CRB_ERR_ARG = -1)
    i32 = lambda n: torch.empty((n,), dtype=torch.int32, device=dev)
    nbytes = int(lib.crb_dyn_voxelize_workspace_bytes(2))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    rc = lib.crb_dyn_voxelize(ptr(pts), 2, 5, 1, dyn_vfe.VOXEL, host_f32x3(cases.PCR[:3]), host_f32x3(cases.VOXEL['voxel']),
                              host_i32x3(cases.GRID['voxel']), 1, ptr(i32(2)), ptr(i32(2)), ptr(i32(4)), ptr(i32(2)), ptr(ws), nbytes,
                              cur_stream(dev))
    assert rc == -1
    rc = lib.crb_dyn_voxelize(ptr(pts), 2, 5, 1, dyn_vfe.VOXEL, host_f32x3(cases.PCR[:3]), host_f32x3(cases.VOXEL['voxel']),
                              host_i32x3(cases.GRID['voxel']), 2, ptr(i32(2)), ptr(i32(3)), ptr(i32(8)), ptr(i32(2)), ptr(ws), 16,
                              cur_stream(dev))
    assert rc == -2                                                          # CRB_ERR_WORKSPACE


def test_second_trains_behind_the_dynamic_vfe(dev):
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    cfg = second_cfg()
    cfg.MODEL.VFE.NAME = 'DynMeanVFE'
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2)).to(dev).train()
    pts, off, gt = kitti_batch(0, 2, 8000)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))[:, None]
    batch = {'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': 2}
    ret, tb, _ = model(batch)
    ret['loss'].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(ret['loss'])
    missing = [n for n, t in model.named_parameters() if t.grad is None or not torch.isfinite(t.grad).all()]
    assert not missing, missing
