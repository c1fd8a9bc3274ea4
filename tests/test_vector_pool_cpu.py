"""CPU: VectorPool aggregation. The numpy restatements of the reference kernels (tests/vector_pool_cases.py) against
tests/golden/ref_vector_pool.npz, written by the reference's own autograd Functions and VectorPoolAggregationModuleMSG on the CPU
(tests/golden/make_goldens_vector_pool.py); the torch route of the port's ops and modules on host tensors against the same file; the
parameter names; the config builder; what raises."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vector_pool_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))
_gold = {}
t = torch.from_numpy


def gold():
    if not _gold:
        _gold.update(np.load(os.path.join(HERE, 'golden', 'ref_vector_pool.npz')))
    return _gold


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize('name', sorted(vc.three_nn_cases()))
def test_three_nn_restatement_and_host_route_reproduce_the_reference(name):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    c, g = vc.three_nn_cases()[name], gold()
    idx, dist, lens = vc.three_nn(c['support'], c['xyz_cnt'], c['new_xyz'], c['new_cnt'], c['centers'], c['R'] * c['mult'], c['nsample'], c['ntype'])
    assert np.array_equal(idx, g['nn/%s/idx' % name])
    # the golden's square root is the generating host's vectorised f32 sqrt, which is not correctly rounded: one ulp; the squared
    # distances behind it are the restatement's own (the reference's Function only takes their root)
    want = g['nn/%s/dist' % name]
    assert np.array_equal(np.isinf(dist), np.isinf(want))
    fin = np.isfinite(want)
    assert (np.abs(dist[fin] - want[fin]) <= np.spacing(want[fin])).all()
    d2, i2, avg = pu.three_nn_for_vector_pool_by_two_step(t(c['support']), t(c['xyz_cnt']), t(c['new_xyz']), t(c['centers']), t(c['new_cnt']),
                                                          c['R'], c['nsample'], c['ntype'], 123, c['centers'].shape[1], c['mult'])
    assert i2.dtype == torch.int32 and np.array_equal(i2.numpy(), idx) and np.array_equal(bits(d2.numpy()), bits(dist))
    assert int(avg) == 123                                                   # handed back: nothing is sized by it
    # what the case is there for
    if name.startswith('count_'):
        k = int(name.split('_')[1])
        assert lens.tolist() == [k]
        assert bool((idx[0, :, 2] == idx[0, :, 0]).all()) == (k < 3) and bool((idx[0, :, 1] == idx[0, :, 0]).all()) == (k < 2)
    if name == 'past_1000':
        assert lens.tolist() == [1000] and idx.max() < 1000
        d = np.linalg.norm(c['support'][:, None, :].astype(np.float64) - c['centers'][0][None], axis=2)
        assert (np.argsort(d, axis=0)[:3] >= 1000).all()                     # the three nearest of EVERY cell lie past the cap
    if name == 'nsample_5':
        assert lens.tolist() == [5, 5, 5] and idx.max() < 5
    if name == 'other_frame':
        assert (idx[0] == -1).all() and np.isinf(dist[0]).all() and (idx[1] >= 20).all() and (idx[2] == -1).all()
    if name == 'n_zero':
        assert (idx == -1).all() and np.isposinf(dist).all()
    if name.startswith('lattice'):
        local = c['support'][None] - c['new_xyz'][:, None]
        q = np.float32(c['R'] * c['mult'])
        on = (np.abs(local).max(2) == q) if c['ntype'] == 0 else ((local * local).sum(2) == q * q)
        assert on.sum() >= 3                                                 # points exactly on the face / sphere exist and stay
        lists = vc.query_neighbors(c['support'], c['xyz_cnt'], c['new_xyz'], c['new_cnt'], q, -1, c['ntype'])
        assert all(set(np.nonzero(on[m])[0]) <= set(lists[m]) for m in range(len(lists)))
        assert any(len(np.unique(dist[m, g_])) < 3 for m in range(dist.shape[0]) for g_ in range(dist.shape[1]))   # exact ties
    if name.startswith('frames'):
        assert len(c['new_xyz']) % 4 != 0 and 0 in c['new_cnt'].tolist() and c['xyz_cnt'].tolist() == [0, 1, 301]


@pytest.mark.parametrize('name', sorted(vc.voxel_cases()))
def test_voxel_pool_restatement_and_host_route_reproduce_the_reference(name):
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as pu
    c, g = vc.voxel_cases()[name], gold()
    pre = 'voxel/%s/' % name
    f, l, cnt, pick = vc.voxel_pool(c['support'], c['xyz_cnt'], c['feats'], c['new_xyz'], c['new_cnt'], c['grid'], c['R'], c['nsample'], c['ntype'])
    assert np.array_equal(bits(f), bits(g[pre + 'features'])) and np.array_equal(bits(l), bits(g[pre + 'local_xyz']))
    assert np.array_equal(cnt, g[pre + 'cnt'])
    grad = vc.voxel_pool_grad(g[pre + 'probe'], pick, len(c['support']))
    assert np.array_equal(bits(grad), bits(g[pre + 'grad']))
    feats = t(c['feats']).requires_grad_(True)
    f2, l2, mean, cnt2 = pu.vector_pool_with_voxel_query_op(t(c['support']), t(c['xyz_cnt']), feats, t(c['new_xyz']), t(c['new_cnt']), *c['grid'],
                                                           c['R'], c['feats'].shape[1], 1, 77, c['nsample'], c['ntype'], 1)
    assert np.array_equal(bits(f2.detach().numpy()), bits(f)) and np.array_equal(bits(l2.numpy()), bits(l))
    assert cnt2.dtype == torch.int32 and np.array_equal(cnt2.numpy(), cnt) and mean.tolist() == [77] and not l2.requires_grad
    if len(c['support']):
        (f2 * t(g[pre + 'probe'])).sum().backward()
        np.testing.assert_allclose(feats.grad.numpy(), grad, rtol=1e-6, atol=1e-6)
    limit = c['nsample'] if c['nsample'] > 0 else 27
    assert cnt.sum(1).max() <= limit
    if name == 'voxel_t0_n-1':
        # local = +R on every axis: per-axis index 3, combined 39, clamped to the last cell; -R: the first cell
        assert pick[0, 26] == 0 and pick[0, 0] == 1
        # (+R, -R, 0.25) -> 3 * 9 + 0 + 2 = 29 -> clamped to cell 26 (taken), not to cell (2, 0, 2) = 20: the clamp comes after combining
        assert pick[0, 20] != 2 and 2 not in pick[0]
        # (-R, 0.25, +R) -> 0 + 2 * 3 + 3 = 9: lands in cell (1, 0, 0) as in the reference
        assert pick[0, 9] == 9
        assert pick[0, 1 * 9 + 2 * 3 + 1] == 3                               # the boundaries -0.25 / 0.25 belong to the upper cell
        assert pick[0, 13] == 6 and 7 not in pick[0]                         # two points in the centre cell: the lower row wins
        assert (pick[4] == -1).all() and (pick[5:7] == -1).all() and (pick[9] == -1).all()   # nothing near / no support points / other frame
        assert (pick[7:9][pick[7:9] >= 0] >= 131).all() and (pick[7:9] >= 0).any()


@pytest.mark.parametrize('name', sorted(vc.module_cfgs()))
def test_module_on_the_host_matches_the_reference_module(name):
    """the same f32 expressions on the same host: rounding differences only (1e-4 of the largest output, 1e-3 of the largest
    gradient entry after four train-mode BatchNorm layers over 37 rows)"""
    vc.check_module(name, gold(), vc.run_module(name, gold(), 'cpu'), 1e-4, 1e-3)


def test_dense_voxel_centres_are_z_fastest():
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules import VectorPoolAggregationModule as M
    new = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.25]], np.float32)
    for grid, R in (((2, 2, 2), 0.2), ((3, 3, 3), 0.4), ((1, 2, 3), 1.2)):
        got = M.get_dense_voxels_by_center(t(new), R, grid).numpy()
        assert got.shape == (2, int(np.prod(grid)), 3)
        np.testing.assert_allclose(got, vc.grid_centers(new, R, grid), rtol=0, atol=1e-6)
    assert got[0, 1, 2] > got[0, 0, 2] and got[0, 1, 0] == got[0, 0, 0]


def test_what_raises():
    from pcdet.config import EasyDict
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm, pointnet2_utils as pu
    _, cfg = vc.module_cfgs()['voxel']
    cfg = dict(cfg, LOCAL_AGGREGATION_TYPE='voxel_avg_pool')
    with pytest.raises(NotImplementedError, match='voxel_avg_pool'):
        pm.build_local_aggregation_module(8, EasyDict(cfg))
    c = vc.voxel_cases()['voxel_t0_n-1']
    args = (t(c['support']), t(c['xyz_cnt']), t(c['feats']), t(c['new_xyz']), t(c['new_cnt']), 3, 3, 3, c['R'])
    with pytest.raises(NotImplementedError, match='pooling_type 0'):
        pu.vector_pool_with_voxel_query_op(*args, 4, 1, 20, -1, 0, 0)
    with pytest.raises(NotImplementedError, match='num_c_in'):
        pu.vector_pool_with_voxel_query_op(*args, 2, 1, 20, -1, 0, 1)
    # a StackSAModuleMSG section with only its NAME changed cannot describe the layer: the message names what is missing
    sa = EasyDict({'NAME': 'VectorPoolAggregationModuleMSG', 'MLPS': [[8, 8]], 'POOL_RADIUS': [0.4], 'NSAMPLE': [16]})
    with pytest.raises(NotImplementedError) as e:
        pm.build_local_aggregation_module(4, sa)
    msg = str(e.value)
    assert all(k in msg for k in ('vector_pool', 'pv_rcnn_plusplus_cfg', 'NUM_GROUPS', 'GROUP_CFG_0', 'MSG_POST_MLPS', 'LOCAL_AGGREGATION_TYPE'))
    with pytest.raises(NotImplementedError):
        pm.build_local_aggregation_module(4, EasyDict({'NAME': 'SomethingElse'}))


def test_config_builder():
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    for kind in ('kitti', 'waymo'):
        assert pv_rcnn_plusplus_cfg(kind) == pv_rcnn_plusplus_cfg(kind, aggregation='sa')
        base, c = pv_rcnn_plusplus_cfg(kind).MODEL, pv_rcnn_plusplus_cfg(kind, aggregation='vector_pool').MODEL
        assert 'NAME' not in base.ROI_HEAD.ROI_GRID_POOL and 'MLPS' in base.PFE.SA_LAYER.raw_points
        sa, pool = c.PFE.SA_LAYER, c.ROI_HEAD.ROI_GRID_POOL
        assert sorted(sa.keys()) == ['raw_points', 'x_conv3', 'x_conv4']
        for src, radius, reduced, msg, dists in (('raw_points', 2.4, 1 if kind == 'kitti' else 2, [32], (0.2, 0.4)),
                                                 ('x_conv3', 4.0, 32, [128], (1.2, 2.4)), ('x_conv4', 6.4, 32, [128], (2.4, 4.8))):
            s = sa[src]
            assert s.NAME == 'VectorPoolAggregationModuleMSG' and s.NUM_GROUPS == 2 and s.LOCAL_AGGREGATION_TYPE == 'local_interpolation'
            assert s.NUM_REDUCED_CHANNELS == reduced and s.NUM_CHANNELS_OF_LOCAL_AGGREGATION == 32 and s.MSG_POST_MLPS == msg
            assert s.FILTER_NEIGHBOR_WITH_ROI is True and s.RADIUS_OF_NEIGHBOR_WITH_ROI == radius
            assert (s.GROUP_CFG_0.MAX_NEIGHBOR_DISTANCE, s.GROUP_CFG_1.MAX_NEIGHBOR_DISTANCE) == dists
            assert s.GROUP_CFG_0.NEIGHBOR_NSAMPLE == -1 and s.GROUP_CFG_1.NUM_LOCAL_VOXEL == [3, 3, 3]
        assert sa.raw_points.GROUP_CFG_0.NUM_LOCAL_VOXEL == [2, 2, 2] and sa.raw_points.GROUP_CFG_0.POST_MLPS == [32, 32]
        assert sa.x_conv3.DOWNSAMPLE_FACTOR == 4 and sa.x_conv4.DOWNSAMPLE_FACTOR == 8 and sa.x_conv4.INPUT_CHANNELS == 64
        assert pool.NAME == 'VectorPoolAggregationModuleMSG' and pool.LOCAL_AGGREGATION_TYPE == 'voxel_random_choice' and pool.GRID_SIZE == 6
        assert pool.NUM_REDUCED_CHANNELS == 30 and pool.MSG_POST_MLPS == [128]
        assert (pool.GROUP_CFG_0.MAX_NEIGHBOR_DISTANCE, pool.GROUP_CFG_1.MAX_NEIGHBOR_DISTANCE) == (0.8, 1.6)
        assert pool.GROUP_CFG_0.NEIGHBOR_NSAMPLE == 32 and pool.GROUP_CFG_1.POST_MLPS == [64, 64]
        c.PFE.SA_LAYER = base.PFE.SA_LAYER
        c.ROI_HEAD.ROI_GRID_POOL = base.ROI_HEAD.ROI_GRID_POOL
        assert c == base                                                     # nothing else differs


def test_detector_builds_with_the_reference_parameter_names():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules import VectorPoolAggregationModuleMSG
    G = np.load(os.path.join(HERE, 'golden', 'ref_pvrcnn_plusplus_vp.npz'))
    cfg = pv_rcnn_plusplus_cfg('kitti', aggregation='vector_pool').MODEL
    cfg.ROI_HEAD.DP_RATIO = 0.0                                              # (as the golden's step: no Dropout module in shared_fc_layer)
    model = build_network(cfg, 3, SyntheticDataset(num_frames=2, n_points=2000))
    assert type(model).__name__ == 'PVRCNNPlusPlus'
    keys = sorted(model.state_dict().keys())
    assert keys == list(G['pv_keys'])
    for part in ('layer_0.separate_local_aggregation_layer.0.weight', 'layer_1.separate_local_aggregation_layer.1.running_var',
                 'layer_1.post_mlps.3.weight', 'msg_post_mlps.1.num_batches_tracked'):
        assert 'roi_head.roi_grid_pool_layer.' + part in keys and 'pfe.SA_rawpoints.' + part in keys and 'pfe.SA_layers.1.' + part in keys
    assert all(isinstance(m, VectorPoolAggregationModuleMSG) for m in (model.pfe.SA_rawpoints, model.pfe.SA_layers[0], model.roi_head.roi_grid_pool_layer))
    w = model.pfe.SA_layers[0].layer_0.separate_local_aggregation_layer[0].weight
    assert tuple(w.shape) == (27 * 32, 32 + 9, 1)
    assert tuple(model.roi_head.roi_grid_pool_layer.layer_0.separate_local_aggregation_layer[0].weight.shape) == (27 * 32, 30 + 3, 1)
