"""CPU: SPC keypoint sampling. The torch route (the reference's expressions as torch ops, pcdet/models/backbones_3d/pfe/
voxel_set_abstraction.py) on host tensors against tests/golden/ref_spc.npz, written by the reference's own sample_points_with_roi,
sector_fps and VoxelSetAbstraction.get_sampled_points (tests/golden/make_goldens_spc.py): masks, segment lengths, quotas and
picked rows bit-equal. The case generator's margins, the quota rule, the config builder, the two NotImplementedErrors, and the FPS
branch of get_sampled_points as it was."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spc_cases as cases

KS = ((64, 6), (7, 6), (64, 1), (7, 1))
_gold = {}


def gold():
    if not _gold:
        _gold.update(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_spc.npz')))
    return _gold


def vsa(K, S, method='SPC'):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d.pfe.voxel_set_abstraction import VoxelSetAbstraction
    cfg = EasyDict({'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': K, 'NUM_OUTPUT_FEATURES': 8,
                    'SAMPLE_METHOD': method, 'SPC_SAMPLING': {'NUM_SECTORS': S, 'SAMPLE_RADIUS_WITH_ROI': cases.RADIUS},
                    'FEATURES_SOURCE': ['raw_points'],
                    'SA_LAYER': {'raw_points': {'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]}}})
    return VoxelSetAbstraction(cfg, [0.05, 0.05, 0.1], [-70.4, -70.4, -3, 70.4, 70.4, 1], num_rawpoint_features=4)


@pytest.mark.parametrize('seed', [0, 1])
def test_case_generator_is_stable_and_within_its_cap(seed):
    """the generator asserts its own margins and the f32 / f64 agreement; here: at most 2 % of the points removed, the stored inputs"""
    c, g = cases.frame_case(seed), gold()
    assert c['removed'] <= cases.MAX_REMOVED
    pre = 'case%d/' % seed
    assert np.array_equal(c['points'].view(np.int32), g[pre + 'points'].view(np.int32))       # (bits: the +-0 pair)
    assert c['counts'] == g[pre + 'counts'].tolist() and np.array_equal(c['rois'], g[pre + 'rois'])
    assert len(c['special']) == 2 and np.signbit(c['points'][c['special'], 1]).tolist() == [False, True]
    assert min(c['counts']) < 64 and len(c['counts']) == 3


@pytest.mark.parametrize('seed', [0, 1])
def test_torch_route_reproduces_the_reference(seed):
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as m
    g = gold()
    pre = 'case%d/' % seed
    pts, counts, rois = torch.from_numpy(g[pre + 'points']), g[pre + 'counts'].tolist(), torch.from_numpy(g[pre + 'rois'])
    off = np.concatenate([[0], np.cumsum(counts)])
    kept = []
    for b in range(len(counts)):
        p = pts[off[b]:off[b + 1]]
        sampled, mask = m.sample_points_with_roi(rois[b], p, cases.RADIUS, 700)
        want = torch.from_numpy(g[pre + 'mask'][off[b]:off[b + 1]])
        assert torch.equal(mask, want)
        assert torch.equal(sampled, p[want] if want.any() else p[:1])
        assert torch.equal(m.roi_mask_torch(rois[b], p, cases.RADIUS), want)
        kept.append(sampled)
    assert not g[pre + 'mask'][off[1]:off[2]].any()                          # the frame that keeps points[:1]
    bidx = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).float()
    batch = {'batch_size': len(counts), 'points': torch.cat([bidx[:, None], pts, torch.zeros(len(pts), 1)], 1), 'rois': rois}
    for K, S in KS:
        key = pre + 'K%d_S%d/' % (K, S)
        seg_n, seg_m = [], []
        for b in range(len(counts)):
            picked, n, q = m.sector_fps_torch(kept[b], K, S)
            seg_n += n
            seg_m += q
            assert torch.equal(m.sector_fps(kept[b], K, S), picked)
        assert seg_n == g[key + 'seg_n'].tolist() and seg_m == g[key + 'seg_m'].tolist()
        got = vsa(K, S).get_sampled_points(batch)
        want = torch.from_numpy(g[key + 'keypoints'])
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32))
        assert torch.bincount(got[:, 0].long(), minlength=3).tolist() == [sum(q for f, q in zip(g[key + 'seg_frame'], seg_m) if f == b)
                                                                          for b in range(3)]


def test_empty_frame_yields_no_keypoints():
    """a frame without points: no keypoints (the reference fails there)"""
    c = cases.frame_case(0)
    n0 = c['counts'][0]
    pts = torch.from_numpy(c['points'][:n0])
    batch = {'batch_size': 2, 'points': torch.cat([torch.zeros(n0, 1), pts, torch.zeros(n0, 1)], 1),
             'rois': torch.from_numpy(c['rois'][[0, 0]])}
    got = vsa(64, 6).get_sampled_points(batch)
    assert len(got) > 64 and bool((got[:, 0] == 0).all())


def test_clamped_fallback_quota():
    """every point on the clamped sector: one segment of all points, m = min(n, K) (the reference asks its kernel for K > n picks)"""
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as m
    pts = torch.tensor([[-5.0, 0.0, 0.0], [-9.0, 0.0, 1.0], [-2.0, 0.0, 0.5]])
    sector = (torch.atan2(pts[:, 1], pts[:, 0]) + np.pi) / (np.pi * 2 / 6)
    if bool((sector.floor() >= 6).all()):
        picked, n, q = m.sector_fps_torch(pts, 64, 6)
        assert n == [3] and q == [3] and len(picked) == 3
        assert m.sector_fps_torch(pts, 2, 6)[2] == [2]
    else:                                                                    # (this host's atan2 leaves them in the last sector)
        assert m.sector_fps_torch(pts, 64, 6)[1] == [3]


def test_quota_rule_is_the_python_expression():
    from pcdet.models.backbones_3d.pfe.voxel_set_abstraction import sector_quota, sector_fps_torch
    differs = 0
    for n in range(2, 120):
        for nk in range(1, n + 1):
            for K in (7, 25, 64, 100, 2048):
                want = min(nk, math.ceil((nk / n) * K))
                assert sector_quota(nk, n, K) == want == cases.quota(nk, n, K)
                differs += want != min(nk, math.ceil(Fraction(nk, n) * K))
    assert differs > 0                                                       # the f64 expression is not the exact rational
    q, g = cases.quota_case(), gold()
    assert np.array_equal(q['points'], g['quota/points'])
    _, n, m = sector_fps_torch(torch.from_numpy(q['points']), q['K'], q['S'])
    assert n == [14, 28, 8] and m == q['quotas'] == g['quota/seg_m'].tolist() and m != q['exact']


@pytest.mark.parametrize('name', sorted(cases.fps_cases()))
def test_fps_emulations_agree_with_the_recorded_picks(name):
    from pcdet.models.backbones_3d.pfe.voxel_set_abstraction import stack_fps_torch
    xyz, cnt, m = cases.fps_cases()[name]
    want = gold()['fps/' + name]
    assert len(want) == sum(min(a, b) for a, b in zip(cnt, m))
    assert np.array_equal(cases.fps_order(xyz, cnt, m), want)
    assert np.array_equal(stack_fps_torch(torch.from_numpy(xyz), cnt, m).numpy(), want)


def test_config_builder():
    from pcdet.model_cfgs import pv_rcnn_cfg, pv_rcnn_plusplus_cfg
    for kind in ('kitti', 'waymo'):
        c, base = pv_rcnn_plusplus_cfg(kind).MODEL, pv_rcnn_cfg(kind).MODEL
        assert c.NAME == 'PVRCNNPlusPlus' and c.PFE.SAMPLE_METHOD == 'SPC'
        assert dict(c.PFE.SPC_SAMPLING) == {'NUM_SECTORS': 6, 'SAMPLE_RADIUS_WITH_ROI': 1.6}
        assert c.PFE.FEATURES_SOURCE == ['bev', 'x_conv3', 'x_conv4', 'raw_points'] and c.PFE.NUM_OUTPUT_FEATURES == 90
        assert c.PFE.NUM_KEYPOINTS == base.PFE.NUM_KEYPOINTS
        for src, radius in (('raw_points', 2.4), ('x_conv3', 4.0), ('x_conv4', 6.4)):
            sa = c.PFE.SA_LAYER[src]
            assert sa.FILTER_NEIGHBOR_WITH_ROI is True and sa.RADIUS_OF_NEIGHBOR_WITH_ROI == radius
            assert sa.get('NAME', 'StackSAModuleMSG') == 'StackSAModuleMSG' and sa.MLPS == base.PFE.SA_LAYER[src].MLPS
        assert c.ROI_HEAD.NMS_CONFIG.TRAIN.NMS_POST_MAXSIZE == 512 and c.ROI_HEAD.NMS_CONFIG.TEST.NMS_POST_MAXSIZE == 100
        assert c.ROI_HEAD.NMS_CONFIG.TEST.NMS_PRE_MAXSIZE == 1024 and c.ROI_HEAD.NMS_CONFIG.TEST.NMS_THRESH == 0.7
        assert 'NAME' not in c.ROI_HEAD.ROI_GRID_POOL and c.DENSE_HEAD == base.DENSE_HEAD
    from pcdet.models import detectors
    from pcdet.models.detectors.pv_rcnn_plusplus import PVRCNNPlusPlus
    assert detectors.__all__['PVRCNNPlusPlus'] is PVRCNNPlusPlus


def test_record_layout_and_detector_build():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    from pcdet.query_strategies.scoring import RecordLayout
    cfg = pv_rcnn_plusplus_cfg('kitti')
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=2000))
    assert type(model).__name__ == 'PVRCNNPlusPlus'
    names = [type(m).__name__ for m in model.scheduled_modules()]
    assert names.index('AnchorHeadSingle') < names.index('VoxelSetAbstraction') < names.index('PointHeadSimple') < names.index('PVRCNNHead')
    layout = RecordLayout.for_model(model)
    assert (layout.max_box, layout.num_class) == (100, 3)
    # prefetch_keypoints has nothing to start for SPC (the sampling needs the rois)
    batch = {'points': torch.zeros(4, 5), 'batch_size': 1}
    model.pfe.prefetch_keypoints(batch)
    assert '_keypoints_prefetched' not in batch


def test_vector_pool_and_llal_raise():
    from pcdet.datasets import SyntheticDataset
    from pcdet.config import EasyDict
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    ds = SyntheticDataset(num_frames=2, n_points=2000)
    cfg = pv_rcnn_plusplus_cfg('kitti')
    cfg.MODEL.PFE.SA_LAYER.raw_points.NAME = 'VectorPoolAggregationModuleMSG'
    with pytest.raises(NotImplementedError, match='vector_pool'):
        build_network(cfg.MODEL, 3, ds)
    cfg = pv_rcnn_plusplus_cfg('kitti')
    cfg.MODEL.ROI_HEAD.LOSS_NET = EasyDict({'SHARED_FC': [256, 256]})
    with pytest.raises(NotImplementedError, match='NUM_KEYPOINTS'):
        build_network(cfg.MODEL, 3, ds)


def test_fps_branch_of_get_sampled_points_is_unchanged(monkeypatch):
    """SAMPLE_METHOD FPS: equal frames share one call, ragged frames go one by one, a frame shorter than NUM_KEYPOINTS repeats its
    picks - with the device sampler answered by the oracle's restatement of the reference kernel"""
    import oracle
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils
    def host_fps(xyz, k):                                                   # (B, n, 3) -> (B, k); past n picks the entries are unspecified
        n = xyz.shape[1]
        idx = oracle.fps(xyz.numpy(), min(int(k), n))
        return torch.from_numpy(np.concatenate([idx, np.zeros((len(idx), max(int(k) - n, 0)), np.int32)], 1))
    monkeypatch.setattr(pointnet2_utils, 'farthest_point_sample', host_fps)
    rng = np.random.default_rng(3)
    K = 16
    pfe = vsa(K, 6, method='FPS')
    for counts in ([40, 40], [40, 9, 23]):
        pts = rng.uniform(-20, 20, (sum(counts), 4)).astype(np.float32)
        bidx = np.repeat(np.arange(len(counts), dtype=np.float32), counts)
        got = pfe.get_sampled_points({'batch_size': len(counts), 'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1))})
        assert got.shape == (len(counts) * K, 4)
        s = 0
        for b, n in enumerate(counts):
            idx = oracle.fps(pts[None, s:s + n, :3].copy(), min(K, n))[0]
            if n < K:
                idx = np.tile(idx, K // n + 1)[:K]
            want = np.concatenate([np.full((K, 1), b, np.float32), pts[s:s + n, :3][idx]], 1)
            assert np.array_equal(got[b * K:(b + 1) * K].numpy(), want)
            s += n
