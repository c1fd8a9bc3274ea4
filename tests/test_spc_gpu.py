"""GPU: sectorized proposal-centric keypoint sampling (csrc/spc_sampling.hip through crbhip.spc) and FILTER_NEIGHBOR_WITH_ROI.

Each kernel alone on the cases of tests/spc_cases.py: the mask against its f64 definition, the plan (segments, counts, quotas)
against the numpy restatement of sector_fps, the picks against the numpy emulation of the reference's stack FPS kernel. The fused
route against the torch route on the device, bit for bit. Everything here is integer-valued or copied: the bar is equality. The two
clamp-quirk points of a case take the sector the torch route gives them on this device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spc_cases as cases
from test_gt_sampling_gpu import _ReadBacks

pytestmark = pytest.mark.gpu

_cache = {}


def _case(seed):
    if seed not in _cache:
        _cache[seed] = cases.frame_case(seed)
    return _cache[seed]


def _dev_case(c, dev, extra_cols=1):
    """-> points (N, 1 + 3 + extra) [b, x, y, z, ...], offsets (B + 1) i32, rois (B, 8, 7) on the device"""
    from crbhip import spc
    n = len(c['points'])
    bidx = np.repeat(np.arange(len(c['counts']), dtype=np.float32), c['counts'])
    feat = np.linspace(0, 1, n * extra_cols, dtype=np.float32).reshape(n, extra_cols)
    pts = torch.from_numpy(np.concatenate([bidx[:, None], c['points'], feat], 1)).to(dev)
    off = spc.frame_offsets(torch.tensor(c['counts'], dtype=torch.int32, device=dev))
    return pts, off, torch.from_numpy(c['rois']).to(dev)


def _torch_sector(xyz, S):
    """the reference's expression on the device (division by a host scalar as torch performs it there)"""
    ang = torch.atan2(xyz[:, 1], xyz[:, 0]) + np.pi
    return (ang / (np.pi * 2 / S)).floor().clamp(min=0, max=S).long()


def _expected_sector(c, S, pts):
    sec = cases.sector_f64(c['points'], S)[0]
    sp = c['special']
    sec[sp] = _torch_sector(pts[sp, 1:4], S).cpu().numpy()
    return sec


def _f64_mask(c):
    out, near, s = [], [], 0
    for b, n in enumerate(c['counts']):
        m, k, _, _ = cases.mask_f64(c['points'][s:s + n], c['rois'][b], c['radius'])
        out.append(m)
        near.append(k)
        s += n
    return np.concatenate(out), np.concatenate(near)


@pytest.mark.parametrize('seed', [0, 1])
def test_mask_equals_its_f64_definition(dev, seed):
    from crbhip import spc
    c = _case(seed)
    pts, off, rois = _dev_case(c, dev)
    mask, nearest = spc.roi_proximity_mask(pts, 1, off, rois, c['radius'], want_nearest=True)
    want, want_near = _f64_mask(c)
    assert want.any() and not want.all() and not want[sum(c['counts'][:1]):sum(c['counts'][:2])].any()
    np.testing.assert_array_equal(mask.cpu().numpy(), want)              # (the clamp-quirk points are far from the threshold)
    np.testing.assert_array_equal(nearest.cpu().numpy(), want_near)
    # a permutation of the frames' RoI rows leaves the mask unchanged
    perm = torch.from_numpy(np.random.default_rng(seed).permutation(rois.shape[1])).to(dev)
    assert torch.equal(spc.roi_proximity_mask(pts, 1, off, rois[:, perm].contiguous(), c['radius']), mask)
    # the (N, 3) layout (voxel centres) and RoI rows with more than 7 columns
    wide = torch.cat([rois, torch.ones_like(rois[:, :, :2])], -1)
    assert torch.equal(spc.roi_proximity_mask(pts[:, 1:4].contiguous(), 0, off, wide, c['radius']), mask)


@pytest.mark.parametrize('K,S', [(64, 6), (7, 6), (64, 1), (7, 1)])
def test_plan_equals_sector_fps_bookkeeping(dev, K, S):
    from crbhip import spc
    c = _case(0)
    pts, off, rois = _dev_case(c, dev)
    mask = spc.roi_proximity_mask(pts, 1, off, rois, c['radius'])
    plan = spc.spc_plan(pts, 1, off, mask, S, K)
    sec = _expected_sector(c, S, pts)
    np.testing.assert_array_equal(plan['sector'].cpu().numpy(), sec)
    want = cases.plan_numpy(c['counts'], mask.cpu().numpy(), sec, K, S)
    header = plan['header'].cpu().numpy()
    nseg, rows = len(want['seg']), len(want['src'])
    per_frame = [sum(m for b, _, _, m in want['seg'] if b == f) for f in range(len(c['counts']))]
    assert header.tolist() == [nseg, rows, sum(per_frame)] + per_frame
    assert per_frame[1] == 1                                              # the frame whose RoIs miss every point keeps points[:1]
    seg = plan['seg'].cpu().numpy()[:nseg]
    n = np.array([s[2] for s in want['seg']])
    m = np.array([s[3] for s in want['seg']])
    np.testing.assert_array_equal(seg[:, 1], n)
    np.testing.assert_array_equal(seg[:, 2], m)
    np.testing.assert_array_equal(seg[:, 0], np.cumsum(n) - n)
    np.testing.assert_array_equal(seg[:, 3], np.cumsum(m) - m)
    np.testing.assert_array_equal(seg[:, 4], [s[0] for s in want['seg']])
    np.testing.assert_array_equal(plan['src'].cpu().numpy()[:rows], want['src'])
    np.testing.assert_array_equal(plan['xyz'].cpu().numpy()[:rows], c['points'][want['src']])


def test_quota_follows_the_f64_expression(dev):
    from crbhip import spc
    q = cases.quota_case()
    pts = torch.from_numpy(q['points']).to(dev)
    off = torch.tensor([0, len(pts)], dtype=torch.int32, device=dev)
    plan = spc.spc_plan(pts, 0, off, torch.ones(len(pts), dtype=torch.bool, device=dev), q['S'], q['K'])
    got = plan['seg'].cpu().numpy()[:3, 2].tolist()
    assert got == q['quotas'] and got != q['exact'], got


def test_clamped_fallback_and_empty_frames(dev):
    """frame 0: three points at azimuth pi (y = +0, x < 0), which the clamp sends to sector S on this device or leaves in S - 1:
    either way the plan is sector_fps's for the sectors the torch expression gives here (all in S: one segment of all kept points,
    m = min(n, K)); frame 1 has no points and yields no keypoints; frame 2 has one"""
    from crbhip import spc
    xyz = torch.tensor([[-5.0, 0.0, 0.0], [-9.0, 0.0, 1.0], [-2.0, 0.0, 0.5], [3.0, 1.0, 0.0]], device=dev)
    counts, S = [3, 0, 1], 6
    off = spc.frame_offsets(torch.tensor(counts, dtype=torch.int32, device=dev))
    sec = _torch_sector(xyz, S).cpu().numpy()
    print('sectors of the azimuth-pi points on this device:', sec[:3])
    for K in (64, 2):
        plan = spc.spc_plan(xyz, 0, off, torch.ones(4, dtype=torch.bool, device=dev), S, K)
        np.testing.assert_array_equal(plan['sector'].cpu().numpy(), sec)
        want = cases.plan_numpy(counts, np.ones(4, bool), sec, K, S)
        per_frame = [sum(m for b, _, _, m in want['seg'] if b == f) for f in range(3)]
        assert per_frame[1] == 0 and per_frame[0] == min(3, K)
        assert plan['header'].cpu().tolist() == [len(want['seg']), len(want['src']), sum(per_frame)] + per_frame
        got = plan['seg'].cpu().numpy()[:len(want['seg'])]
        np.testing.assert_array_equal(got[:, [4, 1, 2]], [[b, n, m] for b, _, n, m in want['seg']])
        np.testing.assert_array_equal(plan['src'].cpu().numpy()[:len(want['src'])], want['src'])


@pytest.mark.parametrize('name', sorted(cases.fps_cases()))
def test_fps_segments_equal_the_reference_kernel(dev, name):
    from crbhip import spc
    xyz, cnt, m = cases.fps_cases()[name]
    want = cases.fps_order(xyz, cnt, m)
    x = torch.from_numpy(xyz).to(dev)
    got = spc.stack_fps(x, cnt, m)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    again = spc.stack_fps(x, torch.tensor(cnt), torch.tensor(m))
    assert torch.equal(got, again)
    # the keypoint output: the picked rows, tagged with the frame of the table row
    seg = torch.zeros((len(cnt), spc.SEG_ROW), dtype=torch.int32)
    seg[:, 1], seg[:, 2] = torch.tensor(cnt), torch.tensor(m)
    seg[:, 0], seg[:, 3] = torch.cumsum(seg[:, 1], 0) - seg[:, 1], torch.cumsum(seg[:, 2], 0) - seg[:, 2]
    seg[:, 4] = torch.arange(len(cnt)) // 2
    nseg = torch.tensor([len(cnt)], dtype=torch.int32, device=dev)
    idx, kp = spc.fps_segments(x, seg.to(dev), nseg, len(want) + 3, want_idx=True, want_keypoints=True)
    np.testing.assert_array_equal(idx.cpu().numpy()[:len(want)], want)
    np.testing.assert_array_equal(kp.cpu().numpy()[:len(want), 1:], xyz[want])
    np.testing.assert_array_equal(kp.cpu().numpy()[:len(want), 0], np.repeat(np.arange(len(cnt)) // 2, np.minimum(m, cnt)))
    assert not kp[len(want):].any() and not idx[len(want):].any()       # rows past the last segment stay untouched
    # table rows past *num_segments do nothing
    nseg[0] = 1
    idx1, _ = spc.fps_segments(x, seg.to(dev), nseg, len(want))
    k0 = min(m[0], cnt[0])
    np.testing.assert_array_equal(idx1.cpu().numpy()[:k0], want[:k0])
    assert not idx1[k0:].any()


def _vsa(K, S, filter_radius=None):
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d.pfe.voxel_set_abstraction import VoxelSetAbstraction
    raw = {'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]}
    if filter_radius is not None:
        raw.update({'FILTER_NEIGHBOR_WITH_ROI': True, 'RADIUS_OF_NEIGHBOR_WITH_ROI': filter_radius})
    cfg = EasyDict({'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': K, 'NUM_OUTPUT_FEATURES': 8,
                    'SAMPLE_METHOD': 'SPC', 'SPC_SAMPLING': {'NUM_SECTORS': S, 'SAMPLE_RADIUS_WITH_ROI': cases.RADIUS},
                    'FEATURES_SOURCE': ['raw_points'], 'SA_LAYER': {'raw_points': raw}})
    torch.manual_seed(3)
    return VoxelSetAbstraction(cfg, [0.05, 0.05, 0.1], [-70.4, -70.4, -3, 70.4, 70.4, 1], num_rawpoint_features=4)


@pytest.mark.parametrize('K,S', [(64, 6), (7, 6), (64, 1), (7, 1)])
def test_fused_route_equals_the_torch_route_on_the_device(dev, K, S):
    """get_sampled_points through the kernels and through the reference's torch expressions (one frame and one sector at a time),
    every case including the +-0 points: the same bytes; two calls: the same bytes; one read-back per call"""
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    pfe = _vsa(K, S).to(dev)
    for seed in (0, 1):
        c = _case(seed)
        pts, off, rois = _dev_case(c, dev)
        batch = {'batch_size': len(c['counts']), 'points': pts, 'rois': rois}
        pfe.get_sampled_points(batch)                                      # (first call: allocator warm-up)
        with _ReadBacks() as rb:
            got = pfe.get_sampled_points(batch)
        assert rb.count == 1, rb.count
        assert torch.equal(pfe.get_sampled_points(batch), got)
        vsa_mod.SPC_DEVICE_ROUTE = False
        try:
            want = pfe.get_sampled_points(batch)
        finally:
            vsa_mod.SPC_DEVICE_ROUTE = True
        assert got.shape == want.shape and got.shape[1] == 4 and got.shape[0] > K
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_voxel_centres_as_the_point_source(dev):
    """POINT_SOURCE voxel_centers: the keypoints are voxel centres of their own frame, between 1 and K + S per frame (voxel centres
    sit on a grid and keep no margin from the thresholds, so the two routes are not compared bit for bit here)"""
    from pcdet.utils import common_utils
    K, S = 64, 6
    pfe = _vsa(K, S).to(dev)
    pfe.model_cfg.POINT_SOURCE = 'voxel_centers'
    c = _case(0)
    pts, off, rois = _dev_case(c, dev)
    vs, lo = torch.tensor(pfe.voxel_size, device=dev), torch.tensor(pfe.point_cloud_range[:3], device=dev)
    coords = torch.cat([pts[:, :1], torch.floor((pts[:, 1:4] - lo) / vs).flip(-1)], 1).int()
    coords = coords[(coords[:, 1] >= 0) & (coords[:, 1] < 40)]
    got = pfe.get_sampled_points({'batch_size': 3, 'voxel_coords': coords, 'rois': rois})
    centres = common_utils.get_voxel_centers(coords[:, 1:4], 1, pfe.voxel_size, pfe.point_cloud_range)
    per_frame = torch.bincount(got[:, 0].long(), minlength=3).tolist()
    assert all(1 <= m <= K + S for m in per_frame) and per_frame[1] == 1
    for b in range(3):
        own, kp = centres[coords[:, 0] == b], got[got[:, 0] == b][:, 1:4]
        assert bool((kp[:, None, :] == own[None, :, :]).all(-1).any(1).all())


def test_module_level_functions_on_the_device(dev):
    """sample_points_with_roi / sector_fps with the reference's signatures: the device route and the torch route agree"""
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    c = _case(1)
    n0 = c['counts'][0]
    p, r = torch.from_numpy(c['points'][:n0]).to(dev), torch.from_numpy(c['rois'][0]).to(dev)
    res = {}
    for route in (True, False):
        vsa_mod.SPC_DEVICE_ROUTE = route
        try:
            kept, mask = vsa_mod.sample_points_with_roi(r, p, cases.RADIUS, 500)
            res[route] = (kept, mask, vsa_mod.sector_fps(kept, 64, 6))
        finally:
            vsa_mod.SPC_DEVICE_ROUTE = True
    for a, b in zip(res[True], res[False]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert res[True][2].shape[0] >= 64


# ---- FILTER_NEIGHBOR_WITH_ROI --------------------------------------------------------------------------------------------------
def _filter_inputs(dev, spread, kp_offset=0.5):
    """keypoints within kp_offset (per axis) of RoI centres; source points around them (spread: sigma in m), one feature column"""
    c = _case(0)
    rng = np.random.default_rng(11)
    cnt, xyz, new_xyz, new_cnt = [], [], [], []
    for b in (0, 2):
        centres = c['rois'][b][:6, 0:3]
        kp = centres[rng.integers(0, 6, 40)] + rng.uniform(-kp_offset, kp_offset, (40, 3)).astype(np.float32)
        p = kp[rng.integers(0, 40, 900)] + rng.normal(0, spread, (900, 3)).astype(np.float32)
        xyz.append(p.astype(np.float32)); cnt.append(900); new_xyz.append(kp.astype(np.float32)); new_cnt.append(40)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rois = t(c['rois'][[0, 2]])
    bs = t(np.repeat(np.arange(2, dtype=np.float32), cnt))
    feat = t(rng.normal(0, 1, (1800, 1)).astype(np.float32))
    return t(np.concatenate(xyz)), feat, bs, t(np.concatenate(new_xyz)), torch.tensor(new_cnt, dtype=torch.int32, device=dev), rois


def _pooled(pfe, inp, **kw):
    xyz, feat, bs, new_xyz, new_cnt, rois = inp
    return pfe.aggregate_keypoint_features_from_one_source(batch_size=2, aggregate_func=pfe.SA_rawpoints, xyz=xyz, xyz_features=feat,
                                                           xyz_bs_idxs=bs, new_xyz=new_xyz, new_xyz_batch_cnt=new_cnt, **kw)


def test_filter_that_removes_no_neighbour_changes_nothing(dev):
    """radius 6.4 m: every source point within the 0.8 m pool radius of a keypoint (itself within 0.9 m of a RoI centre) passes,
    points further out do not all: the pooled features are those of the unfiltered call, bit for bit"""
    from crbhip import spc
    pfe = _vsa(64, 6).to(dev).eval()
    inp = _filter_inputs(dev, spread=6.0)
    off = spc.frame_offsets(torch.tensor([900, 900], dtype=torch.int32, device=dev))
    kept = spc.roi_proximity_mask(inp[0], 0, off, inp[5], 6.4)
    assert 0 < int(kept.sum()) < 1800
    with torch.no_grad():
        plain = _pooled(pfe, inp)
        filtered = _pooled(pfe, inp, filter_neighbors_with_roi=True, radius_of_neighbor=6.4, rois=inp[5])
    assert plain.abs().sum() > 0 and torch.equal(plain, filtered)


def test_filter_equals_the_torch_filtered_route_forward_and_gradient(dev):
    """keypoints up to 2.5 m per axis off the RoI centres, radius 0.3 m: the filter removes neighbours. The pooled features equal the torch-filtered route's; the gradient reaches the kept feature rows
    and equals that route's up to the order of the f32 atomic sums of the grouping backward (1e-5 of the largest entry: at most
    32 neighbours x 40 keypoints add into one row, f32 eps 6e-8 each)"""
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as vsa_mod
    pfe = _vsa(64, 6).to(dev).train()
    out, grad = {}, {}
    for route in (True, False):
        inp = list(_filter_inputs(dev, spread=0.5, kp_offset=2.5))
        inp[1] = inp[1].clone().requires_grad_(True)
        vsa_mod.SPC_DEVICE_ROUTE = route
        try:
            out[route] = _pooled(pfe, inp, filter_neighbors_with_roi=True, radius_of_neighbor=0.3, rois=inp[5])
        finally:
            vsa_mod.SPC_DEVICE_ROUTE = True
        (out[route] * torch.linspace(-1, 1, out[route].numel(), device=dev).view_as(out[route])).sum().backward()
        grad[route] = inp[1].grad.clone()
    with torch.no_grad():
        plain = _pooled(pfe, _filter_inputs(dev, spread=0.5, kp_offset=2.5))
    assert not torch.equal(plain, out[True].detach())                      # the filter did remove neighbours
    assert torch.equal(out[True], out[False])
    valid = vsa_mod.roi_mask_torch(inp[5][0], inp[0][:900], 0.3)
    assert grad[True][:900][~valid].abs().max() == 0 and grad[True].abs().max() > 0
    err = float((grad[True] - grad[False]).abs().max() / grad[False].abs().max())
    print('feature gradient: device-filtered vs torch-filtered route %.2e of the largest entry' % err)
    assert err <= 1e-5
