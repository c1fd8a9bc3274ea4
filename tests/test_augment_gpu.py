"""crb_augment_mask_points / crb_augment_boxes (csrc/augment.hip) and the device route of
DeviceDataProcessor.process_batch(..., augmentor=...) against the host mirror (pcdet.datasets.augmentor + the host DataProcessor
range masks), bit for bit, and against the reference's own outputs (tests/golden/ref_augmentor.npz)."""
import numpy as np
import pytest
import torch

from augment_cases import CASES, RUN_NAMES, U, golden, host_route, queue, rotation_bound, run_inputs
from pcdet.config import EasyDict
from pcdet.datasets.augmentor import DataAugmentor, DeviceDataAugmentor
from pcdet.datasets.augmentor import augmentor_utils

PCR = [0, -40, -3, 70.4, 40, 1]
NAMES = ['Car', 'Pedestrian', 'Cyclist']
# an empty frame, a one-point frame, frame boundaries inside a wave (1027 + 1 = 16 * 64 + 4) and inside a 256-thread workgroup,
# counts that are no multiple of 64, several workgroups; once with the empty frame first and once with it last
COUNTS = {'empty_first': [0, 1027, 1, 2500], 'empty_last': [2500, 1, 1027, 0]}
SEED = 29


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_same_bits(got, want, what=''):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _points(counts, C, seed=5):
    rng = np.random.default_rng(seed)
    frames = [rng.uniform([-12, -52, -4, 0, 0][:C], [82, 52, 2, 1, 1][:C], size=(n, C)).astype(np.float32) for n in counts]
    for f in frames:                                   # signed zeros must survive the steps that are skipped
        if len(f) > 3:
            f[1, 0], f[2, 1], f[3, 2] = -0.0, -0.0, -0.0
    return frames


def _boxes(W, seed=6):
    """B = 4 frames: many boxes straddling the range, none, three that are all removed, a few. (G_k, W) with the class last"""
    rng = np.random.default_rng(seed)

    def make(n, far=False):
        lo, hi = ([400, 400, -2.5], [500, 500, 0.5]) if far else ([-6, -46, -2.5], [77, 46, 0.5])
        cols = [rng.uniform(lo, hi, size=(n, 3)), rng.uniform(0.6, 4.5, size=(n, 3)), rng.uniform(-3.1, 3.1, size=(n, 1))]
        if W == 10:
            cols.append(rng.uniform(-5, 5, size=(n, 2)))
        cols.append(rng.integers(1, 4, size=(n, 1)))
        return np.concatenate(cols, 1).astype(np.float32)
    return [make(37), np.zeros((0, W), np.float32), make(3, far=True), make(5)]


def _draw(case, B, seed=SEED):
    np.random.seed(seed)
    return DeviceDataAugmentor(queue(case)).draw_batch(B)


_host_cache = {}


def _host(case, order, C, mask):
    """host mirror + host DataProcessor mask on the frames of _points, computed once per configuration and shared"""
    key = (case, order, C, mask)
    if key not in _host_cache:
        frames = _points(COUNTS[order], C)
        none = [np.zeros((0, 8), np.float32)] * len(frames)
        if case == 'identity':
            keep = [(p[:, 0] >= PCR[0]) & (p[:, 0] <= PCR[3]) & (p[:, 1] >= PCR[1]) & (p[:, 1] <= PCR[4]) if mask
                    else np.ones(len(p), bool) for p in frames]
            _host_cache[key] = [p[k] for p, k in zip(frames, keep)]
        else:
            _host_cache[key] = [p for p, _ in host_route(case, SEED, frames, none, PCR, mask=mask)]
    return _host_cache[key]


def _layouts(frames, dev):
    """the same rows as (tensor, xyz_col): dense (N, C); a view into wider rows (row_stride > C); the batch layout (N, 1 + C) with
    a frame column in front; that layout inside wider rows"""
    flat = torch.from_numpy(np.concatenate(frames, 0)).to(dev)
    n, C = flat.shape
    wide = torch.full((n, C + 3), 7.0, device=dev)
    wide[:, :C] = flat
    lead = torch.cat([torch.full((n, 1), -1.0, device=dev), flat], 1)
    wide_lead = torch.full((n, C + 4), 7.0, device=dev)
    wide_lead[:, :C + 1] = lead
    return [(flat, 0), (wide[:, :C], 0), (lead, 1), (wide_lead[:, :C + 1], 1)]


@pytest.mark.gpu
@pytest.mark.parametrize('mask', [True, False])
@pytest.mark.parametrize('case', ['identity', 'flip', 'rot', 'scale', 'trans', 'kitti'])
def test_points_bit_equal_to_host_mirror(dev, case, mask):
    """every step alone and the KITTI queue, mask on and off, C = 4 and 5, both xyz_col layouts, padded rows, the empty frame first
    and last: rows, order and new offsets equal the host mirror + host range mask bit for bit (identity: the input restricted by
    the mask, signed zeros included)"""
    from crbhip import augment
    for order, counts in COUNTS.items():
        B = len(counts)
        params, _ = DeviceDataAugmentor.identity(B) if case == 'identity' else _draw(case, B)
        params = torch.from_numpy(params).to(dev)
        off = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
        for C in (4, 5):
            want = _host(case, order, C, mask)
            want_off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
            want_rows = np.concatenate(want, 0)
            for pts, xyz_col in _layouts(_points(counts, C), dev):
                for frame_col in (False, True):
                    out, new_off = augment.augment_mask_points(pts, off, params, PCR, mask=mask, xyz_col=xyz_col, frame_col=frame_col)
                    what = '%s %s C=%d xyz_col=%d stride=%d frame_col=%d' % (case, order, C, xyz_col, pts.stride(0), frame_col)
                    assert new_off.cpu().tolist() == want_off.tolist(), what
                    got = out.cpu().numpy()
                    if frame_col:
                        np.testing.assert_array_equal(got[:, 0], np.repeat(np.arange(B), np.diff(want_off)), err_msg=what)
                        got = got[:, 1:]
                    assert_same_bits(got, want_rows, what)
    if mask:
        assert 0 < len(want_rows) < sum(counts)


@pytest.mark.gpu
def test_frame_whose_points_all_leave_the_range(dev):
    from crbhip import augment
    rng = np.random.default_rng(2)
    far = rng.uniform([200, -5, -1, 0], [300, 5, 1, 1], size=(300, 4)).astype(np.float32)
    near = _points([700], 4)[0]
    for frames in ([far, near], [near, far], [far]):
        params, _ = _draw('kitti', len(frames))
        off = torch.tensor(np.concatenate([[0], np.cumsum([len(f) for f in frames])]), dtype=torch.int32, device=dev)
        out, new_off = augment.augment_mask_points(torch.from_numpy(np.concatenate(frames)).to(dev), off,
                                                   torch.from_numpy(params).to(dev), PCR, mask=True)
        none = [np.zeros((0, 8), np.float32)] * len(frames)
        want = [p for p, _ in host_route('kitti', SEED, frames, none, PCR)]
        assert [len(w) for w in want if len(w) == 0], 'one frame must come out empty'
        assert new_off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        assert_same_bits(out.cpu().numpy(), np.concatenate(want, 0))


@pytest.mark.gpu
@pytest.mark.parametrize('W', [8, 10])
@pytest.mark.parametrize('case', ['identity', 'flip', 'rot', 'scale', 'trans', 'kitti'])
def test_boxes_bit_equal_to_host_mirror(dev, case, W):
    """transform + limit_period + range test + in-frame compaction: bit-equal to the host mirror (which has no matmul) followed by
    the same-expression range test; a frame without boxes, a frame whose boxes are all removed; padding exactly zero; counts; class"""
    from crbhip import augment
    from pcdet.utils import box_utils
    gts = _boxes(W)
    B, G = len(gts), max(len(g) for g in gts)
    pad = np.zeros((B, G, W), np.float32)
    for k, g in enumerate(gts):
        pad[k, :len(g)] = g
    params, angles = DeviceDataAugmentor.identity(B) if case == 'identity' else _draw(case, B)
    aug = DataAugmentor(None, [] if case == 'identity' else queue(case), NAMES)
    np.random.seed(SEED)
    want = []
    for g in gts:
        d = aug.forward({'points': np.zeros((1, 4), np.float32), 'gt_boxes': g[:, :-1].copy()})
        want.append(np.concatenate([d['gt_boxes'], g[:, -1:]], 1))
    t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    counts = t(np.array([len(g) for g in gts], np.int32))
    for mask in (False, True):
        out, new_counts = augment.augment_boxes(t(pad), counts, t(params), t(angles), PCR, mask=mask)
        out, new_counts = out.cpu().numpy(), new_counts.cpu().tolist()
        for k, w in enumerate(want):
            if mask:
                keep = augmentor_utils.mask_boxes_outside_range_f32(w, PCR)
                # (the torch corner path of the host DataProcessor decides the same on these boxes)
                np.testing.assert_array_equal(keep, box_utils.mask_boxes_outside_range_numpy(w, np.asarray(PCR, np.float32)))
                w = w[keep]
            assert new_counts[k] == len(w), (case, W, mask, k)
            assert_same_bits(out[k, :len(w)], w, '%s W=%d mask=%d frame %d' % (case, W, mask, k))
            assert not _bits(out[k, len(w):]).any()                     # removed rows and padding: exactly +0.0
            np.testing.assert_array_equal(out[k, :len(w), -1], w[:, -1])
        if mask:
            assert new_counts[1] == 0 and new_counts[2] == 0 and 0 < new_counts[0] < len(gts[0])
        h = out[..., 6]
        assert (h >= -np.pi - 1e-6).all() and (h <= np.pi + 1e-6).all()


@pytest.mark.gpu
@pytest.mark.parametrize('name', RUN_NAMES)
def test_against_reference_golden(dev, name):
    """the reference's own outputs: kept rows and counts equal (the golden keeps 1e-3 clear of every bound), everything that is not
    a rotated coordinate equal, rotated coordinates within the derived bound (augment_cases.rotation_bound)"""
    from crbhip import augment
    g = golden()
    case, seed, pts, boxes = run_inputs(name)
    params, angles = _draw(case, 1, seed)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    off = torch.tensor([0, len(pts)], dtype=torch.int32, device=dev)
    out, new_off = augment.augment_mask_points(t(pts), off, t(params), PCR, mask=True)
    keep = g[name + '/keep_points']
    ref = g[name + '/points_xyz'][keep]
    out = out.cpu().numpy()
    assert new_off.cpu().tolist() == [0, int(keep.sum())]
    np.testing.assert_array_equal(out[:, 3:], pts[keep][:, 3:])
    rotated = any(code == 2 for code, _, _ in g[name + '/ops'])
    cls = (np.arange(len(boxes)) % 3 + 1).astype(np.float32)[:, None]
    bout, cnt = augment.augment_boxes(t(np.concatenate([boxes, cls], 1)[None]), t(np.array([len(boxes)], np.int32)), t(params),
                                      t(angles), PCR, mask=True)
    keep_b = g[name + '/keep_boxes']
    ref_b = g[name + '/boxes'][keep_b]
    assert cnt.cpu().tolist() == [int(keep_b.sum())]
    bout = bout.cpu().numpy()[0, :len(ref_b)]
    np.testing.assert_array_equal(bout[:, -1], cls[keep_b][:, 0])
    np.testing.assert_array_equal(bout[:, 2:7], ref_b[:, 2:7])
    np.testing.assert_array_equal(out[:, 2], ref[:, 2])
    if not rotated:
        np.testing.assert_array_equal(out[:, :3], ref)
        np.testing.assert_array_equal(bout[:, :-1], ref_b)
        return
    pairs = [(out[:, :2], ref[:, :2], pts[keep][:, :2], True), (bout[:, :2], ref_b[:, :2], boxes[keep_b][:, :2], True)]
    if boxes.shape[1] > 7:
        pairs.append((bout[:, 7:9], ref_b[:, 7:9], boxes[keep_b][:, 7:9], False))
    for got, want, xy_in, scaled in pairs:
        bound = rotation_bound(name, xy_in) if scaled else 4 * U * np.abs(xy_in.astype(np.float64)).sum(1)
        diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
        assert (diff <= bound[:, None]).all(), (name, diff.max())


def _dp_cfgs(shuffle=False):
    return [EasyDict({'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}),
            EasyDict({'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': EasyDict({'train': shuffle, 'test': False})}),
            EasyDict({'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.05, 0.05, 0.1], 'MAX_POINTS_PER_VOXEL': 5,
                      'MAX_NUMBER_OF_VOXELS': EasyDict({'train': 16000, 'test': 40000})})]


@pytest.mark.gpu
def test_process_batch_device_route(dev):
    """identity parameters == process_batch without an augmentor (points, offsets, boxes); the KITTI queue == the host route frame by
    frame; two calls give identical bits; the shuffle permutes inside the frames"""
    from pcdet.datasets.processor.data_processor import DeviceDataProcessor
    frames, gts = _points(COUNTS['empty_first'], 4), _boxes(8)
    dp = DeviceDataProcessor(_dp_cfgs(), PCR, True, 4, device=dev)
    plain = dp.process_batch(frames, gts, list('abcd'))
    same = dp.process_batch(frames, gts, list('abcd'), augmentor=DeviceDataAugmentor([]))
    assert torch.equal(plain['points'].view(torch.int32), same['points'].view(torch.int32))
    assert torch.equal(plain['point_frame_offsets'], same['point_frame_offsets'])
    assert same['gt_boxes'].shape == plain['gt_boxes'].shape
    np.testing.assert_array_equal(same['gt_boxes'][..., [0, 1, 2, 3, 4, 5, 7]].cpu().numpy(),
                                  plain['gt_boxes'][..., [0, 1, 2, 3, 4, 5, 7]].cpu().numpy())      # (the heading is limited to [-pi, pi))
    aug = DeviceDataAugmentor(queue('kitti'))
    np.random.seed(SEED)
    a = dp.process_batch(frames, gts, list('abcd'), augmentor=aug)
    np.random.seed(SEED)
    b = dp.process_batch(frames, gts, list('abcd'), augmentor=aug)
    assert torch.equal(a['points'].view(torch.int32), b['points'].view(torch.int32))
    assert torch.equal(a['gt_boxes'].view(torch.int32), b['gt_boxes'].view(torch.int32))
    want = host_route('kitti', SEED, frames, gts, PCR)
    off = a['point_frame_offsets'].cpu().tolist()
    assert off == np.concatenate([[0], np.cumsum([len(p) for p, _ in want])]).tolist()
    assert a['gt_boxes'].shape[1] == max(1, max(len(x) for _, x in want)) and a['frame_id'].tolist() == list('abcd')
    for k, (p, x) in enumerate(want):
        seg = a['points'][off[k]:off[k + 1]].cpu().numpy()
        assert (seg[:, 0] == k).all()
        assert_same_bits(seg[:, 1:], p)
        assert_same_bits(a['gt_boxes'][k, :len(x)].cpu().numpy(), x)
        assert not a['gt_boxes'][k, len(x):].cpu().numpy().any()
    np.random.seed(SEED)
    s = DeviceDataProcessor(_dp_cfgs(True), PCR, True, 4, device=dev).process_batch(frames, gts, augmentor=aug)
    assert s['point_frame_offsets'].cpu().tolist() == off and not torch.equal(s['points'], a['points'])
    for k, (p, _) in enumerate(want):
        seg = s['points'][off[k]:off[k + 1], 1:].cpu().numpy()
        np.testing.assert_array_equal(seg[np.lexsort(seg.T)], p[np.lexsort(p.T)])


@pytest.mark.gpu
def test_augmented_batch_feeds_a_second_training_step(dev):
    """B = 2: process_batch(..., augmentor) -> SECOND forward + backward with a finite loss; the voxel coordinates equal the host
    route (host augmentor, host DataProcessor, VoxelGeneratorWrapper) under the same seed"""
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.processor.data_processor import DataProcessor, DeviceDataProcessor
    from pcdet.datasets.synthetic import kitti_frame
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    frames, gts = zip(*[kitti_frame(60 + f, 6000) for f in range(2)])
    dp = DeviceDataProcessor(_dp_cfgs(), PCR, True, 4, device=dev)
    np.random.seed(SEED)
    batch = dp.process_batch(list(frames), list(gts), ['a', 'b'], augmentor=DeviceDataAugmentor(queue('kitti')))
    torch.manual_seed(0)
    model = build_network(second_cfg('kitti').MODEL, 3, SyntheticDataset(num_frames=2)).to(dev).train()
    ret, _, _ = model(batch)
    assert torch.isfinite(ret['loss'])
    ret['loss'].backward()
    coords = batch['voxel_coords'].cpu().numpy()
    host = DataProcessor(_dp_cfgs()[2:], PCR, training=True, num_point_features=4)
    start = 0
    for k, (p, _) in enumerate(host_route('kitti', SEED, list(frames), list(gts), PCR)):
        d = host.forward({'points': p, 'use_lead_xyz': True})
        m = int((coords[:, 0] == k).sum())
        np.testing.assert_array_equal(coords[start:start + m, 1:], d['voxel_coords'])
        start += m
    assert start == len(coords) and start > 0


@pytest.mark.gpu
def test_cpu_tensors_and_bad_shapes_raise(dev):
    from crbhip import augment, CrbHipError
    params, angles = DeviceDataAugmentor.identity(1)
    pts, off = torch.zeros(10, 4), torch.tensor([0, 10], dtype=torch.int32)
    with pytest.raises(CrbHipError):
        augment.augment_mask_points(pts, off, torch.from_numpy(params), PCR)
    with pytest.raises(CrbHipError):
        augment.augment_boxes(torch.zeros(1, 2, 8), torch.tensor([2], dtype=torch.int32), torch.from_numpy(params))
    with pytest.raises(CrbHipError):                                                    # (B, 8) parameters for B = 1 only
        augment.augment_mask_points(pts.to(dev), torch.tensor([0, 5, 10], dtype=torch.int32, device=dev),
                                    torch.from_numpy(params).to(dev), PCR)
    with pytest.raises(CrbHipError):
        augment.augment_boxes(torch.zeros(1, 2, 9, device=dev), torch.tensor([2], dtype=torch.int32, device=dev),
                              torch.from_numpy(params).to(dev))
