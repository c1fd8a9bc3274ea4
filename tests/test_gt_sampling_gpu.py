"""GPU: crb_gt_sample_select / crb_gt_sample_paste (csrc/gt_sampling.hip) and the device route of gt_sampling.

select is checked against a torch composition of boxes_iou_bev on the same device - the same device function, so equality is exact.
paste and process_batch are checked bit for bit against the host mirror (pcdet.datasets.augmentor.database_sampler) whose BEV IoU is
left at its default, the HIP kernel. The golden test checks the device route against the reference's own sampler."""
import numpy as np
import pytest
import torch

import gt_sampling_cases as gc
from pcdet.config import EasyDict
from pcdet.datasets.augmentor import DataAugmentor
from pcdet.datasets.augmentor.data_augmentor import DeviceDataAugmentor
from pcdet.datasets.augmentor.database_sampler import DataBaseSampler

PCR = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
SIZES = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_same_bits(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# select against a torch composition of boxes_iou_bev
# ---------------------------------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(37, [20, 15, 15]), (0, [7, 0, 0]), (5, [0, 0, 0]), (3, [0, 0, 1])]     # (G, group sizes) per frame
SELECT_SEED = 4          # (chosen on the CPU oracle so that each of the four cases below occurs at least three times)


def _dense_boxes(rng, n, side):
    cls = rng.integers(1, 4, n)
    out = np.zeros((n, 8), np.float32)
    for i, c in enumerate(cls):
        out[i] = [rng.uniform(0, side), rng.uniform(0, side), rng.uniform(-1.2, -0.6), *SIZES[int(c)], rng.uniform(-np.pi, np.pi), c]
    return out


def _select_inputs():
    rng = np.random.default_rng(SELECT_SEED)
    B, G, S, K = len(SELECT_SHAPES), 37, 50, 3
    gt = np.zeros((B, G, 8), np.float32)
    counts = np.zeros(B, np.int32)
    cand = np.zeros((B, S, 20), np.float32)
    cand_obj = np.zeros((B, S), np.int32)
    goff = np.zeros((B, K + 1), np.int32)
    obj_counts = rng.integers(0, 9, 40)
    for b, (g, sizes) in enumerate(SELECT_SHAPES):
        side = 34.0 if b == 0 else 9.0
        gt[b, :g] = _dense_boxes(rng, g, side)
        counts[b] = g
        n = sum(sizes)
        boxes = _dense_boxes(rng, n, side)
        cand[b, :n, 0:7] = boxes[:, :7]
        cand[b, :n, 7] = np.repeat([1, 2, 3], sizes)
        cand[b, :n, 8] = np.where(rng.uniform(size=n) < 0.5, 0, rng.uniform(-0.4, 0.4, n)).astype(np.float32)
        cand_obj[b, :n] = rng.integers(0, 40, n)
        goff[b] = np.concatenate([[0], np.cumsum(sizes)])
    gt[3, 3:] = 7.0                                             # rows behind a frame's count are padding and must not be read
    return gt, counts, cand, cand_obj, goff, obj_counts


@pytest.mark.gpu
def test_select_equals_torch_composition_of_boxes_iou_bev(dev):
    from crbhip import gt_sampling, CrbHipError
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    gt, counts, cand, cand_obj, goff, obj_counts = _select_inputs()
    B, G, S = gt.shape[0], gt.shape[1], cand.shape[1]
    db = {'points': torch.zeros((int(obj_counts.sum()), 4), device=dev),
          'obj_offsets': torch.from_numpy(np.concatenate([[0], np.cumsum(obj_counts)]).astype(np.int32)).to(dev)}
    t = lambda a: torch.from_numpy(a).to(dev)
    args = (t(gt), t(counts), t(cand), t(cand_obj), t(goff), db)
    valid, out_boxes, new_counts, cand_rows, paste_counts = [x.cpu().numpy() for x in gt_sampling.select(*args)]
    again = [x.cpu().numpy() for x in gt_sampling.select(*args)]
    assert np.array_equal(valid, again[0]) and np.array_equal(bits(out_boxes), bits(again[1])) and np.array_equal(cand_rows, again[3])
    cases = dict.fromkeys(['frame box', 'same group, both dropped', 'accepted earlier candidate only', 'accepted next to a rejected one'], 0)
    for b, (g, sizes) in enumerate(SELECT_SHAPES):
        existed = t(gt[b, :g, :7])
        is_cand = np.zeros(g, bool)
        rejected = torch.zeros((0, 7), device=dev)
        want_valid, want_rows = np.zeros(S, np.uint8), gt[b, :g].copy()
        for k in range(3):
            s0, s1 = goff[b, k], goff[b, k + 1]
            if s1 == s0:
                continue
            sb = t(cand[b, s0:s1, :7])
            iou2 = iou3d_nms_utils.boxes_iou_bev(sb, sb)
            iou2.fill_diagonal_(0)
            hit_same = (iou2 != 0).any(1).cpu().numpy()
            iou1 = iou3d_nms_utils.boxes_iou_bev(sb, existed).cpu().numpy() if len(existed) else np.zeros((s1 - s0, 0), np.float32)
            hit_frame, hit_acc = (iou1[:, ~is_cand] != 0).any(1), (iou1[:, is_cand] != 0).any(1)
            ok = ~(hit_frame | hit_acc | hit_same)
            hit_rej = (iou3d_nms_utils.boxes_iou_bev(sb, rejected) != 0).any(1).cpu().numpy() if len(rejected) else np.zeros(s1 - s0, bool)
            cases['frame box'] += int(hit_frame.sum())
            cases['same group, both dropped'] += int((hit_same & ~hit_frame & ~hit_acc).sum())
            cases['accepted earlier candidate only'] += int((hit_acc & ~hit_frame & ~hit_same).sum())
            cases['accepted next to a rejected one'] += int((ok & hit_rej).sum())
            want_valid[s0:s1] = ok
            rows = np.concatenate([cand[b, s0:s1, :7], cand[b, s0:s1, 7:8]], 1)[ok]
            rows[:, 2] = rows[:, 2] - cand[b, s0:s1, 8][ok]
            want_rows = np.concatenate([want_rows, rows], 0)
            existed = torch.cat([existed, sb[torch.from_numpy(ok).to(dev)]], 0)
            rejected = torch.cat([rejected, sb[torch.from_numpy(~ok).to(dev)]], 0)
            is_cand = np.concatenate([is_cand, np.ones(int(ok.sum()), bool)])
        np.testing.assert_array_equal(valid[b], want_valid)
        assert new_counts[b] == len(want_rows)
        assert_same_bits(out_boxes[b, :len(want_rows)], want_rows)
        assert not out_boxes[b, len(want_rows):].any()                                   # zero padding
        npts = np.where(want_valid[:sum(sizes)] > 0, obj_counts[cand_obj[b, :sum(sizes)]], 0)
        want_cr = -np.ones(S, np.int64)
        want_cr[:sum(sizes)][want_valid[:sum(sizes)] > 0] = (np.cumsum(npts) - npts)[want_valid[:sum(sizes)] > 0]
        np.testing.assert_array_equal(cand_rows[b], want_cr)
        assert paste_counts[b] == npts.sum()
    print('select cases:', cases)
    assert all(v > 0 for v in cases.values()), cases
    assert valid[0].sum() > 0 and (valid[0, :50] == 0).sum() > 0
    # above capacity: S > 256, and G + S > 512
    for g_big, s_big in ((1, 257), (300, 250)):
        with pytest.raises(CrbHipError, match='UNSUPPORTED'):
            gt_sampling.select(torch.zeros((1, g_big, 8), device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                               torch.zeros((1, s_big, 20), device=dev), torch.zeros((1, s_big), dtype=torch.int32, device=dev),
                               torch.zeros((1, 4), dtype=torch.int32, device=dev), db)


# ---------------------------------------------------------------------------------------------------------------------------------
# paste against the host mirror
# ---------------------------------------------------------------------------------------------------------------------------------
OBJ_POINTS = [0, 1, 63, 64, 65, 7, 30, 2, 5, 12]
OBJ_CLASS = [1, 1, 1, 1, 2, 2, 2, 3, 3, 3]


def _grid_database(C):
    """ten objects that do not touch each other, on a grid 8 m apart; every call draws all of them (sample numbers = class sizes)"""
    rng = np.random.default_rng(9)
    infos = {n: [] for n in gc.CLASS_NAMES}
    for o, (n, c) in enumerate(zip(OBJ_POINTS, OBJ_CLASS)):
        box = np.array([8.0 + 8 * (o % 4) + rng.uniform(-1, 1), -8.0 + 8 * (o // 4) + rng.uniform(-1, 1), rng.uniform(-1.1, -0.7),
                        *SIZES[c], rng.uniform(-np.pi, np.pi)], np.float32)
        pts = np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)) * box[3:6], rng.uniform(0, 1, (n, C - 3))], 1).astype(np.float32)
        infos[gc.CLASS_NAMES[c - 1]].append({'name': gc.CLASS_NAMES[c - 1], 'path': None, 'points': pts, 'image_idx': '%06d' % o,
                                             'gt_idx': 0, 'box3d_lidar': box, 'num_points_in_gt': n, 'difficulty': 0})
    return infos


def _paste_frames(infos, counts, C):
    rng = np.random.default_rng(10)
    giant = np.array([[20.0, 0.0, -1.0, 90.0, 90.0, 2.0, 0.3, 1]], np.float32)
    car0, ped1 = infos['Car'][0]['box3d_lidar'], infos['Pedestrian'][1]['box3d_lidar']
    frames, gts = [], []
    for n in counts:
        pts = np.concatenate([rng.uniform([0, -16, -2.2], [40, 16, 0.4], (n, 3)), rng.uniform(0, 1, (n, C - 3))], 1).astype(np.float32)
        if n == 0:                                  # two frame boxes that sit on database objects: those two are rejected
            g = np.stack([np.concatenate([car0 + np.float32([0.5, 0.2, 0, 0, 0, 0, 0.1]), [1]]),
                          np.concatenate([ped1 + np.float32([0.1, 0.1, 0, 0, 0, 0, 0.4]), [2]])]).astype(np.float32)
        elif n == 1:                                # the frame's only point lies inside an object that is accepted: nothing is left
            pts[0, :3] = infos['Car'][1]['box3d_lidar'][:3]
            g = np.zeros((0, 8), np.float32)
        elif n == 2500:                             # one box over everything: every candidate is rejected
            g = giant.copy()
        else:
            g = np.zeros((0, 8), np.float32)
        frames.append(pts)
        gts.append(g)
    return frames, gts


def _device_sample(aug, frames, gts, dev, road=False, lazy=False):
    """draw_batch + one upload + select + paste -> (per-frame points, per-frame boxes (G', 8), valid (B, S), draw)"""
    from crbhip import gt_sampling
    B = len(frames)
    names = np.array(gc.CLASS_NAMES)
    kw = {'road_planes': [gc.ROAD_PLANE] * B, 'calibs': [gc.AffineCalib()] * B} if road else {}
    _, _, draw = aug.draw_batch(B, gt_names=[names[g[:, 7].astype(np.int64) - 1] for g in gts], **kw)
    G = max(1, max(len(g) for g in gts))
    pad = np.zeros((B, G, 8), np.float32)
    for k, g in enumerate(gts):
        pad[k, :len(g)] = g
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    db = aug.database.device_tensors(dev)
    cand, cand_obj = t(draw['cand']), t(draw['cand_obj'])
    valid, boxes, new_counts, cand_rows, paste_counts = gt_sampling.select(
        t(pad), t(np.array([len(g) for g in gts], np.int32)), cand, cand_obj, t(draw['group_offsets']), db)
    pts = t(np.concatenate(frames, 0))
    off = t(np.concatenate([[0], np.cumsum([len(p) for p in frames])]).astype(np.int32))
    cap = len(pts) + draw['n_cand_points']
    out, new_off = gt_sampling.paste(pts, off, cand, cand_obj, valid, cand_rows, paste_counts, db, capacity=cap, lazy=lazy)
    if lazy:
        assert out.shape[0] == cap and new_off.numel() == B + 2 and int(new_off[B + 1]) == cap
    o = new_off.cpu().tolist()
    out_h, boxes_h, nc = out.cpu().numpy(), boxes.cpu().numpy(), new_counts.cpu().tolist()
    for b in range(B):
        assert not boxes_h[b, nc[b]:].any()
    return [out_h[o[b]:o[b + 1]] for b in range(B)], [boxes_h[b, :nc[b]] for b in range(B)], valid.cpu().numpy(), draw


def _host_sample(sampler, frames, gts, labelled=None, road=False):
    outs = []
    for p, g in zip(frames, gts):
        d = {'points': p.copy(), 'gt_boxes': g[:, :7].copy(), 'gt_names': np.array(gc.CLASS_NAMES)[g[:, 7].astype(np.int64) - 1],
             'sample_id_list': labelled}
        if road:
            d['road_plane'], d['calib'] = gc.ROAD_PLANE.copy(), gc.AffineCalib()
        d = sampler(d)
        cls = np.array([gc.CLASS_NAMES.index(n) + 1 for n in d['gt_names']], np.float32).reshape(-1, 1)
        outs.append((d['points'], np.concatenate([d['gt_boxes'], cls], 1), sampler.last_valid.copy()))
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize('C,extra,road,reverse', [(4, 0.0, False, False), (5, 0.2, True, True), (4, 0.2, False, True),
                                                  (5, 0.0, True, False)])
def test_paste_bit_equal_to_host_mirror(dev, C, extra, road, reverse):
    infos = _grid_database(C)
    counts = [0, 1027, 1, 2500][::-1] if reverse else [0, 1027, 1, 2500]
    frames, gts = _paste_frames(infos, counts, C)
    cfg = EasyDict({'NAME': 'gt_sampling', 'USE_ROAD_PLANE': road, 'SAMPLE_GROUPS': ['Car:4', 'Pedestrian:3', 'Cyclist:3'],
                    'NUM_POINT_FEATURES': C, 'REMOVE_EXTRA_WIDTH': [extra] * 3, 'LIMIT_WHOLE_SCENE': False})
    host = DataBaseSampler(None, cfg, gc.CLASS_NAMES, db_infos=infos)                  # (bev_iou: the default, the HIP kernel)
    np.random.seed(21)
    want = _host_sample(host, frames, gts, road=road)
    aug = DeviceDataAugmentor([cfg], gc.CLASS_NAMES, db_infos=infos)
    np.random.seed(21)
    got_p, got_b, valid, draw = _device_sample(aug, frames, gts, dev, road=road)
    np.random.seed(21)
    again_p, again_b, _, _ = _device_sample(aug, frames, gts, dev, road=road, lazy=True)
    assert draw['cand'].shape[1] == 10 and (draw['group_offsets'] == [0, 4, 7, 10]).all()
    for b, n in enumerate(counts):
        p, x, v = want[b]
        np.testing.assert_array_equal(valid[b].astype(bool), v)
        assert_same_bits(got_p[b], p)
        assert_same_bits(got_b[b], x)
        assert_same_bits(again_p[b], got_p[b])
        assert_same_bits(again_b[b], got_b[b])
        pasted = sum(OBJ_POINTS[o] for o, ok in zip(draw['cand_obj'][b], v) if ok)
        if n == 2500:
            assert not v.any() and len(p) == 2500                                        # every candidate rejected: the frame as it was
            assert_same_bits(p, frames[b])
        elif n == 1:
            assert v.all() and len(p) == pasted == sum(OBJ_POINTS)                       # the only scene point was removed
        elif n == 0:
            assert v.sum() == 8 and len(p) == pasted
        else:
            assert v.all() and pasted < len(p) < pasted + n                              # some scene points removed, some kept
        if road:
            assert np.abs(draw['cand'][b, :, 8]).min() > 0
        else:
            assert not draw['cand'][b, :, 8].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's golden through the device route
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('run', list(gc.RUNS))
def test_device_route_against_reference_golden(dev, run):
    """all 8 calls of a run as one batch: the reference's valid masks, boxes, pasted points and kept-point sets"""
    g = gc.golden()
    infos = gc.db_infos(run)
    aug = DeviceDataAugmentor([gc.sampler_cfg(run)], gc.CLASS_NAMES, db_infos=infos)
    aug.set_labelled(gc.labelled_ids(run))
    frames = [g['frame_points_%d' % c] for c in range(gc.N_CALLS)]
    gts = [g['frame_boxes'][c] for c in range(gc.N_CALLS)]
    np.random.seed(gc.RUNS[run]['seed'])
    got_p, got_b, valid, draw = _device_sample(aug, frames, gts, dev, road=gc.RUNS[run]['road'])
    for c in range(gc.N_CALLS):
        key = '%s/%d/' % (run, c)
        n = len(g[key + 'valid'])
        chosen = [infos[name][i]['obj_id'] for name, picked in draw['groups'][c] for i in picked]
        assert chosen == g[key + 'chosen'].tolist()
        np.testing.assert_array_equal(valid[c, :n].astype(bool), g[key + 'valid'])
        assert not valid[c, n:].any()
        assert_same_bits(got_b[c][:, :7], g[key + 'boxes'])
        assert got_b[c][:, 7].tolist() == g[key + 'names'].tolist()
        assert_same_bits(got_p[c], gc.expected_points(run, c))


# ---------------------------------------------------------------------------------------------------------------------------------
# process_batch
# ---------------------------------------------------------------------------------------------------------------------------------
def _dp_cfgs():
    return [EasyDict({'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}),
            EasyDict({'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': EasyDict({'train': False, 'test': False})}),
            EasyDict({'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.05, 0.05, 0.1], 'MAX_POINTS_PER_VOXEL': 5,
                      'MAX_NUMBER_OF_VOXELS': EasyDict({'train': 16000, 'test': 40000})})]


_kitti = {}


def _kitti_setup(n_frames=6, n_points=3000):
    """the KITTI queue (sampling + flip + rotation + scaling) over the in-memory database of a small synthetic dataset"""
    if not _kitti:
        from pcdet.datasets import SyntheticDataset
        from pcdet.model_cfgs import kitti_augmentor_cfg
        ds = SyntheticDataset(num_frames=n_frames, n_points=n_points)
        cfgs = kitti_augmentor_cfg()
        cfgs[0].PREPARE['filter_by_min_points'] = ['Car:2', 'Pedestrian:2', 'Cyclist:2']
        _kitti.update(ds=ds, cfgs=cfgs, infos=ds.create_groundtruth_database(None))
    return _kitti['ds'], _kitti['cfgs'], _kitti['infos']


class _ReadBacks(object):
    """counts the calls that bring device values to the host while it is active"""
    NAMES = ('cpu', 'item', 'tolist', '__int__', '__bool__', '__index__', '__float__', 'numpy')

    def __enter__(self):
        self.count, self.saved = 0, {}
        for name in self.NAMES:
            orig = getattr(torch.Tensor, name)
            self.saved[name] = orig

            def counted(t, *a, _orig=orig, **k):
                if t.is_cuda:
                    self.count += 1
                return _orig(t, *a, **k)
            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(torch.Tensor, name, orig)


@pytest.mark.gpu
def test_process_batch_full_kitti_queue(dev):
    """sampling + flip + rotation + scaling + range masks == the host DataAugmentor + host DataProcessor frame by frame under one
    seed, points and boxes; one read-back; with a labelled set every pasted object comes from a labelled frame"""
    from pcdet.datasets.processor.data_processor import DataProcessor, DeviceDataProcessor
    from pcdet.datasets import synthetic as syn
    ds, cfgs, infos = _kitti_setup()
    frames, gts = zip(*[syn.kitti_frame(40 + f, 3000) for f in range(4)])
    frames, gts = list(frames), list(gts)
    labelled = ds.sample_id_list[:3]
    aug = DeviceDataAugmentor(cfgs, ds.class_names, db_infos=infos)
    aug.set_labelled(labelled)
    dp = DeviceDataProcessor(_dp_cfgs(), PCR, True, 4, device=dev)
    np.random.seed(5)
    dp.process_batch(frames, gts, list('abcd'), augmentor=aug)                           # (uploads the database)
    np.random.seed(6)
    with _ReadBacks() as rb:
        a = dp.process_batch(frames, gts, list('abcd'), augmentor=aug)
    assert rb.count == 1, rb.count
    host_aug = DataAugmentor(None, cfgs, ds.class_names, db_infos=infos)
    host_dp = DataProcessor(_dp_cfgs()[:1], PCR, training=True, num_point_features=4)
    names = np.array(ds.class_names)
    np.random.seed(6)
    off = a['point_frame_offsets'].cpu().tolist()
    valid = a['gt_sampling_valid'].cpu().numpy()
    n_pasted = 0
    for k, (p, x) in enumerate(zip(frames, gts)):
        d = host_aug.forward({'points': p.copy(), 'gt_boxes': x[:, :7].copy(), 'gt_names': names[x[:, 7].astype(np.int64) - 1],
                              'sample_id_list': labelled})
        cls = np.array([ds.class_names.index(n) + 1 for n in d['gt_names']], np.float32).reshape(-1, 1)
        d['gt_boxes'] = np.concatenate([d['gt_boxes'], cls], 1)
        d = host_dp.forward(d)
        seg = a['points'][off[k]:off[k + 1]].cpu().numpy()
        assert (seg[:, 0] == k).all()
        assert_same_bits(seg[:, 1:], d['points'])
        assert_same_bits(a['gt_boxes'][k, :len(d['gt_boxes'])].cpu().numpy(), d['gt_boxes'])
        assert not a['gt_boxes'][k, len(d['gt_boxes']):].cpu().numpy().any()
        assert a['gt_sampling_groups'][k] == host_aug.db_sampler.last_groups
        np.testing.assert_array_equal(valid[k, :len(host_aug.db_sampler.last_valid)].astype(bool), host_aug.db_sampler.last_valid)
        flat = [(name, i) for name, picked in a['gt_sampling_groups'][k] for i in picked]
        for (name, i), ok in zip(flat, valid[k]):
            if ok:
                n_pasted += 1
                assert infos_after_prepare(aug)[name][i]['image_idx'] in labelled
    assert n_pasted > 0 and len(off) == 5
    # the CPU device of the same processor goes through the host mirror and gives the same batch
    np.random.seed(6)
    c = DeviceDataProcessor(_dp_cfgs(), PCR, True, 4, device='cpu').process_batch(frames, gts, list('abcd'), augmentor=aug)
    assert_same_bits(c['points'].numpy(), a['points'].cpu().numpy())
    assert_same_bits(c['gt_boxes'].numpy(), a['gt_boxes'].cpu().numpy())


def infos_after_prepare(aug):
    return aug.sampler.db_infos


@pytest.mark.gpu
def test_sampled_batch_feeds_a_second_training_step(dev):
    """B = 2: process_batch with gt_sampling in the queue -> SECOND forward + backward with a finite loss"""
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.processor.data_processor import DeviceDataProcessor
    from pcdet.datasets import synthetic as syn
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    ds, cfgs, infos = _kitti_setup()
    frames, gts = zip(*[syn.kitti_frame(60 + f, 6000) for f in range(2)])
    aug = DeviceDataAugmentor(cfgs, ds.class_names, db_infos=infos)
    dp = DeviceDataProcessor(_dp_cfgs(), PCR, True, 4, device=dev)
    np.random.seed(8)
    batch = dp.process_batch(list(frames), list(gts), ['a', 'b'], augmentor=aug)
    assert int(batch['gt_sampling_valid'].sum()) > 0 and batch['gt_boxes'].shape[1] > 12
    torch.manual_seed(0)
    model = build_network(second_cfg('kitti').MODEL, 3, SyntheticDataset(num_frames=2)).to(dev).train()
    ret, _, _ = model(batch)
    assert torch.isfinite(ret['loss'])
    ret['loss'].backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@pytest.mark.gpu
def test_bad_input_raises(dev):
    from crbhip import gt_sampling, CrbHipError
    from crbhip.gt_database import DeviceGtDatabase
    infos = _grid_database(4)
    cfg = EasyDict({'NAME': 'gt_sampling', 'USE_ROAD_PLANE': False, 'SAMPLE_GROUPS': ['Car:4'], 'NUM_POINT_FEATURES': 4,
                    'REMOVE_EXTRA_WIDTH': [0, 0, 0]})
    flip = EasyDict({'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']})
    with pytest.raises(NotImplementedError):
        DeviceDataAugmentor([flip, cfg], gc.CLASS_NAMES, db_infos=infos)
    aug = DeviceDataAugmentor([cfg, flip], gc.CLASS_NAMES, db_infos=infos)
    with pytest.raises(CrbHipError):
        aug.database.device_tensors('cpu')
    db = aug.database.device_tensors(dev)
    assert isinstance(aug.database, DeviceGtDatabase) and db['points'].shape == (sum(OBJ_POINTS), 4)
    z = lambda *s, dt=torch.float32, d=dev: torch.zeros(s, dtype=dt, device=d)
    good = dict(gt_boxes=z(1, 2, 8), gt_counts=z(1, dt=torch.int32), cand=z(1, 3, 20), cand_obj=z(1, 3, dt=torch.int32),
                group_offsets=z(1, 2, dt=torch.int32), db=db)
    gt_sampling.select(**good)
    for key, bad in (('gt_boxes', z(1, 2, 8, d='cpu')), ('gt_boxes', z(1, 2, 10)), ('cand', z(1, 3, 19)),
                     ('cand_obj', z(1, 4, dt=torch.int32)), ('gt_counts', z(1)), ('group_offsets', z(2, 2, dt=torch.int32))):
        with pytest.raises(CrbHipError):
            gt_sampling.select(**dict(good, **{key: bad}))
    valid, _, _, rows, pc = gt_sampling.select(**good)
    pgood = dict(points=z(5, 4), frame_offsets=torch.tensor([0, 5], dtype=torch.int32, device=dev), cand=good['cand'],
                 cand_obj=good['cand_obj'], valid=valid, cand_rows=rows, paste_counts=pc, db=db, capacity=5)
    gt_sampling.paste(**pgood)
    for key, bad in (('points', z(5, 4, d='cpu')), ('points', z(5, 5)), ('capacity', 4), ('valid', valid.int()),
                     ('frame_offsets', torch.tensor([0, 2, 5], dtype=torch.int32, device=dev))):
        with pytest.raises(CrbHipError):
            gt_sampling.paste(**dict(pgood, **{key: bad}))
