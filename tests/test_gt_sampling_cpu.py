"""CPU: the host gt_sampling mirror (pcdet.datasets.augmentor.database_sampler) against the reference's own DataBaseSampler
(tests/golden/ref_gt_sampling.npz), the synthetic ground-truth database, and the draws of the device route. BEV IoU is the oracle's
C restatement (bev_iou=), so nothing here needs a GPU."""
import logging
import pickle

import numpy as np
import pytest

import oracle
import gt_sampling_cases as gc
from pcdet.config import EasyDict
from pcdet.datasets import SyntheticDataset
from pcdet.datasets import synthetic as syn
from pcdet.datasets.augmentor import DataAugmentor
from pcdet.datasets.augmentor.data_augmentor import DeviceDataAugmentor
from pcdet.datasets.augmentor.database_sampler import DataBaseSampler
from pcdet.model_cfgs import kitti_augmentor_cfg


def oracle_iou(a, b):
    return oracle.boxes_pairwise(a, b, 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize('run', list(gc.RUNS))
def test_against_reference_golden(run):
    """call by call under the run's seed: chosen database entries, pointers and permutation heads, valid mask, boxes, names and
    output points all equal the reference's (points: f32 additions of identical operands, removals margin-safe)"""
    g = gc.golden()
    infos = gc.db_infos(run)
    sampler = DataBaseSampler(None, gc.sampler_cfg(run), gc.CLASS_NAMES, bev_iou=oracle_iou, db_infos=infos)
    np.random.seed(gc.RUNS[run]['seed'])
    pasted_any = 0
    for c in range(gc.N_CALLS):
        key = '%s/%d/' % (run, c)
        d = sampler(gc.call_input(run, c))
        chosen = [infos[name][i]['obj_id'] for name, picked in sampler.last_groups for i in picked]
        assert chosen == g[key + 'chosen'].tolist(), (run, c)
        sizes = dict((name, len(picked)) for name, picked in sampler.last_groups)
        off = np.concatenate([[0], np.cumsum([sizes.get(name, 0) for name in sampler.sample_groups])])
        assert off.tolist() == g[key + 'group_offsets'].tolist()
        assert [grp['pointer'] for grp in sampler.sample_groups.values()] == g[key + 'pointer'].tolist()
        for k, grp in enumerate(sampler.sample_groups.values()):
            head = g[key + 'perm'][k]
            head = head[head >= 0]
            assert list(grp['indices'][:len(head)]) == head.tolist()
        np.testing.assert_array_equal(sampler.last_valid, g[key + 'valid'])
        np.testing.assert_array_equal(bits(d['gt_boxes']), bits(g[key + 'boxes']))
        assert [gc.CLASS_NAMES.index(n) + 1 for n in d['gt_names']] == g[key + 'names'].tolist()
        assert d['gt_boxes_mask'].all() and len(d['gt_boxes_mask']) == len(d['gt_boxes'])
        want = gc.expected_points(run, c)
        assert d['points'].dtype == np.float32 and d['points'].shape == want.shape
        np.testing.assert_array_equal(bits(d['points']), bits(want))
        pasted_any += int(g[key + 'valid'].any())
        if gc.RUNS[run]['road']:
            assert 'calib' not in d or not g[key + 'valid'].any()
    assert pasted_any > 0


def test_groundtruth_database_files_memory_and_counts(tmp_path):
    ds = SyntheticDataset(num_frames=3, n_points=3000)
    mem = ds.create_groundtruth_database(None)
    disk = ds.create_groundtruth_database(str(tmp_path))
    with open(str(tmp_path / 'dbinfos_train.pkl'), 'rb') as f:
        assert sorted(pickle.load(f)) == sorted(disk)
    assert sorted(mem) == sorted(disk) == sorted(ds.class_names)
    n_obj = 0
    for name in mem:
        assert len(mem[name]) == len(disk[name])
        for a, b in zip(mem[name], disk[name]):
            for k in ('name', 'image_idx', 'gt_idx', 'num_points_in_gt', 'difficulty', 'score'):
                assert a[k] == b[k]
            np.testing.assert_array_equal(a['box3d_lidar'], b['box3d_lidar'])
            pts = np.fromfile(str(tmp_path / b['path']), dtype=np.float32).reshape(-1, 4)
            np.testing.assert_array_equal(bits(pts), bits(a['points']))
            assert b['path'] == 'gt_database/%s_%s_%d.bin' % (b['image_idx'], name, b['gt_idx']) and a['path'] is None
            n_obj += 1
    assert n_obj == 3 * 12
    for fid in ds.sample_id_list:                       # counts and members: the oracle's points_in_boxes_cpu (the CPU twin's rule)
        pts, boxes = syn.kitti_frame(int(fid), 3000)
        member = oracle.points_in_boxes_cpu(boxes[:, :7], pts[:, :3])
        for name in mem:
            for info in mem[name]:
                if info['image_idx'] == fid:
                    i = info['gt_idx']
                    assert info['num_points_in_gt'] == int(member[i].sum())
                    np.testing.assert_array_equal(bits(info['points'][:, :3]), bits(pts[member[i] > 0][:, :3] - boxes[i, :3]))
    # both forms through the sampler: same draws, same output
    cfg = kitti_augmentor_cfg(['dbinfos_train.pkl'])[0]
    cfg.PREPARE['filter_by_min_points'] = ['Car:2', 'Pedestrian:2', 'Cyclist:2']
    a = DataBaseSampler(tmp_path, cfg, ds.class_names, bev_iou=oracle_iou)
    cfg2 = EasyDict(dict(cfg, DB_INFO_PATH=[]))
    b = DataBaseSampler(None, cfg2, ds.class_names, bev_iou=oracle_iou, db_infos=mem)
    pts, boxes = syn.kitti_frame(7, 2000)
    outs = []
    for s in (a, b):
        np.random.seed(2)
        outs.append(s({'points': pts.copy(), 'gt_boxes': boxes[:, :7].copy(), 'gt_names': np.array(ds.class_names)[boxes[:, 7].astype(int) - 1]}))
    np.testing.assert_array_equal(bits(outs[0]['points']), bits(outs[1]['points']))
    np.testing.assert_array_equal(bits(outs[0]['gt_boxes']), bits(outs[1]['gt_boxes']))
    assert len(outs[0]['gt_boxes']) > len(boxes)
    w = SyntheticDataset(num_frames=2, n_points=2000, kind='waymo').create_groundtruth_database(None)
    info = w['Vehicle'][0]
    assert info['sequence_name'] == SyntheticDataset.WAYMO_SEQUENCE and info['sample_idx'] == 0 and info['points'].shape[1] == 5


def test_prepare_filters():
    infos = {'Car': [{'name': 'Car', 'num_points_in_gt': n, 'difficulty': d, 'image_idx': '0', 'box3d_lidar': np.zeros(7, np.float32)}
                     for n, d in [(1, 0), (5, 0), (9, -1), (7, 1), (4, 0)]],
             'Pedestrian': [{'name': 'Pedestrian', 'num_points_in_gt': 1, 'difficulty': 0, 'image_idx': '0',
                             'box3d_lidar': np.zeros(7, np.float32)}]}
    cfg = EasyDict({'PREPARE': {'filter_by_min_points': ['Car:5', 'Pedestrian:0'], 'filter_by_difficulty': [-1]},
                    'SAMPLE_GROUPS': ['Car:2', 'Pedestrian:1', 'Truck:3'], 'NUM_POINT_FEATURES': 4, 'REMOVE_EXTRA_WIDTH': [0, 0, 0]})
    s = DataBaseSampler(None, cfg, ['Car', 'Pedestrian'], db_infos=infos)
    assert [(i['num_points_in_gt'], i['difficulty']) for i in s.db_infos['Car']] == [(5, 0), (7, 1)]
    assert len(s.db_infos['Pedestrian']) == 1 and list(s.sample_groups) == ['Car', 'Pedestrian']
    assert s.sample_groups['Car']['pointer'] == 2
    state = pickle.loads(pickle.dumps(s))
    assert state.logger is None and list(state.sample_groups) == ['Car', 'Pedestrian']


def test_gt_sampling_in_the_augmentor_queue():
    """DataAugmentor takes gt_sampling like the reference; the steps that are not provided keep raising"""
    infos = gc.db_infos('plain')
    steps = [gc.sampler_cfg('plain'), EasyDict({'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']})]
    aug = DataAugmentor(None, steps, gc.CLASS_NAMES, bev_iou=oracle_iou, db_infos=infos)
    assert isinstance(aug.db_sampler, DataBaseSampler) and len(aug.data_augmentor_queue) == 2
    np.random.seed(3)
    d = aug.forward(gc.call_input('plain', 0))
    g = gc.golden()
    assert 'gt_boxes_mask' not in d and len(d['gt_boxes']) == len(d['gt_names']) == len(g['plain/0/boxes'])
    assert len(d['points']) == len(gc.expected_points('plain', 0))
    with pytest.raises(NotImplementedError):
        DataAugmentor(None, [EasyDict({'NAME': 'random_local_rotation'})], gc.CLASS_NAMES)
    with pytest.raises(NotImplementedError):                  # the device route: gt_sampling first or not at all
        DeviceDataAugmentor(steps[::-1], gc.CLASS_NAMES, bev_iou=oracle_iou, db_infos=infos)


def test_class_without_a_labelled_object_is_skipped(caplog):
    """the deviation: the reference recurses without end; the mirror skips the class, draws nothing for it and logs once"""
    infos = gc.db_infos('plain')
    car_frames = {i['image_idx'] for i in infos['Car']}
    ped_frames = {i['image_idx'] for i in infos['Pedestrian']}
    only_car = sorted(car_frames - ped_frames)
    assert only_car, 'the golden database has a frame with cars and no pedestrian'
    cfg = EasyDict(dict(gc.sampler_cfg('plain'), SAMPLE_GROUPS=['Pedestrian:3', 'Car:2']))
    log = logging.getLogger('gt_sampling_test')
    a = DataBaseSampler(None, cfg, gc.CLASS_NAMES, logger=log, bev_iou=oracle_iou, db_infos=infos)
    b = DataBaseSampler(None, EasyDict(dict(cfg, SAMPLE_GROUPS=['Car:2'])), gc.CLASS_NAMES, bev_iou=oracle_iou, db_infos=infos)
    with caplog.at_level(logging.INFO, logger='gt_sampling_test'):
        for c in range(3):
            outs = []
            for s in (a, b):
                np.random.seed(40 + c)
                d = gc.call_input('plain', c)
                d['sample_id_list'] = only_car[:1]
                outs.append(s(d))
                state = np.random.get_state()
                outs.append((state[1].tolist(), state[2]))
            assert outs[1] == outs[3]                                         # no random number went to the skipped class
            np.testing.assert_array_equal(bits(outs[0]['points']), bits(outs[2]['points']))
            assert [n for n, _ in a.last_groups] == ['Car']
    assert sum('Pedestrian' in r.getMessage() for r in caplog.records) == 1


def test_device_draws_consume_np_random_like_the_host_route():
    """DeviceDataAugmentor.draw_batch on 4 frames == the host sampler followed by the world steps on those frames in order: the same
    generator state afterwards, the same candidates, the same world parameters"""
    infos = gc.db_infos('road')
    steps = [gc.sampler_cfg('road'), EasyDict({'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']}),
             EasyDict({'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]}),
             EasyDict({'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]})]
    host = DataAugmentor(None, steps, gc.CLASS_NAMES, bev_iou=oracle_iou, db_infos=infos)
    dev = DeviceDataAugmentor(steps, gc.CLASS_NAMES, bev_iou=oracle_iou, db_infos=infos)
    dev.set_labelled(gc.labelled_ids('road'))
    ins = [gc.call_input('road', c) for c in range(4)]
    np.random.seed(11)
    groups = []
    for d in ins:
        host.forward(dict(d, points=d['points'].copy(), gt_boxes=d['gt_boxes'].copy()))
        groups.append(host.db_sampler.last_groups)
    want = np.random.get_state()
    np.random.seed(11)
    params, angles, draw = dev.draw_batch(4, gt_names=[d['gt_names'] for d in ins], road_planes=[d['road_plane'] for d in ins],
                                          calibs=[d['calib'] for d in ins])
    got = np.random.get_state()
    assert got[2] == want[2] and np.array_equal(got[1], want[1])
    assert draw['groups'] == groups and params.shape == (4, 8) and angles.shape == (4,)
    B, S, W = draw['cand'].shape
    assert W == 20 and S == max(sum(len(p) for _, p in g) for g in groups) and draw['group_offsets'].shape == (4, 4)
    db = dev.database
    assert db.num_objects == sum(len(v) for v in infos.values()) and db.points.shape == (int(db.obj_counts.sum()), 4)
    for b, g in enumerate(groups):
        objs = [db.class_base[name] + i for name, picked in g for i in picked]
        n = len(objs)
        assert draw['cand_obj'][b, :n].tolist() == objs and draw['group_offsets'][b, -1] == n
        np.testing.assert_array_equal(draw['cand'][b, :n, 0:7], db.boxes[objs])
        np.testing.assert_array_equal(draw['cand'][b, :n, 7], db.classes[objs])
        np.testing.assert_array_equal(draw['cand'][b, :n, 17:20], db.boxes[objs][:, :3])
        np.testing.assert_array_equal(draw['cand'][b, :n, 11], db.boxes[objs][:, 2] - draw['cand'][b, :n, 8])
        np.testing.assert_array_equal(draw['cand'][b, :n, 12:15], db.boxes[objs][:, 3:6] + np.float32(0.2))
        assert np.abs(draw['cand'][b, :n, 8]).max() > 0 and not draw['cand'][b, n:].any()
    assert draw['n_cand_points'] == sum(int(db.obj_counts[db.class_base[name] + i]) for g in groups for name, picked in g for i in picked)
