"""CPU: the host route of the KITTI evaluator against the reference's recorded run (tests/golden/ref_kitti_eval.npz), and the
evaluation hooks of the synthetic dataset (calibration, camera-frame box functions against tests/golden/ref_kitti_hooks.npz,
generate_prediction_dicts, evaluation). Bars as in tests/test_kitti_eval_gpu.py, whose checks this file runs with route='host'."""
import os

import numpy as np
import pytest
import torch

import kitti_eval_cases as kc
import test_kitti_eval_gpu as shared
from pcdet.datasets import SyntheticDataset
from pcdet.datasets import synthetic as syn
from pcdet.utils import box_utils

FACTOR = 4
HOOKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_kitti_hooks.npz')


@pytest.mark.parametrize('case', shared.CASES)
def test_host_route_against_reference(case):
    bad = shared.check_case(case, shared.run(*shared.annos(case), route='host'))
    assert not bad, bad


def test_host_route_alpha_switched_off():
    gt, dt = shared.annos('small_noalpha')
    r = shared.run(gt, dt, route='host')
    bad = shared.check_against(shared.golden(), 'small_noalpha', r, full=False)
    assert not bad and 'aos' not in r['text'] and len(r['ret']) == 27, bad


def test_host_route_one_class_and_public_shapes():
    gt, dt = shared.annos('small')
    z = shared.golden()
    text, ret = shared.kitti_eval.get_official_eval_result(gt, dt, 'Cyclist', route='host')
    assert len(ret) == 12 and text.startswith('Cyclist AP@0.50, 0.50, 0.50:')
    for k in ret:                                                      # the class column of min_overlaps is the Cyclist's
        assert abs(ret[k] - z['small/ret_vals'][list(z['small/ret_keys']).index(k)]) <= 1e-7
    overlaps, parted, n_first, n_second = shared.kitti_eval.calculate_iou_partly(dt, gt, 1, route='host')
    assert all(o.shape == (len(d['name']), len(g['name'])) for o, g, d in zip(overlaps, gt, dt)) and len(parted) == 1
    assert parted[0].shape == (n_first.sum(), n_second.sum())
    with pytest.raises(ValueError):
        shared.kitti_eval.calculate_iou_partly(dt, gt, 3, route='host')


def test_rotated_intersection_closed_forms():
    f = shared.kitti_eval.rotated_intersection
    a = np.array([[0., 0., 4., 2., 0.3]])
    assert abs(f(a, a)[0] - 8.0) < 1e-12                                             # identical boxes
    assert abs(f(a, a + [0, 0, 0, 0, np.pi])[0] - 8.0) < 1e-12                       # turned by half a turn
    assert abs(f(np.array([[0., 0., 2., 2., 0.]]), np.array([[0., 0., 2., 2., np.pi / 4]]))[0] - (8 * np.sqrt(2) - 8)) < 1e-12
    assert f(a, a + [10, 0, 0, 0, 0])[0] == 0.0
    # a positive angle turns clockwise: the long axis of [4 x 1] at +45 degrees points to (+x, -y)
    c = shared.kitti_eval._corners(np.array([[0., 0., 4., 1., np.pi / 4]]))[0]
    assert c[np.argmax(c[:, 0]), 1] < 0


def test_hooks_against_reference():
    z = np.load(HOOKS)
    calib = syn.Calibration({k: z[k] for k in ('P2', 'R0', 'Tr_velo2cam')})
    for k, v in (('P2', syn.KITTI_P2), ('R0', syn.KITTI_R0), ('Tr_velo2cam', syn.KITTI_TR_VELO2CAM)):
        assert np.array_equal(z[k], np.array(v))
    assert tuple(z['image_shape']) == syn.KITTI_IMAGE_SHAPE
    boxes = z['boxes_lidar']
    cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes, calib)
    rect = calib.lidar_to_rect(boxes[:, 0:3])
    img, depth = calib.rect_to_img(rect)
    got = {'camera': cam, 'corners': box_utils.boxes3d_to_corners3d_kitti_camera(cam),
           'imageboxes': box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib),
           'imageboxes_clipped': box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=z['image_shape']),
           'rect': rect, 'lidar_back': calib.rect_to_lidar(rect), 'img': img, 'depth': depth,
           'rect_back': calib.img_to_rect(img[:, 0], img[:, 1], depth)}
    for k, v in got.items():
        err = np.abs(v - z[k]).max()
        print(k, err, 'bar', FACTOR * z['e_' + k])
        assert v.shape == z[k].shape and err <= FACTOR * z['e_' + k], k
    assert np.abs(got['lidar_back'] - boxes[:, 0:3]).max() < 1e-9 and np.array_equal(boxes, z['boxes_lidar'])


def test_generate_prediction_dicts(tmp_path):
    ds = SyntheticDataset(num_frames=2, n_points=500)
    boxes = torch.tensor(syn.kitti_frame_boxes(0)[:5, :7])
    pred = [{'pred_boxes': boxes, 'pred_scores': torch.linspace(0.9, 0.5, 5), 'pred_labels': torch.tensor([1, 1, 2, 3, 2])},
            {'pred_boxes': torch.zeros(0, 7), 'pred_scores': torch.zeros(0), 'pred_labels': torch.zeros(0, dtype=torch.long)}]
    annos = ds.generate_prediction_dicts({'frame_id': np.array(ds.sample_id_list)}, pred, ds.class_names, output_path=tmp_path)
    keys = {'name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score', 'boxes_lidar', 'frame_id'}
    assert all(set(a) == keys for a in annos) and [a['frame_id'] for a in annos] == ds.sample_id_list
    a, e = annos
    assert a['name'].tolist() == ['Car', 'Car', 'Pedestrian', 'Cyclist', 'Pedestrian'] and a['score'].dtype == np.float32
    assert a['bbox'].shape == (5, 4) and a['dimensions'].shape == (5, 3) and a['location'].shape == (5, 3) and a['boxes_lidar'].shape == (5, 7)
    cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes.numpy(), ds.calib)
    assert np.array_equal(a['location'], cam[:, 0:3]) and np.array_equal(a['dimensions'][:, 0], boxes.numpy()[:, 3])
    assert np.allclose(a['alpha'], -np.arctan2(-boxes.numpy()[:, 1], boxes.numpy()[:, 0]) + cam[:, 6])
    assert (a['bbox'][:, [0, 2]] <= 1241).all() and (a['bbox'] >= 0).all()
    # a frame without boxes keeps the template, whose name is np.zeros(0) as in the reference
    assert e['name'].dtype == np.float64 and e['name'].shape == (0,) and e['bbox'].shape == (0, 4) and e['boxes_lidar'].shape == (0, 7)
    lines = open(os.path.join(str(tmp_path), '%s.txt' % ds.sample_id_list[0])).read().splitlines()
    assert len(lines) == 5 and open(os.path.join(str(tmp_path), '%s.txt' % ds.sample_id_list[1])).read() == ''
    want = 'Car -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f' % (
        a['alpha'][0], *a['bbox'][0], a['dimensions'][0][1], a['dimensions'][0][2], a['dimensions'][0][0], *a['location'][0],
        a['rotation_y'][0], a['score'][0])
    assert lines[0] == want and len(lines[0].split()) == 16


def test_ground_truth_fed_back_scores_100():
    """A class / difficulty reaches 100.0 only from 40 valid boxes on: get_thresholds samples 41 recall points and leaves the rest
    of the table zero. 256 frames give every class / difficulty at least that many, which is asserted."""
    ds = SyntheticDataset(num_frames=256, n_points=500)
    gt = [info['annos'] for info in ds.kitti_infos]
    assert 'annos' not in SyntheticDataset(num_frames=1).kitti_infos[0].keys()          # made on first use only
    levels = np.concatenate([g['occluded'] for g in gt])
    assert set(levels.tolist()) == {0, 1, 2, 3}
    dt = [dict(g, score=np.ones(len(g['name']), dtype=np.float32)) for g in gt]
    detail = {}
    text, ap = ds.evaluation(dt, ds.class_names, route='host', detail=detail)
    assert detail['num_valid_gt'].min() >= 40 and len(ap) == 36
    assert all(v == 100.0 for v in ap.values()), ap
    with pytest.raises(NotImplementedError):
        SyntheticDataset(num_frames=1, kind='waymo').evaluation([], ['Vehicle'])


def test_batches_unchanged():
    ds = SyntheticDataset(num_frames=2, n_points=500)
    ds.kitti_infos[0]['annos']
    item = ds[0]
    assert set(item) == {'points', 'gt_boxes', 'frame_id', 'use_lead_xyz'}
    batch = ds.collate_batch([item, ds[1]])
    assert set(batch) == {'points', 'point_frame_offsets', 'gt_boxes', 'frame_id', 'use_lead_xyz', 'batch_size'}
    assert ds.kitti_infos[1] == {'point_cloud': {'lidar_idx': ds.sample_id_list[1]}, 'frame_id': ds.sample_id_list[1]}
    assert np.array_equal(ds.kitti_infos[0]['annos']['gt_boxes_lidar'],
                          syn.kitti_frame(0, 500)[1][ds.kitti_infos[0]['annos']['index'], :7].astype(np.float64))
    assert ds.image_shape.tolist() == [375, 1242] and ds.calib.P2.shape == (3, 4)
