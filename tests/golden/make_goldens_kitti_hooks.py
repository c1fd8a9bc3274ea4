"""Generate ref_kitti_hooks.npz from the reference's own box_utils and calibration_kitti.Calibration (companion of make_goldens.py).

Runs ONLY where the reference tree is mounted; the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_kitti_hooks.py

Inputs: seeded lidar boxes (N, 7) over the synthetic KITTI range, some of them beside the camera's view so that their projection
leaves the image partly or wholly, and the synthetic frames' calibration matrices (read from the mirror's
pcdet/datasets/synthetic.py by path; the reference's Calibration accepts them as a dict).
Stored: boxes_lidar, P2, R0, Tr_velo2cam, image_shape; from an f64 run camera (N, 7) = boxes3d_lidar_to_kitti_camera, corners (N, 8, 3)
= boxes3d_to_corners3d_kitti_camera, imageboxes / imageboxes_clipped (N, 4) = boxes3d_kitti_camera_to_imageboxes without / with
image_shape, rect (N, 3) = lidar_to_rect of the centres, lidar_back = rect_to_lidar(rect), img / depth = rect_to_img(rect), rect_back
= img_to_rect(u, v, depth); e_<name>: max |f32 run - f64 run| of each, the unit of the test's bars."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402


def run(box_utils, Calibration, boxes, mats, image_shape, dtype):
    calib = Calibration({k: v.astype(dtype) for k, v in mats.items()})
    boxes = boxes.astype(dtype)
    cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes, calib)
    rect = calib.lidar_to_rect(boxes[:, 0:3])
    img, depth = calib.rect_to_img(rect)
    return {'camera': cam, 'corners': box_utils.boxes3d_to_corners3d_kitti_camera(cam),
            'imageboxes': box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib),
            'imageboxes_clipped': box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=image_shape),
            'rect': rect, 'lidar_back': calib.rect_to_lidar(rect), 'img': img, 'depth': depth,
            'rect_back': calib.img_to_rect(img[:, 0], img[:, 1], depth)}


def main():
    mg.import_reference()
    from pcdet.utils import box_utils
    from pcdet.utils.calibration_kitti import Calibration
    spec = importlib.util.spec_from_file_location(
        'crb_synthetic', os.path.join(os.path.dirname(os.path.dirname(HERE)), 'crb-active-3ddet_amd', 'pcdet', 'datasets', 'synthetic.py'))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    mats = {'P2': np.array(syn.KITTI_P2), 'R0': np.array(syn.KITTI_R0), 'Tr_velo2cam': np.array(syn.KITTI_TR_VELO2CAM)}
    image_shape = np.array(syn.KITTI_IMAGE_SHAPE)
    rng = np.random.default_rng(404)
    n = 48
    boxes = np.concatenate([rng.uniform([5, -30, -2.2], [65, 30, -0.5], (n, 3)), rng.uniform([0.5, 0.4, 1.2], [4.5, 2.0, 2.0], (n, 3)),
                            rng.uniform(-np.pi, np.pi, (n, 1))], 1)
    boxes[:8, 0], boxes[:8, 1] = rng.uniform(5, 9, 8), rng.uniform(3.5, 9, 8) * rng.choice([-1, 1], 8)      # beside the view
    r64 = run(box_utils, Calibration, boxes, mats, image_shape, np.float64)
    r32 = run(box_utils, Calibration, boxes, mats, image_shape, np.float32)
    out = dict(r64, boxes_lidar=boxes, image_shape=image_shape, **mats)
    for k in r64:
        out['e_' + k] = np.abs(r32[k].astype(np.float64) - r64[k]).max()
        print(k, r64[k].shape, 'f32 - f64', out['e_' + k])
    ib, ic = r64['imageboxes'], r64['imageboxes_clipped']
    partly = (np.abs(ib - ic).max(1) > 0) & (ic[:, 2] > ic[:, 0]) & (ic[:, 3] > ic[:, 1])
    print('boxes that leave the image partly: %d, wholly: %d' % (partly.sum(), ((ic[:, 2] <= ic[:, 0]) | (ic[:, 3] <= ic[:, 1])).sum()))
    assert partly.sum() >= 2 and (np.abs(ib - ic).max(1) == 0).sum() >= 10
    mg.save('ref_kitti_hooks.npz', out)


if __name__ == '__main__':
    main()
