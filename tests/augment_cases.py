"""Shared by tests/test_augmentor_cpu.py and tests/test_augment_gpu.py: the queues behind tests/golden/ref_augmentor.npz (the same
configs as CASES in tests/golden/make_goldens_augment.py, checked against the arrays stored in the golden), its runs, the
host route, and the derived bound on the rotated coordinates."""
import os

import numpy as np

from pcdet.config import EasyDict

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'ref_augmentor.npz')
QUARTER_PI = 0.78539816
CASES = {
    'flip': [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x', 'y']}],
    'rot': [{'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-QUARTER_PI, QUARTER_PI]}],
    'scale': [{'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}],
    'trans': [{'NAME': 'random_world_translation', 'WORLD_TRANSLATION_RANGE': [-1.5, 1.5], 'ALONG_AXIS_LIST': ['x', 'y', 'z']}],
    'kitti': [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
              {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-QUARTER_PI, QUARTER_PI]},
              {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}],
}
U = 2.0 ** -24          # unit roundoff of f32
_golden = {}


def queue(case):
    return [EasyDict(c) for c in CASES[case]]


def golden():
    if not _golden:
        g = np.load(GOLDEN)
        _golden.update({k: g[k] for k in g.files})
        step_code = {'random_world_flip': 0, 'random_world_rotation': 2, 'random_world_scaling': 3, 'random_world_translation': 4}
        for case, cfgs in CASES.items():            # the configs above are the ones the golden was generated with
            rows = _golden['case_' + case]
            assert len(rows) == len(cfgs)
            for row, c in zip(rows, cfgs):
                rg = c.get('WORLD_ROT_ANGLE') or c.get('WORLD_SCALE_RANGE') or c.get('WORLD_TRANSLATION_RANGE') or [0, 0]
                assert list(row) == [step_code[c['NAME']], rg[0], rg[1], sum(1 << 'xyz'.index(a) for a in c.get('ALONG_AXIS_LIST', []))]
    return _golden


def runs():
    """-> [(name, case, seed, C, W, n)]"""
    out = []
    for name in golden()['runs']:
        case, s, c, w, n = str(name).split('_')
        out.append((str(name), case, int(s[1:]), int(c[1:]), int(w[1:]), int(n[1:])))
    return out


RUN_NAMES = ['flip_s1_c4_w7_n500', 'flip_s4_c5_w9_n500', 'flip_s6_c4_w9_n500', 'rot_s11_c4_w9_n500', 'rot_s12_c5_w7_n500',
             'scale_s21_c5_w9_n500', 'trans_s31_c4_w9_n500', 'trans_s32_c5_w7_n500', 'kitti_s41_c4_w7_n2000',
             'kitti_s44_c5_w9_n2000', 'kitti_s45_c4_w9_n500']


def run_inputs(name):
    """-> case, seed, points (n, C), boxes (G, W - class column: 7 or 9 coordinates)"""
    g = golden()
    case, s, c, w, n = name.split('_')
    C, W, n = int(c[1:]), int(w[1:]), int(n[1:])
    pts = np.concatenate([g['points4'], g['extra5']], 1)[:n, :C]
    return case, int(s[1:]), np.ascontiguousarray(pts), np.ascontiguousarray(g['boxes9'][:, :W])


def rotation_bound(name, xy_in):
    """The derived bound of the issue on a rotated coordinate against the reference (whose rotation is a torch matmul with
    c = cos(f32(a)) that may fuse or reorder): 4 u (|x| + |y|) for the rotation alone on the coordinates entering it; composed
    with the scaling, times the scale and plus one rounding of the result. xy_in (n, 2): the coordinates that enter the rotation
    (|.| is flip invariant). -> (n) bound per point, valid for both x and y"""
    ops = golden()[name + '/ops']
    k = [v for code, _, v in ops if code == 3]
    b = 4 * U * (np.abs(xy_in[:, 0].astype(np.float64)) + np.abs(xy_in[:, 1].astype(np.float64)))
    if k:
        r = np.abs(xy_in.astype(np.float64)).sum(1) * k[0]          # |result| <= (|x| + |y|) k
        b = b * k[0] + U * r
    return b


def host_route(case, seed, frames, boxes_with_class, pcr, mask=True, training=True):
    """host DataAugmentor, then the host DataProcessor range masks, frame after frame under one np.random.seed
    -> [(points, boxes_with_class)]"""
    from pcdet.datasets.augmentor import DataAugmentor
    from pcdet.datasets.processor.data_processor import DataProcessor
    aug = DataAugmentor(None, queue(case), ['Car', 'Pedestrian', 'Cyclist'])
    dp = DataProcessor([EasyDict({'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True})] if mask else [],
                       pcr, training=training, num_point_features=frames[0].shape[1])
    np.random.seed(seed)
    out = []
    for p, b in zip(frames, boxes_with_class):
        d = aug.forward({'points': p.copy(), 'gt_boxes': b[:, :-1].copy()})
        d['gt_boxes'] = np.concatenate([d['gt_boxes'], b[:, -1:]], 1)
        d = dp.forward(d)
        out.append((d['points'], d['gt_boxes']))
    return out
