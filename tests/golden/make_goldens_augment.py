"""Generate ref_augmentor.npz from the reference's own DataAugmentor (companion of make_goldens.py, whose import recipe it reuses).

Runs ONLY where the reference tree is mounted; the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_augment.py

Stored (arrays and short names only):
  points4 (N,4) / extra5 (N,1): the input frame with C = 4, and the fifth feature column of its C = 5 twin
  boxes9 (G,9): input boxes [x,y,z,dx,dy,dz,heading,vx,vy]; the width-7 set is its first seven columns
  pcr (6): the range the masks use
  runs: names of the runs, '<case>_s<seed>_c<C>_w<W>_n<points used>'; per run, under '<run>/':
    seed, ops (K,3) f64 rows [code, axis, value] - the draws recovered by replaying the seed with the reference's np.random calls
      (code 0 flip x, 1 flip y, 2 rotation [value = angle], 3 scaling, 4 translation [axis 0/1/2])
    points_xyz (n,3): the reference's augmented xyz (feature columns pass through and are not stored)
    boxes (G,W): the reference's augmented boxes, heading limited
    keep_points (n) / keep_boxes (G) bool: the reference's mask_points_by_range / mask_boxes_outside_range_numpy on them
  case_<case>: the queue of each case as rows [step code, lo, hi, axes bitmask] (see CASES for the configs themselves)

Margin rule: inputs that land on a decision boundary after the REFERENCE's transform in any run are dropped from the inputs, so no
stored decision is a near-tie: points whose transformed x or y is within 1e-3 of a range bound, boxes with a corner within 1e-3 of
a bound, boxes whose heading / (2 pi) + 0.5 is within 1e-4 of an integer (before limit_period)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import import_reference, save, EasyDict  # noqa: E402

PCR = np.array([0, -40, -3, 70.4, 40, 1], dtype=np.float32)
N_POINTS, N_BOXES, N_SMALL = 2000, 28, 500
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
# (case, seed, C, W, points used)
RUNS = [('flip', 1, 4, 7, N_SMALL), ('flip', 4, 5, 9, N_SMALL), ('flip', 6, 4, 9, N_SMALL),
        ('rot', 11, 4, 9, N_SMALL), ('rot', 12, 5, 7, N_SMALL),
        ('scale', 21, 5, 9, N_SMALL), ('trans', 31, 4, 9, N_SMALL), ('trans', 32, 5, 7, N_SMALL),
        ('kitti', 41, 4, 7, N_POINTS), ('kitti', 44, 5, 9, N_POINTS), ('kitti', 45, 4, 9, N_SMALL)]


def run_name(case, seed, C, W, n):
    return '%s_s%d_c%d_w%d_n%d' % (case, seed, C, W, n)


def replay(cfgs, seed):
    """the reference's np.random calls for this queue, in its order -> rows [code, axis, value]"""
    np.random.seed(seed)
    ops = []
    for c in cfgs:
        if c['NAME'] == 'random_world_flip':
            for a in c['ALONG_AXIS_LIST']:
                if np.random.choice([False, True], replace=False, p=[0.5, 0.5]):
                    ops.append([0 if a == 'x' else 1, 0, 1])
        elif c['NAME'] == 'random_world_rotation':
            ops.append([2, 0, np.random.uniform(c['WORLD_ROT_ANGLE'][0], c['WORLD_ROT_ANGLE'][1])])
        elif c['NAME'] == 'random_world_scaling':
            ops.append([3, 0, np.random.uniform(c['WORLD_SCALE_RANGE'][0], c['WORLD_SCALE_RANGE'][1])])
        else:
            for a in c['ALONG_AXIS_LIST']:
                ops.append([4, 'xyz'.index(a), np.random.uniform(*c['WORLD_TRANSLATION_RANGE'])])
    return np.array(ops, dtype=np.float64).reshape(-1, 3)


def heading_before_limit(h, ops):
    h = h.astype(np.float64)
    for code, _, v in ops:
        if code == 0:
            h = -h
        elif code == 1:
            h = -(h + np.pi)
        elif code == 2:
            h = h + v
    return h


def near(v, bounds, eps):
    return np.any([np.abs(v - b) < eps for b in bounds], axis=0)


def main():
    import_reference()
    from pcdet.datasets.augmentor.data_augmentor import DataAugmentor
    from pcdet.utils import box_utils, common_utils

    rng = np.random.default_rng(77)
    pts5 = rng.uniform([-12, -52, -4, 0, 0], [82, 52, 2, 1, 1], size=(N_POINTS + 400, 5)).astype(np.float32)
    boxes9 = np.concatenate([rng.uniform([-6, -46, -2.5], [77, 46, 0.5], size=(N_BOXES + 12, 3)),
                             rng.uniform(0.6, 4.5, size=(N_BOXES + 12, 3)), rng.uniform(-3.1, 3.1, size=(N_BOXES + 12, 1)),
                             rng.uniform(-5, 5, size=(N_BOXES + 12, 2))], 1).astype(np.float32)

    def reference_run(case, seed, C, W, n, pts5, boxes9):
        aug = DataAugmentor(None, [EasyDict(c) for c in CASES[case]], ['Car', 'Pedestrian', 'Cyclist'])
        np.random.seed(seed)
        d = aug.forward({'points': pts5[:n, :C].copy(), 'gt_boxes': boxes9[:, :W].copy()})
        return d['points'], d['gt_boxes']

    # pass 1: find what sits on a decision boundary in any run; pass 2: run again without it
    bad_p, bad_b = np.zeros(len(pts5), bool), np.zeros(len(boxes9), bool)
    for case, seed, C, W, n in RUNS:
        p, b = reference_run(case, seed, C, W, len(pts5), pts5, boxes9)
        bad_p |= near(p[:, 0], PCR[[0, 3]], 1e-3) | near(p[:, 1], PCR[[1, 4]], 1e-3)
        corners = box_utils.boxes_to_corners_3d(b[:, :7])
        for ax in range(3):
            bad_b |= near(corners[:, :, ax], PCR[[ax, ax + 3]], 1e-3).any(axis=1)
        t = heading_before_limit(boxes9[:, 6], replay(CASES[case], seed)) / (2 * np.pi) + 0.5
        bad_b |= np.abs(t - np.round(t)) < 1e-4
    print('margin rule: dropped %d of %d points, %d of %d boxes' % (bad_p.sum(), len(pts5), bad_b.sum(), len(boxes9)))
    pts5, boxes9 = pts5[~bad_p][:N_POINTS], boxes9[~bad_b][:N_BOXES]
    assert len(pts5) == N_POINTS and len(boxes9) == N_BOXES

    out = {'points4': pts5[:, :4].copy(), 'extra5': pts5[:, 4:5].copy(), 'boxes9': boxes9, 'pcr': PCR,
           'runs': np.array([run_name(*r) for r in RUNS])}
    step_code = {'random_world_flip': 0, 'random_world_rotation': 2, 'random_world_scaling': 3, 'random_world_translation': 4}
    for case, cfgs in CASES.items():
        rows = []
        for c in cfgs:
            rg = c.get('WORLD_ROT_ANGLE') or c.get('WORLD_SCALE_RANGE') or c.get('WORLD_TRANSLATION_RANGE') or [0, 0]
            rows.append([step_code[c['NAME']], rg[0], rg[1], sum(1 << 'xyz'.index(a) for a in c.get('ALONG_AXIS_LIST', []))])
        out['case_' + case] = np.array(rows, dtype=np.float64)
    sides_p, sides_c = np.zeros((4, 2), bool), np.zeros((6, 2), bool)
    kept_any = removed_any = False
    for case, seed, C, W, n in RUNS:
        p, b = reference_run(case, seed, C, W, n, pts5, boxes9)
        np.testing.assert_array_equal(p[:, 3:], pts5[:n, 3:C])                    # feature columns pass through
        keep_p = common_utils.mask_points_by_range(p, PCR)
        keep_b = box_utils.mask_boxes_outside_range_numpy(b, PCR, min_num_corners=1)
        corners = box_utils.boxes_to_corners_3d(b[:, :7])
        assert not (near(p[:, 0], PCR[[0, 3]], 1e-3) | near(p[:, 1], PCR[[1, 4]], 1e-3)).any()
        for ax in range(3):
            assert not near(corners[:, :, ax], PCR[[ax, ax + 3]], 1e-3).any()
            for hi in range(2):
                v = corners[:, :, ax] - PCR[ax + 3 * hi]
                sides_c[ax + 3 * hi] |= [(v < 0).any(), (v > 0).any()]
        for k, (col, bound) in enumerate([(0, 0), (0, 3), (1, 1), (1, 4)]):
            sides_p[k] |= [(p[:, col] < PCR[bound]).any(), (p[:, col] > PCR[bound]).any()]
        kept_any |= bool(keep_b.any())
        removed_any |= bool((~keep_b).any())
        assert keep_p.any() and (~keep_p).any()
        name = run_name(case, seed, C, W, n)
        out[name] = {'seed': np.int64(seed), 'ops': replay(CASES[case], seed), 'points_xyz': p[:, :3].copy(), 'boxes': b,
                     'keep_points': keep_p, 'keep_boxes': keep_b}
        print(name, 'ops', out[name]['ops'].tolist(), 'points kept %d / %d, boxes kept %d / %d' % (keep_p.sum(), n, keep_b.sum(), len(b)))
    # points and box corners on both sides of every bound, boxes both kept and removed
    assert sides_p.all() and sides_c.all() and kept_any and removed_any, (sides_p, sides_c)
    save('ref_augmentor.npz', out)


if __name__ == '__main__':
    main()
