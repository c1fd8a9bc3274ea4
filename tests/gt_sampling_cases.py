"""Shared by tests/golden/make_goldens_gt_sampling.py, tests/test_gt_sampling_cpu.py and tests/test_gt_sampling_gpu.py: the runs
behind tests/golden/ref_gt_sampling.npz (configs, labelled sets, calib and road plane), the golden's loader and the builders that
turn its arrays back into database infos and sampler configs."""
import os

import numpy as np

from pcdet.config import EasyDict

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'ref_gt_sampling.npz')
CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
N_DB_FRAMES, N_DB_POINTS = 10, 3000          # the database: objects of synthetic frames 0..9 at 3000 points
N_CALLS, N_FRAME_POINTS = 8, 2400            # the scenes: synthetic frames 0..7 at 2400 points (same boxes as the database frames)
MAX_OBJ_POINTS, MIN_OBJ_POINTS = 24, 2
PERM_HEAD = 8

# name: seed, active (labelled database frames, None = non-active branch), SAMPLE_GROUPS, LIMIT_WHOLE_SCENE, REMOVE_EXTRA_WIDTH,
# USE_ROAD_PLANE, single (class that keeps one labelled object only)
RUNS = {
    'plain': dict(seed=3, active=None, groups=['Car:20', 'Pedestrian:15', 'Cyclist:15'], limit=False, extra=[0.0, 0.0, 0.0],
                  road=False, single=None),
    'active3': dict(seed=4, active=[0, 3, 6], groups=['Car:3', 'Pedestrian:2', 'Cyclist:2'], limit=False, extra=[0.0, 0.0, 0.0],
                    road=False, single=None),
    'single': dict(seed=5, active=[0, 3, 6], groups=['Car:8', 'Pedestrian:6', 'Cyclist:6'], limit=False, extra=[0.2, 0.2, 0.2],
                   road=False, single='Pedestrian'),
    'limit': dict(seed=6, active=None, groups=['Car:10', 'Pedestrian:6', 'Cyclist:6'], limit=True, extra=[0.2, 0.2, 0.2],
                  road=False, single=None),
    'road': dict(seed=7, active=[1, 4, 7], groups=['Car:8', 'Pedestrian:6', 'Cyclist:6'], limit=False, extra=[0.2, 0.2, 0.2],
                 road=True, single=None),
    'lonely': dict(seed=8, active=[3], groups=['Car:8', 'Pedestrian:6', 'Cyclist:6'], limit=True, extra=[0.0, 0.0, 0.0],
                   road=False, single=None),
}
ROAD_PLANE = np.array([0.01, -1.0, 0.02, 1.65], dtype=np.float32)


class AffineCalib(object):
    """a fixed lidar <-> rect map in f32, written out element by element (rect x = -lidar y, rect y = -lidar z + 0.08,
    rect z = lidar x + 0.27) so that a row's result does not depend on how many rows are converted together"""
    TY, TZ = np.float32(0.08), np.float32(0.27)

    def lidar_to_rect(self, pts):
        pts = np.asarray(pts, dtype=np.float32)
        return np.stack([-pts[:, 1], -pts[:, 2] + self.TY, pts[:, 0] + self.TZ], axis=1)

    def rect_to_lidar(self, pts):
        pts = np.asarray(pts, dtype=np.float32)
        return np.stack([pts[:, 2] - self.TZ, -pts[:, 0], -(pts[:, 1] - self.TY)], axis=1)


def frame_id(f):
    return '%06d' % f


def sampler_cfg(run, db_info_path=None):
    r = RUNS[run]
    return EasyDict({'NAME': 'gt_sampling', 'USE_ROAD_PLANE': r['road'], 'DB_INFO_PATH': [db_info_path] if db_info_path else [],
                     'PREPARE': {'filter_by_min_points': ['%s:%d' % (c, MIN_OBJ_POINTS) for c in CLASS_NAMES],
                                 'filter_by_difficulty': [-1]},
                     'SAMPLE_GROUPS': list(r['groups']), 'NUM_POINT_FEATURES': 4, 'DATABASE_WITH_FAKELIDAR': False,
                     'REMOVE_EXTRA_WIDTH': list(r['extra']), 'LIMIT_WHOLE_SCENE': r['limit']})


def labelled_ids(run):
    a = RUNS[run]['active']
    return None if a is None else [frame_id(f) for f in a]


_golden = {}


def golden():
    if not _golden:
        g = np.load(GOLDEN)
        _golden.update({k: g[k] for k in g.files})
    return _golden


def db_infos(run, g=None, with_points=True):
    """the database of a run as {class: [info]} from the golden's object table, in the order the reference saw it"""
    g = g or golden()
    infos = {}
    for k, name in enumerate(CLASS_NAMES):
        infos[name] = []
        for o in g[run + '/db_' + name]:
            o = int(o)
            info = {'name': name, 'path': None, 'image_idx': frame_id(int(g['db_frame'][o])), 'gt_idx': int(g['db_gt_idx'][o]),
                    'box3d_lidar': g['db_boxes'][o].copy(), 'num_points_in_gt': int(g['db_offsets'][o + 1] - g['db_offsets'][o]),
                    'difficulty': 0, 'bbox': np.zeros((4,), dtype=np.float32), 'score': -1.0, 'obj_id': o}
            if with_points:
                info['points'] = g['db_points'][g['db_offsets'][o]:g['db_offsets'][o + 1]].copy()
            infos[name].append(info)
    return infos


def call_input(run, c, g=None):
    """-> data_dict of call c of a run (fresh copies)"""
    g = g or golden()
    boxes = g['frame_boxes'][c]
    d = {'points': g['frame_points_%d' % c].copy(), 'gt_boxes': boxes[:, :7].copy(),
         'gt_names': np.array(CLASS_NAMES)[boxes[:, 7].astype(np.int64) - 1], 'sample_id_list': labelled_ids(run)}
    if RUNS[run]['road']:
        d['road_plane'], d['calib'] = ROAD_PLANE.copy(), AffineCalib()
    return d


def expected_points(run, c, g=None):
    """the reference's output points of a call: its pasted points, then the scene points it kept (stored as a mask)"""
    g = g or golden()
    key = '%s/%d/' % (run, c)
    return np.concatenate([g[key + 'pasted'], g['frame_points_%d' % c][g[key + 'kept']]], axis=0)
