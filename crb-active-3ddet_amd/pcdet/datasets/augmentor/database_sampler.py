"""gt_sampling (pcdet/datasets/augmentor/database_sampler.py:8-234 of the reference): paste objects of a ground-truth database into
a training frame, with the reference's active-learning rule that an object may only come from a frame labelled so far.

DataBaseSampler is the host mirror with the reference's surface and its np.random call order. It is also the arithmetic
definition that crbhip.gt_sampling (csrc/gt_sampling.hip) reproduces bit for bit. A call is three stages, which the device
route (DeviceDataAugmentor) takes apart:
  draw    the candidate walk of every SAMPLE_GROUPS class (sample_with_fixed_number): all of the random numbers, and nothing that
          depends on a collision result - the pointer moves whether a candidate is accepted or not
  select  per group: a candidate is valid iff its largest BEV IoU against all boxes existing so far (the frame's own and the valid
          candidates of earlier groups) is 0 and its largest against the other candidates of its group is 0
  paste   points of the valid objects, then the scene points outside every valid object's (enlarged) box

Deviations from the reference:
  * labelled set: data_dict['sample_id_list'] as in the reference; None (or absent) selects the non-active branch, where the
    reference reads the global cfg.ACTIVE_TRAIN. It is held as a set (the reference tests `in list`, O(n) per database entry).
  * a class without any labelled object: the reference recurses without end; here the class is skipped for the call, consumes no
    random numbers, and the fact is logged once per class.
  * bev_iou= replaces the BEV IoU function; the default is pcdet.ops.iou3d_nms.iou3d_nms_utils.boxes_bev_iou_cpu, which the HIP
    kernel answers (so the default needs a GPU, loader workers included; CPU-only callers pass another function).
  * point removal is numpy f32 with the CPU twin's rule (roiaware_pool3d.cpp:121-140, 1e-2 margin on x / y, none on z), see
    points_in_removal_boxes; the package's points_in_boxes_cpu follows the .cu kernel's rule and is not used.
  * every array is f32 and every operation is rounded once in f32: database boxes stored as f64 are cast first, and the road-plane
    shift is cast to f32 before it is subtracted from boxes and points (the reference subtracts whatever dtype the calib returns).
  * database infos may carry their points in memory ('points') instead of a file path."""
import pickle
from pathlib import Path

import numpy as np

MARGIN_F = np.float32(1e-2)
HALF_PI = np.pi / 2


def removal_boxes(boxes, extra_width=(0, 0, 0)):
    """(S, 7+) f32 boxes -> (S, 8) f32 rows [cx, cy, cz, dx + ex, dy + ey, dz + ez, cosa, sina] with cosa = f32(cos(-(f64)rz)),
    sina = f32(sin(-(f64)rz)): enlarge_box3d followed by the constants of lidar_to_local_coords_cpu"""
    boxes = np.asarray(boxes, dtype=np.float32)
    out = np.empty((len(boxes), 8), dtype=np.float32)
    out[:, 0:3] = boxes[:, 0:3]
    out[:, 3:6] = boxes[:, 3:6] + np.asarray(extra_width, dtype=np.float32)[None, :]
    rz = boxes[:, 6].astype(np.float64)
    out[:, 6] = np.cos(-rz).astype(np.float32)
    out[:, 7] = np.sin(-rz).astype(np.float32)
    return out


def points_in_removal_boxes(xyz, rem):
    """xyz (n, 3) f32, rem (S, 8) from removal_boxes -> (S, n) bool, check_pt_in_box3d_cpu of the reference: inside iff
    !(|z - cz| > dz / 2) and (f64)|lx| < (f64)dx / 2 + (f64)f32(1e-2) and the same for ly / dy, with
    lx = sx * cosa + sy * (-sina), ly = sx * sina + sy * cosa in f32, every product and sum rounded once"""
    xyz = np.asarray(xyz, dtype=np.float32)
    rem = np.asarray(rem, dtype=np.float32)
    x, y, z = xyz[None, :, 0], xyz[None, :, 1], xyz[None, :, 2]
    cosa, sina = rem[:, 6:7], rem[:, 7:8]
    with np.errstate(invalid='ignore'):
        z_in = ~(np.abs(z - rem[:, 2:3]) > rem[:, 5:6] / np.float32(2))
        sx, sy = x - rem[:, 0:1], y - rem[:, 1:2]
        lx = sx * cosa + sy * (-sina)
        ly = sx * sina + sy * cosa
        half_x = rem[:, 3:4].astype(np.float64) / 2.0 + np.float64(MARGIN_F)
        half_y = rem[:, 4:5].astype(np.float64) / 2.0 + np.float64(MARGIN_F)
        return z_in & (np.abs(lx).astype(np.float64) < half_x) & (np.abs(ly).astype(np.float64) < half_y)


def fakelidar_to_lidar(boxes):
    """box_utils.boxes3d_kitti_fakelidar_to_lidar in f32: [x, y, z bottom, w, l, h, r] -> [x, y, z + h / 2, l, w, h, -(r + pi / 2)]"""
    b = np.array(boxes, dtype=np.float32)
    out = b.copy()
    out[:, 2] = b[:, 2] + b[:, 5] / np.float32(2)
    out[:, 3], out[:, 4] = b[:, 4], b[:, 3]
    out[:, 6] = -(b[:, 6] + np.float32(HALF_PI))
    return out


def info_sample_id(info):
    """the frame an object was cut from, in the form the labelled set holds: KITTI image_idx, Waymo
    sequence_name + '_' + sample_idx padded to three digits (database_sampler.py:98-109)"""
    if 'sequence_name' in info:
        return '%s_%03d' % (info['sequence_name'], int(info['sample_idx']))
    return info['image_idx']


def _default_bev_iou(boxes_a, boxes_b):
    from ...ops.iou3d_nms import iou3d_nms_utils
    return iou3d_nms_utils.boxes_bev_iou_cpu(boxes_a, boxes_b)


class DataBaseSampler(object):
    def __init__(self, root_path, sampler_cfg, class_names, logger=None, bev_iou=None, db_infos=None):
        """db_infos: {class name: [info]} given directly (infos of SyntheticDataset.create_groundtruth_database(None)), in
        addition to the pickles sampler_cfg.DB_INFO_PATH names under root_path"""
        self.root_path = Path(root_path) if root_path is not None else None
        self.class_names = class_names
        self.sampler_cfg = sampler_cfg
        self.logger = logger
        self.bev_iou = bev_iou
        self.db_infos = {name: [] for name in class_names}
        self.sample_id_list = None
        for db_info_path in sampler_cfg.get('DB_INFO_PATH', None) or []:
            with open(str(self.root_path.resolve() / db_info_path), 'rb') as f:
                infos = pickle.load(f)
            for name in class_names:
                self.db_infos[name].extend(infos.get(name, []))
        for name in class_names:
            self.db_infos[name].extend((db_infos or {}).get(name, []))
        for func_name, val in (sampler_cfg.get('PREPARE', None) or {}).items():
            self.db_infos = getattr(self, func_name)(self.db_infos, val)

        self.limit_whole_scene = sampler_cfg.get('LIMIT_WHOLE_SCENE', False)
        self.sample_groups = {}
        self.sample_class_num = {}
        for x in sampler_cfg.SAMPLE_GROUPS:
            class_name, sample_num = x.split(':')
            if class_name not in class_names:
                continue
            self.sample_class_num[class_name] = sample_num
            self.sample_groups[class_name] = {'sample_num': sample_num, 'pointer': len(self.db_infos[class_name]),
                                              'indices': np.arange(len(self.db_infos[class_name]))}
        self._info_ids = {name: [info_sample_id(i) for i in self.db_infos[name]] for name in self.sample_groups}
        self._labelled = (None, {})          # (the labelled set, {class: bool per database entry})
        self._warned = set()
        self.last_groups, self.last_valid = [], np.zeros((0,), dtype=bool)

    def __getstate__(self):
        d = dict(self.__dict__)
        del d['logger']
        d['_labelled'] = (None, {})
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.logger = None

    # ---- PREPARE ---------------------------------------------------------------------------------------------------------------
    def filter_by_difficulty(self, db_infos, removed_difficulty):
        out = {}
        for key, dinfos in db_infos.items():
            out[key] = [info for info in dinfos if info['difficulty'] not in removed_difficulty]
            if self.logger is not None:
                self.logger.info('Database filter by difficulty %s: %d => %d' % (key, len(dinfos), len(out[key])))
        return out

    def filter_by_min_points(self, db_infos, min_gt_points_list):
        for name_num in min_gt_points_list:
            name, min_num = name_num.split(':')
            min_num = int(min_num)
            if min_num > 0 and name in db_infos:
                kept = [info for info in db_infos[name] if info['num_points_in_gt'] >= min_num]
                if self.logger is not None:
                    self.logger.info('Database filter by min points %s: %d => %d' % (name, len(db_infos[name]), len(kept)))
                db_infos[name] = kept
        return db_infos

    # ---- draw ------------------------------------------------------------------------------------------------------------------
    def _labelled_mask(self, class_name):
        """bool per database entry of the class: cut from a labelled frame; None in the non-active branch"""
        ids = self.sample_id_list
        if ids is None:
            return None
        key = ids if isinstance(ids, (set, frozenset)) else frozenset(ids)
        if self._labelled[0] is None or self._labelled[0] != key:
            self._labelled = (key, {})
        masks = self._labelled[1]
        if class_name not in masks:
            masks[class_name] = np.fromiter((i in key for i in self._info_ids[class_name]), dtype=bool,
                                            count=len(self._info_ids[class_name]))
        return masks[class_name]

    def sample_with_fixed_number(self, class_name, sample_group, as_indices=False):
        """-> the sampled infos (database indices with as_indices). Advances the group's pointer and re-permutes at the end of
        the permutation with the reference's np.random.permutation calls at the reference's moments."""
        n = len(self.db_infos[class_name])
        sample_num, pointer, indices = int(sample_group['sample_num']), sample_group['pointer'], sample_group['indices']
        labelled = self._labelled_mask(class_name)
        while True:
            if pointer >= n:
                indices = np.random.permutation(n)
                pointer = 0
            if labelled is not None:
                # the reference walks indices[pointer:] entry by entry, takes the labelled ones, stops at the sample_num-th, and
                # moves the pointer behind the last entry it looked at
                hits = np.nonzero(labelled[indices[pointer:]])[0]
                if len(hits) >= sample_num:
                    hits = hits[:sample_num]
                    walked = int(hits[-1]) + 1
                else:
                    walked = n - pointer
                picked = indices[pointer + hits]
                pointer += walked
            else:
                picked = indices[pointer:pointer + sample_num]
                pointer += sample_num
            if len(picked):          # (an empty walk: the pointer was close to the end and no labelled entry was left; again)
                break
        sample_group['pointer'] = pointer
        sample_group['indices'] = indices
        picked = [int(i) for i in picked]
        return picked if as_indices else [self.db_infos[class_name][i] for i in picked]

    def draw(self, gt_names, sample_id_list=None):
        """the candidate walk of one frame -> [(class name, [database indices])], one entry per sampled group, in SAMPLE_GROUPS
        order. Consumes np.random exactly like the reference's __call__."""
        self.sample_id_list = sample_id_list
        gt_names = np.asarray(gt_names).astype(str)
        groups = []
        for class_name, sample_group in self.sample_groups.items():
            if self.limit_whole_scene:
                num_gt = int(np.sum(class_name == gt_names))
                sample_group['sample_num'] = str(int(self.sample_class_num[class_name]) - num_gt)
            if int(sample_group['sample_num']) <= 0:
                continue
            labelled = self._labelled_mask(class_name)
            if len(self.db_infos[class_name]) == 0 or (labelled is not None and not labelled.any()):
                if class_name not in self._warned:
                    self._warned.add(class_name)
                    if self.logger is not None:
                        self.logger.info('gt_sampling: no %s object comes from a labelled frame, class skipped' % class_name)
                continue
            groups.append((class_name, self.sample_with_fixed_number(class_name, sample_group, as_indices=True)))
        return groups

    # ---- candidate boxes -------------------------------------------------------------------------------------------------------
    def candidate_boxes(self, class_name, picked):
        """(S, 7) f32 boxes of the picked database entries as they enter the collision test"""
        boxes = np.stack([np.asarray(self.db_infos[class_name][i]['box3d_lidar'], dtype=np.float32)[:7] for i in picked], axis=0)
        if self.sampler_cfg.get('DATABASE_WITH_FAKELIDAR', False):
            boxes = fakelidar_to_lidar(boxes)
        return boxes

    @staticmethod
    def put_boxes_on_road_planes(gt_boxes, road_planes, calib):
        """moves the boxes onto the plane a x + b y + c z + d = 0 of the rect frame -> (gt_boxes (modified in place), mv_height).
        calib: any object with lidar_to_rect / rect_to_lidar on (N, 3) arrays. The shift is cast to f32 and subtracted in f32."""
        a, b, c, d = road_planes
        center_cam = calib.lidar_to_rect(gt_boxes[:, 0:3])
        center_cam[:, 1] = (-d - a * center_cam[:, 0] - c * center_cam[:, 2]) / b
        cur_lidar_height = calib.rect_to_lidar(center_cam)[:, 2]
        mv_height = np.asarray(gt_boxes[:, 2] - gt_boxes[:, 5] / 2 - cur_lidar_height, dtype=np.float32)
        gt_boxes[:, 2] -= mv_height
        return gt_boxes, mv_height

    def object_points(self, info):
        """(n, NUM_POINT_FEATURES) f32 copy of the object's points, xyz relative to the box centre"""
        if info.get('points', None) is not None:
            pts = np.array(info['points'], dtype=np.float32)
        else:
            pts = np.fromfile(str(self.root_path / info['path']), dtype=np.float32)
        return pts.reshape([-1, self.sampler_cfg.NUM_POINT_FEATURES])

    # ---- select ----------------------------------------------------------------------------------------------------------------
    def select(self, gt_boxes, groups):
        """-> (candidate boxes (S, 7) of all groups in order, valid (S) bool)"""
        iou_fn = self.bev_iou or _default_bev_iou
        existed = np.asarray(gt_boxes, dtype=np.float32)[:, 0:7]
        all_boxes, all_valid = [], []
        for class_name, picked in groups:
            sampled = self.candidate_boxes(class_name, picked)
            iou2 = np.array(iou_fn(sampled, sampled))
            iou2[range(len(sampled)), range(len(sampled))] = 0
            iou1 = np.asarray(iou_fn(sampled, existed)) if existed.shape[0] > 0 else iou2
            valid = (iou1.max(axis=1) + iou2.max(axis=1)) == 0
            existed = np.concatenate((existed, sampled[valid]), axis=0)
            all_boxes.append(sampled)
            all_valid.append(valid)
        if not all_boxes:
            return np.zeros((0, 7), dtype=np.float32), np.zeros((0,), dtype=bool)
        return np.concatenate(all_boxes, axis=0), np.concatenate(all_valid, axis=0)

    # ---- paste -----------------------------------------------------------------------------------------------------------------
    def add_sampled_boxes_to_scene(self, data_dict, sampled_gt_boxes, total_valid_sampled_dict):
        gt_boxes_mask = data_dict['gt_boxes_mask']
        gt_boxes = data_dict['gt_boxes'][gt_boxes_mask]
        gt_names = data_dict['gt_names'][gt_boxes_mask]
        points = data_dict['points']
        mv_height = None
        if self.sampler_cfg.get('USE_ROAD_PLANE', False):
            sampled_gt_boxes, mv_height = self.put_boxes_on_road_planes(sampled_gt_boxes, data_dict['road_plane'],
                                                                        data_dict['calib'])
            data_dict.pop('calib')
            data_dict.pop('road_plane')
        obj_points_list = []
        for idx, info in enumerate(total_valid_sampled_dict):
            obj_points = self.object_points(info)
            obj_points[:, :3] += np.asarray(info['box3d_lidar'], dtype=np.float32)[:3]
            if mv_height is not None and mv_height[idx] != 0:
                obj_points[:, 2] -= mv_height[idx]
            obj_points_list.append(obj_points)
        obj_points = np.concatenate(obj_points_list, axis=0)
        sampled_gt_names = np.array([x['name'] for x in total_valid_sampled_dict])
        rem = removal_boxes(sampled_gt_boxes[:, 0:7], self.sampler_cfg.REMOVE_EXTRA_WIDTH)
        points = points[~points_in_removal_boxes(points[:, 0:3], rem).any(axis=0)]
        data_dict['points'] = np.concatenate([obj_points, points.astype(np.float32, copy=False)], axis=0)
        data_dict['gt_names'] = np.concatenate([gt_names, sampled_gt_names], axis=0)
        data_dict['gt_boxes'] = np.concatenate([gt_boxes, sampled_gt_boxes], axis=0)
        return data_dict

    def __call__(self, data_dict):
        """data_dict: points (N, NUM_POINT_FEATURES), gt_boxes (G, 7 + C), gt_names (G), optional gt_boxes_mask, sample_id_list
        (the labelled frames; None / absent = non-active branch), road_plane + calib with USE_ROAD_PLANE.
        On return gt_boxes_mask is all ones; the caller's mask is applied only when something was pasted (as in the reference)."""
        gt_boxes = np.asarray(data_dict['gt_boxes'], dtype=np.float32)
        data_dict['gt_boxes'] = gt_boxes
        if 'gt_boxes_mask' not in data_dict:
            data_dict['gt_boxes_mask'] = np.ones(gt_boxes.shape[0], dtype=np.bool_)
        groups = self.draw(data_dict['gt_names'], data_dict.get('sample_id_list', None))
        cand_boxes, valid = self.select(gt_boxes, groups)
        infos = [self.db_infos[name][i] for name, picked in groups for i in picked]
        valid_infos = [info for info, ok in zip(infos, valid) if ok]
        self.last_groups, self.last_valid = groups, valid          # (for tools and tests: what the call drew and accepted)
        if len(valid_infos) > 0:
            sampled_gt_boxes = cand_boxes[valid]
            if gt_boxes.shape[1] > 7:              # (the reference's concatenation fails here: the database carries no velocities)
                raise ValueError('gt_sampling: boxes of width %d, the database holds 7 coordinates' % gt_boxes.shape[1])
            data_dict = self.add_sampled_boxes_to_scene(data_dict, sampled_gt_boxes, valid_infos)
        data_dict['gt_boxes_mask'] = np.ones(data_dict['gt_boxes'].shape[0], dtype=np.bool_)
        return data_dict
