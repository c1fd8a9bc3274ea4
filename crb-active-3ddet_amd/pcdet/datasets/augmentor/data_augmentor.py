"""DATA_AUGMENTOR queue (pcdet/datasets/augmentor/data_augmentor.py:9-117,229-258 of the reference): gt_sampling and the four
world steps.

DataAugmentor is the host mirror for loader workers, with the reference's surface. DeviceDataAugmentor makes the same draws
for a whole batch and packs them into the candidate records of crb_gt_sample_select / crb_gt_sample_paste and the per-frame
parameter rows of crb_augment_mask_points / crb_augment_boxes.
The image, frustum, pyramid and local augmentors are not provided: naming one raises NotImplementedError."""
from functools import partial

import numpy as np

from . import augmentor_utils
from . import database_sampler

WORLD_STEPS = ('random_world_flip', 'random_world_rotation', 'random_world_scaling', 'random_world_translation')


def _config_list(augmentor_configs):
    """a plain list of step configs, or a config with AUG_CONFIG_LIST and DISABLE_AUG_LIST -> the enabled step configs"""
    if isinstance(augmentor_configs, list):
        return list(augmentor_configs)
    disabled = augmentor_configs.DISABLE_AUG_LIST
    return [c for c in augmentor_configs.AUG_CONFIG_LIST if c.NAME not in disabled]


def draw_step(config):
    """the random draws of one queue step, in the reference's order and with its calls -> list of operations
    ('flip_x',) | ('flip_y',) | ('rot', angle) | ('scale', factor) | ('t', axis, offset)"""
    name = config['NAME']
    ops = []
    if name == 'random_world_flip':
        for axis in config['ALONG_AXIS_LIST']:
            assert axis in ['x', 'y']
            if augmentor_utils.draw_flip():
                ops.append(('flip_' + axis,))
    elif name == 'random_world_rotation':
        rot_range = config['WORLD_ROT_ANGLE']
        if not isinstance(rot_range, list):
            rot_range = [-rot_range, rot_range]
        ops.append(('rot', augmentor_utils.draw_uniform(rot_range[0], rot_range[1])))
    elif name == 'random_world_scaling':
        scale_range = config['WORLD_SCALE_RANGE']
        if augmentor_utils.scaling_is_drawn(scale_range):
            ops.append(('scale', augmentor_utils.draw_uniform(scale_range[0], scale_range[1])))
    elif name == 'random_world_translation':
        offset_range = config['WORLD_TRANSLATION_RANGE']
        for axis in config['ALONG_AXIS_LIST']:
            assert axis in ['x', 'y', 'z']
            ops.append(('t', axis, augmentor_utils.draw_uniform(offset_range[0], offset_range[1])))
    else:
        raise NotImplementedError('DATA_AUGMENTOR step %s' % name)
    return ops


def apply_ops(gt_boxes, points, ops):
    for op in ops:
        if op[0] == 'flip_x':
            gt_boxes, points = augmentor_utils.flip_along_x(gt_boxes, points)
        elif op[0] == 'flip_y':
            gt_boxes, points = augmentor_utils.flip_along_y(gt_boxes, points)
        elif op[0] == 'rot':
            gt_boxes, points = augmentor_utils.rotate(gt_boxes, points, op[1])
        elif op[0] == 'scale':
            gt_boxes, points = augmentor_utils.scale(gt_boxes, points, op[1])
        else:
            gt_boxes, points = augmentor_utils.translate(gt_boxes, points, op[1], op[2])
    return gt_boxes, points


class DataAugmentor(object):
    def __init__(self, root_path, augmentor_configs, class_names, logger=None, bev_iou=None, db_infos=None):
        """bev_iou, db_infos: handed to the DataBaseSampler of a gt_sampling step (see database_sampler.DataBaseSampler)"""
        self.root_path = root_path
        self.class_names = class_names
        self.logger = logger
        self._sampler_args = {'bev_iou': bev_iou, 'db_infos': db_infos}
        self.db_sampler = None
        self.data_augmentor_queue = []
        for cur_cfg in _config_list(augmentor_configs):
            if cur_cfg.NAME not in WORLD_STEPS + ('gt_sampling',):
                raise NotImplementedError('DATA_AUGMENTOR step %s is not provided (gt_sampling and world flip, rotation, scaling '
                                          'and translation are)' % cur_cfg.NAME)
            self.data_augmentor_queue.append(getattr(self, cur_cfg.NAME)(config=cur_cfg))

    def gt_sampling(self, config=None):
        if not (config.get('DB_INFO_PATH', None) or self._sampler_args['db_infos']):
            raise NotImplementedError('DATA_AUGMENTOR step gt_sampling needs a ground-truth database: DB_INFO_PATH pickles under '
                                      'root_path (SyntheticDataset.create_groundtruth_database writes them) or db_infos=')
        self.db_sampler = database_sampler.DataBaseSampler(root_path=self.root_path, sampler_cfg=config,
                                                           class_names=self.class_names, logger=self.logger,
                                                           **self._sampler_args)
        return self.db_sampler

    def __getstate__(self):
        d = dict(self.__dict__)
        del d['logger']
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.logger = None

    def _step(self, data_dict, config):
        gt_boxes, points = apply_ops(data_dict['gt_boxes'], data_dict['points'], draw_step(config))
        data_dict['gt_boxes'] = gt_boxes
        data_dict['points'] = points
        return data_dict

    def random_world_flip(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_flip, config=config)
        return self._step(data_dict, config)

    def random_world_rotation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_rotation, config=config)
        return self._step(data_dict, config)

    def random_world_scaling(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_scaling, config=config)
        return self._step(data_dict, config)

    def random_world_translation(self, data_dict=None, config=None):
        if data_dict is None:
            return partial(self.random_world_translation, config=config)
        return self._step(data_dict, config)

    def forward(self, data_dict):
        """points (N, 3 + C), gt_boxes (G, 7 + C) [x, y, z, dx, dy, dz, heading, ...], optional gt_names / gt_boxes_mask; with a
        gt_sampling step gt_names is needed, sample_id_list (the labelled frames) selects the active branch"""
        for cur_augmentor in self.data_augmentor_queue:
            data_dict = cur_augmentor(data_dict=data_dict)
        data_dict['gt_boxes'][:, 6] = augmentor_utils.limit_heading(data_dict['gt_boxes'][:, 6])
        data_dict.pop('calib', None)
        data_dict.pop('road_plane', None)
        if 'gt_boxes_mask' in data_dict:
            gt_boxes_mask = data_dict.pop('gt_boxes_mask')
            data_dict['gt_boxes'] = data_dict['gt_boxes'][gt_boxes_mask]
            data_dict['gt_names'] = data_dict['gt_names'][gt_boxes_mask]
            if 'gt_boxes2d' in data_dict:
                data_dict['gt_boxes2d'] = data_dict['gt_boxes2d'][gt_boxes_mask]
        return data_dict


class DeviceDataAugmentor(object):
    """The same queue for a whole batch on the GPU: the draws stay on the host (np.random, frame after frame, the calls and the
    order of DataAugmentor, so one np.random.seed gives the same augmentation as the host mirror run on the frames in order), the
    arithmetic runs in crb_gt_sample_select / crb_gt_sample_paste and crb_augment_mask_points / crb_augment_boxes
    (DeviceDataProcessor.process_batch(..., augmentor=self)).

    The kernels apply a frame's steps in one fixed order - gt_sampling, flip x, flip y, rotation, scaling, translation - so the
    queue must name its steps in that order (the order of every configuration of the reference), each at most once; gt_sampling
    can only be the first step.

    gt_sampling: the candidate walk never depends on a collision result, so draw_batch draws everything up front and packs, per
    candidate, the record csrc/gt_sampling.hip documents (box, class, road-plane shift, removal box with the host's cos / sin,
    point offset). The object database lives on the device (crbhip.gt_database.DeviceGtDatabase, uploaded on first use).
    set_labelled(ids) gives the labelled frames of the active branch, None selects the non-active branch."""

    PARAM_WIDTH = 8          # [flip_x, flip_y, c, s, scale, tx, ty, tz]
    CAND_WIDTH = 20          # [box 7, class, shift, removal box 8, point offset 3]
    MAX_CANDIDATES = 256     # per frame (crb_gt_sample_select)

    def __init__(self, augmentor_configs, class_names=None, root_path=None, logger=None, bev_iou=None, db_infos=None):
        cfgs = _config_list(augmentor_configs)
        if any(c.NAME == 'gt_sampling' for c in cfgs[1:]):
            raise NotImplementedError('device augmentation takes gt_sampling as the first step of the queue only')
        self.host = DataAugmentor(root_path, cfgs, class_names, logger=logger, bev_iou=bev_iou, db_infos=db_infos)
        self.class_names = class_names
        self.sampler = self.host.db_sampler
        self.step_configs = cfgs[1:] if self.sampler is not None else cfgs
        self.labelled = None
        self._database = None
        rank = {'flip_x': 0, 'flip_y': 1, 'rot': 2, 'scale': 3, 't_x': 4, 't_y': 5, 't_z': 6}
        seq = []
        for cfg in self.step_configs:
            if cfg.NAME == 'random_world_flip':
                seq += ['flip_' + a for a in cfg['ALONG_AXIS_LIST']]
            elif cfg.NAME == 'random_world_translation':
                seq += ['t_' + a for a in cfg['ALONG_AXIS_LIST']]
            else:
                seq.append({'random_world_rotation': 'rot', 'random_world_scaling': 'scale'}[cfg.NAME])
        order = [rank[s] for s in seq]
        if order != sorted(set(order)):
            raise NotImplementedError('device augmentation applies flip x, flip y, rotation, scaling, translation in this fixed '
                                      'order, each at most once; the queue asks for %s' % seq)

    def set_labelled(self, ids):
        """the frames labelled so far (the reference's data_dict['sample_id_list']); None = non-active branch"""
        self.labelled = None if ids is None else frozenset(ids)

    @property
    def database(self):
        """the object database behind the sampler (host arrays; .device_tensors(device) uploads once)"""
        if self._database is None and self.sampler is not None:
            from crbhip.gt_database import DeviceGtDatabase
            self._database = DeviceGtDatabase.from_sampler(self.sampler)
        return self._database

    def draw_frame(self):
        """one frame's world draws -> list of operations (see draw_step)"""
        ops = []
        for cfg in self.step_configs:
            ops += draw_step(cfg)
        return ops

    @staticmethod
    def pack(ops):
        """operations of one frame -> (parameter row (8) f32, f32 rotation angle)"""
        row = np.array([0, 0, 1, 0, 1, 0, 0, 0], dtype=np.float32)
        angle = np.float32(0)
        for op in ops:
            if op[0] == 'flip_x':
                row[0] = 1
            elif op[0] == 'flip_y':
                row[1] = 1
            elif op[0] == 'rot':
                row[2], row[3] = augmentor_utils.rotation_cs(op[1])
                angle = np.float32(op[1])
            elif op[0] == 'scale':
                row[4] = np.float32(op[1])
            else:
                row[5 + 'xyz'.index(op[1])] = np.float32(op[2])
        return row, angle

    def draw_candidates(self, gt_names, road_plane=None, calib=None):
        """one frame's candidate walk -> (groups [(class, [database indices])], records (S, 20) f32, objects (S) i32 database
        object ids, group offsets (K + 1) i32 over ALL SAMPLE_GROUPS classes, a class that was not sampled having no members)"""
        sp, db = self.sampler, self.database
        groups = dict(sp.draw(gt_names, self.labelled))
        recs, objs, off = [], [], [0]
        for name in sp.sample_groups:
            picked = groups.get(name, [])
            if picked:
                boxes = sp.candidate_boxes(name, picked)
                placed, shift = boxes.copy(), np.zeros((len(picked),), dtype=np.float32)
                if sp.sampler_cfg.get('USE_ROAD_PLANE', False):
                    placed, shift = sp.put_boxes_on_road_planes(placed, road_plane, calib)
                rec = np.empty((len(picked), self.CAND_WIDTH), dtype=np.float32)
                rec[:, 0:7] = boxes
                rec[:, 7] = self.class_names.index(name) + 1
                rec[:, 8] = shift
                rec[:, 9:17] = database_sampler.removal_boxes(placed, sp.sampler_cfg.REMOVE_EXTRA_WIDTH)
                rec[:, 17:20] = [np.asarray(sp.db_infos[name][i]['box3d_lidar'], dtype=np.float32)[:3] for i in picked]
                recs.append(rec)
                objs += [db.class_base[name] + i for i in picked]
            off.append(off[-1] + len(picked))
        recs = np.concatenate(recs, 0) if recs else np.zeros((0, self.CAND_WIDTH), dtype=np.float32)
        return list(groups.items()), recs, np.asarray(objs, dtype=np.int32), np.asarray(off, dtype=np.int32)

    def draw_batch(self, batch_size, gt_names=None, road_planes=None, calibs=None):
        """-> params (B, 8) f32, angles (B) f32; consumes np.random exactly like DataAugmentor.forward on B frames in order.
        With a gt_sampling step: gt_names = per-frame arrays of the frames' box names (road_planes / calibs per frame with
        USE_ROAD_PLANE), and a third value is returned, the packed candidates of the batch:
          cand (B, S, 20) f32, cand_obj (B, S) i32, group_offsets (B, K + 1) i32 (S = the largest candidate count, at least 1;
          rows behind a frame's candidates are zero), n_cand_points = the point count of all candidates, groups = per frame
          [(class, [database indices])]"""
        params = np.empty((batch_size, self.PARAM_WIDTH), dtype=np.float32)
        angles = np.empty((batch_size,), dtype=np.float32)
        frames = []
        for b in range(batch_size):
            if self.sampler is not None:
                frames.append(self.draw_candidates(gt_names[b], road_planes[b] if road_planes is not None else None,
                                                   calibs[b] if calibs is not None else None))
            params[b], angles[b] = self.pack(self.draw_frame())
        if self.sampler is None:
            return params, angles
        S = max(1, max(len(f[1]) for f in frames))
        if S > self.MAX_CANDIDATES:
            raise NotImplementedError('gt_sampling on the device takes up to %d candidates per frame, a frame drew %d'
                                      % (self.MAX_CANDIDATES, S))
        K = len(self.sampler.sample_groups)
        cand = np.zeros((batch_size, S, self.CAND_WIDTH), dtype=np.float32)
        cand_obj = np.zeros((batch_size, S), dtype=np.int32)
        group_off = np.zeros((batch_size, K + 1), dtype=np.int32)
        counts = self.database.obj_counts
        n_cand_points = 0
        for b, (_, recs, objs, off) in enumerate(frames):
            cand[b, :len(recs)] = recs
            cand_obj[b, :len(objs)] = objs
            group_off[b] = off
            n_cand_points += int(counts[objs].sum())
        return params, angles, {'cand': cand, 'cand_obj': cand_obj, 'group_offsets': group_off, 'n_cand_points': n_cand_points,
                                'groups': [f[0] for f in frames]}

    @classmethod
    def identity(cls, batch_size):
        params = np.tile(np.array([0, 0, 1, 0, 1, 0, 0, 0], dtype=np.float32), (batch_size, 1))
        return params, np.zeros((batch_size,), dtype=np.float32)
