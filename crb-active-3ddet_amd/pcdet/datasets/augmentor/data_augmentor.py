"""DATA_AUGMENTOR queue (pcdet/datasets/augmentor/data_augmentor.py:9-117,229-258 of the reference): the four world steps.

DataAugmentor is the host mirror for loader workers, with the reference's surface. DeviceDataAugmentor makes the same draws
for a whole batch and packs them into the per-frame parameter rows of crb_augment_mask_points / crb_augment_boxes.
gt_sampling (needs the ground-truth database of a real dataset) and the image, frustum, pyramid and local augmentors are not
provided: naming one raises NotImplementedError."""
from functools import partial

import numpy as np

from . import augmentor_utils

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
    def __init__(self, root_path, augmentor_configs, class_names, logger=None):
        self.root_path = root_path
        self.class_names = class_names
        self.logger = logger
        self.data_augmentor_queue = []
        for cur_cfg in _config_list(augmentor_configs):
            if cur_cfg.NAME not in WORLD_STEPS:
                raise NotImplementedError('DATA_AUGMENTOR step %s is not provided (world flip, rotation, scaling and translation '
                                          'are)' % cur_cfg.NAME)
            self.data_augmentor_queue.append(getattr(self, cur_cfg.NAME)(config=cur_cfg))

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
        """points (N, 3 + C), gt_boxes (G, 7 + C) [x, y, z, dx, dy, dz, heading, ...], optional gt_names / gt_boxes_mask"""
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
    arithmetic runs in crb_augment_mask_points / crb_augment_boxes (DeviceDataProcessor.process_batch(..., augmentor=self)).

    The kernels apply a frame's steps in one fixed order - flip x, flip y, rotation, scaling, translation - so the queue must
    name its steps in that order (the order of every configuration of the reference), each at most once."""

    PARAM_WIDTH = 8          # [flip_x, flip_y, c, s, scale, tx, ty, tz]

    def __init__(self, augmentor_configs, class_names=None):
        self.step_configs = _config_list(augmentor_configs)
        self.host = DataAugmentor(None, self.step_configs, class_names)
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

    def draw_frame(self):
        """one frame's draws -> list of operations (see draw_step)"""
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

    def draw_batch(self, batch_size):
        """-> params (B, 8) f32, angles (B) f32; consumes np.random exactly like DataAugmentor.forward on B frames in order"""
        params = np.empty((batch_size, self.PARAM_WIDTH), dtype=np.float32)
        angles = np.empty((batch_size,), dtype=np.float32)
        for b in range(batch_size):
            params[b], angles[b] = self.pack(self.draw_frame())
        return params, angles

    @classmethod
    def identity(cls, batch_size):
        params = np.tile(np.array([0, 0, 1, 0, 1, 0, 0, 0], dtype=np.float32), (batch_size, 1))
        return params, np.zeros((batch_size,), dtype=np.float32)
