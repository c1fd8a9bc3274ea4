"""Synthetic KITTI / Waymo shaped dataset exposing what Detector3DTemplate.build_networks and Strategy read
(SURVEY Appendix D): class_names, point_feature_encoder.num_point_features, grid_size, point_cloud_range, voxel_size,
depth_downsample_factor, sample_id_list / kitti_infos, collate_batch.

Two batch layouts:
  device_voxelize=True  (default, MI355X path): batches carry raw points only; MeanVFE runs the HIP voxel generator.
  device_voxelize=False (reference layout): each frame is voxelized through VoxelGeneratorWrapper (HIP kernel behind
                         the spconv.utils.Point2VoxelCPU3d surface) and collated exactly like the reference."""
from collections import defaultdict

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from . import synthetic as syn
from .sampler import DistributedSampler


class _PointFeatureEncoder(object):
    def __init__(self, n):
        self.num_point_features = n


class SyntheticDataset(Dataset):
    def __init__(self, num_frames=64, n_points=20000, kind='kitti', training=True, first_frame=0,
                 device_voxelize=True, class_names=None, point_cloud_range=None, voxel_size=None, max_points_per_voxel=None,
                 max_num_voxels=None):
        assert kind in ('kitti', 'waymo')
        self.kind, self.training = kind, training
        self.n_points, self.first_frame = n_points, first_frame
        self.device_voxelize = device_voxelize
        if kind == 'kitti':
            self.point_cloud_range = np.array(syn.KITTI_RANGE, dtype=np.float32)
            self.voxel_size = list(syn.KITTI_VOXEL)
            self.class_names = class_names or ['Car', 'Pedestrian', 'Cyclist']
            self.max_num_voxels = {'train': 16000, 'test': 40000}
            nfeat = 4
        else:
            self.point_cloud_range = np.array(syn.WAYMO_RANGE, dtype=np.float32)
            self.voxel_size = list(syn.WAYMO_VOXEL)
            self.class_names = class_names or ['Vehicle', 'Pedestrian', 'Cyclist']
            self.max_num_voxels = {'train': 150000, 'test': 150000}
            nfeat = 5
        self.max_points_per_voxel = 5
        # another voxel grid over the same frames (PointPillars: pcdet.model_cfgs.pointpillar_dataset_args()); grid_size follows
        if point_cloud_range is not None:
            self.point_cloud_range = np.array(point_cloud_range, dtype=np.float32)
        if voxel_size is not None:
            self.voxel_size = [float(v) for v in voxel_size]
        if max_points_per_voxel is not None:
            self.max_points_per_voxel = int(max_points_per_voxel)
        if max_num_voxels is not None:
            self.max_num_voxels = {k: int(v) for k, v in dict(max_num_voxels).items()}
        self.point_feature_encoder = _PointFeatureEncoder(nfeat)
        g = (self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(self.voxel_size)
        self.grid_size = np.round(g).astype(np.int64)
        self.depth_downsample_factor = None
        self.sample_id_list = ['%06d' % (first_frame + i) for i in range(num_frames)]
        # (KITTI kind: info['annos'], the frame's ground truth in KITTI form, appears on first use - syn.FrameInfo)
        info = syn.FrameInfo if kind == 'kitti' else dict
        self.kitti_infos = [info({'point_cloud': {'lidar_idx': s}, 'frame_id': s}) for s in self.sample_id_list]
        self.frame_ids = self.sample_id_list
        self.infos = self.kitti_infos
        self._voxel_generator = None
        self.data_augmentor = self._range_mask = None
        self.active_sampling = True

    def set_data_augmentor(self, augmentor_configs, root_path=None, logger=None, active=True, **sampler_args):
        """dataset_cfg.DATA_AUGMENTOR: in training mode __getitem__ runs the host DataAugmentor and then the host DataProcessor
        range masks on points and boxes (DatasetTemplate.prepare_data, pcdet/datasets/dataset.py:106-158).
        root_path: where a gt_sampling step finds its DB_INFO_PATH pickles and gt_database files; sampler_args (bev_iou=, db_infos=)
        go to its DataBaseSampler. active: the sampler only pastes objects cut from the frames of sample_id_list (the reference's
        cfg.ACTIVE_TRAIN branch); False selects the non-active branch."""
        from ..config import EasyDict
        from .augmentor import DataAugmentor
        from .processor.data_processor import DataProcessor
        self.data_augmentor = DataAugmentor(root_path, augmentor_configs, self.class_names, logger=logger, **sampler_args)
        self.active_sampling = bool(active)
        self._range_mask = DataProcessor(
            [EasyDict({'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True})], self.point_cloud_range,
            training=True, num_point_features=self.point_feature_encoder.num_point_features)

    WAYMO_SEQUENCE = 'segment-synthetic'

    def database_sample_id(self, fid):
        """the id under which the object database files a frame: KITTI the frame id itself (image_idx), Waymo
        sequence_name + '_' + three-digit sample_idx (what the reference's Waymo branch of the sampler assembles)"""
        return fid if self.kind == 'kitti' else '%s_%03d' % (self.WAYMO_SEQUENCE, int(fid))

    def labelled_sample_ids(self):
        """sample_id_list in the form above, as a set (rebuilt when the active loop re-assigns the list)"""
        key = (id(self.sample_id_list), len(self.sample_id_list))
        if getattr(self, '_labelled_ids', (None, None))[0] != key:
            self._labelled_ids = (key, frozenset(self.database_sample_id(f) for f in self.sample_id_list))
        return self._labelled_ids[1]

    def create_groundtruth_database(self, save_path=None, used_classes=None):
        """the ground-truth database of this dataset's frames in the reference's format (kitti_dataset.py:224-274): per object of
        every frame the (un-augmented) points inside its box, xyz relative to the box centre, membership by the CPU twin's rule
        (database_sampler.points_in_removal_boxes, no extra width).
        save_path: writes gt_database/<frame>_<Name>_<i>.bin (f32 rows of num_point_features columns) and dbinfos_train.pkl
        = {class name: [{'name', 'path', 'image_idx', 'gt_idx', 'box3d_lidar', 'num_points_in_gt', 'difficulty': 0, 'bbox',
        'score'}]} (+ 'sequence_name', 'sample_idx' for the Waymo kind) under it. None: nothing is written and the infos carry the
        arrays under 'points' with 'path' None. -> the infos"""
        import pickle
        from pathlib import Path
        from .augmentor import database_sampler as dbs
        if save_path is not None:
            (Path(save_path) / 'gt_database').mkdir(parents=True, exist_ok=True)
        all_db_infos = {}
        for fid in self.sample_id_list:
            points, boxes = syn.kitti_frame(int(fid), self.n_points, waymo=(self.kind == 'waymo'))
            inside = dbs.points_in_removal_boxes(points[:, 0:3], dbs.removal_boxes(boxes[:, :7]))
            for i in range(len(boxes)):
                name = self.class_names[int(boxes[i, 7]) - 1]
                gt_points = points[inside[i]].copy()
                gt_points[:, :3] -= boxes[i, :3]
                info = {'name': name, 'path': None, 'image_idx': fid, 'gt_idx': i, 'box3d_lidar': boxes[i, :7].copy(),
                        'num_points_in_gt': gt_points.shape[0], 'difficulty': 0,
                        'bbox': np.zeros((4,), dtype=np.float32), 'score': -1.0}
                if self.kind == 'waymo':
                    info.update({'sequence_name': self.WAYMO_SEQUENCE, 'sample_idx': int(fid)})
                if save_path is not None:
                    info['path'] = 'gt_database/%s_%s_%d.bin' % (fid, name, i)
                    gt_points.tofile(str(Path(save_path) / info['path']))
                else:
                    info['points'] = gt_points
                if used_classes is None or name in used_classes:
                    all_db_infos.setdefault(name, []).append(info)
        if save_path is not None:
            with open(str(Path(save_path) / 'dbinfos_train.pkl'), 'wb') as f:
                pickle.dump(all_db_infos, f)
        return all_db_infos

    def sync_id_views(self, waymo=False):
        """the active loop re-assigns (sample_id_list, kitti_infos) for KITTI or (frame_ids, infos) for Waymo
        (pcdet/datasets/__init__.py:111-147); keep the other pair of names pointing at the same lists"""
        if waymo:
            self.sample_id_list, self.kitti_infos = self.frame_ids, self.infos
        else:
            self.frame_ids, self.infos = self.sample_id_list, self.kitti_infos

    @property
    def calib(self):
        """the one calibration of the synthetic KITTI frames (syn.Calibration); image_shape next to it"""
        if self.kind != 'kitti':
            raise NotImplementedError('the synthetic Waymo frames have no camera: calib / image_shape exist for kind="kitti" only')
        if getattr(self, '_calib', None) is None:
            self._calib = syn.Calibration()
        return self._calib

    @property
    def image_shape(self):
        self.calib
        return np.array(syn.KITTI_IMAGE_SHAPE, dtype=np.int32)

    def generate_prediction_dicts(self, batch_dict, pred_dicts, class_names, output_path=None):
        """KittiDataset.generate_prediction_dicts (pcdet/datasets/kitti/kitti_dataset.py:277-351): per frame the ten KITTI keys
        + frame_id from pred_boxes / pred_scores / pred_labels; a frame without boxes keeps the reference's template, whose `name`
        is np.zeros(0). output_path: a directory that receives <frame_id>.txt label files in the reference's format.
        calib and image_shape come from the dataset, not from the batch."""
        from ..utils import box_utils
        calib, image_shape = self.calib, self.image_shape
        to_np = lambda v: (v[0] if isinstance(v, list) else v).detach().cpu().numpy() if not isinstance(v, np.ndarray) else v
        annos = []
        for index, box_dict in enumerate(pred_dicts):
            scores, boxes, labels = (to_np(box_dict[k]) for k in ('pred_scores', 'pred_boxes', 'pred_labels'))
            n = scores.shape[0]
            d = {'name': np.zeros(n), 'truncated': np.zeros(n), 'occluded': np.zeros(n), 'alpha': np.zeros(n), 'bbox': np.zeros([n, 4]),
                 'dimensions': np.zeros([n, 3]), 'location': np.zeros([n, 3]), 'rotation_y': np.zeros(n), 'score': np.zeros(n),
                 'boxes_lidar': np.zeros([n, 7])}
            if n:
                cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes, calib)
                d.update({'name': np.array(class_names)[labels.astype(np.int64) - 1],
                          'alpha': -np.arctan2(-boxes[:, 1], boxes[:, 0]) + cam[:, 6],
                          'bbox': box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=image_shape),
                          'dimensions': cam[:, 3:6], 'location': cam[:, 0:3], 'rotation_y': cam[:, 6], 'score': scores,
                          'boxes_lidar': boxes})
            d['frame_id'] = batch_dict['frame_id'][index]
            annos.append(d)
            if output_path is not None:
                import os
                with open(os.path.join(str(output_path), '%s.txt' % d['frame_id']), 'w') as f:
                    bbox, loc, dims = d['bbox'], d['location'], d['dimensions']          # dims: lhw -> hwl in the file
                    for i in range(len(bbox)):
                        print('%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f'
                              % (d['name'][i], d['alpha'][i], bbox[i][0], bbox[i][1], bbox[i][2], bbox[i][3], dims[i][1], dims[i][2],
                                 dims[i][0], loc[i][0], loc[i][1], loc[i][2], d['rotation_y'][i], d['score'][i]), file=f)
        return annos

    def evaluation(self, det_annos, class_names, **kwargs):
        """-> (ap_result_str, ap_dict) of det_annos (one per entry of kitti_infos, in its order) against the frames' ground truth
        through pcdet.datasets.kitti.kitti_object_eval_python (kwargs: route='device' | 'host', PR_detail_dict=, detail=)"""
        if self.kind != 'kitti':
            raise NotImplementedError('only the KITTI metrics are provided: the Waymo metrics of the reference need TensorFlow '
                                      '(waymo_open_dataset), which this stack does not have')
        import copy
        from .kitti.kitti_object_eval_python import eval as kitti_eval
        gt_annos = [copy.deepcopy(info['annos']) for info in self.kitti_infos]
        keep = {k: kwargs[k] for k in ('route', 'PR_detail_dict', 'detail') if k in kwargs}
        return kitti_eval.get_official_eval_result(gt_annos, copy.deepcopy(det_annos), class_names, **keep)

    @property
    def mode(self):
        return 'train' if self.training else 'test'

    def __len__(self):
        return len(self.sample_id_list)

    def __getitem__(self, index):
        fid = self.sample_id_list[index]
        pts, boxes = syn.kitti_frame(int(fid), self.n_points, waymo=(self.kind == 'waymo'))
        if self.data_augmentor is not None and self.training:
            # the augmentor sees the box coordinates only; the class column joins again behind it (as in the reference)
            names = np.array(self.class_names)
            a = self.data_augmentor.forward({
                'points': pts, 'gt_boxes': boxes[:, :-1].copy(), 'gt_names': names[boxes[:, -1].astype(np.int64) - 1],
                'sample_id_list': self.labelled_sample_ids() if self.active_sampling else None})
            # (gt_sampling appends boxes: the class column follows the names)
            cls = np.array([self.class_names.index(n) + 1 for n in a['gt_names']], dtype=np.float32).reshape(-1, 1)
            a['gt_boxes'] = np.concatenate([a['gt_boxes'], cls], axis=1)
            a = self._range_mask.forward(a)
            pts, boxes = a['points'], a['gt_boxes']
        d = {'points': pts, 'gt_boxes': boxes, 'frame_id': fid, 'use_lead_xyz': True}
        if not self.device_voxelize:
            from .processor.data_processor import VoxelGeneratorWrapper
            if self._voxel_generator is None:
                self._voxel_generator = VoxelGeneratorWrapper(
                    vsize_xyz=self.voxel_size, coors_range_xyz=self.point_cloud_range,
                    num_point_features=self.point_feature_encoder.num_point_features,
                    max_num_points_per_voxel=self.max_points_per_voxel,
                    max_num_voxels=self.max_num_voxels[self.mode])
            v, c, n = self._voxel_generator.generate(pts)
            d.update({'voxels': v, 'voxel_coords': c, 'voxel_num_points': n})
        return d

    @staticmethod
    def collate_batch(batch_list, _unused=False):
        """same key layout as DatasetTemplate.collate_batch (pcdet/datasets/dataset.py:160-229)"""
        data = defaultdict(list)
        for s in batch_list:
            for k, v in s.items():
                data[k].append(v)
        B = len(batch_list)
        ret = {}
        for key, val in data.items():
            if key in ('voxels', 'voxel_num_points'):
                ret[key] = np.concatenate(val, axis=0)
            elif key in ('points', 'voxel_coords'):
                ret[key] = np.concatenate([np.pad(c, ((0, 0), (1, 0)), mode='constant', constant_values=i)
                                           for i, c in enumerate(val)], axis=0)
                if key == 'points':
                    ret['point_frame_offsets'] = np.concatenate([[0], np.cumsum([len(c) for c in val])]).astype(np.int32)
            elif key == 'gt_boxes':
                mx = max(len(x) for x in val)
                g = np.zeros((B, mx, val[0].shape[-1]), dtype=np.float32)
                for k in range(B):
                    g[k, :len(val[k])] = val[k]
                ret[key] = g
            elif key == 'frame_id':
                ret[key] = np.array(val)
            else:
                ret[key] = np.stack(val, axis=0)
        ret['batch_size'] = B
        return ret


def to_device_batch(batch, device):
    """host batch -> device tensors with the dtypes the HIP path wants (offsets int32, the rest float32)"""
    out = {}
    for k, v in batch.items():
        if isinstance(v, np.ndarray) and k == 'point_frame_offsets':
            out[k] = torch.from_numpy(v).to(device=device, dtype=torch.int32)
        elif isinstance(v, np.ndarray) and v.dtype.kind in 'fiu' and k not in ('frame_id',):
            out[k] = torch.from_numpy(v).float().to(device)
        else:
            out[k] = v
    return out


def build_synthetic_dataloader(dataset, batch_size, dist=False, workers=0, shuffle=False, rank=None, world=None):
    sampler = DistributedSampler(dataset, world, rank, shuffle=shuffle) if dist else None
    return DataLoader(dataset, batch_size=batch_size, pin_memory=True, num_workers=workers,
                      shuffle=(sampler is None) and shuffle, collate_fn=dataset.collate_batch, drop_last=False,
                      sampler=sampler, timeout=0)
