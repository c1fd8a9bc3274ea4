"""The ground-truth object database of gt_sampling, resident on the device (read by crb_gt_sample_select / crb_gt_sample_paste).

All objects of all classes in one table, class after class in the order of class_names and inside a class in the order of the
sampler's db_infos AFTER its PREPARE filters - so `class_base[name] + i` is the object the sampler calls db_infos[name][i]:
  points       (P, C) f32   every object's points, xyz relative to the box centre, as the database files hold them
  obj_offsets  (N + 1) i32  object o owns rows [obj_offsets[o], obj_offsets[o + 1])
  boxes        (N, 7) f32   box3d_lidar of the infos (as stored: before any fake-lidar conversion)
  classes      (N) i32      1-based index into class_names
The host arrays are built once (files read or in-memory points taken); device_tensors(device) uploads them once per device."""
import numpy as np


class DeviceGtDatabase(object):
    def __init__(self, db_infos, class_names, num_point_features, load_points):
        """db_infos {class: [info]}; load_points(info) -> (n, C) f32"""
        self.class_names = list(class_names)
        self.num_point_features = int(num_point_features)
        self.class_base = {}
        pts, counts, boxes, classes = [], [], [], []
        for k, name in enumerate(self.class_names):
            self.class_base[name] = len(counts)
            for info in db_infos.get(name, []):
                p = np.asarray(load_points(info), dtype=np.float32).reshape(-1, self.num_point_features)
                pts.append(p)
                counts.append(len(p))
                boxes.append(np.asarray(info['box3d_lidar'], dtype=np.float32)[:7])
                classes.append(k + 1)
        self.obj_counts = np.asarray(counts, dtype=np.int64)
        assert int(self.obj_counts.sum()) < 2 ** 31 - 256
        self.obj_offsets = np.concatenate([[0], np.cumsum(self.obj_counts)]).astype(np.int32)
        self.points = np.concatenate(pts, 0) if pts else np.zeros((0, self.num_point_features), dtype=np.float32)
        self.boxes = np.stack(boxes, 0) if boxes else np.zeros((0, 7), dtype=np.float32)
        self.classes = np.asarray(classes, dtype=np.int32)
        self._device = {}

    @classmethod
    def from_sampler(cls, sampler):
        """the database behind a pcdet.datasets.augmentor.database_sampler.DataBaseSampler (its filtered db_infos)"""
        return cls(sampler.db_infos, sampler.class_names, sampler.sampler_cfg.NUM_POINT_FEATURES, sampler.object_points)

    @property
    def num_objects(self):
        return len(self.obj_counts)

    @property
    def nbytes(self):
        """resident size on a device"""
        return self.points.nbytes + self.obj_offsets.nbytes + self.boxes.nbytes + self.classes.nbytes

    def device_tensors(self, device):
        """-> {'points', 'obj_offsets', 'boxes', 'classes'} on the device, uploaded on the first call"""
        import torch
        device = torch.device(device)
        if device.type != 'cuda':
            from ._lib import CrbHipError
            raise CrbHipError('DeviceGtDatabase lives on a GPU: the HIP path has no CPU fallback')
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        if key not in self._device:
            self._device[key] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                                 for k in ('points', 'obj_offsets', 'boxes', 'classes')}
        return self._device[key]
