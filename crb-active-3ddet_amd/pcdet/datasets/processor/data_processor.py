"""VoxelGeneratorWrapper (pcdet/datasets/processor/data_processor.py:15-60) over the gfx950 voxel generator."""
import numpy as np


class VoxelGeneratorWrapper():
    def __init__(self, vsize_xyz, coors_range_xyz, num_point_features, max_num_points_per_voxel, max_num_voxels):
        from spconv.utils import Point2VoxelCPU3d as VoxelGenerator
        self.spconv_ver = 2
        self._voxel_generator = VoxelGenerator(
            vsize_xyz=vsize_xyz, coors_range_xyz=coors_range_xyz, num_point_features=num_point_features,
            max_num_points_per_voxel=max_num_points_per_voxel, max_num_voxels=max_num_voxels)

    def generate(self, points):
        """points (n,C) float32 numpy -> voxels (M,T,C), coordinates (M,3)[z,y,x], num_points (M)"""
        import cumm.tensorview as tv
        tv_voxels, tv_coordinates, tv_num_points = self._voxel_generator.point_to_voxel(
            tv.from_numpy(np.ascontiguousarray(points, dtype=np.float32)))
        return tv_voxels.numpy(), tv_coordinates.numpy(), tv_num_points.numpy()


class DataProcessor(object):
    """Config-driven per-frame processor queue (pcdet/datasets/processor/data_processor.py:62-143), host arrays in and out:
    mask_points_and_boxes_outside_range, shuffle_points, transform_points_to_voxels(_placeholder). Voxelisation goes
    through VoxelGeneratorWrapper (the gfx950 voxel generator behind spconv's Point2VoxelCPU3d interface).
    `sample_points` belongs to the point-based detectors (PointRCNN) and is not provided."""

    def __init__(self, processor_configs, point_cloud_range, training, num_point_features):
        from functools import partial
        self._partial = partial
        self.point_cloud_range = np.asarray(point_cloud_range, dtype=np.float32)
        self.training = training
        self.num_point_features = num_point_features
        self.mode = 'train' if training else 'test'
        self.grid_size = self.voxel_size = None
        self.voxel_generator = None
        self.data_processor_queue = []
        for cur_cfg in processor_configs:
            if not hasattr(self, cur_cfg.NAME):
                raise NotImplementedError('DATA_PROCESSOR step %s' % cur_cfg.NAME)
            self.data_processor_queue.append(getattr(self, cur_cfg.NAME)(config=cur_cfg))

    def mask_points_and_boxes_outside_range(self, data_dict=None, config=None):
        if data_dict is None:
            return self._partial(self.mask_points_and_boxes_outside_range, config=config)
        from ...utils import box_utils, common_utils
        if data_dict.get('points', None) is not None:
            mask = common_utils.mask_points_by_range(data_dict['points'], self.point_cloud_range)
            data_dict['points'] = data_dict['points'][mask]
        if data_dict.get('gt_boxes', None) is not None and config.REMOVE_OUTSIDE_BOXES and self.training:
            mask = box_utils.mask_boxes_outside_range_numpy(data_dict['gt_boxes'], self.point_cloud_range,
                                                            min_num_corners=config.get('min_num_corners', 1))
            data_dict['gt_boxes'] = data_dict['gt_boxes'][mask]
        return data_dict

    def shuffle_points(self, data_dict=None, config=None):
        if data_dict is None:
            return self._partial(self.shuffle_points, config=config)
        if config.SHUFFLE_ENABLED[self.mode]:
            points = data_dict['points']
            data_dict['points'] = points[np.random.permutation(points.shape[0])]
        return data_dict

    def _bind_grid(self, config):
        grid_size = (self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(config.VOXEL_SIZE)
        self.grid_size = np.round(grid_size).astype(np.int64)
        self.voxel_size = config.VOXEL_SIZE

    def transform_points_to_voxels_placeholder(self, data_dict=None, config=None):
        if data_dict is None:
            self._bind_grid(config)
            return self._partial(self.transform_points_to_voxels_placeholder, config=config)
        return data_dict

    def transform_points_to_voxels(self, data_dict=None, config=None):
        if data_dict is None:
            self._bind_grid(config)
            return self._partial(self.transform_points_to_voxels, config=config)
        if self.voxel_generator is None:
            self.voxel_generator = VoxelGeneratorWrapper(
                vsize_xyz=config.VOXEL_SIZE, coors_range_xyz=self.point_cloud_range,
                num_point_features=self.num_point_features, max_num_points_per_voxel=config.MAX_POINTS_PER_VOXEL,
                max_num_voxels=config.MAX_NUMBER_OF_VOXELS[self.mode])
        voxels, coordinates, num_points = self.voxel_generator.generate(data_dict['points'])
        if not data_dict['use_lead_xyz']:
            voxels = voxels[..., 3:]
        data_dict['voxels'] = voxels
        data_dict['voxel_coords'] = coordinates
        data_dict['voxel_num_points'] = num_points
        return data_dict

    def forward(self, data_dict):
        for cur_processor in self.data_processor_queue:
            data_dict = cur_processor(data_dict=data_dict)
        return data_dict


class DeviceDataProcessor(object):
    """the same queue for a whole BATCH on the GPU. Raw per-frame point arrays cross PCIe once (pinned,
    non-blocking); range mask, per-frame shuffle and frame concatenation run as device ops, voxelisation is left to
    MeanVFE's crb_voxelize call (points + point_frame_offsets in the batch, no (M,5,C) voxel tensor at all). GT boxes are a
    few dozen rows per frame and stay on the host path.

    Differences from the host queue: the shuffle draws from a torch device generator, not np.random (another permutation
    of the same points: 'first 5 points per voxel / first M voxels' pick different but equally valid members)."""

    def __init__(self, processor_configs, point_cloud_range, training, num_point_features, device='cuda'):
        import torch
        self.torch = torch
        self.device = torch.device(device)
        self.point_cloud_range = np.asarray(point_cloud_range, dtype=np.float32)
        self.training = training
        self.mode = 'train' if training else 'test'
        self.num_point_features = num_point_features
        self.mask_cfg = self.shuffle = None
        self.voxel_cfg = None
        for cfg in processor_configs:
            if cfg.NAME == 'mask_points_and_boxes_outside_range':
                self.mask_cfg = cfg
            elif cfg.NAME == 'shuffle_points':
                self.shuffle = bool(cfg.SHUFFLE_ENABLED[self.mode])
            elif cfg.NAME in ('transform_points_to_voxels', 'transform_points_to_voxels_placeholder'):
                self.voxel_cfg = cfg
            else:
                raise NotImplementedError('DATA_PROCESSOR step %s' % cfg.NAME)
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(0)
        if self.voxel_cfg is not None:
            g = (self.point_cloud_range[3:6] - self.point_cloud_range[0:3]) / np.array(self.voxel_cfg.VOXEL_SIZE)
            self.grid_size = np.round(g).astype(np.int64)
            self.voxel_size = self.voxel_cfg.VOXEL_SIZE

    def process_batch(self, points_list, gt_boxes_list=None, frame_ids=None, augmentor=None):
        """points_list: per-frame (n_i, C) float32 numpy arrays -> batch dict with device 'points' (N,1+C),
        'point_frame_offsets' (B+1) int32, host-padded 'gt_boxes' (B,G,8) on the device.
        augmentor: a DeviceDataAugmentor (pcdet.datasets.augmentor), or None for un-augmented frames. On a CUDA device the frames
        are transformed, range-masked and concatenated by crb_augment_mask_points and the boxes by crb_augment_boxes; on
        device='cpu' every frame goes through the host DataAugmentor first (same draws, same arithmetic)."""
        torch = self.torch
        from ...utils import box_utils, common_utils
        if augmentor is not None:
            if self.device.type == 'cuda':
                return self._process_batch_augmented(points_list, gt_boxes_list, frame_ids, augmentor)
            points_list, gt_boxes_list = self._host_augment(points_list, gt_boxes_list, augmentor)
        B = len(points_list)
        counts = [len(p) for p in points_list]
        host = torch.from_numpy(np.concatenate(points_list, 0).astype(np.float32, copy=False))
        pts = (host.pin_memory() if self.device.type == 'cuda' else host).to(self.device, non_blocking=True)
        bidx = torch.repeat_interleave(torch.arange(B, device=self.device),
                                       torch.tensor(counts, device=self.device))
        if self.mask_cfg is not None:
            r = self.point_cloud_range
            keep = (pts[:, 0] >= float(r[0])) & (pts[:, 0] <= float(r[3])) & (pts[:, 1] >= float(r[1])) & \
                   (pts[:, 1] <= float(r[4]))
            pts, bidx = pts[keep], bidx[keep]                   # the one device->host size read-back of the batch
        if self.shuffle:
            key = bidx.double() + torch.rand(bidx.shape[0], device=self.device, generator=self.generator,
                                             dtype=torch.float64)
            order = torch.argsort(key)
            pts = pts[order]
        n_per = common_utils.batch_counts(bidx, B)
        off = torch.zeros((B + 1,), dtype=torch.int32, device=self.device)
        off[1:] = torch.cumsum(n_per, 0)
        batch = {'points': torch.cat([bidx.float().unsqueeze(1), pts], 1), 'point_frame_offsets': off, 'batch_size': B}
        if gt_boxes_list is not None:
            gts = []
            for g in gt_boxes_list:
                g = np.asarray(g, dtype=np.float32)
                if self.mask_cfg is not None and self.mask_cfg.REMOVE_OUTSIDE_BOXES and self.training and len(g):
                    g = g[box_utils.mask_boxes_outside_range_numpy(g, self.point_cloud_range,
                                                                   self.mask_cfg.get('min_num_corners', 1))]
                gts.append(g)
            mx = max(1, max(len(g) for g in gts))
            width = gts[0].shape[-1] if len(gts[0].shape) == 2 and gts[0].shape[-1] else 8
            pad = np.zeros((B, mx, width), dtype=np.float32)
            for k, g in enumerate(gts):
                pad[k, :len(g)] = g
            batch['gt_boxes'] = torch.from_numpy(pad).to(self.device, non_blocking=True)
        if frame_ids is not None:
            batch['frame_id'] = np.array(frame_ids)
        return batch

    @staticmethod
    def _host_augment(points_list, gt_boxes_list, augmentor):
        """the host route: DataAugmentor.forward on copies of the frames, one by one and in order. The boxes of a batch carry their
        class in the last column, which the augmentor never sees (the reference appends it after augmentation); a gt_sampling step
        gets the names that column stands for and the augmentor's labelled set, and the column is rebuilt from the names behind it"""
        pts_out, gt_out = [], []
        names = np.array(augmentor.class_names) if augmentor.sampler is not None else None
        for k, p in enumerate(points_list):
            g = np.asarray(gt_boxes_list[k], dtype=np.float32) if gt_boxes_list is not None else None
            if g is None or g.ndim != 2 or g.shape[1] == 0:
                g = np.zeros((0, 8), dtype=np.float32)
            d = {'points': np.array(p, dtype=np.float32), 'gt_boxes': g[:, :-1].copy()}
            if names is not None:
                d['gt_names'] = names[g[:, -1].astype(np.int64) - 1] if len(g) else np.zeros((0,), dtype=names.dtype)
                d['sample_id_list'] = augmentor.labelled
            d = augmentor.host.forward(d)
            cls = g[:, -1:]
            if names is not None:
                cls = np.array([[augmentor.class_names.index(n) + 1] for n in d['gt_names']], dtype=np.float32).reshape(-1, 1)
            pts_out.append(d['points'])
            gt_out.append(np.concatenate([d['gt_boxes'], cls], axis=1))
        return pts_out, (gt_out if gt_boxes_list is not None else None)

    def _process_batch_augmented(self, points_list, gt_boxes_list, frame_ids, augmentor):
        """the device route: one upload of the raw frames, of the drawn parameters and of the padded boxes; transform + range mask +
        frame concatenation in crb_augment_mask_points (three launches), the boxes in crb_augment_boxes (one); one read-back of
        the kept totals. Replaces the comparison / boolean-index / repeat_interleave launches of the un-augmented path.
        With a gt_sampling step the drawn candidates travel in the same two uploads; crb_gt_sample_select and crb_gt_sample_paste
        run in front (collision test, point removal and paste against the device-resident object database), their outputs feed
        the two kernels above, and the read-back stays the only one. The batch then also carries 'gt_sampling_valid' (B, S) u8 on
        the device and 'gt_sampling_groups', the per-frame [(class, [database indices])] that were drawn."""
        torch = self.torch
        from crbhip import augment
        dev = self.device
        B = len(points_list)
        have_boxes = gt_boxes_list is not None
        sampling = getattr(augmentor, 'sampler', None) is not None
        if have_boxes:
            gts = [np.asarray(g, dtype=np.float32) for g in gt_boxes_list]
            width = gts[0].shape[-1] if len(gts[0].shape) == 2 and gts[0].shape[-1] else 8
            G = max(1, max(len(g) for g in gts))
            pad = np.zeros((B, G, width), dtype=np.float32)
            for k, g in enumerate(gts):
                pad[k, :len(g)] = g
        draw = None
        if sampling:
            if not have_boxes or width != 8:
                raise ValueError('gt_sampling needs the frames\' boxes as (G, 8) rows [7 coordinates, class]')
            names = np.array(augmentor.class_names)
            params_h, angles_h, draw = augmentor.draw_batch(
                B, gt_names=[names[g[:, -1].astype(np.int64) - 1] if len(g) else np.zeros((0,), dtype=names.dtype) for g in gts])
            # one more identity row: the frame that stands for the unused tail of the paste buffer (see below)
            params_h = np.concatenate([params_h, augmentor.identity(1)[0]], 0)
        else:
            params_h, angles_h = augmentor.draw_batch(B)
        P = len(params_h)
        counts = [len(p) for p in points_list]
        host = torch.from_numpy(np.concatenate(points_list, 0).astype(np.float32, copy=False))
        pts = host.pin_memory().to(dev, non_blocking=True)
        # the small operands travel as one f32 and one i32 buffer:
        # [params (P,8) | angles (B) | boxes (B,G,W) | candidates (B,S,20)], [offsets (B+1) | box counts (B) | objects (B,S) | groups (B,K+1)]
        f_parts = [params_h.ravel(), angles_h] + ([pad.ravel()] if have_boxes else [])
        i_parts = [[0], np.cumsum(counts), [len(g) for g in gts] if have_boxes else []]
        if sampling:
            f_parts.append(draw['cand'].ravel())
            i_parts += [draw['cand_obj'].ravel(), draw['group_offsets'].ravel()]
        f_host = np.concatenate(f_parts)
        i_host = np.concatenate(i_parts).astype(np.int32)
        f_dev = torch.from_numpy(f_host).pin_memory().to(dev, non_blocking=True)
        i_dev = torch.from_numpy(i_host).pin_memory().to(dev, non_blocking=True)
        params, angles = f_dev[:8 * P].view(P, 8), f_dev[8 * P:8 * P + B]
        f_at = 8 * P + B
        off, box_counts = i_dev[:B + 1], i_dev[B + 1:2 * B + 1]
        if have_boxes:
            boxes_in = f_dev[f_at:f_at + B * G * width].view(B, G, width)
            f_at += B * G * width
        valid = None
        if sampling:
            from crbhip import gt_sampling
            S, K1 = draw['cand'].shape[1], draw['group_offsets'].shape[1]
            cand = f_dev[f_at:f_at + B * S * 20].view(B, S, 20)
            cand_obj = i_dev[2 * B + 1:2 * B + 1 + B * S].view(B, S)
            group_off = i_dev[2 * B + 1 + B * S:].view(B, K1)
            db = augmentor.database.device_tensors(dev)
            valid, boxes_in, box_counts, cand_rows, paste_counts = gt_sampling.select(boxes_in, box_counts, cand, cand_obj,
                                                                                      group_off, db)
            # the paste buffer holds the scene points plus the points of ALL candidates (known here, no read-back); its offsets
            # end with [total, capacity], so that to crb_augment_mask_points the untouched tail is frame B, behind the real ones
            pts, off = gt_sampling.paste(pts, off, cand, cand_obj, valid, cand_rows, paste_counts, db,
                                         capacity=len(host) + draw['n_cand_points'], lazy=True)
        r = [float(v) for v in self.point_cloud_range]
        out, new_off = augment.augment_mask_points(pts, off, params, r, mask=self.mask_cfg is not None, xyz_col=0,
                                                   frame_col=True, lazy=True)
        new_off = new_off[:B + 1]
        sizes = new_off
        if have_boxes:
            mask_boxes = bool(self.mask_cfg is not None and self.mask_cfg.REMOVE_OUTSIDE_BOXES and self.training)
            boxes, new_counts = augment.augment_boxes(
                boxes_in, box_counts, params[:B], angles, r, mask=mask_boxes,
                min_num_corners=self.mask_cfg.get('min_num_corners', 1) if mask_boxes else 1)
            sizes = torch.cat([new_off, new_counts])
        sizes_h = sizes.cpu().tolist()                          # the one device->host size read-back of the batch
        out = out[:sizes_h[B]]
        if self.shuffle:
            key = out[:, 0].double() + torch.rand(out.shape[0], device=dev, generator=self.generator, dtype=torch.float64)
            out = out[torch.argsort(key)]
        batch = {'points': out, 'point_frame_offsets': new_off, 'batch_size': B}
        if have_boxes:
            batch['gt_boxes'] = boxes[:, :max(1, max(sizes_h[B + 1:]))].contiguous()
        if sampling:
            batch['gt_sampling_valid'] = valid
            batch['gt_sampling_groups'] = draw['groups']
        if frame_ids is not None:
            batch['frame_id'] = np.array(frame_ids)
        return batch
