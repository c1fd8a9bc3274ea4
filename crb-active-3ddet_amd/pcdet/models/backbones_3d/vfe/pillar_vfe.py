"""PillarVFE / PFNLayer (pcdet/models/backbones_3d/vfe/pillar_vfe.py:8-123): the reference's module tree and state-dict keys
(pfn_layers.<i>.linear.weight, pfn_layers.<i>.norm.*).

Three routes:
  * torch route (host tensors, or a config the kernels do not take): the reference's formulation step by step - (M, T, K) augmented
    points, Linear, BatchNorm1d on (M, 64, T), ReLU, max over T. The definition of the other two. Taken on a device tensor because of
    the config it says so in a warning.
  * device tensors + batch_dict['voxels'] (loader-side voxels): the fused kernels of crbhip.pillar_vfe - moments for the batch
    statistics, one forward launch, one backward launch, nothing of size (M, T, .) in either direction.
  * device tensors + raw 'points' and no 'voxels': crbhip.voxel.voxelize first (the padded (M, T, C) tensor, no mean), then the same.
    One read-back of the voxel count: this detector has no 3-D backbone to share it with.

The fused route takes the configuration of every PointPillars yaml of the reference: one PFN layer of 64 filters, USE_NORM,
USE_ABSLOTE_XYZ, no WITH_DISTANCE, 4 or 5 point features, at most 32 points per pillar.

Kept quirks of the reference: the BatchNorm1d sees all M * T rows, the padded ones (exact zeros: the linear layer has no bias)
included, and the padded slots take part in the max with relu(BN(0)). Slots behind voxel_num_points are never trusted to be zero:
both routes mask them (the reference multiplies the augmented features by the mask, which a NaN or an infinity in a padded slot
survives; the voxel generator here leaves those slots unwritten).
One deviation: for a single pillar the reference's .squeeze() returns (64,); here pillar_features is always (M, 64)."""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from .vfe_template import VFETemplate


class PFNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, use_norm=True, last_layer=False):
        super().__init__()
        self.last_vfe = last_layer
        self.use_norm = use_norm
        if not self.last_vfe:
            out_channels = out_channels // 2
        if self.use_norm:
            self.linear = nn.Linear(in_channels, out_channels, bias=False)
            self.norm = nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01)
        else:
            self.linear = nn.Linear(in_channels, out_channels, bias=True)

    def forward(self, inputs):
        x = self.linear(inputs)
        x = self.norm(x.permute(0, 2, 1)).permute(0, 2, 1) if self.use_norm else x
        x = F.relu(x)
        x_max = torch.max(x, dim=1, keepdim=True)[0]
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max.repeat(1, inputs.shape[1], 1)], dim=2)


class PillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, point_cloud_range, grid_size=None, max_num_voxels=None,
                 max_points_per_voxel=None, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = self.model_cfg.USE_NORM
        self.with_distance = self.model_cfg.WITH_DISTANCE
        self.use_absolute_xyz = self.model_cfg.USE_ABSLOTE_XYZ
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = self.model_cfg.NUM_FILTERS
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + list(self.num_filters)
        self.pfn_layers = nn.ModuleList([PFNLayer(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2))
                                         for i in range(len(num_filters) - 1)])
        self.voxel_x, self.voxel_y, self.voxel_z = (float(v) for v in voxel_size)
        self.x_offset = self.voxel_x / 2 + float(point_cloud_range[0])
        self.y_offset = self.voxel_y / 2 + float(point_cloud_range[1])
        self.z_offset = self.voxel_z / 2 + float(point_cloud_range[2])
        # what the device voxel generator needs (DATA_PROCESSOR.transform_points_to_voxels values, handed over by the dataset)
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = None if grid_size is None else [int(v) for v in grid_size]
        self.max_points_per_voxel = int(max_points_per_voxel or 32)
        self.max_voxels = dict(max_num_voxels or dict(train=16000, test=40000))

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def get_paddings_indicator(self, actual_num, max_num, axis=0):
        actual_num = torch.unsqueeze(actual_num, axis + 1)
        max_num_shape = [1] * len(actual_num.shape)
        max_num_shape[axis + 1] = -1
        max_num = torch.arange(max_num, dtype=torch.int, device=actual_num.device).view(max_num_shape)
        return actual_num.int() > max_num

    def unsupported_reason(self, C, T):
        """None when the fused kernels take this module on (M, T, C) voxels, else why not"""
        from crbhip import pillar_vfe as _pv
        if len(self.pfn_layers) != 1:
            return '%d PFN layers (one supported)' % len(self.pfn_layers)
        if not self.use_norm or not self.use_absolute_xyz or self.with_distance:
            return 'USE_NORM / USE_ABSLOTE_XYZ / no WITH_DISTANCE expected'
        cout = int(self.pfn_layers[0].linear.weight.shape[0])
        if not _pv.supported(C, T, cout) or int(self.pfn_layers[0].linear.weight.shape[1]) != C + 6:
            return 'C = %d, T = %d, %d filters (C in {4, 5}, T <= 32, 64 filters supported)' % (C, T, cout)
        if self.pfn_layers[0].linear.weight.dtype != torch.float32:
            return 'parameters are not float32'
        if self.training and self.pfn_layers[0].norm.momentum is None:
            return 'cumulative moving average (momentum None)'
        if not self.training and self.pfn_layers[0].norm.running_mean is None:
            return 'no running statistics'
        return None

    def _forward_torch(self, voxel_features, voxel_num_points, coords):
        T = voxel_features.shape[1]
        valid = self.get_paddings_indicator(voxel_num_points, T, axis=0).unsqueeze(-1)
        voxel_features = torch.where(valid, voxel_features, torch.zeros_like(voxel_features))     # the fill is not trusted
        points_mean = voxel_features[:, :, :3].sum(dim=1, keepdim=True) / voxel_num_points.type_as(voxel_features).view(-1, 1, 1)
        f_cluster = voxel_features[:, :, :3] - points_mean
        f_center = torch.zeros_like(voxel_features[:, :, :3])
        dt = voxel_features.dtype
        f_center[:, :, 0] = voxel_features[:, :, 0] - (coords[:, 3].to(dt).unsqueeze(1) * self.voxel_x + self.x_offset)
        f_center[:, :, 1] = voxel_features[:, :, 1] - (coords[:, 2].to(dt).unsqueeze(1) * self.voxel_y + self.y_offset)
        f_center[:, :, 2] = voxel_features[:, :, 2] - (coords[:, 1].to(dt).unsqueeze(1) * self.voxel_z + self.z_offset)
        features = [voxel_features if self.use_absolute_xyz else voxel_features[..., 3:], f_cluster, f_center]
        if self.with_distance:
            features.append(torch.norm(voxel_features[:, :, :3], 2, 2, keepdim=True))
        features = torch.cat(features, dim=-1) * valid.type_as(voxel_features)
        for pfn in self.pfn_layers:
            features = pfn(features)
        return features.squeeze(1)

    def _forward_fused(self, voxels, num_points, coords):
        from crbhip import pillar_vfe as _pv
        pfn = self.pfn_layers[0]
        norm = pfn.norm
        out = _pv.pillar_vfe(voxels, num_points.to(torch.int32), coords.to(torch.int32), pfn.linear.weight, norm.weight, norm.bias,
                             norm.running_mean, norm.running_var, self.training, norm.momentum, norm.eps, self.voxel_size,
                             [self.x_offset, self.y_offset, self.z_offset])
        if self.training and norm.num_batches_tracked is not None:
            norm.num_batches_tracked += 1
        return out

    def _voxelize_on_device(self, batch_dict):
        from crbhip import voxel as _vx
        pts = batch_dict['points']
        B = int(batch_dict['batch_size'])
        if 'point_frame_offsets' in batch_dict:
            off = batch_dict['point_frame_offsets']
        else:
            counts = torch.bincount(pts[:, 0].long(), minlength=B)
            off = torch.zeros(B + 1, dtype=torch.int32, device=pts.device)
            off[1:] = torch.cumsum(counts, 0).int()
        r = _vx.voxelize(pts[:, 1:].contiguous(), off, self.point_cloud_range, self.voxel_size,
                         self.max_voxels['train' if self.training else 'test'], self.max_points_per_voxel, want_voxels=True,
                         want_mean=False, grid_xyz=self.grid_size)
        batch_dict['voxel_coords'] = r['coords']
        batch_dict['voxel_num_points'] = r['num_points']
        return r['voxels']

    def forward(self, batch_dict, **kwargs):
        if 'voxels' in batch_dict:
            voxels = batch_dict['voxels']
        else:
            voxels = self._voxelize_on_device(batch_dict)             # (raises on host tensors: the generator is a HIP kernel)
        num_points, coords = batch_dict['voxel_num_points'], batch_dict['voxel_coords']
        if voxels.shape[0] == 0:
            # no pillar at all (every point outside the range): nothing to normalise over; an empty map follows. The reference's
            # BatchNorm1d raises on the empty tensor in training mode.
            batch_dict['pillar_features'] = voxels.new_zeros((0, self.get_output_feature_dim()), dtype=self.pfn_layers[0].linear.weight.dtype)
            return batch_dict
        why = None
        if voxels.is_cuda:
            why = 'voxels are not float32' if voxels.dtype != torch.float32 else self.unsupported_reason(int(voxels.shape[2]), int(voxels.shape[1]))
            if why is not None:
                warnings.warn('PillarVFE: torch route ((M, T, K) and (M, T, 64) tensors): ' + why)
        if voxels.is_cuda and why is None:
            batch_dict['pillar_features'] = self._forward_fused(voxels, num_points, coords)
        else:
            batch_dict['pillar_features'] = self._forward_torch(voxels, num_points, coords)
        return batch_dict
