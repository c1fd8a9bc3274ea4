"""DynamicPillarVFE / PFNLayerV2 (pcdet/models/backbones_3d/vfe/dynamic_pillar_vfe.py:14-142), registered as DynPillarVFE: the
reference's constructor arguments, module tree and state-dict keys (pfn_layers.<i>.linear.weight, pfn_layers.<i>.norm.*). Reads
batch_dict['points'] (N, 1 + C) [b, x, y, z, ...] and 'batch_size'; writes 'pillar_features' (M, 64) and 'voxel_coords' (M, 4) int32
[b, 0, y, x], pillars in ascending order of (b * nx + x) * ny + y.

Two routes:
  * torch route (host tensors, or a config the kernels do not take): the reference's formulation step by step on plain torch ops -
    torch.unique(return_inverse), index_add_ for the pillar mean (the reference's torch_scatter.scatter_mean), scatter_reduce
    'amax' for the per-pillar max (its scatter_max). The definition of the other route. Taken on a device tensor because of the
    config, it says so in a warning.
  * fused route (device tensors, supported config): crbhip.dyn_vfe - crb_dyn_voxelize in pillar mode, then the two-layer net of
    csrc/dyn_pillar_vfe.hip, which keeps nothing of size (N, .) but the sorted point order.

The fused route takes the configuration of waymo_models/centerpoint_dyn_pillar_1x.yaml: NUM_FILTERS [64, 64], USE_NORM,
USE_ABSLOTE_XYZ, no WITH_DISTANCE, 4 or 5 point features.

Kept quirks of the reference: z is not masked (a point above or below the range stays in its pillar); the BatchNorm1d layers see the
n = Nk kept points and update their running statistics with the unbiased variance n / (n - 1); the maximum goes through the ReLU, so a
pillar and channel whose maximum is <= 0 passes no gradient. Deviations, the same on both routes: 64-bit keys; a point with a NaN
coordinate and a row whose frame index lies outside 0 .. batch_size - 1 are dropped; with several maximal points the first one in
input order receives the gradient (torch's scatter_reduce splits it evenly among them)."""
import warnings

import torch
import torch.nn as nn

from .dynamic_mean_vfe import dynamic_cells
from .vfe_template import VFETemplate


def segment_max(x, inv, M):
    """per-segment maximum of the rows of x (N, D) -> (M, D); every segment holds at least one row"""
    return torch.zeros((M, x.shape[1]), dtype=x.dtype, device=x.device).scatter_reduce(0, inv[:, None].expand_as(x), x, 'amax', include_self=False)


class PFNLayerV2(nn.Module):
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
        self.relu = nn.ReLU()

    def forward(self, inputs, unq_inv, num_segments=None):
        x = self.linear(inputs)
        x = self.norm(x) if self.use_norm else x
        x = self.relu(x)
        M = int(unq_inv.max()) + 1 if num_segments is None else num_segments
        x_max = segment_max(x, unq_inv, M)
        if self.last_vfe:
            return x_max
        return torch.cat([x, x_max[unq_inv, :]], dim=1)


class DynamicPillarVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.use_norm = self.model_cfg.USE_NORM
        self.with_distance = self.model_cfg.WITH_DISTANCE
        self.use_absolute_xyz = self.model_cfg.USE_ABSLOTE_XYZ
        self.num_raw_features = int(num_point_features)
        num_point_features += 6 if self.use_absolute_xyz else 3
        if self.with_distance:
            num_point_features += 1
        self.num_filters = self.model_cfg.NUM_FILTERS
        assert len(self.num_filters) > 0
        num_filters = [num_point_features] + list(self.num_filters)
        self.pfn_layers = nn.ModuleList([PFNLayerV2(num_filters[i], num_filters[i + 1], self.use_norm, last_layer=(i >= len(num_filters) - 2))
                                         for i in range(len(num_filters) - 1)])
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = [int(v) for v in grid_size]
        self.voxel_x, self.voxel_y, self.voxel_z = self.voxel_size
        self.x_offset = self.voxel_x / 2 + self.point_cloud_range[0]
        self.y_offset = self.voxel_y / 2 + self.point_cloud_range[1]
        self.z_offset = self.voxel_z / 2 + self.point_cloud_range[2]
        self.scale_xy = self.grid_size[0] * self.grid_size[1]
        self.scale_y = self.grid_size[1]

    def get_output_feature_dim(self):
        return self.num_filters[-1]

    def unsupported_reason(self, C):
        """None when the fused kernels take this module on (N, 1 + C) points, else why not"""
        from crbhip import dyn_vfe as _dv
        if not self.use_norm or not self.use_absolute_xyz or self.with_distance:
            return 'USE_NORM / USE_ABSLOTE_XYZ / no WITH_DISTANCE expected'
        if not _dv.pillar_supported(C, self.num_filters) or C != self.num_raw_features:
            return 'C = %d, NUM_FILTERS %s (C in {4, 5}, [64, 64] supported)' % (C, list(self.num_filters))
        if self.pfn_layers[0].linear.weight.dtype != torch.float32:
            return 'parameters are not float32'
        norms = [p.norm for p in self.pfn_layers]
        if self.training and any(n.momentum is None for n in norms):
            return 'cumulative moving average (momentum None)'
        if not self.training and any(n.running_mean is None for n in norms):
            return 'no running statistics'
        return None

    def _forward_torch(self, points, batch_size):
        mask, cells = dynamic_cells(points, batch_size, self.point_cloud_range, self.voxel_size, self.grid_size, (0, 1))
        mask = mask & ~torch.isnan(points[:, 3])
        points, cells = points[mask], cells[mask]
        xyz = points[:, [1, 2, 3]].contiguous()
        merge = points[:, 0].int().long() * self.scale_xy + cells[:, 0] * self.scale_y + cells[:, 1]
        unq, inv, cnt = torch.unique(merge, return_inverse=True, return_counts=True)
        M = int(unq.shape[0])
        mean = torch.zeros((M, 3), dtype=xyz.dtype, device=xyz.device).index_add_(0, inv, xyz) / cnt.to(xyz.dtype).clamp(min=1)[:, None]
        f_cluster = xyz - mean[inv, :]
        f_center = torch.zeros_like(xyz)
        f_center[:, 0] = xyz[:, 0] - (cells[:, 0].to(xyz.dtype) * self.voxel_x + self.x_offset)
        f_center[:, 1] = xyz[:, 1] - (cells[:, 1].to(xyz.dtype) * self.voxel_y + self.y_offset)
        f_center[:, 2] = xyz[:, 2] - self.z_offset
        features = [points[:, 1:] if self.use_absolute_xyz else points[:, 4:], f_cluster, f_center]
        if self.with_distance:
            features.append(torch.norm(points[:, 1:4], 2, dim=1, keepdim=True))
        features = torch.cat(features, dim=-1)
        coords = torch.stack((unq // self.scale_xy, torch.zeros_like(unq), unq % self.scale_y, (unq % self.scale_xy) // self.scale_y), dim=1).int()
        if M == 0:
            return features.new_zeros((0, self.get_output_feature_dim())), coords
        for pfn in self.pfn_layers:
            features = pfn(features, inv, M)
        return features, coords

    def _forward_fused(self, points, batch_size):
        from crbhip import dyn_vfe as _dv
        seg = _dv.dyn_voxelize(points, batch_size, self.point_cloud_range, self.voxel_size, self.grid_size, _dv.PILLAR)
        l1, l2 = self.pfn_layers
        out = _dv.dyn_pillar_net(points, seg, l1.linear.weight, l1.norm.weight, l1.norm.bias, l2.linear.weight, l2.norm.weight, l2.norm.bias,
                                 (l1.norm.running_mean, l1.norm.running_var), (l2.norm.running_mean, l2.norm.running_var), self.training,
                                 l1.norm.momentum, l1.norm.eps, self.voxel_size, [self.x_offset, self.y_offset, self.z_offset])
        if self.training and seg['M'] > 0:
            for l in (l1, l2):
                if l.norm.num_batches_tracked is not None:
                    l.norm.num_batches_tracked += 1
        return out, seg['coords']

    def forward(self, batch_dict, **kwargs):
        points = batch_dict['points']
        B = int(batch_dict['batch_size'])
        why = None
        if points.is_cuda:
            why = 'points are not float32' if points.dtype != torch.float32 else self.unsupported_reason(int(points.shape[1]) - 1)
            if why is not None:
                warnings.warn('DynPillarVFE: torch route ((N, 64) tensors kept for the backward pass): ' + why)
        if points.is_cuda and why is None:
            feats, coords = self._forward_fused(points, B)
        else:
            feats, coords = self._forward_torch(points, B)
        batch_dict['pillar_features'] = feats
        batch_dict['voxel_coords'] = coords
        return batch_dict
