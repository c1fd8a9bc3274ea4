"""DynamicMeanVFE (pcdet/models/backbones_3d/vfe/dynamic_mean_vfe.py:14-76), registered as DynMeanVFE: dynamic voxelization - every
point inside the range belongs to its voxel, no cap on points per voxel, none on voxels - and the mean of the point features per
voxel. Reads batch_dict['points'] (N, 1 + C) [b, x, y, z, ...] and 'batch_size'; writes 'voxel_features' (M, C) and 'voxel_coords'
(M, 4) int32 [b, z, y, x], voxels in ascending order of ((b * nx + x) * ny + y) * nz + z, so VoxelBackBone8x runs behind it unchanged.

Two routes:
  * torch route (host tensors): the reference's formulation step by step on plain torch ops - floor / mask / merge_coords /
    torch.unique(return_inverse) / index_add_ for the mean (the reference's torch_scatter.scatter_mean). The definition of the other.
  * device tensors: crbhip.dyn_vfe (csrc/dyn_voxelize.hip) - one stable radix sort of (key, point index) pairs and a segmented
    f64 mean; one read-back of the voxel count. There is no eager route on device tensors: a failing kernel call raises.

Deviations from the reference, the same on both routes: the key is formed in 64 bits (the reference's int32 key overflows beyond
2^31 cells); a point with a NaN coordinate is dropped (the reference's floor(NaN).int() is undefined), and so is a
row whose frame index lies outside 0 .. batch_size - 1 (the reference would emit a voxel of a frame that does not exist)."""
import torch

from .vfe_template import VFETemplate


def dynamic_cells(points, batch_size, point_cloud_range, voxel_size, grid_size, axes):
    """the reference's cell arithmetic on the coordinate columns `axes` (0 = x ..): points (N, 1 + C) -> (kept mask (N), cells (N, len
    (axes)) int64, valid where kept). Range and voxel size are f32 tensors as the reference's constructor makes them (an f64 input is
    promoted against them). NaN coordinates are dropped, and so are rows whose frame index .int() is outside 0 .. batch_size - 1."""
    cols = [1 + a for a in axes]
    lo = torch.tensor([point_cloud_range[a] for a in axes], dtype=torch.float32, device=points.device)
    vs = torch.tensor([voxel_size[a] for a in axes], dtype=torch.float32, device=points.device)
    gs = torch.tensor([grid_size[a] for a in axes], dtype=torch.int64, device=points.device)
    c = torch.floor((points[:, cols] - lo) / vs)
    mask = ((c >= 0) & (c < gs.to(c.dtype))).all(dim=1)       # a NaN fails both comparisons
    mask = mask & (points[:, 0] > -1) & (points[:, 0] < batch_size)
    return mask, torch.where(mask[:, None], c, torch.zeros_like(c)).long()


class DynamicMeanVFE(VFETemplate):
    def __init__(self, model_cfg, num_point_features, voxel_size, grid_size, point_cloud_range, **kwargs):
        super().__init__(model_cfg=model_cfg)
        self.num_point_features = num_point_features
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.grid_size = [int(v) for v in grid_size]
        self.scale_xyz = self.grid_size[0] * self.grid_size[1] * self.grid_size[2]
        self.scale_yz = self.grid_size[1] * self.grid_size[2]
        self.scale_z = self.grid_size[2]

    def get_output_feature_dim(self):
        return self.num_point_features

    def _forward_torch(self, points, batch_size):
        mask, cells = dynamic_cells(points, batch_size, self.point_cloud_range, self.voxel_size, self.grid_size, (0, 1, 2))
        points, cells = points[mask], cells[mask]
        merge = points[:, 0].int().long() * self.scale_xyz + cells[:, 0] * self.scale_yz + cells[:, 1] * self.scale_z + cells[:, 2]
        unq, inv, cnt = torch.unique(merge, return_inverse=True, return_counts=True)
        data = points[:, 1:].contiguous()
        mean = torch.zeros((unq.shape[0], data.shape[1]), dtype=data.dtype, device=data.device).index_add_(0, inv, data)
        mean = mean / cnt.to(data.dtype).clamp(min=1)[:, None]
        coords = torch.stack((unq // self.scale_xyz, unq % self.scale_z, (unq % self.scale_yz) // self.scale_z,
                              (unq % self.scale_xyz) // self.scale_yz), dim=1).int()
        return mean.contiguous(), coords.contiguous()

    def _forward_fused(self, points, batch_size):
        from crbhip import dyn_vfe as _dv
        r = _dv.dyn_voxelize(points, batch_size, self.point_cloud_range, self.voxel_size, self.grid_size, _dv.VOXEL)
        return _dv.dyn_mean(points, r['perm'], r['seg_offsets']), r['coords']

    @torch.no_grad()
    def forward(self, batch_dict, **kwargs):
        points = batch_dict['points']
        if points.is_cuda:
            if points.dtype != torch.float32:
                raise TypeError('DynMeanVFE: device points must be float32 (the kernels of crbhip.dyn_vfe take nothing else)')
            feats, coords = self._forward_fused(points, int(batch_dict['batch_size']))
        else:
            feats, coords = self._forward_torch(points, int(batch_dict['batch_size']))
        batch_dict['voxel_features'] = feats
        batch_dict['voxel_coords'] = coords
        return batch_dict
