"""PointPillarScatter (pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:5-37): pillar rows -> the (B, C, ny, nx) BEV map.

Device tensors: crbhip.sparse.to_bev_channels_last, the scatter HeightCompression uses - the map is born in channels_last memory, the
gradient comes back through crb_dense_to_sparse_nhwc (a gather). The batch size is batch_dict['batch_size'], not coords[:, 0].max():
no read-back. Host tensors: the reference's loop."""
import torch
import torch.nn as nn


class PointPillarScatter(nn.Module):
    def __init__(self, model_cfg, grid_size, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = self.model_cfg.NUM_BEV_FEATURES
        self.nx, self.ny, self.nz = (int(v) for v in grid_size)
        assert self.nz == 1

    def forward(self, batch_dict, **kwargs):
        pillar_features, coords = batch_dict['pillar_features'], batch_dict['voxel_coords']
        if pillar_features.is_cuda:
            from crbhip import sparse as _sp
            batch_dict['spatial_features'] = _sp.to_bev_channels_last(pillar_features, coords.to(torch.int32).contiguous(),
                                                                      int(batch_dict['batch_size']), [1, self.ny, self.nx])
            return batch_dict
        batch_size = int(batch_dict['batch_size']) if 'batch_size' in batch_dict else coords[:, 0].max().int().item() + 1
        maps = []
        for batch_idx in range(batch_size):
            spatial_feature = torch.zeros(self.num_bev_features, self.nz * self.nx * self.ny, dtype=pillar_features.dtype,
                                          device=pillar_features.device)
            batch_mask = coords[:, 0] == batch_idx
            this_coords = coords[batch_mask, :]
            indices = (this_coords[:, 1] + this_coords[:, 2] * self.nx + this_coords[:, 3]).type(torch.long)
            spatial_feature[:, indices] = pillar_features[batch_mask, :].t()
            maps.append(spatial_feature)
        batch_dict['spatial_features'] = torch.stack(maps, 0).view(batch_size, self.num_bev_features * self.nz, self.ny, self.nx)
        return batch_dict
