"""NeighborVoxelSAModuleMSG (pcdet/ops/pointnet2/pointnet2_stack/voxel_pool_modules.py:8-130): the reference's submodules, weight
shapes, state-dict keys, init and forward signature.

Per scale: mlps_in (rows GEMM + BatchNorm1d on F.linear), then
  * HIP route (handed the level's SparseConvTensor, device tensors, C in {32, 64}, nsample <= 32, ranges <= 4): crb_voxel_query on the
    tensor's site hash, and ONE launch each way for grouping + mlps_pos + add + ReLU + pooling (crbhip.voxel_pool). mlps_pos is
    linear in the relative position d, so its BatchNorm2d folds into A (C,3), b (C): in training its batch statistics over all
    M * nsample slots are w_c . mu and w_c^T Sigma w_c with mu / Sigma the mean / covariance of d (nine numbers, reduced on the
    device in f64); A, b and the running-statistics update are formed here in f64 from (W, gamma, beta, mu, Sigma), so autograd
    carries dA, db back into W, gamma, beta including the variance's dependence on W.
  * torch route (a dense voxel2point_indices, host tensors, or a shape the kernel does not take): the reference step by step -
    dense index, materialised (M, C, nsample) groups, Conv2d + BatchNorm2d. The definition of the other route.
then mlps_out on rows."""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from ....utils import common_utils
from . import voxel_query_utils

# CRB_VOXEL_POOL_FUSED=0: every scale takes the torch route (A/B, tools/time_voxel_rcnn.py)
FUSED = __import__('os').environ.get('CRB_VOXEL_POOL_FUSED', '1') == '1'


def _rows(seq, x):
    """Conv1d(k=1) / BatchNorm1d / ReLU modules on (N, C) rows (the reference runs them on a (1, C, N) view: the same statistics)"""
    for m in seq:
        x = F.linear(x, m.weight.squeeze(-1), m.bias) if isinstance(m, nn.Conv1d) else m(x)
    return x


def fold_pos_bn(conv, bn, mu=None, sigma=None, n=None):
    """mlps_pos = Conv2d(3, C, 1, bias=False) + BatchNorm2d as pos(d) = A d + b -> A (C,3), b (C) f32.
    mu (3) / sigma (3,3) f64 given (training): batch statistics mean_c = w_c . mu, var_c = w_c^T sigma w_c over n slots, and the
    running statistics are updated as nn.BatchNorm2d does (unbiased variance, momentum or cumulative average, num_batches_tracked).
    Otherwise the running statistics."""
    W = conv.weight.view(conv.weight.shape[0], 3).double()
    if mu is not None:
        mean = W @ mu
        var = ((W @ sigma) * W).sum(1).clamp(min=0)
        if bn.track_running_stats and bn.running_mean is not None:
            with torch.no_grad():
                bn.num_batches_tracked += 1
                mom = bn.momentum if bn.momentum is not None else 1.0 / bn.num_batches_tracked.double()
                bn.running_mean.mul_(1 - mom).add_((mom * mean).to(bn.running_mean.dtype))
                bn.running_var.mul_(1 - mom).add_((mom * var * (n / max(n - 1.0, 1.0))).to(bn.running_var.dtype))
    else:
        mean, var = bn.running_mean.double(), bn.running_var.double()
    scale = bn.weight.double() / torch.sqrt(var + bn.eps)
    return (scale[:, None] * W).float(), (bn.bias.double() - scale * mean).float()


class NeighborVoxelSAModuleMSG(nn.Module):
    def __init__(self, *, query_ranges, radii, nsamples, mlps, use_xyz=True, pool_method='max_pool'):
        super().__init__()
        assert len(query_ranges) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps_in = nn.ModuleList()
        self.mlps_pos = nn.ModuleList()
        self.mlps_out = nn.ModuleList()
        for i in range(len(query_ranges)):
            self.groupers.append(voxel_query_utils.VoxelQueryAndGrouping(query_ranges[i], radii[i], nsamples[i]))
            spec = mlps[i]
            self.mlps_in.append(nn.Sequential(nn.Conv1d(spec[0], spec[1], kernel_size=1, bias=False), nn.BatchNorm1d(spec[1])))
            self.mlps_pos.append(nn.Sequential(nn.Conv2d(3, spec[1], kernel_size=1, bias=False), nn.BatchNorm2d(spec[1])))
            self.mlps_out.append(nn.Sequential(nn.Conv1d(spec[1], spec[2], kernel_size=1, bias=False), nn.BatchNorm1d(spec[2]), nn.ReLU()))
        self.relu = nn.ReLU()
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        """the reference's initialisation: Kaiming-normal convolution weights (no convolution here has a bias), unit BatchNorm scale,
        zero BatchNorm shift"""
        for stack in (self.mlps_in, self.mlps_pos, self.mlps_out):
            for seq in stack:
                conv, bn = seq[0], seq[1]
                nn.init.kaiming_normal_(conv.weight)
                nn.init.ones_(bn.weight)
                nn.init.zeros_(bn.bias)

    # ---- routes -------------------------------------------------------------------------------------------------------------
    def fused_route(self, k, features_in, sparse_tensor):
        """None when scale k runs on the HIP route, else the reason it does not"""
        if not voxel_query_utils._is_sparse_tensor(sparse_tensor):
            return 'a dense voxel2point_indices was handed over'
        if not features_in.is_cuda:
            return 'host tensors'
        if not FUSED:
            return 'CRB_VOXEL_POOL_FUSED=0'
        if self.pool_method not in ('max_pool', 'avg_pool'):
            raise NotImplementedError(self.pool_method)
        from crbhip import voxel_pool
        g = self.groupers[k]
        if not (voxel_pool.supported(features_in.shape[1], g.nsample) and voxel_pool.query_supported(g.nsample, g.max_range)):
            return 'C = %d, nsample = %d, ranges %s: the kernel takes C in {32, 64}, nsample <= 32, ranges <= 4' % (
                features_in.shape[1], g.nsample, list(g.max_range))
        if self.pool_method == 'avg_pool' and torch.are_deterministic_algorithms_enabled() and features_in.requires_grad:
            return 'avg_pool under deterministic algorithms (its scatter has no single selected row)'
        return None

    def _pool_fused(self, k, features_in, xyz, new_xyz, new_coords, sparse_tensor):
        from crbhip import voxel_pool
        g = self.groupers[k]
        idx, cnt = voxel_query_utils.voxel_query_hip(g.max_range, g.radius, g.nsample, xyz, new_xyz, new_coords, sparse_tensor)
        conv, bn = self.mlps_pos[k][0], self.mlps_pos[k][1]
        if bn.training or bn.running_mean is None:
            mu, sigma = voxel_pool.moments(xyz, new_xyz, idx, cnt)
            A, b = fold_pos_bn(conv, bn, mu, sigma, float(idx.numel()))
        else:
            A, b = fold_pos_bn(conv, bn)
        return voxel_pool.voxel_pool(features_in, A, b, xyz, new_xyz, idx, cnt, self.pool_method)

    def _pool_torch(self, k, features_in, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, voxel2point_indices):
        """voxel_pool_modules.py:96-120 as written"""
        grouped_features, grouped_xyz, empty_ball_mask = self.groupers[k](
            new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features_in, voxel2point_indices)
        keep = (~empty_ball_mask).view(-1, 1, 1)
        grouped_features = (grouped_features * keep.to(grouped_features.dtype)).permute(1, 0, 2).unsqueeze(dim=0)       # (1, C, M, ns)
        grouped_xyz = (grouped_xyz - new_xyz.unsqueeze(-1)) * keep.to(grouped_xyz.dtype)
        grouped_xyz = grouped_xyz.permute(1, 0, 2).unsqueeze(0)                                                          # (1, 3, M, ns)
        pool = {'max_pool': F.max_pool2d, 'avg_pool': F.avg_pool2d}.get(self.pool_method)
        if pool is None:
            raise NotImplementedError(self.pool_method)
        activated = self.relu(grouped_features + self.mlps_pos[k](grouped_xyz))                                        # (1, C, M, ns)
        return pool(activated, kernel_size=(1, activated.shape[-1]))[0, :, :, 0].t()                                   # (M, C)

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, features, voxel2point_indices):
        """xyz (N,3) voxel centres, new_xyz (M,3) grid points, new_coords (M,4) [b, x, y, z] at this level, features (N,C_in),
        voxel2point_indices: the reference's dense (B,Z,Y,X) tensor, or the level's SparseConvTensor -> (M, sum_k mlps[k][-1])"""
        # [b, x, y, z] -> [b, z, y, x] (a Python index list would be uploaded per call: a host synchronisation)
        new_coords = torch.cat([new_coords[:, :1], new_coords[:, 1:].flip(1)], dim=1).contiguous()
        dense = None
        outs = []
        for k in range(len(self.groupers)):
            features_in = _rows(self.mlps_in[k], features)                                      # (N, C)
            why = self.fused_route(k, features_in, voxel2point_indices)
            if why is None:
                pooled = self._pool_fused(k, features_in, xyz, new_xyz, new_coords, voxel2point_indices)
            else:
                if voxel_query_utils._is_sparse_tensor(voxel2point_indices):
                    if features_in.is_cuda:
                        warnings.warn('NeighborVoxelSAModuleMSG: torch route (dense index, grouped tensors): ' + why)
                    if dense is None:
                        dense = common_utils.generate_voxel2pinds(voxel2point_indices)
                else:
                    dense = voxel2point_indices
                pooled = self._pool_torch(k, features_in, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, new_coords, dense)
            outs.append(_rows(self.mlps_out[k], pooled))
        return torch.cat(outs, dim=1)
