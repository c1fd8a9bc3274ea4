"""StackSAModuleMSG / build_local_aggregation_module (pointnet2_modules.py:10-112): multi-scale set abstraction on
stacked batches: ball query + grouping (HIP) -> shared 1x1 MLP (+BN+ReLU) -> max over the neighbourhood.
VectorPoolLocalInterpolateModule / VectorPoolAggregationModule / VectorPoolAggregationModuleMSG (pointnet2_modules.py:160-470): per new
point a grid of cells, per cell three-NN interpolation (or one picked point) -> grouped 1x1 convolution -> post MLPs (csrc/vector_pool.hip)."""
from typing import List

import torch
import torch.nn as nn
import torch.nn.functional as F

from crbhip import bnrelu

from . import pointnet2_utils
from ....utils.fold_utils import fold_conv_bn
from ....utils.linear_rows import LinearRows as _LinearRows


def _split_first_layer(w, b):
    """(h1, 3+C, 1, 1) -> W1x (3, h1), W1f^T (C, h1), b1: the operand layout of crb_sa_mlp2_max_stack"""
    w = w.flatten(1)
    return w[:, :3].t().contiguous(), w[:, 3:].t().contiguous(), b.contiguous()


def _transpose_second_layer(w, b):
    return w.flatten(1).t().contiguous(), b.contiguous()


FUSED_SA_EVAL = True   # inference: group + 2-layer MLP + max in one HIP kernel (crb_sa_mlp2_max_stack)
ROWS_TRAIN = True      # training: row-major grouped matrix -> GEMM + fused BN/ReLU row kernels -> max (no MIOpen BN2d / transposes)
SPLIT_FIRST_LAYER = True   # training rows path: layer 1 = gather of per-source-point products + offset term (no grouped matrix)
FUSED_BN_MAX = True        # training rows path: last BatchNorm+ReLU, max over nsample and the concat of the scales in one op
FUSED_FIRST_BN = True      # training rows path: first conv + BatchNorm + ReLU as one node, BN backward inside the gradient kernel
FUSED_GROUP = True     # one HIP launch builds the (1, 3+C, M, ns) MLP input (False: QueryAndGroup + permute copy)
# training, two-layer MLPs: the whole module as one autograd node that keeps no (M*ns, H) activation (csrc/sa_mlp_train.hip:
# statistics passes recompute the layers from the ball-query indices); CRB_SA_TRAIN_FUSED=0 = the rows path below (A/B)
FUSED_TRAIN = __import__('os').environ.get('CRB_SA_TRAIN_FUSED', '1') == '1'


# VectorPool layers: the fused kernels of csrc/vector_pool.hip + the grouped 1x1 convolution as G batched GEMMs;
# CRB_VECTOR_POOL_FUSED=0 = the reference's torch expressions on the same three-NN / voxel-query results (A/B, test reference)
VECTOR_POOL_FUSED = __import__('os').environ.get('CRB_VECTOR_POOL_FUSED', '1') == '1'
_VECTOR_POOL_KEYS = ('NUM_GROUPS', 'LOCAL_AGGREGATION_TYPE', 'NUM_CHANNELS_OF_LOCAL_AGGREGATION', 'MSG_POST_MLPS')


def build_local_aggregation_module(input_channels, config):
    name = config.get('NAME', 'StackSAModuleMSG')
    if name == 'VectorPoolAggregationModuleMSG':
        missing = [k for k in _VECTOR_POOL_KEYS if k not in config]
        missing += ['GROUP_CFG_%d' % k for k in range(int(config.get('NUM_GROUPS', 1))) if 'GROUP_CFG_%d' % k not in config]
        if missing:
            raise NotImplementedError('%s cannot be built from this section: it has no %s (a StackSAModuleMSG section with only its '
                                      'NAME changed does not describe a vector_pool layer; pcdet.model_cfgs.pv_rcnn_plusplus_cfg(kind, '
                                      "aggregation='vector_pool') installs complete ones)" % (name, ', '.join(missing)))
        return VectorPoolAggregationModuleMSG(input_channels=input_channels, config=config), config.MSG_POST_MLPS[-1]
    if name != 'StackSAModuleMSG':
        raise NotImplementedError(name)
    mlps = [[input_channels] + list(m) for m in config.MLPS]
    layer = StackSAModuleMSG(radii=config.POOL_RADIUS, nsamples=config.NSAMPLE, mlps=mlps, use_xyz=True,
                             pool_method='max_pool')
    return layer, sum(m[-1] for m in mlps)


class StackSAModuleMSG(nn.Module):
    def __init__(self, *, radii: List[float], nsamples: List[int], mlps: List[List[int]], use_xyz: bool = True,
                 pool_method='max_pool'):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz))
            spec = list(spec)
            if use_xyz:
                spec[0] += 3
            layers = []
            for c_in, c_out in zip(spec[:-1], spec[1:]):
                layers += [nn.Conv2d(c_in, c_out, kernel_size=1, bias=False), nn.BatchNorm2d(c_out), nn.ReLU()]
            self.mlps.append(nn.Sequential(*layers))
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    @staticmethod
    def _mlp_eval_folded(mlp, x):
        """inference: BatchNorm2d folded into the preceding 1x1 conv (w' = w * gamma/sqrt(var+eps), b' = beta - mean*that);
        the grouped tensors are GB-sized (RoI grid: (1,131,442k,16)), so the separate BN pass was the single largest
        item of the CRB scoring profile"""
        mods = list(mlp)
        i = 0
        while i < len(mods):
            w, b = fold_conv_bn(mods[i], mods[i + 1])
            x = F.relu(F.conv2d(x, w, b), inplace=True)
            i += 3
        return x

    @staticmethod
    def _folded_pair(mlp):
        """kernel operands of a Conv-BN-ReLU-Conv-BN-ReLU stack with eval BN folded (cached on the convs), or None"""
        mods = list(mlp)
        if len(mods) != 6:
            return None
        for conv, bn in ((mods[0], mods[1]), (mods[3], mods[4])):
            if not isinstance(conv, nn.Conv2d) or not isinstance(bn, nn.BatchNorm2d) or bn.training:
                return None
        w1x, w1f_t, b1 = fold_conv_bn(mods[0], mods[1], _split_first_layer)
        w2t, b2 = fold_conv_bn(mods[3], mods[4], _transpose_second_layer)
        return w1x, w1f_t, b1, w2t, b2

    def _forward_fused_eval(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, query_group=None):
        folded = [self._folded_pair(m) for m in self.mlps]
        if any(f is None or not pointnet2_utils.sa_mlp2_max_supported(f[3].shape[0], f[3].shape[1]) for f in folded):
            return None
        widths = [f[3].shape[1] for f in folded]
        out = torch.empty((new_xyz.shape[0], sum(widths)), dtype=torch.float32, device=xyz.device)
        col = 0
        balls = self._balls(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, query_group)
        for grouper, f, w, ball in zip(self.groupers, folded, widths, balls):
            pointnet2_utils.sa_mlp2_max(grouper.radius, grouper.nsample, xyz, xyz_batch_cnt, new_xyz,
                                        new_xyz_batch_cnt, features, *f, out[:, col:col + w], ball=ball)
            col += w
        return out

    def _balls(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, query_group=None):
        """ball queries of all scales; two scales share one scan of the points (crb_ball_query2_stack)"""
        gs = list(self.groupers)
        if len(gs) == 2:
            return pointnet2_utils.ball_query_pair(gs[0].radius, gs[0].nsample, gs[1].radius, gs[1].nsample, xyz,
                                                   xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, group=query_group)
        return [None] * len(gs)

    def _train_fused_ok(self):
        """every scale is Conv(1x1, no bias)-BN-ReLU-Conv(1x1, no bias)-BN-ReLU with train-mode BatchNorms and a shape the
        recompute kernels have (widths 16 / 32 / 64, nsample a multiple of 16); per-frame statistics (batched CRB stage 2) keep
        the rows path"""
        if bnrelu.frame_groups_active():
            return False
        for grouper, mlp in zip(self.groupers, self.mlps):
            mods = list(mlp)
            if len(mods) != 6 or mods[0].bias is not None or mods[3].bias is not None:
                return False
            for bn in (mods[1], mods[4]):
                if not (bn.training and bn.momentum is not None and bn.affine and bn.track_running_stats and
                        bn.running_mean.is_contiguous() and bn.running_var.is_contiguous()):
                    return False
            if not pointnet2_utils.sa_mlp2_train_supported(mods[0].out_channels, mods[3].out_channels, grouper.nsample):
                return False
        return True

    @staticmethod
    def _rows_ok(mlp, features):
        mods = list(mlp)
        if len(mods) % 3:
            return False
        x = features.new_empty((2, 4))
        for i in range(0, len(mods), 3):
            conv, bn, act = mods[i], mods[i + 1], mods[i + 2]
            if not (isinstance(conv, nn.Conv2d) and conv.kernel_size == (1, 1) and isinstance(bn, nn.BatchNorm2d)
                    and isinstance(act, nn.ReLU)):
                return False
            if not bnrelu.supported(x.new_empty((2, conv.out_channels)), bn):
                return False
        return True

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True,
                query_group=None):
        """xyz (N,3), features (N,C), new_xyz (M,3) -> new_xyz, new_features (M, sum C_out). query_group (not in the reference
        signature): the caller's promise that new_xyz comes in spatially compact groups of that many consecutive rows inside
        one frame; only lets the ball query prefilter per group, the result does not depend on it."""
        if FUSED_SA_EVAL and not self.training and not torch.is_grad_enabled() and features is not None \
                and xyz.is_cuda and self.pool_method == 'max_pool' and all(g.use_xyz for g in self.groupers):
            fused = self._forward_fused_eval(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, query_group)
            if fused is not None:
                return new_xyz, fused
        outs = []
        if ROWS_TRAIN and features is not None and xyz.is_cuda and self.pool_method == 'max_pool' \
                and all(g.use_xyz for g in self.groupers) and all(self._rows_ok(m, features) for m in self.mlps):
            M = new_xyz.shape[0]
            balls = self._balls(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, query_group)
            if FUSED_TRAIN and self.training and M > 0 and self._train_fused_ok():
                return new_xyz, pointnet2_utils.sa_mlp2_train_concat(self.groupers, self.mlps, balls, xyz, xyz_batch_cnt, new_xyz,
                                                                     new_xyz_batch_cnt, features)
            fuse_max = FUSED_BN_MAX and self.training and M > 0 and \
                all(list(m)[-2].training and list(m)[-2].momentum is not None for m in self.mlps)
            for grouper, mlp, ball in zip(self.groupers, self.mlps, balls):
                mods = list(mlp)
                split = SPLIT_FIRST_LAYER and mods[0].bias is None and mods[0].out_channels in (16, 32, 64, 128)
                if not split:
                    x, _ = pointnet2_utils.query_and_group_rows(grouper.radius, grouper.nsample, xyz, xyz_batch_cnt,
                                                                new_xyz, new_xyz_batch_cnt, features, ball=ball)   # (M*ns, 3+C)
                for i in range(0, len(mods), 3):
                    conv, bn = mods[i], mods[i + 1]
                    if i == 0 and split and FUSED_FIRST_BN and (i + 3 < len(mods) or not fuse_max) and bn.training and \
                            bn.momentum is not None and M > 0 and not bnrelu.frame_groups_active() and \
                            bn.running_mean.is_contiguous() and bn.running_var.is_contiguous():
                        # first conv + its BatchNorm + ReLU as one autograd node: the BatchNorm backward is applied inside the
                        # gather-scatter gradient kernel (no (M*ns, H) gradient of the conv output in HBM)
                        x = pointnet2_utils.grouped_first_layer_bn_relu(grouper.radius, grouper.nsample, xyz, xyz_batch_cnt,
                                                                        new_xyz, new_xyz_batch_cnt, features,
                                                                        conv.weight.flatten(1), bn, ball=ball)
                        continue
                    if i == 0 and split:
                        x = pointnet2_utils.grouped_first_layer_rows(grouper.radius, grouper.nsample, xyz, xyz_batch_cnt,
                                                                     new_xyz, new_xyz_batch_cnt, features,
                                                                     conv.weight.flatten(1), ball=ball)    # (M*ns, H)
                    else:
                        x = _LinearRows.apply(x, conv.weight.flatten(1))
                    if conv.bias is not None:
                        x = x + conv.bias
                    if i + 3 < len(mods) or not fuse_max:
                        x = bnrelu.bn_relu(x, bn, relu=True)
                if fuse_max:
                    outs.append(x)                                         # pre-BN rows of the last layer
                else:
                    outs.append(x.view(M, grouper.nsample, x.shape[1]).max(dim=1).values)
            if fuse_max:
                return new_xyz, bnrelu.bn_relu_max_concat(outs, [g.nsample for g in self.groupers],
                                                          [list(m)[-2] for m in self.mlps])
            return new_xyz, torch.cat(outs, dim=1)
        for grouper, mlp in zip(self.groupers, self.mlps):
            if FUSED_GROUP and features is not None and grouper.use_xyz and xyz.is_cuda:
                x_in, _ = pointnet2_utils.query_and_group_fused(grouper.radius, grouper.nsample, xyz, xyz_batch_cnt,
                                                                new_xyz, new_xyz_batch_cnt, features)   # (1, 3+C, M, ns)
            else:
                grouped, _ = grouper(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features)  # (M, C, ns)
                x_in = grouped.permute(1, 0, 2).unsqueeze(0)
            if not self.training and not torch.is_grad_enabled():
                x = self._mlp_eval_folded(mlp, x_in)
            else:
                x = mlp(x_in)                                                                   # (1, C', M, ns)
            if self.pool_method == 'max_pool':
                x = F.max_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)
            elif self.pool_method == 'avg_pool':
                x = F.avg_pool2d(x, kernel_size=[1, x.size(3)]).squeeze(-1)
            else:
                raise NotImplementedError
            outs.append(x.squeeze(0).permute(1, 0))
        return new_xyz, torch.cat(outs, dim=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# VectorPool aggregation (reference: pointnet2_modules.py:160-470). Parameter and buffer names are the reference's.
# ---------------------------------------------------------------------------------------------------------------------------------
def _three_interpolate(features, idx, weight):
    """features (N, C), idx (E, 3), weight (E, 3) -> (E, C): w0 f0 + w1 f1 + w2 f2"""
    if features.is_cuda:
        return pointnet2_utils.three_interpolate(features, idx, weight)
    i = idx.long()
    return weight[:, 0:1] * features[i[:, 0]] + weight[:, 1:2] * features[i[:, 1]] + weight[:, 2:3] * features[i[:, 2]]


def _bn_relu_rows(bn, x):
    """relu(bn(x)) on (M, C) rows; the fused row kernels where they cover the width"""
    if x.is_cuda and bnrelu.supported(x, bn) and (not bn.training or bn.momentum is not None):
        return bnrelu.bn_relu(x, bn, relu=True)
    return F.relu(bn(x))


def _conv1d_rows(seq, x):
    """an nn.Sequential of Conv1d(k = 1, no bias) / BatchNorm1d / ReLU triples on (M, C) rows"""
    mods = list(seq)
    for i in range(0, len(mods), 3):
        x = _bn_relu_rows(mods[i + 1], _LinearRows.apply(x, mods[i].weight.flatten(1)) if x.is_cuda else F.linear(x, mods[i].weight.flatten(1)))
    return x


class VectorPoolLocalInterpolateModule(nn.Module):
    def __init__(self, mlp, num_voxels, max_neighbour_distance, nsample, neighbor_type, use_xyz=True,
                 neighbour_distance_multiplier=1.0, xyz_encoding_type='concat'):
        """neighbor_type 1: ball, others: cube; nsample: all (-1) or a limit (> 0)"""
        super().__init__()
        self.num_voxels = num_voxels
        self.num_total_grids = self.num_voxels[0] * self.num_voxels[1] * self.num_voxels[2]
        self.max_neighbour_distance = max_neighbour_distance
        self.neighbor_distance_multiplier = neighbour_distance_multiplier
        self.nsample = nsample
        self.neighbor_type = neighbor_type
        self.use_xyz = use_xyz
        self.xyz_encoding_type = xyz_encoding_type
        if self.use_xyz and self.xyz_encoding_type != 'concat':
            raise NotImplementedError('xyz_encoding_type ' + str(xyz_encoding_type))
        if mlp is not None:
            mlp = list(mlp)
            if self.use_xyz:
                mlp[0] += 9
            layers = []
            for c_in, c_out in zip(mlp[:-1], mlp[1:]):
                layers += [nn.Conv2d(c_in, c_out, kernel_size=1, bias=False), nn.BatchNorm2d(c_out), nn.ReLU()]
            self.mlp = nn.Sequential(*layers)
        else:
            self.mlp = None
        self.num_avg_length_of_neighbor_idxs = 1000        # (handed through the op and back: nothing is sized by it)

    def three_nn(self, support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt):
        with torch.no_grad():
            dist, idx, _ = pointnet2_utils.three_nn_for_vector_pool_by_two_step(
                support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt, self.max_neighbour_distance, self.nsample,
                self.neighbor_type, self.num_avg_length_of_neighbor_idxs, self.num_total_grids, self.neighbor_distance_multiplier)
        return dist, idx

    def forward_cells(self, support_xyz, support_features, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt):
        """the fused route: -> (G, M, C + 9), cell-major, what the grouped convolution reads as G GEMMs"""
        from crbhip import vector_pool
        assert self.use_xyz and self.mlp is None
        dist, idx = self.three_nn(support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt)
        return vector_pool.interpolate(support_features, idx, dist, new_xyz_grid_centers.detach(), support_xyz.detach())

    def forward(self, support_xyz, support_features, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt):
        """the reference's expressions: -> (M * G, C + 9) rows (C_out of the mlp when there is one)"""
        dist, idx = self.three_nn(support_xyz, xyz_batch_cnt, new_xyz, new_xyz_grid_centers, new_xyz_batch_cnt)
        M, G = idx.shape[0], idx.shape[1]
        dist_recip = 1.0 / (dist + 1e-8)
        norm = torch.sum(dist_recip, dim=-1, keepdim=True)
        weight = dist_recip / torch.clamp_min(norm, min=1e-8)
        idx = idx.view(-1, 3)
        empty_mask = idx[:, 0] == -1
        idx = torch.where(empty_mask[:, None], torch.zeros_like(idx), idx)
        if support_features.shape[0] == 0:                                      # (the reference reads row 0 for empty cells)
            width = support_features.shape[1] + (9 if self.use_xyz else 0)
            new_features = support_features.new_zeros((M * G, width))
        else:
            new_features = _three_interpolate(support_features, idx, weight.view(-1, 3))
            if self.use_xyz:
                near = support_xyz[idx.long()].view(-1, 3, 3)
                local_xyz = (new_xyz_grid_centers.view(-1, 1, 3) - near).view(-1, 9)
                new_features = torch.cat((new_features, local_xyz), dim=-1)
            new_features = new_features.masked_fill(empty_mask[:, None], 0)
        if self.mlp is not None:
            new_features = self.mlp(new_features.permute(1, 0)[None, :, :, None])
            new_features = new_features.squeeze(dim=0).squeeze(dim=-1).permute(1, 0)
        return new_features


class VectorPoolAggregationModule(nn.Module):
    def __init__(self, input_channels, num_local_voxel=(3, 3, 3), local_aggregation_type='local_interpolation',
                 num_reduced_channels=30, num_channels_of_local_aggregation=32, post_mlps=(128,),
                 max_neighbor_distance=None, neighbor_nsample=-1, neighbor_type=0, neighbor_distance_multiplier=2.0):
        super().__init__()
        self.num_local_voxel = num_local_voxel
        self.total_voxels = self.num_local_voxel[0] * self.num_local_voxel[1] * self.num_local_voxel[2]
        self.local_aggregation_type = local_aggregation_type
        assert self.local_aggregation_type in ['local_interpolation', 'voxel_avg_pool', 'voxel_random_choice']
        if self.local_aggregation_type == 'voxel_avg_pool':
            raise NotImplementedError('LOCAL_AGGREGATION_TYPE voxel_avg_pool is not built (local_interpolation and '
                                      'voxel_random_choice are)')
        self.input_channels = input_channels
        self.num_reduced_channels = input_channels if num_reduced_channels is None else num_reduced_channels
        self.num_channels_of_local_aggregation = num_channels_of_local_aggregation
        self.max_neighbour_distance = max_neighbor_distance
        self.neighbor_nsample = neighbor_nsample
        self.neighbor_type = neighbor_type
        if self.local_aggregation_type == 'local_interpolation':
            self.local_interpolate_module = VectorPoolLocalInterpolateModule(
                mlp=None, num_voxels=self.num_local_voxel, max_neighbour_distance=self.max_neighbour_distance,
                nsample=self.neighbor_nsample, neighbor_type=self.neighbor_type,
                neighbour_distance_multiplier=neighbor_distance_multiplier)
            num_c_in = (self.num_reduced_channels + 9) * self.total_voxels
        else:
            self.local_interpolate_module = None
            num_c_in = (self.num_reduced_channels + 3) * self.total_voxels
        num_c_out = self.total_voxels * self.num_channels_of_local_aggregation
        self.separate_local_aggregation_layer = nn.Sequential(
            nn.Conv1d(num_c_in, num_c_out, kernel_size=1, groups=self.total_voxels, bias=False), nn.BatchNorm1d(num_c_out), nn.ReLU())
        layers, c_in = [], num_c_out
        for c in post_mlps:
            layers += [nn.Conv1d(c_in, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            c_in = c
        self.post_mlps = nn.Sequential(*layers)
        self.num_mean_points_per_grid = 20                 # (handed through the op and back: nothing is sized by it)
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d) or isinstance(m, nn.Conv1d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d) or isinstance(m, nn.BatchNorm1d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def extra_repr(self) -> str:
        return f'radius={self.max_neighbour_distance}, local_voxels=({self.num_local_voxel}, ' \
               f'local_aggregation_type={self.local_aggregation_type}, ' \
               f'num_c_reduction={self.input_channels}->{self.num_reduced_channels}, ' \
               f'num_c_local_aggregation={self.num_channels_of_local_aggregation}'

    def vector_pool_with_voxel_query(self, xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt):
        """-> (M, G, 3 + C) [local xyz, features] per cell, point_cnt_of_grid (M, G)"""
        new_features, new_local_xyz, _, point_cnt_of_grid = pointnet2_utils.vector_pool_with_voxel_query_op(
            xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt, self.num_local_voxel[0], self.num_local_voxel[1],
            self.num_local_voxel[2], self.max_neighbour_distance, self.num_reduced_channels, 1, self.num_mean_points_per_grid,
            self.neighbor_nsample, self.neighbor_type, 1)
        M = new_features.shape[0]
        cells = torch.cat((new_local_xyz.view(M, -1, 3), new_features.view(M, -1, self.num_reduced_channels)), dim=-1)
        return cells, point_cnt_of_grid

    @staticmethod
    def get_dense_voxels_by_center(point_centers, max_neighbour_distance, num_voxels):
        """point_centers (N, 3) -> voxel centres (N, total_voxels, 3), z fastest"""
        R = max_neighbour_distance
        device = point_centers.device
        x_grids = torch.arange(-R + R / num_voxels[0], R - R / num_voxels[0] + 1e-5, 2 * R / num_voxels[0], device=device)
        y_grids = torch.arange(-R + R / num_voxels[1], R - R / num_voxels[1] + 1e-5, 2 * R / num_voxels[1], device=device)
        z_grids = torch.arange(-R + R / num_voxels[2], R - R / num_voxels[2] + 1e-5, 2 * R / num_voxels[2], device=device)
        x_offset, y_offset, z_offset = torch.meshgrid(x_grids, y_grids, z_grids, indexing='ij')
        xyz_offset = torch.cat((x_offset.contiguous().view(-1, 1), y_offset.contiguous().view(-1, 1),
                                z_offset.contiguous().view(-1, 1)), dim=-1)
        return point_centers[:, None, :] + xyz_offset[None, :, :]

    def vector_pool_with_local_interpolate(self, xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt):
        """-> (M, total_voxels * (C + 9)), the reference's expressions"""
        voxel_centers = self.get_dense_voxels_by_center(new_xyz, self.max_neighbour_distance, self.num_local_voxel)
        voxel_features = self.local_interpolate_module.forward(
            support_xyz=xyz, support_features=features, xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz,
            new_xyz_grid_centers=voxel_centers, new_xyz_batch_cnt=new_xyz_batch_cnt)
        return voxel_features.contiguous().view(-1, self.total_voxels * voxel_features.shape[-1])

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, **kwargs):
        """xyz (N, 3), features (N, C), new_xyz (M, 3) -> new_xyz, new_features (M, post_mlps[-1])"""
        N, C = features.shape
        assert C % self.num_reduced_channels == 0, \
            f'the input channels ({C}) should be an integral multiple of num_reduced_channels({self.num_reduced_channels})'
        features = features.view(N, C // self.num_reduced_channels, self.num_reduced_channels).sum(dim=1)   # (N = 0 is legal)
        interp =self.local_aggregation_type == 'local_interpolation'
        if VECTOR_POOL_FUSED and xyz.is_cuda and not bnrelu.frame_groups_active():
            G, M = self.total_voxels, new_xyz.shape[0]
            if interp:
                centers = self.get_dense_voxels_by_center(new_xyz, self.max_neighbour_distance, self.num_local_voxel)
                cells = self.local_interpolate_module.forward_cells(xyz, features, xyz_batch_cnt, new_xyz, centers.contiguous(),
                                                                    new_xyz_batch_cnt)              # (G, M, C + 9)
            else:
                cells = self.vector_pool_with_voxel_query(xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt)[0].transpose(0, 1)
            conv, bn = self.separate_local_aggregation_layer[0], self.separate_local_aggregation_layer[1]
            w = conv.weight.view(G, self.num_channels_of_local_aggregation, -1)       # (G * 32, C + 9, 1): the G GEMM operands
            rows = torch.bmm(cells, w.transpose(1, 2)).permute(1, 0, 2).reshape(M, -1)   # (M, G * 32), the conv's channel order
            return new_xyz, _conv1d_rows(self.post_mlps, _bn_relu_rows(bn, rows))
        if interp:
            vector_features = self.vector_pool_with_local_interpolate(xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt)
        else:
            cells, _ = self.vector_pool_with_voxel_query(xyz, xyz_batch_cnt, features, new_xyz, new_xyz_batch_cnt)
            vector_features = cells.reshape(cells.shape[0], -1)
        vector_features = vector_features.permute(1, 0)[None, :, :]                # (1, G * C', M)
        new_features = self.post_mlps(self.separate_local_aggregation_layer(vector_features))
        return new_xyz, new_features.squeeze(dim=0).permute(1, 0)


class VectorPoolAggregationModuleMSG(nn.Module):
    def __init__(self, input_channels, config):
        super().__init__()
        self.model_cfg = config
        self.num_groups = self.model_cfg.NUM_GROUPS
        self.layers = []
        c_in = 0
        for k in range(self.num_groups):
            cur = self.model_cfg[f'GROUP_CFG_{k}']
            layer = VectorPoolAggregationModule(
                input_channels=input_channels, num_local_voxel=cur.NUM_LOCAL_VOXEL, post_mlps=cur.POST_MLPS,
                max_neighbor_distance=cur.MAX_NEIGHBOR_DISTANCE, neighbor_nsample=cur.NEIGHBOR_NSAMPLE,
                local_aggregation_type=self.model_cfg.LOCAL_AGGREGATION_TYPE,
                num_reduced_channels=self.model_cfg.get('NUM_REDUCED_CHANNELS', None),
                num_channels_of_local_aggregation=self.model_cfg.NUM_CHANNELS_OF_LOCAL_AGGREGATION, neighbor_distance_multiplier=2.0)
            self.__setattr__(f'layer_{k}', layer)
            c_in += cur.POST_MLPS[-1]
        c_in += 3                                          # the new points' xyz
        layers = []
        for c in self.model_cfg.MSG_POST_MLPS:
            layers += [nn.Conv1d(c_in, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            c_in = c
        self.msg_post_mlps = nn.Sequential(*layers)

    def forward(self, **kwargs):
        """xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features; other keywords (PVRCNNHead's query_group) are ignored"""
        outs = []
        for k in range(self.num_groups):
            cur_xyz, cur_features = self.__getattr__(f'layer_{k}')(**kwargs)
            outs.append(cur_features)
        features = torch.cat([cur_xyz] + outs, dim=-1)
        if VECTOR_POOL_FUSED and features.is_cuda and not bnrelu.frame_groups_active():
            return cur_xyz, _conv1d_rows(self.msg_post_mlps, features)
        new_features = self.msg_post_mlps(features.permute(1, 0)[None, :, :])
        return cur_xyz, new_features.squeeze(dim=0).permute(1, 0)
