"""PartA2FCHead (pcdet/models/roi_heads/partA2_head.py:10-224): RoI-aware pooling of the point head's part offsets (avg)
and point features (max) into an out^3 grid per RoI, two SubM conv stacks over the occupied cells of all B*N grids as ONE
sparse tensor (batch index = RoI), dense flatten, shared FC, class / box branches.

Everything numeric runs on the HIP entry points the other heads already use: crb_roiaware_pool3d_forward / _backward
(RoIAwarePool3d), the subm rulebook + gather-GEMM of the spconv mirror (4->64, 64->64, C_in->64), crb_sparse_to_dense.
What it consumes is in the tree: `point_features` / `point_coords` at the voxel centres from UNetV2 (backbones_3d/spconv_unet.py),
`point_part_offset` / `point_cls_scores` from PointIntraPartOffsetHead (dense_heads/point_intra_part_head.py); PartA2Net
(detectors/part_a2_net.py) chains them.

By default the pooled rows of the sparse tensor come straight from csrc/roiaware_sparse.hip (one launch sequence for all frames,
one read-back, no dense grid); CRB_ROIAWARE_SPARSE=0, DISABLE_PART, a grid beyond the kernel's LDS histogram, a negative part
feature inside a RoI and fewer than 3 rows take the dense route (roiaware_pool + nonzero + gather), which gives the same bits."""
import torch
import torch.nn as nn

from crbhip import roiaware_sparse
from crbhip.part_head import frame_offsets
from ...ops.roiaware_pool3d import roiaware_pool3d_utils
from ...utils.spconv_utils import spconv
from .roi_head_template import RoIHeadTemplate


class PartA2FCHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        pool_cfg = self.model_cfg.ROI_AWARE_POOL
        c0 = pool_cfg.NUM_FEATURES // 2
        block = self.post_act_block
        self.conv_part = spconv.SparseSequential(block(4, 64, 3, padding=1, indice_key='rcnn_subm1'),
                                                 block(64, c0, 3, padding=1, indice_key='rcnn_subm1_1'))
        self.conv_rpn = spconv.SparseSequential(block(input_channels, 64, 3, padding=1, indice_key='rcnn_subm2'),
                                                block(64, c0, 3, padding=1, indice_key='rcnn_subm1_2'))
        pre = pool_cfg.NUM_FEATURES * pool_cfg.POOL_SIZE ** 3
        shared = []
        n_fc = len(self.model_cfg.SHARED_FC)
        for k, c in enumerate(self.model_cfg.SHARED_FC):
            shared += [nn.Conv1d(pre, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            pre = c
            if k != n_fc - 1 and self.model_cfg.DP_RATIO > 0:
                shared.append(nn.Dropout(self.model_cfg.DP_RATIO))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.cls_layers = self.make_fc_layers(input_channels=pre, output_channels=self.num_class,
                                              fc_list=self.model_cfg.CLS_FC)
        self.reg_layers = self.make_fc_layers(input_channels=pre, output_channels=self.box_coder.code_size * self.num_class,
                                              fc_list=self.model_cfg.REG_FC)
        self.roiaware_pool3d_layer = roiaware_pool3d_utils.RoIAwarePool3d(
            out_size=pool_cfg.POOL_SIZE, max_pts_each_voxel=pool_cfg.MAX_POINTS_PER_VOXEL)
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        init = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_, 'normal': nn.init.normal_}[weight_init]
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init(m.weight, mean=0, std=0.001)
                else:
                    init(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.reg_layers[-1].weight, mean=0, std=0.001)

    @staticmethod
    def post_act_block(in_channels, out_channels, kernel_size, indice_key, stride=1, padding=0, conv_type='subm'):
        if conv_type == 'subm':
            conv = spconv.SubMConv3d(in_channels, out_channels, kernel_size, bias=False, indice_key=indice_key)
        elif conv_type == 'spconv':
            conv = spconv.SparseConv3d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=False,
                                       indice_key=indice_key)
        elif conv_type == 'inverseconv':
            conv = spconv.SparseInverseConv3d(in_channels, out_channels, kernel_size, indice_key=indice_key, bias=False)
        else:
            raise NotImplementedError(conv_type)
        return spconv.SparseSequential(conv, nn.BatchNorm1d(out_channels, eps=1e-3, momentum=0.01), nn.ReLU())

    def roiaware_pool(self, batch_dict):
        """-> pooled part features (B*N, o, o, o, 4) [avg of (part offset | xyz, score)], pooled point features
        (B*N, o, o, o, C) [max]; points below SEG_MASK_SCORE_THRESH contribute zero part offsets"""
        batch_size = batch_dict['batch_size']
        batch_idx = batch_dict['point_coords'][:, 0]
        xyz = batch_dict['point_coords'][:, 1:4]
        part = self.part_features(batch_dict)
        feats = batch_dict['point_features']
        rois = batch_dict['rois']
        pooled_part, pooled_rpn = [], []
        for b in range(batch_size):
            m = batch_idx == b
            cur_xyz, cur_roi = xyz[m].contiguous(), rois[b][:, 0:7].contiguous()
            pooled_part.append(self.roiaware_pool3d_layer(cur_roi, cur_xyz, part[m].contiguous(), pool_method='avg'))
            pooled_rpn.append(self.roiaware_pool3d_layer(cur_roi, cur_xyz, feats[m].contiguous(), pool_method='max'))
        return torch.cat(pooled_part, dim=0), torch.cat(pooled_rpn, dim=0)

    def part_features(self, batch_dict):
        """(N, 4): part offsets (xyz with DISABLE_PART), zeroed below SEG_MASK_SCORE_THRESH, and the detached score"""
        score = batch_dict['point_cls_scores'].view(-1, 1).detach()
        lead = batch_dict['point_coords'][:, 1:4] if self.model_cfg.get('DISABLE_PART', False) else batch_dict['point_part_offset']
        lead = torch.where(score < self.model_cfg.SEG_MASK_SCORE_THRESH, torch.zeros_like(lead), lead)
        return torch.cat((lead, score), dim=1)

    def roiaware_pool_sparse(self, batch_dict):
        """-> (coords (T,4) i32, part rows (T,4), point-feature rows (T,C)) exactly as `pooled_part.sum(-1).nonzero()` and the
        gather of roiaware_pool's two grids give them, or None when this call belongs to the dense route"""
        pool = self.roiaware_pool3d_layer
        if not roiaware_sparse.ENABLED or self.model_cfg.get('DISABLE_PART', False) or not roiaware_sparse.supported(pool.out_size):
            return None
        rois = batch_dict['rois'][..., 0:7]
        if rois.shape[0] * rois.shape[1] == 0:
            return None
        coords = batch_dict['point_coords']
        frame, xyz = coords[:, 0].contiguous(), coords[:, 1:4]
        part, feats = self.part_features(batch_dict), batch_dict['point_features']
        # UNetV2's rows are grouped by frame; whether they are rides in the pooling's read-back, and rows that are not are
        # sorted stably by frame once
        ungrouped = (frame[1:] < frame[:-1]).any().view(1)
        for _ in range(2):
            seen = []
            out = roiaware_pool3d_utils.roiaware_pool_sparse(
                rois, xyz, frame_offsets(frame.view(-1, 1), batch_dict['batch_size']), part, feats, pool.out_size,
                pool.max_pts_each_voxel, extra_flags=ungrouped, extra_out=seen)
            if not seen[0]:
                break
            order = torch.sort(frame, stable=True)[1]
            frame, xyz, part, feats = frame[order], xyz[order], part[order], feats[order]
            ungrouped = torch.zeros_like(ungrouped)
        if out is None or out[0].shape[0] < 3:
            return None
        return out[0], out[1], out[2]

    @staticmethod
    def fake_sparse_idx(sparse_idx, batch_size_rcnn):
        """fewer than 3 occupied cells in the whole batch: cell (0,0,0) of every RoI stands in (BatchNorm needs values)"""
        z = sparse_idx.new_zeros((batch_size_rcnn, 3))
        return torch.cat((torch.arange(batch_size_rcnn, device=z.device).type_as(z).view(-1, 1), z), dim=1)

    @staticmethod
    def run_fc(layers, x):
        """the reference's kernel-size-1 Conv1d stacks on (n, C, 1) as row GEMMs on (n, C): same parameters, same arithmetic per
        output, but reproducible - the vendor convolution the Conv1d module reaches sums its K = NUM_FEATURES * POOL_SIZE^3
        products in an order that changes from launch to launch, forward and backward (two identical calls differ in the last
        bits), which a GEMM through F.linear does not"""
        for m in layers:
            if isinstance(m, nn.Conv1d):
                assert m.kernel_size == (1,) and m.stride == (1,) and m.groups == 1
                x = torch.nn.functional.linear(x, m.weight.squeeze(2), m.bias)
            else:
                x = m(x)
        return x

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict,
                                           nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)        # injected RoI sample (tests / measurements)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']

        rows = self.roiaware_pool_sparse(batch_dict)
        if rows is not None:
            coords, part_rows, rpn_rows = rows
            n_rcnn = batch_dict['rois'].shape[0] * batch_dict['rois'].shape[1]
            sparse_shape = list(roiaware_sparse.out_xyz(self.roiaware_pool3d_layer.out_size))
        else:
            pooled_part, pooled_rpn = self.roiaware_pool(batch_dict)
            n_rcnn = pooled_part.shape[0]
            sparse_shape = [int(v) for v in pooled_part.shape[1:4]]
            sparse_idx = pooled_part.sum(dim=-1).nonzero()              # (cells, 4): roi, x, y, z — lexicographic
            if sparse_idx.shape[0] < 3:
                sparse_idx = self.fake_sparse_idx(sparse_idx, n_rcnn)
                if self.training:                                        # nothing to learn from such a batch
                    targets_dict['rcnn_cls_labels'].fill_(-1)
                    targets_dict['reg_valid_mask'].fill_(-1)
            r, x, y, z = sparse_idx.unbind(1)
            coords = sparse_idx.int().contiguous()
            part_rows, rpn_rows = pooled_part[r, x, y, z], pooled_rpn[r, x, y, z]
        batch_dict['roi_grid_coords'] = coords
        part = spconv.SparseConvTensor(part_rows, coords, sparse_shape, n_rcnn)
        rpn = spconv.SparseConvTensor(rpn_rows, coords, sparse_shape, n_rcnn)
        x_part = self.conv_part(part)
        x_rpn = self.conv_rpn(rpn)
        merged = torch.cat((x_rpn.features, x_part.features), dim=1)
        shared = spconv.SparseConvTensor(merged, coords, sparse_shape, n_rcnn).dense().view(n_rcnn, -1)
        shared = self.run_fc(self.shared_fc_layer, shared)
        rcnn_cls = self.run_fc(self.cls_layers, shared)                 # (n, 1): the reference's transpose + squeeze of (n, 1, 1)
        rcnn_reg = self.run_fc(self.reg_layers, shared)

        if not self.training:
            cls_preds, box_preds = self.generate_predicted_boxes(batch_size=batch_dict['batch_size'], rois=batch_dict['rois'],
                                                                 cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['batch_cls_preds'] = cls_preds
            batch_dict['batch_box_preds'] = box_preds
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
