"""SECONDHead (pcdet/models/roi_heads/second_head.py:7-178): second stage of SECOND-IoU. A rotated G x G grid of BEV features is
pooled under every first-stage proposal, a shared FC stack and the IoU branch predict the proposal's IoU with its ground truth, the
detector re-scores the boxes with it.

The pooling is one HIP launch over all frames on the NHWC map (crbhip.roi_bev_pool; the reference's per-frame affine_grid +
grid_sample on an NCHW expand is kept as the torch path of CPU tensors and as the definition). The kernel's rows are (grid point,
channel) ordered, the stored first FC weight is (channel, grid point) ordered as in the reference: the weight's columns are
re-ordered for the product (a differentiable view in training, a cached folded copy in eval), the parameter itself never.
tb_dict values are detached 0-dim tensors (no .item() synchronisation in the training step)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...utils import loss_utils
from ...utils.fold_utils import fold_conv_bn
from . import roi_head_template
from .pvrcnn_head import PVRCNNHead, _gc_order
from .roi_head_template import RoIHeadTemplate


class SECONDHead(RoIHeadTemplate):
    reads_spatial_features_2d = True      # roi_grid_pool: the detector keeps the BEV backbone's concatenated map (no deferral)

    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        G = self.model_cfg.ROI_GRID_POOL.GRID_SIZE
        pre = self.model_cfg.ROI_GRID_POOL.IN_CHANNEL * G * G
        shared = []
        n_fc = len(self.model_cfg.SHARED_FC)
        for k, c in enumerate(self.model_cfg.SHARED_FC):
            shared += [nn.Conv1d(pre, c, kernel_size=1, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            pre = c
            if k != n_fc - 1 and self.model_cfg.DP_RATIO > 0:
                shared.append(nn.Dropout(self.model_cfg.DP_RATIO))
        self.shared_fc_layer = nn.Sequential(*shared)
        self.iou_layers = self.make_fc_layers(input_channels=pre, output_channels=1, fc_list=self.model_cfg.IOU_FC)
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

    # ---- pooling ----------------------------------------------------------------------------------------------------
    def _pool_geometry(self, batch_dict):
        ds = batch_dict['dataset_cfg']
        ratio = self.model_cfg.ROI_GRID_POOL.DOWNSAMPLE_RATIO
        vs = ds.DATA_PROCESSOR[-1].VOXEL_SIZE
        return float(ds.POINT_CLOUD_RANGE[0]), float(ds.POINT_CLOUD_RANGE[1]), float(vs[0] * ratio), float(vs[1] * ratio)

    def roi_grid_pool(self, batch_dict):
        """rois (B,R,7+), spatial_features_2d (B,C,H,W) -> (B*R, C, G, G): channel c, grid row j, grid column i, the reference's
        values. Device tensors: the kernel, whose (B*R, G*G, C) rows come back as a permuted view; host tensors: roi_grid_pool_torch."""
        rois = batch_dict['rois'].detach()
        feats = batch_dict['spatial_features_2d'].detach()
        G = self.model_cfg.ROI_GRID_POOL.GRID_SIZE
        x_min, y_min, cell_x, cell_y = self._pool_geometry(batch_dict)
        if not feats.is_cuda:
            return roi_grid_pool_torch(feats, rois, G, x_min, y_min, cell_x, cell_y)
        from crbhip import roi_bev_pool
        nhwc = feats.permute(0, 2, 3, 1)            # the backbone's map is channels_last: a view; an NCHW map is copied to NHWC here
        rows = roi_bev_pool.roi_bev_pool(nhwc.contiguous().float(), rois, G, x_min, y_min, cell_x, cell_y)
        return roi_bev_pool.as_nchw(rows, G)

    # ---- FC stacks on rows ------------------------------------------------------------------------------------------
    @staticmethod
    def _run_rows(mods, x):
        """Conv1d(k=1) / BatchNorm1d / ReLU / Dropout modules on (N, C) rows: a length-1 convolution is rows @ W^T (a GEMM, not a
        convolution solver's choice); BatchNorm1d takes its statistics over N either way"""
        for m in mods:
            if isinstance(m, nn.Conv1d):
                assert m.kernel_size == (1,) and m.stride == (1,) and m.padding == (0,) and m.groups == 1
                x = F.linear(x, m.weight.squeeze(-1), m.bias)
            else:
                x = m(x)
        return x

    def _first_weight_rows(self, pooled):
        """pooled (N, C, G, G) -> (rows (N, K), column permutation flag): the kernel's view flattens (g, c)-ordered without a copy"""
        n, c, g, _ = pooled.shape
        as_rows = pooled.permute(0, 2, 3, 1)
        if as_rows.is_contiguous():
            return as_rows.reshape(n, g * g * c), True
        return pooled.reshape(n, c * g * g), False

    def _iou_branch(self, pooled):
        """pooled (N, C, G, G) -> rcnn_iou (N, 1)"""
        mods = list(self.shared_fc_layer)
        n, c, g, _ = pooled.shape
        g2 = g * g
        x, gc = self._first_weight_rows(pooled)
        conv0 = mods[0]
        fast = (not self.training) and (not torch.is_grad_enabled()) and \
            not any(m.training for m in self.modules() if isinstance(m, nn.BatchNorm1d))
        if fast:
            # eval: Conv1d + BatchNorm1d folded (cached by weight version, fold_utils); the first weight's columns re-ordered inside
            # the cache when the rows are (g, c)-ordered
            w0, b0 = fold_conv_bn(conv0, mods[1], _gc_order(c, g2)) if gc else fold_conv_bn(conv0, mods[1])
            x = torch.addmm(b0, x, w0.reshape(w0.shape[0], -1).t()).unsqueeze(-1)
            x = PVRCNNHead._run_folded(mods[2:], x)
            return PVRCNNHead._run_folded(list(self.iou_layers), x).squeeze(-1)
        w = conv0.weight
        w = w.view(w.shape[0], c, g2).permute(0, 2, 1).reshape(w.shape[0], g2 * c) if gc else w.squeeze(-1)
        x = F.linear(x, w, conv0.bias)
        x = self._run_rows(mods[1:], x)
        return self._run_rows(list(self.iou_layers), x)

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict, nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)        # injected RoI sample (tests / measurements)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled = self.roi_grid_pool(batch_dict)                            # (B*R, C, G, G)
        rcnn_iou = self._iou_branch(pooled)                                # (B*R, 1)
        if not self.training:
            batch_dict['batch_cls_preds'] = rcnn_iou.view(batch_dict['batch_size'], -1, rcnn_iou.shape[-1])
            batch_dict['batch_box_preds'] = batch_dict['rois']
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_iou'] = rcnn_iou
            self.forward_ret_dict = targets_dict
        return batch_dict

    # ---- loss -------------------------------------------------------------------------------------------------------
    def get_loss(self, tb_dict=None):
        tb_dict = {} if tb_dict is None else tb_dict
        rcnn_loss_iou, iou_tb = self.get_box_iou_layer_loss(self.forward_ret_dict)
        tb_dict.update(iou_tb)
        tb_dict['rcnn_loss'] = rcnn_loss_iou.detach()
        return rcnn_loss_iou, tb_dict

    def get_box_iou_layer_loss(self, forward_ret_dict):
        loss_cfgs = self.model_cfg.LOSS_CONFIG
        rcnn_iou = forward_ret_dict['rcnn_iou'].view(-1)
        labels = forward_ret_dict['rcnn_cls_labels'].view(-1).float()
        kind, weight = loss_cfgs.IOU_LOSS, loss_cfgs.LOSS_WEIGHTS['rcnn_iou_weight']
        if kind == 'focalbce':
            # the reference calls loss_utils.sigmoid_focal_cls_loss here (second_head.py:169), which its tree does not define
            raise NotImplementedError('IOU_LOSS focalbce')
        if kind not in ('BinaryCrossEntropy', 'L2', 'smoothL1'):
            raise NotImplementedError(kind)
        if roi_head_template.FUSED_LOSS and rcnn_iou.is_cuda:
            from crbhip import rcnn_loss
            loss, _ = rcnn_loss.rcnn_iou_loss(rcnn_iou, labels, kind, weight)
            return loss, {'rcnn_loss_iou': loss.detach()}
        if kind == 'BinaryCrossEntropy':
            batch_loss = F.binary_cross_entropy_with_logits(rcnn_iou, labels, reduction='none')
        elif kind == 'L2':
            batch_loss = F.mse_loss(rcnn_iou, labels, reduction='none')
        else:
            batch_loss = loss_utils.WeightedSmoothL1Loss.smooth_l1_loss(rcnn_iou - labels, 1.0 / 9.0)
        valid = (labels >= 0).float()
        loss = (batch_loss * valid).sum() / torch.clamp(valid.sum(), min=1.0) * weight
        return loss, {'rcnn_loss_iou': loss.detach()}


def roi_grid_pool_torch(feats, rois, grid_size, x_min, y_min, cell_x, cell_y):
    """the reference's pooling restated on torch ops (second_head.py:77-108): feats (B,C,H,W) in any memory format, rois (B,R,7+)
    -> (B*R, C, G, G). affine_grid / grid_sample with torch's defaults (align_corners=False, bilinear, zeros)."""
    B, C, H, W = feats.shape
    out = []
    for b in range(B):
        r = rois[b]
        x1 = (r[:, 0] - r[:, 3] / 2 - x_min) / cell_x
        x2 = (r[:, 0] + r[:, 3] / 2 - x_min) / cell_x
        y1 = (r[:, 1] - r[:, 4] / 2 - y_min) / cell_y
        y2 = (r[:, 1] + r[:, 4] / 2 - y_min) / cell_y
        c, s = torch.cos(r[:, 6]), torch.sin(r[:, 6])
        theta = torch.stack(((x2 - x1) / (W - 1) * c, (x2 - x1) / (W - 1) * (-s), (x1 + x2 - W + 1) / (W - 1),
                             (y2 - y1) / (H - 1) * s, (y2 - y1) / (H - 1) * c, (y1 + y2 - H + 1) / (H - 1)), dim=1).view(-1, 2, 3)
        theta = theta.to(feats.dtype)
        grid = F.affine_grid(theta, torch.Size((r.shape[0], C, grid_size, grid_size)), align_corners=False)
        out.append(F.grid_sample(feats[b].unsqueeze(0).expand(r.shape[0], C, H, W), grid, mode='bilinear', padding_mode='zeros',
                                 align_corners=False))
    return torch.cat(out, dim=0)
