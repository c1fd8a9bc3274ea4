"""PVRCNNHead (pcdet/models/roi_heads/pvrcnn_head.py:9-242): RoI-grid pooling of keypoint features (HIP ball query +
grouping), shared FC, class / box branches, MC-dropout passes in eval (SAMPLING_ROUND), and with ROI_HEAD.LOSS_NET the LLAL
loss-prediction module on the post-ReLU outputs of the shared FC layers (pvrcnn_head.py:163-180)."""
import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_stack import pointnet2_modules as pointnet2_stack_modules
from ...utils import common_utils
from ...utils.fold_utils import fold_conv_bn
from .loss_net import LossNet
from .roi_head_template import RoIHeadTemplate


_GC_ORDER = {}


def _gc_order(c, g3):
    """fold_conv_bn transform: first FC weight (256, C*G^3, 1) from (c*G^3 + g) to (g*C + c) column order"""
    key = (c, g3)
    if key not in _GC_ORDER:
        def gc_order(w, b, c=c, g3=g3):
            return w.reshape(w.shape[0], c, g3).permute(0, 2, 1).reshape(w.shape[0], g3 * c).contiguous(), b.contiguous()
        gc_order.__name__ = 'gc_order_%d_%d' % key
        _GC_ORDER[key] = gc_order
    return _GC_ORDER[key]


# grid points of the RoI-grid pooling as one launch; CRB_ROI_GRID_POINTS_FUSED=0 = the torch expressions (A/B, test reference)
FUSED_GRID_POINTS = __import__('os').environ.get('CRB_ROI_GRID_POINTS_FUSED', '1') == '1'


class PVRCNNHead(RoIHeadTemplate):
    def __init__(self, input_channels, model_cfg, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        self.roi_grid_pool_layer, num_c_out = pointnet2_stack_modules.build_local_aggregation_module(
            input_channels=input_channels, config=self.model_cfg.ROI_GRID_POOL)
        G = self.model_cfg.ROI_GRID_POOL.GRID_SIZE
        pre = G * G * G * num_c_out
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
        if model_cfg.get('LOSS_NET', None):
            self.loss_net = LossNet(model_cfg=model_cfg)
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

    def predict_loss(self, latents, batch_size):
        """LossNet on the ReLU outputs of the shared FC layers -> (B, 1). Runs on every forward, also while the module is frozen
        (OPTIMIZATION.LOSS_NET_SKIP): its BatchNorm layers update their running statistics in train mode like the reference's."""
        rows = latents[0].shape[0]
        per = self.loss_net.rows_per_frame
        if rows != batch_size * per:
            raise ValueError('ROI_HEAD.LOSS_NET needs exactly TARGET_CONFIG.ROI_PER_IMAGE = %d RoIs per frame, got %d rows for %d '
                             'frames (in eval the RoI count per frame is NMS_CONFIG.TEST.NMS_POST_MAXSIZE = %d)' %
                             (per, rows, batch_size, self.model_cfg.NMS_CONFIG.TEST.NMS_POST_MAXSIZE))
        return self.loss_net(latents, batch_size=batch_size)

    def roi_grid_pool(self, batch_dict):
        """rois (B,N,7), keypoints -> (B*N, G^3, C)"""
        batch_size = batch_dict['batch_size']
        rois = batch_dict['rois']
        point_coords = batch_dict['point_coords']
        point_features = batch_dict['point_features'] * batch_dict['point_cls_scores'].view(-1, 1)
        G = self.model_cfg.ROI_GRID_POOL.GRID_SIZE
        grid_pts, _ = self.get_global_grid_points_of_roi(rois, grid_size=G)
        grid_pts = grid_pts.view(batch_size, -1, 3)
        xyz = point_coords[:, 1:4]
        xyz_batch_cnt = common_utils.batch_counts(point_coords[:, 0], batch_size)
        new_xyz = grid_pts.view(-1, 3)
        new_xyz_batch_cnt = xyz_batch_cnt.new_full((batch_size,), grid_pts.shape[1])
        _, pooled = self.roi_grid_pool_layer(xyz=xyz.contiguous(), xyz_batch_cnt=xyz_batch_cnt, new_xyz=new_xyz.contiguous(),
                                             new_xyz_batch_cnt=new_xyz_batch_cnt, features=point_features.contiguous(),
                                             query_group=G ** 3)      # the G^3 grid points of a RoI are consecutive rows
        return pooled.view(-1, G ** 3, pooled.shape[-1])

    def get_global_grid_points_of_roi(self, rois, grid_size):
        rois = rois.view(-1, rois.shape[-1])
        n = rois.shape[0]
        if FUSED_GRID_POINTS and rois.is_cuda and not rois.requires_grad:
            # one launch (csrc/rcnn_loss.hip crb_roi_grid_points); the local points are not formed (no caller reads them)
            from crbhip import lib, check, ptr, cur_stream
            r = rois.detach().contiguous().float()
            glob = torch.empty((n, grid_size ** 3, 3), dtype=torch.float32, device=r.device)
            check(lib.crb_roi_grid_points(ptr(r), int(r.shape[1]), n, int(grid_size), ptr(glob), cur_stream(r.device)), 'crb_roi_grid_points')
            return glob, None
        local = self.get_dense_grid_points(rois, n, grid_size)
        glob = common_utils.rotate_points_along_z(local.clone(), rois[:, 6]).squeeze(dim=1)
        glob = glob + rois[:, 0:3].unsqueeze(dim=1)
        return glob, local

    @staticmethod
    def get_dense_grid_points(rois, batch_size_rcnn, grid_size):
        g = torch.arange(grid_size, device=rois.device)
        dense_idx = torch.stack(torch.meshgrid(g, g, g, indexing='ij'), dim=-1).view(1, -1, 3).float()   # x,y,z fastest z
        size = rois.view(batch_size_rcnn, -1)[:, 3:6].unsqueeze(1)
        return (dense_idx + 0.5) / grid_size * size - size / 2

    # training / grad path: the reference flattens the pooled tensor channel-major (pvrcnn_head.py:172-176: permute(0, 2, 1) +
    # contiguous of a 226 MB tensor, and the same copy for its gradient). Re-ordering the COLUMNS of the first FC weight instead
    # (28 MB, differentiable) leaves the pooled rows where the pooling wrote them: same products, another K order in the GEMM.
    WEIGHT_SIDE_FLATTEN = __import__('os').environ.get('CRB_ROI_WEIGHT_SIDE_FLATTEN', '1') == '1'

    def _heads_pooled(self, pooled, taps=None):
        """pooled (BN, G^3, C) -> shared, rcnn_cls, rcnn_reg without the channel-major copy of the pooled tensor; `taps` (a list)
        receives the output of every ReLU of shared_fc_layer (the LossNet latents)"""
        mods = list(self.shared_fc_layer)
        n, g3, c = pooled.shape
        conv0 = mods[0]
        if not (self.WEIGHT_SIDE_FLATTEN and isinstance(conv0, nn.Conv1d) and conv0.kernel_size == (1,) and
                conv0.in_channels == g3 * c):
            return self._heads(pooled.permute(0, 2, 1).contiguous().view(n, -1, 1), taps)
        w = conv0.weight.view(conv0.out_channels, c, g3).permute(0, 2, 1).reshape(conv0.out_channels, g3 * c)
        x = torch.nn.functional.linear(pooled.reshape(n, g3 * c), w, conv0.bias).unsqueeze(-1)     # (BN, 256, 1)
        for m in mods[1:]:
            x = m(x)
            if taps is not None and isinstance(m, nn.ReLU):
                taps.append(x)
        shared = x
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        return shared, rcnn_cls, rcnn_reg

    def _heads(self, pooled_flat, taps=None):
        if taps is None:
            shared = self.shared_fc_layer(pooled_flat)
        else:
            shared = pooled_flat
            for m in self.shared_fc_layer:
                shared = m(shared)
                if isinstance(m, nn.ReLU):
                    taps.append(shared)
        rcnn_cls = self.cls_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self.reg_layers(shared).transpose(1, 2).contiguous().squeeze(dim=1)
        return shared, rcnn_cls, rcnn_reg

    # ---- inference fast path (same values up to f32 rounding) -------------------------------------------------------
    @staticmethod
    def _run_folded(mods, x, taps=None):
        """Conv1d(k=1) -> BatchNorm1d(eval) pairs as one folded conv; ReLU / Dropout modules run as they are (Dropout
        stays stochastic when the CRB strategy switched it to train mode); `taps` receives every ReLU output"""
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Conv1d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d):
                w, shift = fold_conv_bn(m, mods[i + 1])
                if x.shape[-1] == 1 and m.kernel_size == (1,) and m.stride == (1,) and m.padding == (0,) and m.groups == 1:
                    # a length-1 signal: the layer is rows @ W^T + shift. As a convolution it goes to MIOpen, whose solver choice for
                    # these (rows, 256, 1) problems depends on process state (workspace it is offered, what ran before): the RoI
                    # head's outputs came out 1.6e-8 apart between two schedules of the same forward pass inside the full test suite
                    x = torch.addmm(shift, x.squeeze(-1), w.squeeze(-1).t()).unsqueeze(-1)
                else:
                    x = torch.nn.functional.conv1d(x, w, shift)
                i += 2
            elif isinstance(m, nn.Conv1d) and x.shape[-1] == 1 and m.kernel_size == (1,) and m.stride == (1,) and m.padding == (0,) and \
                    m.groups == 1 and not torch.is_grad_enabled():
                w2 = m.weight.squeeze(-1)
                x = (x.squeeze(-1) @ w2.t() if m.bias is None else torch.addmm(m.bias, x.squeeze(-1), w2.t())).unsqueeze(-1)
                i += 1
            else:
                x = m(x)
                if taps is not None and isinstance(m, nn.ReLU):
                    taps.append(x)
                i += 1
        return x

    def _heads_eval(self, pooled, rounds, taps=None):
        """MC-dropout passes of pvrcnn_head.py:187-202 on pooled (BN, G^3, C) features.
        * Everything before the first Dropout of shared_fc_layer is deterministic in eval mode, so the 27648->256 layer
          (7 M MACs per RoI) runs once instead of `rounds` times. Its weight is re-ordered once (cached) from the reference's
          channel-major flattening (c*G^3 + g) to the pooled tensor's own (g*C + c) order: no permute().contiguous() copy of
          the 226 MB pooled tensor.
        * The `rounds` passes only differ by their dropout masks: they run as ONE batch of rounds*BN rows through the
          remaining layers (independent masks per row and element, as in `rounds` separate calls).
        * `taps` receives the ReLU outputs of the first pass (the LossNet latents): the deterministic prefix and the rows of pass 0
          of the remaining layers, no extra FC pass."""
        mods = list(self.shared_fc_layer)
        first_dp = next((k for k, m in enumerate(mods) if isinstance(m, nn.Dropout)), len(mods))
        n, g3, c = pooled.shape
        conv0, bn0 = mods[0], mods[1]
        if isinstance(conv0, nn.Conv1d) and isinstance(bn0, nn.BatchNorm1d) and conv0.in_channels == g3 * c:
            w0, b0 = fold_conv_bn(conv0, bn0, _gc_order(c, g3))
            x = torch.addmm(b0, pooled.reshape(n, g3 * c), w0.t()).unsqueeze(-1)           # (BN, 256, 1)
            prefix = self._run_folded(mods[2:first_dp], x, taps)
        else:
            prefix = self._run_folded(mods[:first_dp], pooled.permute(0, 2, 1).contiguous().view(n, -1, 1), taps)
        r = max(1, rounds)
        stacked = prefix.repeat(r, 1, 1) if r > 1 else prefix                             # (r*BN, 256, 1)
        later = [] if taps is not None else None
        shared = self._run_folded(mods[first_dp:], stacked, later)
        if taps is not None:
            taps.extend(t if r == 1 else t[:n] for t in later)
        rcnn_cls = self._run_folded(list(self.cls_layers), shared).transpose(1, 2).contiguous().squeeze(dim=1)
        rcnn_reg = self._run_folded(list(self.reg_layers), shared).transpose(1, 2).contiguous().squeeze(dim=1)
        return [(shared[k * n:(k + 1) * n], rcnn_cls[k * n:(k + 1) * n], rcnn_reg[k * n:(k + 1) * n]) for k in range(r)]

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict,
                                           nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)        # injected RoI sample (tests / measurements)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled = self.roi_grid_pool(batch_dict)                                   # (BN, G^3, C)
        n = pooled.shape[0]
        taps = [] if hasattr(self, 'loss_net') else None
        fast = (not self.training) and (not torch.is_grad_enabled()) and \
            not any(m.training for m in self.modules() if isinstance(m, nn.BatchNorm1d))
        # the reference's channel-major flattening (a 226 MB copy at bs=16) is only needed off the fast path
        pooled_flat = None
        if fast:
            rounds = self.model_cfg.get('SAMPLING_ROUND', None) or 1
            passes = self._heads_eval(pooled, rounds, taps)
            shared, rcnn_cls, rcnn_reg = passes[-1]
        elif self.training:
            shared, rcnn_cls, rcnn_reg = self._heads_pooled(pooled, taps)
        else:
            pooled_flat = pooled.permute(0, 2, 1).contiguous().view(n, -1, 1)                        # (BN, C*G^3, 1)
            shared, rcnn_cls, rcnn_reg = self._heads(pooled_flat, taps)
        loss_predictions = self.predict_loss(taps, batch_dict['batch_size']) if taps is not None else None
        if not self.training:
            rounds = self.model_cfg.get('SAMPLING_ROUND', None)
            if rounds:
                if fast:
                    cls_list, reg_list = [p[1] for p in passes], [p[2] for p in passes]
                else:
                    cls_list, reg_list = [rcnn_cls], [rcnn_reg]
                    for _ in range(rounds - 1):
                        shared, rcnn_cls, rcnn_reg = self._heads(pooled_flat)
                        cls_list.append(rcnn_cls)
                        reg_list.append(rcnn_reg)
                batch_dict['rcnn_cls'] = torch.stack(cls_list, 0)
                batch_dict['rcnn_reg'] = torch.stack(reg_list, 0)
            elif self.model_cfg.get('EMBEDDING_REQUIRED', None):
                batch_dict['shared_features'] = shared
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['batch_cls_preds'] = batch_cls_preds
            batch_dict['batch_box_preds'] = batch_box_preds
            batch_dict['cls_preds_normalized'] = False
            if loss_predictions is not None:
                batch_dict['loss_predictions'] = loss_predictions
        else:
            if loss_predictions is not None:
                targets_dict['loss_predictions'] = loss_predictions
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
            batch_dict['rcnn_cls'] = rcnn_cls
            batch_dict['rcnn_reg'] = rcnn_reg
        return batch_dict
