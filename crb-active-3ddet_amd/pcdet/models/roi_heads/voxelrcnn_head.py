"""VoxelRCNNHead (pcdet/models/roi_heads/voxelrcnn_head.py:8-262): second stage of Voxel R-CNN. A G^3 grid under every first-stage
proposal pools the 3D backbone's own sparse feature levels (voxel query + NeighborVoxelSAModuleMSG per FEATURES_SOURCE level),
three nn.Linear stacks refine class score and box.

The grid points come from one launch (crb_roi_grid_points); every level is pooled on the HIP route of
pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules (site hash instead of the reference's dense (B, Z, Y, X) index, no grouped
tensors) when the tensors live on the device, on the torch route otherwise. The pooled rows are (B*R, G^3, sum C_out): already the
order the first Linear(G^3 * C, 256) expects. In eval the Linear + BatchNorm1d pairs run folded (fold_utils). Losses are
RoIHeadTemplate.get_loss (crb_rcnn_loss); tb_dict values are detached tensors."""
import torch
import torch.nn as nn

from ...ops.pointnet2.pointnet2_stack import voxel_pool_modules as voxelpool_stack_modules
from ...utils import common_utils
from ...utils.fold_utils import fold_conv_bn
from .pvrcnn_head import PVRCNNHead
from .roi_head_template import RoIHeadTemplate


class VoxelRCNNHead(RoIHeadTemplate):
    def __init__(self, backbone_channels, model_cfg, point_cloud_range, voxel_size, num_class=1, **kwargs):
        super().__init__(num_class=num_class, model_cfg=model_cfg)
        self.model_cfg = model_cfg
        self.pool_cfg = model_cfg.ROI_GRID_POOL
        layer_cfg = self.pool_cfg.POOL_LAYERS
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        if model_cfg.LOSS_CONFIG.get('GRID_3D_IOU_LOSS', False):
            raise NotImplementedError('GRID_3D_IOU_LOSS')

        c_out = 0
        self.roi_grid_pool_layers = nn.ModuleList()
        for src_name in self.pool_cfg.FEATURES_SOURCE:
            mlps = [[backbone_channels[src_name]] + list(m) for m in layer_cfg[src_name].MLPS]    # (the config is left as it is)
            self.roi_grid_pool_layers.append(voxelpool_stack_modules.NeighborVoxelSAModuleMSG(
                query_ranges=layer_cfg[src_name].QUERY_RANGES, nsamples=layer_cfg[src_name].NSAMPLE,
                radii=layer_cfg[src_name].POOL_RADIUS, mlps=mlps, pool_method=layer_cfg[src_name].POOL_METHOD))
            c_out += sum(x[-1] for x in mlps)

        G = self.pool_cfg.GRID_SIZE
        pre = G * G * G * c_out

        def stack(fc_list, pre, relu_inplace=False):
            layers = []
            for k, c in enumerate(fc_list):
                layers += [nn.Linear(pre, c, bias=False), nn.BatchNorm1d(c), nn.ReLU(inplace=relu_inplace)]
                pre = c
                if k != len(fc_list) - 1 and self.model_cfg.DP_RATIO > 0:
                    layers.append(nn.Dropout(self.model_cfg.DP_RATIO))
            return nn.Sequential(*layers), pre

        self.shared_fc_layer, pre = stack(self.model_cfg.SHARED_FC, pre, relu_inplace=True)
        self.cls_fc_layers, pre_cls = stack(self.model_cfg.CLS_FC, pre)
        self.cls_pred_layer = nn.Linear(pre_cls, self.num_class, bias=True)
        # (the reference chains pre_channel through the class stack into the box stack: equal widths in every config it ships)
        self.reg_fc_layers, pre_reg = stack(self.model_cfg.REG_FC, pre_cls)
        self.reg_pred_layer = nn.Linear(pre_reg, self.box_coder.code_size * self.num_class, bias=True)
        self.init_weights()

    def init_weights(self):
        for module_list in (self.shared_fc_layer, self.cls_fc_layers, self.reg_fc_layers):
            for m in module_list.modules():
                if isinstance(m, nn.Linear):
                    nn.init.xavier_normal_(m.weight)
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.cls_pred_layer.weight, 0, 0.01)
        nn.init.constant_(self.cls_pred_layer.bias, 0)
        nn.init.normal_(self.reg_pred_layer.weight, mean=0, std=0.001)
        nn.init.constant_(self.reg_pred_layer.bias, 0)

    # ---- pooling ----------------------------------------------------------------------------------------------------
    get_global_grid_points_of_roi = PVRCNNHead.get_global_grid_points_of_roi       # crb_roi_grid_points on the device
    get_dense_grid_points = staticmethod(PVRCNNHead.get_dense_grid_points)

    def grid_voxel_coords(self, roi_grid_xyz):
        """(.., 3) grid points -> (.., 3) float [x, y, z] voxel coordinates at stride 1: the reference's expressions
        (voxelrcnn_head.py:130-134), one float `//` by a Python scalar per axis. torch's float `//` is not floorf(a / b) at voxel
        faces (it corrects the quotient by the remainder, and divides by a host scalar through its reciprocal on the device), so
        these steps stay in torch: the integer coordinates are the reference's on every device."""
        lo, vs = self.point_cloud_range, self.voxel_size
        return torch.cat([(roi_grid_xyz[..., k:k + 1] - lo[k]) // vs[k] for k in range(3)], dim=-1)

    @staticmethod
    def level_coords(grid_voxel_coords, batch_idx, stride):
        """second float step and the cast (voxelrcnn_head.py:169-171) -> (.., 4) int32 [b, x, y, z] at the level"""
        return torch.cat([batch_idx, grid_voxel_coords // stride], dim=-1).int()

    def roi_grid_pool(self, batch_dict):
        """rois (B,R,7+), multi_scale_3d_features -> (B*R, G^3, sum C_out)"""
        rois = batch_dict['rois']
        batch_size = batch_dict['batch_size']
        G = self.pool_cfg.GRID_SIZE
        with torch.no_grad():
            roi_grid_xyz, _ = self.get_global_grid_points_of_roi(rois.detach(), grid_size=G)       # (B*R, G^3, 3)
            roi_grid_xyz = roi_grid_xyz.view(batch_size, -1, 3)
            roi_grid_coords = self.grid_voxel_coords(roi_grid_xyz)
            batch_idx = torch.arange(batch_size, device=rois.device, dtype=roi_grid_xyz.dtype).view(-1, 1, 1).expand(
                -1, roi_grid_xyz.shape[1], 1)
            roi_grid_batch_cnt = torch.full((batch_size,), roi_grid_xyz.shape[1], dtype=torch.int32, device=rois.device)
        key = 'multi_scale_3d_features_post' if batch_dict.get('with_voxel_feature_transform', False) else 'multi_scale_3d_features'
        new_xyz = roi_grid_xyz.contiguous().view(-1, 3)
        pooled_list = []
        for k, src_name in enumerate(self.pool_cfg.FEATURES_SOURCE):
            stride = batch_dict['multi_scale_3d_strides'][src_name]
            sp = batch_dict[key][src_name]
            coords = sp.indices
            with torch.no_grad():
                voxel_xyz = common_utils.get_voxel_centers(coords[:, 1:4], downsample_times=stride, voxel_size=self.voxel_size,
                                                           point_cloud_range=self.point_cloud_range)
                voxel_batch_cnt = common_utils.batch_counts(coords[:, 0], batch_size)
                cur_coords = self.level_coords(roi_grid_coords, batch_idx, stride)
            pooled = self.roi_grid_pool_layers[k](
                xyz=voxel_xyz.contiguous(), xyz_batch_cnt=voxel_batch_cnt, new_xyz=new_xyz, new_xyz_batch_cnt=roi_grid_batch_cnt,
                new_coords=cur_coords.contiguous().view(-1, 4), features=sp.features.contiguous(), voxel2point_indices=sp)
            pooled_list.append(pooled.view(-1, G ** 3, pooled.shape[-1]))
        return torch.cat(pooled_list, dim=-1)

    # ---- FC stacks --------------------------------------------------------------------------------------------------
    @staticmethod
    def _run_folded(mods, x):
        """eval: Linear -> BatchNorm1d pairs as one addmm with the folded weight (cached by weight version, fold_utils)"""
        mods = list(mods)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d):
                w, shift = fold_conv_bn(m, mods[i + 1])
                x = torch.addmm(shift, x, w.t())
                i += 2
            else:
                x = m(x)
                i += 1
        return x

    def forward(self, batch_dict):
        targets_dict = self.proposal_layer(batch_dict, nms_config=self.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)        # injected RoI sample (tests / measurements)
            if targets_dict is None:
                targets_dict = self.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
        pooled = self.roi_grid_pool(batch_dict)                            # (B*R, G^3, C)
        pooled = pooled.reshape(pooled.size(0), -1)
        fast = (not self.training) and (not torch.is_grad_enabled()) and \
            not any(m.training for m in self.modules() if isinstance(m, nn.BatchNorm1d))
        run = self._run_folded if fast else (lambda mods, x: mods(x))
        shared = run(self.shared_fc_layer, pooled)
        rcnn_cls = self.cls_pred_layer(run(self.cls_fc_layers, shared))
        rcnn_reg = self.reg_pred_layer(run(self.reg_fc_layers, shared))
        if not self.training:
            batch_cls_preds, batch_box_preds = self.generate_predicted_boxes(
                batch_size=batch_dict['batch_size'], rois=batch_dict['rois'], cls_preds=rcnn_cls, box_preds=rcnn_reg)
            batch_dict['batch_cls_preds'] = batch_cls_preds
            batch_dict['batch_box_preds'] = batch_box_preds
            batch_dict['cls_preds_normalized'] = False
        else:
            targets_dict['rcnn_cls'] = rcnn_cls
            targets_dict['rcnn_reg'] = rcnn_reg
            self.forward_ret_dict = targets_dict
        return batch_dict
