"""PointIntraPartOffsetHead (pcdet/models/dense_heads/point_intra_part_head.py:7-127): foreground segmentation and intra-object part
locations of every voxel centre, the point head of Part-A2; with TARGET_CONFIG.BOX_CODER (PartA2_free.yaml) also a box per point, which
makes the head the proposal generator of the anchor-free Part-A2. Targets and losses run as the launches of csrc/part_head.hip
(crbhip/part_head.py) and, with the box branch, of csrc/point_box.hip (crbhip/point_box.py). Of PointResidualCoder only
`use_mean_size: True` is built (every yaml of the reference uses it); `use_mean_size: False` raises NotImplementedError.

What the box branch leaves for RoIHeadTemplate.proposal_layer (when not training, or with predict_boxes_when_training):
  host route   (host tensors, f64, CRB_POINT_HEAD_FUSED=0 / CRB_PART_HEAD_FUSED=0): the reference's stacked batch_cls_preds (N,C),
               batch_box_preds (N,7), batch_index (N)
  device route the dense, frame-padded batch_cls_preds (B,Amax,C) (-inf past a frame's rows), batch_box_preds (B,Amax,7) and
               batch_counts (B) i32, written by one launch; batch_index is left out
cls_preds_normalized is False on both."""
import torch

from .point_head_template import PointHeadTemplate
from ...utils import box_coder_utils
from ...utils.fc_rows import fc_rows


def build_point_box_coder(target_cfg):
    """TARGET_CONFIG.BOX_CODER of a point head -> the coder; the heads' kernels and torch routes are built for use_mean_size"""
    coder = getattr(box_coder_utils, target_cfg.BOX_CODER)(**target_cfg.BOX_CODER_CONFIG)
    if not getattr(coder, 'use_mean_size', False) or coder.code_size != 8:
        raise NotImplementedError('point head box branch: only PointResidualCoder with use_mean_size: True (code size 8) is built; '
                                  'use_mean_size: False is not')
    return coder


class PointIntraPartOffsetHead(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=self.model_cfg.CLS_FC, input_channels=input_channels, output_channels=num_class)
        self.part_reg_layers = self.make_fc_layers(fc_cfg=self.model_cfg.PART_FC, input_channels=input_channels, output_channels=3)
        self.box_layers = None
        target_cfg = self.model_cfg.TARGET_CONFIG
        if target_cfg.get('BOX_CODER', None) is not None:
            self.box_coder = build_point_box_coder(target_cfg)
            self.box_layers = self.make_fc_layers(fc_cfg=self.model_cfg.REG_FC, input_channels=input_channels,
                                                  output_channels=self.box_coder.code_size)

    def assign_targets(self, input_dict):
        """point_coords (N1 + N2 + ..., 4) [b,x,y,z], gt_boxes (B,M,8) -> point_cls_labels (N) long (0 background, -1 ignored),
        point_part_labels (N,3)"""
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.dim() == 3 and input_dict['point_coords'].dim() == 2
        return self.assign_stack_targets(points=input_dict['point_coords'], gt_boxes=gt_boxes, set_ignore_flag=True,
                                         use_ball_constraint=False, ret_part_labels=True, ret_box_labels=self.box_layers is not None)

    def get_loss(self, tb_dict=None):
        return self.get_part_head_loss(tb_dict)

    def forward(self, batch_dict):
        feats = batch_dict['point_features']
        cls_preds = fc_rows(self.cls_layers, feats)
        part_preds = fc_rows(self.part_reg_layers, feats)
        ret = {'point_cls_preds': cls_preds, 'point_part_preds': part_preds}
        if self.box_layers is not None:
            ret['point_box_preds'] = fc_rows(self.box_layers, feats)
        batch_dict['point_cls_scores'], _ = torch.sigmoid(cls_preds).max(dim=-1)
        batch_dict['point_part_offset'] = torch.sigmoid(part_preds)
        if self.training:
            targets = self.assign_targets(batch_dict)
            ret['point_cls_labels'] = targets['point_cls_labels']
            ret['point_part_labels'] = targets['point_part_labels']
            ret['point_box_labels'] = targets['point_box_labels']
        if self.box_layers is not None and (not self.training or self.predict_boxes_when_training):
            self.predicted_boxes_to_batch(batch_dict, cls_preds, ret['point_box_preds'])
        self.forward_ret_dict = ret
        return batch_dict
