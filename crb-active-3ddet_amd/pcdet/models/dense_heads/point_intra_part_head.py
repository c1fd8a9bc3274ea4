"""PointIntraPartOffsetHead (pcdet/models/dense_heads/point_intra_part_head.py:7-127): foreground segmentation and intra-object part
locations of every voxel centre, the point head of Part-A2. Targets and losses run as the launches of csrc/part_head.hip
(crbhip/part_head.py). The box branch of PartA2_free.yaml (TARGET_CONFIG.BOX_CODER) is not built."""
import torch

from .point_head_template import PointHeadTemplate
from ...utils.fc_rows import fc_rows


class PointIntraPartOffsetHead(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        if self.model_cfg.TARGET_CONFIG.get('BOX_CODER', None) is not None:
            raise NotImplementedError('PointIntraPartOffsetHead: the box branch (TARGET_CONFIG.BOX_CODER, PartA2_free.yaml) is not built')
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=self.model_cfg.CLS_FC, input_channels=input_channels, output_channels=num_class)
        self.part_reg_layers = self.make_fc_layers(fc_cfg=self.model_cfg.PART_FC, input_channels=input_channels, output_channels=3)
        self.box_layers = None

    def assign_targets(self, input_dict):
        """point_coords (N1 + N2 + ..., 4) [b,x,y,z], gt_boxes (B,M,8) -> point_cls_labels (N) long (0 background, -1 ignored),
        point_part_labels (N,3)"""
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.dim() == 3 and input_dict['point_coords'].dim() == 2
        return self.assign_stack_targets(points=input_dict['point_coords'], gt_boxes=gt_boxes, set_ignore_flag=True,
                                         use_ball_constraint=False, ret_part_labels=True, ret_box_labels=False)

    def get_loss(self, tb_dict=None):
        return self.get_part_head_loss(tb_dict)

    def forward(self, batch_dict):
        feats = batch_dict['point_features']
        cls_preds = fc_rows(self.cls_layers, feats)
        part_preds = fc_rows(self.part_reg_layers, feats)
        ret = {'point_cls_preds': cls_preds, 'point_part_preds': part_preds}
        batch_dict['point_cls_scores'], _ = torch.sigmoid(cls_preds).max(dim=-1)
        batch_dict['point_part_offset'] = torch.sigmoid(part_preds)
        if self.training:
            targets = self.assign_targets(batch_dict)
            ret['point_cls_labels'] = targets['point_cls_labels']
            ret['point_part_labels'] = targets['point_part_labels']
            ret['point_box_labels'] = None
        self.forward_ret_dict = ret
        return batch_dict
