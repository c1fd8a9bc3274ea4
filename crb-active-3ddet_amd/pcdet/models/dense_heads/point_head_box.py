"""PointHeadBox (pcdet/models/dense_heads/point_head_box.py:7-115): foreground segmentation and one box per point, the first-stage
head of PointRCNN. A thin module over the entry points of PointIntraPartOffsetHead's box branch (csrc/point_box.hip,
crbhip/point_box.py) without the part branch: one launch for the targets of all frames, one forward / backward pair for point_loss_cls
+ point_loss_box, one launch for the decode into dense proposals (see point_intra_part_head.py for what is left in the batch dict)."""
import torch

from .point_head_template import PointHeadTemplate
from .point_intra_part_head import build_point_box_coder
from ...utils.fc_rows import fc_rows


class PointHeadBox(PointHeadTemplate):
    def __init__(self, num_class, input_channels, model_cfg, predict_boxes_when_training=False, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class)
        self.predict_boxes_when_training = predict_boxes_when_training
        self.cls_layers = self.make_fc_layers(fc_cfg=self.model_cfg.CLS_FC, input_channels=input_channels, output_channels=num_class)
        self.box_coder = build_point_box_coder(self.model_cfg.TARGET_CONFIG)
        self.box_layers = self.make_fc_layers(fc_cfg=self.model_cfg.REG_FC, input_channels=input_channels,
                                              output_channels=self.box_coder.code_size)

    def assign_targets(self, input_dict):
        """point_coords (N1 + N2 + ..., 4) [b,x,y,z], gt_boxes (B,M,8) -> point_cls_labels (N) long (0 background, -1 ignored),
        point_box_labels (N,8)"""
        gt_boxes = input_dict['gt_boxes']
        assert gt_boxes.dim() == 3 and input_dict['point_coords'].dim() == 2
        return self.assign_stack_targets(points=input_dict['point_coords'], gt_boxes=gt_boxes, set_ignore_flag=True,
                                         use_ball_constraint=False, ret_part_labels=False, ret_box_labels=True)

    def get_loss(self, tb_dict=None):
        return self.get_part_head_loss(tb_dict)

    def forward(self, batch_dict):
        before = self.model_cfg.get('USE_POINT_FEATURES_BEFORE_FUSION', False)
        feats = batch_dict['point_features_before_fusion' if before else 'point_features']
        cls_preds = fc_rows(self.cls_layers, feats)
        box_preds = fc_rows(self.box_layers, feats)
        batch_dict['point_cls_scores'] = torch.sigmoid(cls_preds.max(dim=-1)[0])
        ret = {'point_cls_preds': cls_preds, 'point_box_preds': box_preds}
        if self.training:
            targets = self.assign_targets(batch_dict)
            ret['point_cls_labels'] = targets['point_cls_labels']
            ret['point_box_labels'] = targets['point_box_labels']
        if not self.training or self.predict_boxes_when_training:
            self.predicted_boxes_to_batch(batch_dict, cls_preds, box_preds)
        self.forward_ret_dict = ret
        return batch_dict
