"""PartA2Net (pcdet/models/detectors/PartA2_net.py:4-31): MeanVFE -> UNetV2 -> HeightCompression -> BaseBEVBackbone ->
AnchorHeadSingle -> PointIntraPartOffsetHead -> PartA2FCHead. The loss is the dense head's plus the point head's (segmentation
+ intra-object part offsets) plus the RoI head's, with the reference's tb_dict keys.

forward() and post_processing are the template's: the module chain, then either the training loss or the CRB record path."""
from .detector3d_template import Detector3DTemplate


class PartA2Net(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_point, tb_dict = self.point_head.get_loss(tb_dict)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_point + loss_rcnn, tb_dict, {}
