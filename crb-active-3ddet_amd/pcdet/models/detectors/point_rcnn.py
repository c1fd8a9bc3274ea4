"""PointRCNN (pcdet/models/detectors/point_rcnn.py:4-30), the detector class of the models whose proposals come from a point head:
PartA2_free.yaml (MeanVFE -> UNetV2 -> PointIntraPartOffsetHead with a box per point -> PartA2FCHead with DISABLE_PART). The loss is the
point head's plus the RoI head's, with the reference's tb_dict keys.

forward() and post_processing are the template's: the module chain, then either the training loss or the CRB record path."""
from .detector3d_template import Detector3DTemplate


class PointRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def get_training_loss(self):
        loss_point, tb_dict = self.point_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_point + loss_rcnn, tb_dict, {}
