"""PVRCNN (pcdet/models/detectors/pv_rcnn.py:4-43): two-stage detector = RPN (dense head) + keypoint head + RoI head.
forward() is Detector3DTemplate.forward; this class only says how the three losses combine and which second-stage tensors the
training-mode return dict carries (the active-learning code reads them).
With ROI_HEAD.LOSS_NET (LLAL) and the loss net trainable, the three heads return per-frame losses (reduce=False), the step's loss
is their batch mean plus the loss net's ranking loss against them (pv_rcnn.py:29-43); frozen (OPTIMIZATION.LOSS_NET_SKIP), the
step is the ordinary one."""
from .detector3d_template import Detector3DTemplate


class PVRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def training_outputs(self, batch_dict):
        head = self.roi_head.forward_ret_dict
        return {'rcnn_reg_gt': head['rcnn_reg_gt'], 'rcnn_cls_gt': head['rcnn_cls_labels'],
                'rcnn_cls': batch_dict['rcnn_cls'], 'rcnn_reg': batch_dict['rcnn_reg'],
                'rpn_preds': batch_dict['rpn_preds']}

    def get_training_loss(self):
        lal_flag = hasattr(self.roi_head, 'loss_net')
        if lal_flag:
            # trainable loss net -> loss-net phase of LLAL
            lal_flag = list(self.roi_head.loss_net.children())[0].weight.requires_grad
        if not lal_flag:
            total, tb_dict = self.dense_head.get_loss()
            for head in (self.point_head, self.roi_head):
                part, tb_dict = head.get_loss(tb_dict)
                total = total + part
            return total, tb_dict, {}
        loss_rpn, tb_dict = self.dense_head.get_loss(reduce=False)
        loss_point, tb_dict = self.point_head.get_loss(tb_dict, reduce=False)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict, reduce=False)
        loss = loss_rpn + loss_point + loss_rcnn
        loss_loss_net = self.roi_head.get_loss_loss_net(tb_dict, loss)
        return loss.mean() + loss_loss_net, tb_dict, {}
