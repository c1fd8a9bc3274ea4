"""CenterPoint (pcdet/models/detectors/centerpoint.py:4-50): MeanVFE -> VoxelBackBone8x -> HeightCompression -> BaseBEVBackbone ->
CenterHead, one stage, the loss is the dense head's. forward() is Detector3DTemplate.forward; the tb_dict values are detached tensors,
as in the other detectors here.

post_processing takes the head's decoded boxes (CenterHead.generate_predicted_boxes: the K picks of every head for all frames, in
descending score order, with their keep masks) and runs, for all frames at once, ONE batched NMS per head (NMS_PRE_MAXSIZE,
NMS_THRESH, NMS_POST_MAXSIZE) and ONE read-back of the keep counts, where the reference loops over heads and frames
(center_head.py:282-297). Per frame the heads' boxes are concatenated in head order and the labels mapped to the detector's classes
(+ 1), as the reference does. One extension: each pred dict also carries pred_logits (n, num_class), the heatmap logits of all heads
at the box's cell in the detector's class order, which the entropy strategy reads."""
import torch

from ...ops.iou3d_nms import iou3d_nms_utils
from .detector3d_template import Detector3DTemplate


class CenterPoint(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        return loss_rpn, dict(tb_dict, loss_rpn=loss_rpn.detach()), {}

    def post_processing(self, batch_dict):
        cfg = self.model_cfg.POST_PROCESSING
        nms = self.dense_head.model_cfg.POST_PROCESSING.NMS_CONFIG
        B = batch_dict['batch_size']
        kept, nums = [], []
        for head in batch_dict['center_preds']:
            boxes, keep = head['boxes'], head['keep']
            K = boxes.shape[1]
            # the kept picks first, still in descending score order
            order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)
            pre = min(int(nms.NMS_PRE_MAXSIZE), K)
            g = lambda t: torch.gather(t, 1, order.reshape(order.shape + (1,) * (t.dim() - 2)).expand(-1, -1, *t.shape[2:]))[:, :pre]
            counts = keep.sum(1).clamp(max=pre).int()
            sorted_boxes = g(boxes)
            post = min(int(nms.NMS_POST_MAXSIZE), pre)
            sel, num = iou3d_nms_utils.nms_batched(sorted_boxes[..., 0:7].contiguous(), counts, nms.NMS_THRESH, post,
                                                   rotated=(nms.NMS_TYPE == 'nms_gpu'))
            sel = sel.clamp(min=0).long()
            s = lambda t: torch.gather(g(t), 1, sel.reshape(sel.shape + (1,) * (t.dim() - 2)).expand(-1, -1, *t.shape[2:]))
            kept.append({'pred_boxes': s(boxes), 'pred_scores': s(head['scores']), 'pred_labels': s(head['labels']) + 1,
                         'pred_logits': s(head['logits'])})
            nums.append(num)
        nums = torch.stack(nums, 0).cpu().tolist()               # (heads, B): the single read-back of the selection
        recall_dict, pred_dicts = {}, []
        for b in range(B):
            rec = {key: torch.cat([k[key][b, :nums[h][b]] for h, k in enumerate(kept)], 0) for key in kept[0]}
            recall_dict = self.generate_recall_record(box_preds=rec['pred_boxes'], recall_dict=recall_dict, batch_index=b,
                                                      data_dict=batch_dict, thresh_list=cfg.RECALL_THRESH_LIST)
            pred_dicts.append(rec)
        return pred_dicts, recall_dict
