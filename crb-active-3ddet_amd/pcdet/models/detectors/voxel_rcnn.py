"""VoxelRCNN (pcdet/models/detectors/voxel_rcnn.py:4-32): the SECOND trunk + VoxelRCNNHead, which refines the first-stage boxes from
the 3D backbone's own sparse feature levels. The loss is the dense head's plus the RoI head's.

post_processing returns the reference's plain contract (pred_boxes, pred_scores, pred_labels per frame and the recall dict;
detector3d_template.py post_processing without the active-learning record) for all frames at once: one batched NMS, one read-back
of the keep counts. The head is class-agnostic, so the labels are the first stage's roi_labels. One extension, the one SECONDNetIoU
carries: each pred dict also holds pred_logits, the full_cls_scores rows of the kept boxes, which the entropy strategy reads."""
import torch

from .detector3d_template import Detector3DTemplate
from .post_processing import final_nms_batched, generate_recall_record


class VoxelRCNN(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_rcnn, tb_dict, {}

    def post_processing(self, batch_dict):
        cfg = self.model_cfg.POST_PROCESSING
        if cfg.NMS_CONFIG.MULTI_CLASSES_NMS:
            raise NotImplementedError('MULTI_CLASSES_NMS')
        if cfg.OUTPUT_RAW_SCORE:
            raise NotImplementedError('OUTPUT_RAW_SCORE')
        B = batch_dict['batch_size']
        box_preds, cls_preds = batch_dict['batch_box_preds'], batch_dict['batch_cls_preds']
        assert batch_dict.get('batch_index', None) is None and cls_preds.dim() == 3 and cls_preds.shape[-1] in (1, self.num_class)
        if not batch_dict['cls_preds_normalized']:
            cls_preds = torch.sigmoid(cls_preds)
        scores, label_preds = torch.max(cls_preds, dim=-1)
        label_preds = batch_dict['roi_labels'] if batch_dict.get('has_class_labels', False) else label_preds + 1
        sel, valid, num = final_nms_batched(scores, box_preds, cfg.NMS_CONFIG, cfg.SCORE_THRESH)
        boxes = torch.gather(box_preds, 1, sel[..., None].expand(-1, -1, box_preds.shape[-1]))
        out = {'pred_scores': torch.gather(scores, 1, sel), 'pred_labels': torch.gather(label_preds, 1, sel)}
        full = batch_dict.get('full_cls_scores', None)
        logits = torch.gather(full, 1, sel[..., None].expand(-1, -1, full.shape[-1])) if full is not None else None
        num = num.cpu().tolist()                                  # the single read-back of the selection
        recall_dict, pred_dicts = {}, []
        for b in range(B):
            k = num[b]
            recall_dict = generate_recall_record(
                box_preds=boxes[b, :k] if 'rois' not in batch_dict else box_preds[b], recall_dict=recall_dict, batch_index=b,
                data_dict=batch_dict, thresh_list=cfg.RECALL_THRESH_LIST)
            rec = {'pred_boxes': boxes[b, :k]}
            rec.update({key: val[b, :k] for key, val in out.items()})
            rec['pred_logits'] = logits[b, :k] if logits is not None else None
            pred_dicts.append(rec)
        return pred_dicts, recall_dict
