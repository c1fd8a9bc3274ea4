"""SECONDNetIoU (pcdet/models/detectors/second_net_iou.py:7-177): SECOND + the IoU-prediction second stage (SECONDHead). The
loss is the dense head's plus the RoI head's; post-processing re-scores the first-stage boxes with the predicted IoU.

post_processing returns the reference's contract (pred_boxes, pred_scores, pred_labels, pred_cls_scores, pred_iou_scores per frame
and the recall dict) for SCORE_TYPE absent / iou, cls, weighted_iou_cls and score_by_class, computed for all frames at once (one
score sort, one batched NMS, one read-back of the keep counts) instead of the reference's per-frame loop. One extension: each pred
dict also carries pred_logits, the full_cls_scores rows of the kept boxes, which the entropy strategy reads."""
import torch

from ...config import EasyDict
from .detector3d_template import Detector3DTemplate
from .post_processing import final_nms_batched, generate_recall_record


def dataset_cfg_of(dataset):
    """what SECONDHead.roi_grid_pool reads of the dataset config (second_head.py:68-72): the dataset's own dataset_cfg when it has
    one, else the same two entries from the attributes every dataset here carries"""
    cfg = getattr(dataset, 'dataset_cfg', None)
    if cfg is not None:
        return cfg
    return EasyDict({'POINT_CLOUD_RANGE': [float(v) for v in dataset.point_cloud_range],
                     'DATA_PROCESSOR': [{'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [float(v) for v in dataset.voxel_size]}]})


class SECONDNetIoU(Detector3DTemplate):
    def __init__(self, model_cfg, num_class, dataset):
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)
        self.module_list = self.build_networks()

    def forward(self, batch_dict):
        batch_dict['dataset_cfg'] = dataset_cfg_of(self.dataset)
        return super().forward(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_rcnn, tb_dict, {}

    def nms_scores(self, iou_preds, cls_preds, label_preds):
        """(B,N) sigmoid IoU / class scores, (B,N) labels -> the scores the final NMS ranks by (second_net_iou.py:119-146)"""
        cfg = self.model_cfg.POST_PROCESSING.NMS_CONFIG
        kind = cfg.get('SCORE_TYPE', None)
        if cfg.get('SCORE_BY_CLASS', None) and kind == 'score_by_class':
            # set_nms_score_by_class (:59-73) as the reference runs it: it walks i < (number of DISTINCT labels in the frame) and
            # scores label i + 1 by SCORE_BY_CLASS[class_names[i]]; labels it does not reach keep the score 0
            present = torch.zeros((label_preds.shape[0], len(self.class_names) + 1), dtype=torch.bool, device=label_preds.device)
            present.scatter_(1, label_preds.clamp(min=0, max=len(self.class_names)), True)
            n_distinct = present.sum(1, keepdim=True)
            scores = torch.zeros_like(iou_preds)
            for i, name in enumerate(self.class_names):
                how = cfg.SCORE_BY_CLASS[name]
                if how not in ('iou', 'cls'):
                    raise NotImplementedError(how)
                mask = (label_preds == i + 1) & (n_distinct > i)
                scores = torch.where(mask, iou_preds if how == 'iou' else cls_preds, scores)
            return scores
        if kind is None or kind == 'iou':
            return iou_preds
        if kind == 'cls':
            return cls_preds
        if kind == 'weighted_iou_cls':
            return cfg.SCORE_WEIGHTS.iou * iou_preds + cfg.SCORE_WEIGHTS.cls * cls_preds
        # num_pts_iou_cls (:132-144) counts points per box on the host in the reference; not carried over
        raise NotImplementedError(kind)

    def post_processing(self, batch_dict):
        cfg = self.model_cfg.POST_PROCESSING
        if cfg.NMS_CONFIG.MULTI_CLASSES_NMS:
            raise NotImplementedError('MULTI_CLASSES_NMS')
        if cfg.OUTPUT_RAW_SCORE:
            raise NotImplementedError('OUTPUT_RAW_SCORE')
        B = batch_dict['batch_size']
        box_preds = batch_dict['batch_box_preds']
        iou_preds, cls_preds = batch_dict['batch_cls_preds'], batch_dict['roi_scores']
        assert batch_dict.get('batch_index', None) is None and iou_preds.dim() == 3 and iou_preds.shape[-1] in (1, self.num_class)
        if not batch_dict['cls_preds_normalized']:
            iou_preds, cls_preds = torch.sigmoid(iou_preds), torch.sigmoid(cls_preds)
        iou_preds, label_preds = torch.max(iou_preds, dim=-1)
        label_preds = batch_dict['roi_labels'] if batch_dict.get('has_class_labels', False) else label_preds + 1
        scores = self.nms_scores(iou_preds, cls_preds, label_preds)
        sel, valid, num = final_nms_batched(scores, box_preds, cfg.NMS_CONFIG, cfg.SCORE_THRESH)
        g = lambda t: torch.gather(t, 1, sel)
        boxes = torch.gather(box_preds, 1, sel[..., None].expand(-1, -1, box_preds.shape[-1]))
        out = {'pred_scores': g(scores), 'pred_labels': g(label_preds), 'pred_cls_scores': g(cls_preds), 'pred_iou_scores': g(iou_preds)}
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
