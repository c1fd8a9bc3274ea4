"""class_agnostic_nms / multi_classes_nms with the reference's call contract (pcdet/models/model_utils/model_nms_utils.py:6-66).

Both reduce to one step — keep the boxes passing the score threshold, take the NMS_PRE_MAXSIZE best, run the configured
rotated NMS of iou3d_nms_utils on them, keep NMS_POST_MAXSIZE — written once here (`_survivors`)."""
import torch

from ...ops.iou3d_nms import iou3d_nms_utils


def _survivors(scores, boxes, nms_config, score_thresh):
    """indices INTO `scores` of the boxes that survive threshold + top-k + NMS, best first (LongTensor, possibly empty)"""
    cand = torch.arange(scores.shape[0], device=scores.device)
    if score_thresh is not None:
        cand = cand[scores >= score_thresh]
    if cand.numel() == 0:
        return cand
    k = min(int(nms_config.NMS_PRE_MAXSIZE), int(cand.numel()))
    top_scores, order = torch.topk(scores[cand], k=k)
    cand = cand[order]
    nms_fn = getattr(iou3d_nms_utils, nms_config.NMS_TYPE)
    keep, _ = nms_fn(boxes[cand][:, 0:7], top_scores, nms_config.NMS_THRESH, **nms_config)
    return cand[keep[:nms_config.NMS_POST_MAXSIZE]]


def class_agnostic_nms(box_scores, box_preds, nms_config, score_thresh=None):
    """-> (selected indices into the inputs, their scores)"""
    sel = _survivors(box_scores, box_preds, nms_config, score_thresh)
    return sel, box_scores[sel]


def multi_classes_nms(cls_scores, box_preds, nms_config, score_thresh=None, return_index=False):
    """per-class NMS on (N, num_class) scores -> (scores, labels, boxes) concatenated over the classes in class order
    (return_index: and the indices into the inputs)"""
    out_scores, out_labels, out_boxes, out_sel = [], [], [], []
    for cls in range(cls_scores.shape[1]):
        col = cls_scores[:, cls]
        sel = _survivors(col, box_preds, nms_config, score_thresh)
        out_scores.append(col[sel])
        out_labels.append(torch.full((sel.numel(),), cls, dtype=torch.long, device=col.device))
        out_boxes.append(box_preds[sel])
        out_sel.append(sel)
    out = (torch.cat(out_scores, dim=0), torch.cat(out_labels, dim=0), torch.cat(out_boxes, dim=0))
    return out + (torch.cat(out_sel, dim=0),) if return_index else out


def multi_classes_nms_batched(cls_preds, decode_head, label_mapping, nms_config, score_thresh=None):
    """multi_classes_nms for every frame, head and class of a batch as one launch sequence without host synchronisation
    (csrc/multiclass_nms.hip around crb_decode_selected_anchors and crb_nms_batched).
    cls_preds [(B,A_h,C_h)] LOGITS of every head, decode_head(h, idx (B,k) long) -> (B,k,7+) decoded boxes of head h's anchors idx,
    label_mapping [(C_h) long] class id of every head column.
    -> dict of fixed-size tensors, P = sum C_h * NMS_POST_MAXSIZE: pred_boxes (B,P,7), pred_scores (B,P) = torch.sigmoid of the kept
    logits, pred_labels (B,P) long, pred_anchor (B,P) long (index into the box's head's anchors), seg_of (B,P) int32 ((head, class)
    column 0 .. sum C_h - 1), num (B) int32; per frame the survivors in the loop's concatenation order (head, class, best first), zero
    rows past num[b]; top_idx / top_logit / counts: the candidates of every segment (crbhip.multihead.candidates)."""
    from crbhip import multihead
    B = int(cls_preds[0].shape[0])
    pre, post = int(nms_config.NMS_PRE_MAXSIZE), int(nms_config.NMS_POST_MAXSIZE)
    top_idx, top_logit, counts = multihead.candidates(cls_preds, -1.0 if score_thresh is None else score_thresh, pre)
    boxes, row = [], 0
    for h, t in enumerate(cls_preds):
        C = int(t.shape[2])
        picks = decode_head(h, top_idx[row:row + B * C].view(B, C * pre))                    # head h's rows: one (B, C_h * pre) block
        boxes.append(picks[..., 0:7].reshape(B * C, pre, 7))
        row += B * C
    top_boxes = boxes[0] if len(boxes) == 1 else torch.cat(boxes, dim=0)
    keep, num_keep = iou3d_nms_utils.nms_batched(top_boxes, counts, nms_config.NMS_THRESH, post, rotated=(nms_config.NMS_TYPE == 'nms_gpu'))
    label_map = torch.cat([m.reshape(-1) for m in label_mapping]).to(device=top_idx.device, dtype=torch.int64)
    pred_boxes, pred_logit, pred_labels, pred_anchor, seg_of, num = multihead.finish(cls_preds, keep, num_keep, top_idx, top_logit,
                                                                                      top_boxes, label_map)
    live = torch.arange(pred_logit.shape[1], device=num.device)[None, :] < num[:, None]
    scores = torch.where(live, torch.sigmoid(pred_logit), torch.zeros_like(pred_logit))
    return {'pred_boxes': pred_boxes, 'pred_scores': scores, 'pred_labels': pred_labels, 'pred_anchor': pred_anchor, 'seg_of': seg_of,
            'num': num, 'top_idx': top_idx, 'top_logit': top_logit, 'counts': counts}
