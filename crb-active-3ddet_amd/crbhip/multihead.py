"""AnchorHeadMulti's hot path: the RPN losses over head slices (csrc/multihead_loss.hip) and the per-class selection of a whole
batch around the batched NMS (csrc/multiclass_nms.hip).

`multihead_loss(...)` is the multi-head twin of crbhip.rpn_loss.rpn_loss: one forward (+ finalize) and one backward launch for
all heads and frames, (B,3) per-frame {cls, loc, dir} losses normalised by the frame's positives over all heads.
`candidates(...)` / `finish(...)` bracket crb_decode_selected_anchors and crb_nms_batched in
pcdet.models.model_utils.model_nms_utils.multi_classes_nms_batched."""
import ctypes

import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

MAX_HEADS = 16          # CRB_MULTIHEAD_MAX_HEADS
MAX_HEAD_CLASSES = 8    # class columns of one head
MAX_PRE = 4096          # NMS_PRE_MAXSIZE the candidates kernel sorts in LDS


class MultiHeadEntry(ctypes.Structure):
    """CrbMultiHeadEntry of include/crb_hip.h"""
    _fields_ = [('cls', ctypes.c_void_p), ('box', ctypes.c_void_p), ('dir', ctypes.c_void_p), ('d_cls', ctypes.c_void_p),
                ('d_box', ctypes.c_void_p), ('d_dir', ctypes.c_void_p), ('anchor_start', ctypes.c_int32),
                ('anchor_count', ctypes.c_int32), ('class_start', ctypes.c_int32), ('class_count', ctypes.c_int32)]


def _addr(t):
    return None if t is None else t.data_ptr()


def head_table(cls, box=None, dirs=None, class_starts=None, grads=None):
    """cls [(B,A_h,C_h)], box [(B,A_h,7)] or None, dirs [(B,A_h,NB)] or None, grads (d_cls, d_box, d_dir) lists or None
    -> host array of CrbMultiHeadEntry (the tensors must stay referenced by the caller until the launch has been enqueued)"""
    n = len(cls)
    if not 1 <= n <= MAX_HEADS:
        raise CrbHipError('crb_multihead: 1 .. %d heads expected, got %d' % (MAX_HEADS, n))
    table = (MultiHeadEntry * n)()
    start = 0
    for h in range(n):
        B, A, C = (int(v) for v in cls[h].shape)
        for t in (cls[h], None if box is None else box[h], None if dirs is None else dirs[h]):
            if t is not None and (not t.is_contiguous() or t.dtype != torch.float32 or t.shape[:2] != cls[h].shape[:2]):
                raise CrbHipError('crb_multihead: head %d needs contiguous float32 (B, A_h, .) tensors' % h)
        e = table[h]
        e.cls, e.box, e.dir = _addr(cls[h]), _addr(None if box is None else box[h]), _addr(None if dirs is None else dirs[h])
        if grads is not None:
            e.d_cls, e.d_box = _addr(grads[0][h]), _addr(grads[1][h])
            e.d_dir = _addr(None if grads[2] is None else grads[2][h])
        e.anchor_start, e.anchor_count = start, A
        e.class_start, e.class_count = (0 if class_starts is None else int(class_starts[h])), C
        start += A
    return table


class _MultiHeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, labels, reg_targets, anchors, cfg, class_starts, pos_w, neg_w, n, *preds):
        cls, box = list(preds[:n]), list(preds[n:2 * n])
        dirs = list(preds[2 * n:]) or None
        B, A = int(labels.shape[0]), int(labels.shape[1])
        dev = labels.device
        table = head_table(cls, box, dirs, class_starts)
        loss = torch.empty((B, 3), dtype=torch.float32, device=dev)
        npos = torch.empty((B,), dtype=torch.float32, device=dev)
        wsb = lib.crb_multihead_loss_workspace_bytes(B, A)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        check(lib.crb_multihead_loss_forward(table, n, ptr(labels), ptr(reg_targets), ptr(anchors), B, A, ctypes.byref(cfg),
                                             pos_w, neg_w, ptr(loss), ptr(npos), ptr(ws), wsb, cur_stream(dev)),
              'crb_multihead_loss_forward')
        ctx.save_for_backward(labels, reg_targets, anchors, npos, *preds)
        ctx.meta = (cfg, class_starts, pos_w, neg_w, n)
        ctx.mark_non_differentiable(npos)
        return loss, npos

    @staticmethod
    def backward(ctx, grad_loss, _grad_npos):
        labels, reg_targets, anchors, npos = ctx.saved_tensors[:4]
        preds = ctx.saved_tensors[4:]
        cfg, class_starts, pos_w, neg_w, n = ctx.meta
        cls, box = list(preds[:n]), list(preds[n:2 * n])
        dirs = list(preds[2 * n:]) or None
        B, A = int(labels.shape[0]), int(labels.shape[1])
        g = grad_loss.contiguous().float()
        grads = ([torch.empty_like(t) for t in cls], [torch.empty_like(t) for t in box],
                 None if dirs is None else [torch.empty_like(t) for t in dirs])
        table = head_table(cls, box, dirs, class_starts, grads)
        check(lib.crb_multihead_loss_backward(table, n, ptr(labels), ptr(reg_targets), ptr(anchors), B, A, ctypes.byref(cfg),
                                              pos_w, neg_w, ptr(npos), ptr(g), cur_stream(labels.device)),
              'crb_multihead_loss_backward')
        return (None,) * 8 + tuple(grads[0]) + tuple(grads[1]) + (tuple(grads[2]) if grads[2] is not None else ())


def multihead_loss(cls_preds, box_preds, dir_preds, labels, reg_targets, anchors, cfg, class_starts=None, pos_cls_weight=1.0,
                   neg_cls_weight=1.0, return_npos=False):
    """cls_preds [(B,A_h,C_h)], box_preds [(B,A_h,7)], dir_preds [(B,A_h,bins)] or None per head, labels (B,A) i32, reg_targets
    (B,A,7), anchors (A,7) in the multi-head order (A = sum A_h), cfg a crbhip.rpn_loss.RpnLossCfg whose num_class is the head's
    total class count, class_starts[h] = first class column of head h (SEPARATE_MULTIHEAD; None: every head predicts all classes)
    -> (B,3) per-frame {cls, loc, dir} losses"""
    n = len(cls_preds)
    if len(box_preds) != n or (dir_preds is not None and len(dir_preds) != n):
        raise CrbHipError('crb_multihead_loss: one cls / box / dir tensor per head expected')
    require_cuda(labels, reg_targets, anchors, *cls_preds, *box_preds, *(dir_preds or ()))
    B, A = int(labels.shape[0]), int(labels.shape[1])
    f = lambda t, c: t.reshape(B, -1, c).contiguous().float()
    cls = [t.contiguous().float() for t in cls_preds]
    if any(t.dim() != 3 or t.shape[0] != B for t in cls):
        raise CrbHipError('crb_multihead_loss: cls_preds must be (B, A_h, C_h) per head')
    box = [f(t, 7) for t in box_preds]
    dirs = None if dir_preds is None else [f(t, cfg.num_dir_bins) for t in dir_preds]
    if sum(int(t.shape[1]) for t in cls) != A or reg_targets.numel() != B * A * 7 or anchors.numel() != A * 7 or \
            any(b.shape[1] != c.shape[1] for b, c in zip(box, cls)) or \
            (dirs is not None and any(d.shape[1] != c.shape[1] for d, c in zip(dirs, cls))):
        raise CrbHipError('crb_multihead_loss: tensor sizes do not match (B, A) = (%d, %d)' % (B, A))
    if any(t.shape[2] > MAX_HEAD_CLASSES for t in cls):
        raise CrbHipError('crb_multihead_loss: at most %d class columns per head' % MAX_HEAD_CLASSES)
    if labels.dtype != torch.int32:
        labels = labels.to(torch.int32)
    starts = None if class_starts is None else tuple(int(s) for s in class_starts)
    loss, npos = _MultiHeadLoss.apply(labels.contiguous(), reg_targets.contiguous().float(), anchors.contiguous().float(), cfg, starts,
                                      float(pos_cls_weight), float(neg_cls_weight), n, *cls, *box, *(dirs or ()))
    return (loss, npos) if return_npos else loss


def _segments(cls):
    return sum(int(t.shape[2]) for t in cls)


def candidates(cls_preds, score_thresh, pre_max):
    """cls_preds [(B,A_h,C_h)] logits per head -> top_idx (S,pre_max) i64 into the head's anchors, top_logit (S,pre_max), counts (S)
    i32 for the S = B * sum C_h segments in HEAD-major order (head h's rows form one (B, C_h * pre_max) block starting at row
    B * (classes of the heads before h)): per segment the anchors whose f32 sigmoid is >= score_thresh, the best min(pre_max, A_h)
    of them in descending score order, equal scores by ascending index. No host synchronisation."""
    require_cuda(*cls_preds)
    if pre_max > MAX_PRE:
        raise CrbHipError('crb_multiclass_candidates: NMS_PRE_MAXSIZE %d > %d' % (pre_max, MAX_PRE))
    cls = [t.contiguous().float() for t in cls_preds]
    B, dev = int(cls[0].shape[0]), cls[0].device
    S = B * _segments(cls)
    top_idx = torch.empty((S, pre_max), dtype=torch.int64, device=dev)
    top_logit = torch.empty((S, pre_max), dtype=torch.float32, device=dev)
    counts = torch.empty((S,), dtype=torch.int32, device=dev)
    table = head_table(cls)
    check(lib.crb_multiclass_candidates(table, len(cls), B, float(score_thresh), int(pre_max), ptr(top_idx), ptr(top_logit),
                                        ptr(counts), cur_stream(dev)), 'crb_multiclass_candidates')
    return top_idx, top_logit, counts


def finish(cls_preds, keep, num_keep, top_idx, top_logit, top_boxes, label_map):
    """keep (S,post) i32 / num_keep (S) of the batched NMS over the segments of candidates(), top_boxes (S,pre_max,7) the decoded
    picks, label_map (sum C_h) i64 -> pred_boxes (B,P,7), pred_logit (B,P), pred_labels (B,P) i64, pred_anchor (B,P) i64, seg_of
    (B,P) i32, num (B) i32 with P = sum C_h * post: per frame the survivors of its segments one after another (head order, class
    order inside a head, best first inside a class), zero rows past num[b]"""
    cls = [t.contiguous().float() for t in cls_preds]
    B, dev = int(cls[0].shape[0]), cls[0].device
    SEG, pre_max, post = _segments(cls), int(top_idx.shape[1]), int(keep.shape[1])
    if keep.shape[0] != B * SEG or top_boxes.numel() != B * SEG * pre_max * 7 or label_map.numel() != SEG:
        raise CrbHipError('crb_multiclass_finish: tensor sizes do not match %d segments' % (B * SEG))
    P = SEG * post
    pred_boxes = torch.empty((B, P, 7), dtype=torch.float32, device=dev)
    pred_logit = torch.empty((B, P), dtype=torch.float32, device=dev)
    pred_labels = torch.empty((B, P), dtype=torch.int64, device=dev)
    pred_anchor = torch.empty((B, P), dtype=torch.int64, device=dev)
    seg_of = torch.empty((B, P), dtype=torch.int32, device=dev)
    num = torch.empty((B,), dtype=torch.int32, device=dev)
    table = head_table(cls)
    check(lib.crb_multiclass_finish(table, len(cls), B, pre_max, post, ptr(keep.contiguous()), ptr(num_keep.contiguous()),
                                    ptr(top_idx), ptr(top_logit), ptr(top_boxes.contiguous()), ptr(label_map.contiguous()),
                                    ptr(pred_boxes), ptr(pred_logit), ptr(pred_labels), ptr(pred_anchor), ptr(seg_of), ptr(num),
                                    cur_stream(dev)), 'crb_multiclass_finish')
    return pred_boxes, pred_logit, pred_labels, pred_anchor, seg_of, num
