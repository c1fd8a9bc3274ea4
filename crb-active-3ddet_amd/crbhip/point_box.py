"""The box branch of the point heads (PointIntraPartOffsetHead with TARGET_CONFIG.BOX_CODER, PointHeadBox): box targets, the three
losses and the decode into dense proposals (csrc/point_box.hip).

Host mirror of PointHeadTemplate.assign_stack_targets in set_ignore_flag mode with ret_box_labels=True (and optionally
ret_part_labels), get_cls_layer_loss + get_part_layer_loss + get_box_layer_loss, and generate_predicted_boxes
(pcdet/models/dense_heads/point_head_template.py:49-211) with PointResidualCoder (use_mean_size). Three entry points, each with two routes:
  * fused (part_head.FUSED, device f32 tensors): one launch for the targets of all frames, two for the losses and their gradients, one
    for the backward, one for the decode; no host round trip, bit-reproducible;
  * torch route (`*_torch`; CRB_PART_HEAD_FUSED=0, host tensors, f64): the reference's expressions over the whole batch at once. The CPU
    path, the f64 path and the comparison side of the A/B.
point_box_targets -> labels (N) i64, owner (N) i32, box_labels (N,8), part_labels (N,3) or None
point_box_loss    -> point_loss_cls, point_loss_part, point_loss_box, positives (0-dim, f64 on the fused route)
point_box_decode  -> fused: batch_cls_preds (B,Amax,C), batch_box_preds (B,Amax,7), counts (B) i32; torch: the stacked (N,C), (N,7)"""
import ctypes

import torch

from . import part_head
from ._lib import lib, check, ptr, cur_stream, host_f32x3
from .part_head import frame_offsets, _fused_ok

BETA = 1.0 / 9.0


def _host_f32(v, n):
    a = [float(x) for x in v]
    assert len(a) == n, (len(a), n)
    return (ctypes.c_float * n)(*a)


# ---- targets ----------------------------------------------------------------------------------------------------------------
def point_box_targets_torch(points, gt_boxes, extra_width, num_class, coder, with_part=True):
    """the reference's expressions (point_head_template.py:74-122) for all frames at once, in the dtype of `points`: rows without an
    owner are encoded against ground truth 0 of their frame and zeroed"""
    labels, part, owner = part_head.part_targets_torch(points, gt_boxes, extra_width, num_class)
    N = points.shape[0]
    if gt_boxes.shape[1] == 0:
        return labels, owner, points.new_zeros((N, 8)), (part if with_part else None)
    gt = gt_boxes.to(points.dtype)
    fg = owner >= 0
    box = gt[points[:, 0].long(), owner.long().clamp(min=0)]                       # (N,8)
    classes = box[:, 7].long()
    classes = torch.where(fg, classes, torch.ones_like(classes))
    codes = coder.encode_torch(box[:, :7], points[:, 1:4], classes)
    # (a ground truth of zero size gives infinite logs on rows that are masked: where, not a product)
    box_labels = torch.where(fg[:, None], codes, torch.zeros_like(codes))
    return labels, owner, box_labels, (part if with_part else None)


@torch.no_grad()
def point_box_targets(points, gt_boxes, extra_width, num_class, coder, with_part=True, offsets=None):
    """points (N,4) [b,x,y,z] frame-sorted, gt_boxes (B,G,8) zero padded, coder: PointResidualCoder with use_mean_size
    -> point_cls_labels (N) i64, owner (N) i32, point_box_labels (N,8), point_part_labels (N,3) or None"""
    assert points.dim() == 2 and points.shape[1] == 4 and gt_boxes.dim() == 3 and gt_boxes.shape[2] == 8
    assert coder.use_mean_size and coder.code_size == 8
    if not _fused_ok(points, gt_boxes):
        return point_box_targets_torch(points, gt_boxes, extra_width, num_class, coder, with_part)
    pts, gt = points.contiguous(), gt_boxes.contiguous()
    N, (B, G) = int(pts.shape[0]), (int(v) for v in gt.shape[:2])
    off = frame_offsets(pts, B) if offsets is None else offsets.to(torch.int32).contiguous()
    assert off.is_cuda and off.numel() == B + 1
    mean = coder.anchor_sizes(pts)
    labels = torch.empty((N,), dtype=torch.int64, device=pts.device)
    owner = torch.empty((N,), dtype=torch.int32, device=pts.device)
    box = torch.empty((N, 8), dtype=torch.float32, device=pts.device)
    part = torch.empty((N, 3), dtype=torch.float32, device=pts.device) if with_part else None
    check(lib.crb_point_box_targets(ptr(pts), ptr(off), ptr(gt), B, N, G, host_f32x3(extra_width), int(num_class), ptr(mean),
                                    int(mean.shape[0]), ptr(labels), ptr(owner), ptr(box), ptr(part), cur_stream(pts.device)),
          'crb_point_box_targets')
    return labels, owner, box, part


# ---- losses -----------------------------------------------------------------------------------------------------------------
def point_box_loss_torch(cls_preds, part_preds, box_preds, labels, part_labels, box_labels, alpha, gamma, code_weights, beta,
                         cls_weight, part_weight, box_weight):
    """get_cls_layer_loss + get_part_layer_loss + get_box_layer_loss (point_head_template.py:131-195) in the dtype of the predictions,
    the positive count kept on the device; part_preds None: no part branch (point_loss_part = 0)"""
    if part_preds is None:
        loss_cls, _, pos = part_head.part_loss_torch(cls_preds, cls_preds.new_zeros((cls_preds.shape[0], 3)),
                                                     labels, cls_preds.new_zeros((cls_preds.shape[0], 3)), alpha, gamma, cls_weight, 0.0)
        loss_part = torch.zeros_like(loss_cls)
    else:
        loss_cls, loss_part, pos = part_head.part_loss_torch(cls_preds, part_preds, labels, part_labels, alpha, gamma, cls_weight,
                                                             part_weight)
    target = box_labels.to(box_preds.dtype)
    target = torch.where(torch.isnan(target), box_preds, target)
    diff = (box_preds - target) * torch.as_tensor([float(w) for w in code_weights], dtype=box_preds.dtype, device=box_preds.device)
    n = diff.abs()
    src = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    row_w = (labels > 0).to(box_preds.dtype) / torch.clamp(pos, min=1.0)
    loss_box = (src * row_w[:, None]).sum() * box_weight
    return loss_cls, loss_part, loss_box, pos


class _PointBoxLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls_preds, part_preds, box_preds, labels, part_labels, box_labels, alpha, gamma, code_weights, beta, cls_weight,
                part_weight, box_weight):
        c, x = cls_preds.contiguous(), box_preds.contiguous()
        p = None if part_preds is None else part_preds.contiguous()
        n, C = (int(v) for v in c.shape)
        dev = c.device
        out = torch.empty((4,), dtype=torch.float64, device=dev)
        d_cls, d_box = torch.empty_like(c), torch.empty_like(x)
        d_part = None if p is None else torch.empty_like(p)
        wsb = int(lib.crb_point_box_loss_workspace_bytes(n))
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        pl = None if p is None else part_labels.contiguous()
        check(lib.crb_point_box_loss_forward(ptr(c), ptr(p), ptr(x), ptr(labels.contiguous()), ptr(pl), ptr(box_labels.contiguous()), n, C,
                                             alpha, gamma, _host_f32(code_weights, 8), beta, cls_weight, part_weight, box_weight,
                                             ptr(out), ptr(d_cls), ptr(d_part), ptr(d_box), ptr(ws), wsb, cur_stream(dev)),
              'crb_point_box_loss_forward')
        ctx.has_part = p is not None
        ctx.save_for_backward(*((d_cls, d_part, d_box) if ctx.has_part else (d_cls, d_box)))
        loss_cls, loss_part, loss_box, pos = out[0], out[1], out[2], out[3]
        ctx.mark_non_differentiable(pos)
        return loss_cls, loss_part, loss_box, pos

    @staticmethod
    def backward(ctx, g_cls, g_part, g_box, _g_pos):
        if ctx.has_part:
            d_cls, d_part, d_box = ctx.saved_tensors
        else:
            (d_cls, d_box), d_part = ctx.saved_tensors, None
        n, C = (int(v) for v in d_cls.shape)
        g = torch.stack([v.detach().float().reshape(()) for v in (g_cls, g_part, g_box)])
        o_cls, o_box = torch.empty_like(d_cls), torch.empty_like(d_box)
        o_part = None if d_part is None else torch.empty_like(d_part)
        check(lib.crb_point_box_loss_backward(ptr(d_cls), ptr(d_part), ptr(d_box), ptr(g), n, C, ptr(o_cls), ptr(o_part), ptr(o_box),
                                              cur_stream(d_cls.device)), 'crb_point_box_loss_backward')
        return (o_cls, o_part, o_box) + (None,) * 10


def point_box_loss(cls_preds, part_preds, box_preds, labels, part_labels, box_labels, alpha=0.25, gamma=2.0, code_weights=(1.0,) * 8,
                   beta=BETA, cls_weight=1.0, part_weight=1.0, box_weight=1.0):
    """cls_preds (N,C) logits, part_preds (N,3) logits or None, box_preds (N,8), labels (N) i64, part_labels (N,3) or None, box_labels
    (N,8) -> (point_loss_cls, point_loss_part, point_loss_box, positives), 0-dim, the three losses weighted"""
    N = cls_preds.shape[0]
    assert cls_preds.dim() == 2 and box_preds.shape == (N, 8) and box_labels.shape == (N, 8) and labels.shape == (N,) and \
        labels.dtype == torch.int64
    assert part_preds is None or (part_preds.shape == (N, 3) and part_labels.shape == (N, 3))
    args = (float(alpha), float(gamma), tuple(float(w) for w in code_weights), float(beta), float(cls_weight), float(part_weight),
            float(box_weight))
    tensors = [t for t in (cls_preds, part_preds, box_preds, labels, part_labels, box_labels) if t is not None]
    if not _fused_ok(*tensors):
        return point_box_loss_torch(cls_preds, part_preds, box_preds, labels, part_labels, box_labels, *args)
    return _PointBoxLoss.apply(cls_preds, part_preds, box_preds, labels, part_labels, box_labels, *args)


# ---- decode -----------------------------------------------------------------------------------------------------------------
def point_box_decode_torch(points, cls_preds, box_preds, coder):
    """generate_predicted_boxes (point_head_template.py:197-211) -> the stacked point_cls_preds (N,C), point_box_preds (N,7)"""
    _, pred_classes = cls_preds.max(dim=-1)
    return cls_preds, coder.decode_torch(box_preds, points[:, 1:4], pred_classes + 1)


def pack_stacked(batch_index, cls_preds, box_preds, batch_size, counts=None):
    """stacked frame-sorted rows (N,C), (N,7) with their frame (N) -> dense (B,Amax,C) padded with -inf, (B,Amax,7) padded with
    zeros, counts (B) i32: the layout point_box_decode writes. counts: B host ints when the caller has them, else one read-back"""
    frame = batch_index.long()
    if counts is None:
        edges = frame_offsets(batch_index.reshape(-1, 1), batch_size).tolist()
        counts = [edges[b + 1] - edges[b] for b in range(batch_size)]
    cnt = [int(c) for c in counts]
    assert len(cnt) == batch_size and sum(cnt) == cls_preds.shape[0], (cnt, tuple(cls_preds.shape))
    amax = max(cnt) if cnt else 0
    dev = cls_preds.device
    start = torch.tensor([sum(cnt[:b]) for b in range(batch_size)], device=dev, dtype=torch.int64)
    flat = frame * amax + (torch.arange(frame.shape[0], device=dev) - start[frame])
    dense_cls = cls_preds.new_full((batch_size * amax, cls_preds.shape[1]), float('-inf'))
    dense_box = box_preds.new_zeros((batch_size * amax, box_preds.shape[1]))
    dense_cls[flat] = cls_preds
    dense_box[flat] = box_preds
    return dense_cls.view(batch_size, amax, -1), dense_box.view(batch_size, amax, -1), torch.tensor(cnt, dtype=torch.int32, device=dev)


@torch.no_grad()
def point_box_decode(points, cls_preds, box_preds, coder, batch_size, counts=None, offsets=None):
    """points (N,4) [b,x,y,z] frame-sorted, cls_preds (N,C) logits, box_preds (N,8) codes; counts: B host ints (the frames' rows) when
    the caller has them, otherwise the (B+1) offsets are read back once for the padded width. Host counts are TRUSTED beyond their
    length and sum (checking them against the device offsets would be the read-back they save): a wrong split with the right sum
    gives a padded width that is too small and the rows beyond it are dropped. The returned device counts are the frames' true row
    counts, so `counts.max() > Amax` shows it to whoever can afford the look (the proposal layer clamps them to its top-k width)
    -> fused route: batch_cls_preds (B,Amax,C), batch_box_preds (B,Amax,7), counts (B) i32;   torch route: (N,C), (N,7), None"""
    assert coder.use_mean_size and coder.code_size == 8 and box_preds.shape[1] == 8
    if not _fused_ok(points, cls_preds, box_preds):
        return point_box_decode_torch(points, cls_preds, box_preds, coder) + (None,)
    pts, c, x = points.contiguous(), cls_preds.contiguous(), box_preds.contiguous()
    N, C, B = int(pts.shape[0]), int(c.shape[1]), int(batch_size)
    off = frame_offsets(pts, B) if offsets is None else offsets.to(torch.int32).contiguous()
    if counts is not None and (len(counts) != B or sum(int(v) for v in counts) != N):
        counts = None                                                              # (counts of some other set of rows)
    if counts is None:
        edges = off.tolist()                                                      # the one read-back
        counts = [edges[b + 1] - edges[b] for b in range(B)]
    amax = max(int(v) for v in counts) if B else 0
    mean = coder.anchor_sizes(pts)
    dev = pts.device
    o_cls = torch.empty((B, amax, C), dtype=torch.float32, device=dev)
    o_box = torch.empty((B, amax, 7), dtype=torch.float32, device=dev)
    n_rows = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib.crb_point_box_decode(ptr(pts), ptr(off), ptr(c), ptr(x), ptr(mean), B, N, amax, C, int(mean.shape[0]), ptr(o_cls),
                                   ptr(o_box), ptr(n_rows), cur_stream(dev)), 'crb_point_box_decode')
    return o_cls, o_box, n_rows
