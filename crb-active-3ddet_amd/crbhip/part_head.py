"""The point head of Part-A2 in training: segmentation + intra-object part targets and the focal + part-offset losses
(csrc/part_head.hip).

Host mirror of PointHeadTemplate.assign_stack_targets in set_ignore_flag mode with ret_part_labels=True, get_cls_layer_loss and
get_part_layer_loss (pcdet/models/dense_heads/point_head_template.py:49-173). Two entry points, each with two routes:
  * fused (FUSED, device f32 tensors): the kernels - one launch for the targets of all frames, two for the losses and their gradients,
    one for the backward, no host round trip, bit-reproducible;
  * torch route (`*_torch`; CRB_PART_HEAD_FUSED=0, host tensors, f64): the reference's expressions over the whole batch at once. The CPU
    path, the f64 path and the comparison side of the A/B.
part_targets -> labels (N) i64, part_labels (N,3), owner (N) i32
part_loss    -> point_loss_cls, point_loss_part, positives (0-dim, f64 on the fused route; differentiable in the two prediction tensors)"""
import os

import torch

from ._lib import lib, check, ptr, cur_stream, host_f32x3

FUSED = os.environ.get('CRB_PART_HEAD_FUSED', '1') == '1'


def frame_offsets(points, B):
    """(B + 1) i32 row offsets of the frames of frame-sorted stacked rows [b, ...], on the rows' device, without a host read"""
    edges = torch.arange(B + 1, device=points.device, dtype=points.dtype)
    return torch.searchsorted(points[:, 0].contiguous(), edges).to(torch.int32)


def _fused_ok(*tensors):
    return FUSED and all(t.is_cuda and (not t.is_floating_point() or t.dtype == torch.float32) for t in tensors)


# ---- targets ----------------------------------------------------------------------------------------------------------------
def _contains(pts, frame, boxes):
    """pts (N,3), frame (N) long, boxes (B,G,7) -> (N,G) bool: the point-in-box rule of csrc/pt_in_box.h (roiaware_pool3d_kernel.cu:23-36)
    in torch: f32 sin / cos of -heading, f32 rotation, the half-extent comparisons in f64. Tensors of f64 run the same expressions in f64."""
    b = boxes[frame]                                                   # (N,G,7)
    x, y, z = pts[:, None, 0], pts[:, None, 1], pts[:, None, 2]
    ca, sa = torch.cos(-b[..., 6]), torch.sin(-b[..., 6])
    sx, sy = x - b[..., 0], y - b[..., 1]
    lx = sx * ca + sy * (-sa)
    ly = sx * sa + sy * ca
    inz = (z - b[..., 2]).abs().double() <= b[..., 5].double() / 2.0
    margin = float(torch.tensor(1e-5, dtype=torch.float32))
    return inz & (lx.abs().double() < b[..., 3].double() / 2.0 + margin) & (ly.abs().double() < b[..., 4].double() / 2.0 + margin)


def _first(hit):
    """(N,G) bool -> (N) long index of the first true column, -1 when none"""
    if hit.shape[1] == 0:
        return torch.full((hit.shape[0],), -1, dtype=torch.int64, device=hit.device)
    idx = hit.to(torch.uint8).argmax(1)
    return torch.where(hit.any(1), idx, torch.full_like(idx, -1))


def part_targets_torch(points, gt_boxes, extra_width, num_class):
    """the reference's expressions (point_head_template.py:74-122) for all frames at once, in the dtype of `points`"""
    frame = points[:, 0].long()
    pts = points[:, 1:4]
    gt = gt_boxes.to(points.dtype)
    if gt.shape[1] == 0:
        return torch.zeros_like(frame), torch.zeros_like(pts), torch.full_like(frame, -1, dtype=torch.int32)
    large =gt[..., :7].clone()
    large[..., 3:6] += gt.new_tensor([float(w) for w in extra_width])
    inner = _first(_contains(pts, frame, gt[..., :7]))
    outer = _first(_contains(pts, frame, large))
    fg = inner >= 0
    labels = torch.where(fg ^ (outer >= 0), torch.full_like(inner, -1), torch.zeros_like(inner))
    box = gt[frame, inner.clamp(min=0)]                                # (N,8) the owner's row (row 0 for the rest, masked below)
    labels = torch.where(fg, torch.ones_like(labels) if num_class == 1 else box[:, 7].long(), labels)
    d = pts - box[:, 0:3]
    ca, sa = torch.cos(-box[:, 6]), torch.sin(-box[:, 6])
    rot = torch.stack([d[:, 0] * ca - d[:, 1] * sa, d[:, 0] * sa + d[:, 1] * ca, d[:, 2]], 1)
    part = torch.where(fg[:, None], rot / box[:, 3:6] + 0.5, torch.zeros_like(rot))
    return labels, part, inner.to(torch.int32)


@torch.no_grad()
def part_targets(points, gt_boxes, extra_width, num_class, offsets=None):
    """points (N,4) [b,x,y,z] frame-sorted, gt_boxes (B,G,8) zero padded, extra_width: TARGET_CONFIG.GT_EXTRA_WIDTH,
    offsets: (B+1) i32 device row offsets of the frames when the caller has them
    -> point_cls_labels (N) i64, point_part_labels (N,3), owner (N) i32"""
    assert points.dim() == 2 and points.shape[1] == 4 and gt_boxes.dim() == 3 and gt_boxes.shape[2] == 8
    if not _fused_ok(points, gt_boxes):
        return part_targets_torch(points, gt_boxes, extra_width, num_class)
    pts, gt = points.contiguous(), gt_boxes.contiguous()
    N, (B, G) = int(pts.shape[0]), (int(v) for v in gt.shape[:2])
    off = frame_offsets(pts, B) if offsets is None else offsets.to(torch.int32).contiguous()
    assert off.is_cuda and off.numel() == B + 1
    labels = torch.empty((N,), dtype=torch.int64, device=pts.device)
    part = torch.empty((N, 3), dtype=torch.float32, device=pts.device)
    owner = torch.empty((N,), dtype=torch.int32, device=pts.device)
    check(lib.crb_part_targets(ptr(pts), ptr(off), ptr(gt), B, N, G, host_f32x3(extra_width), int(num_class), ptr(labels), ptr(part),
                               ptr(owner), cur_stream(pts.device)), 'crb_part_targets')
    return labels, part, owner


# ---- losses -----------------------------------------------------------------------------------------------------------------
def binary_cross_entropy(p, t):
    """F.binary_cross_entropy(p, t, reduction='none') in its own arithmetic (each log clamped at -100), as torch expressions: the
    containment test lets a point lie 1e-5 outside its box in x / y, so a part label can be -1e-5 or 1 + 1e-5, and the device kernel
    behind F.binary_cross_entropy asserts 0 <= target <= 1 (the process aborts)"""
    return (t - 1) * torch.log(1 - p).clamp(min=-100) - t * torch.log(p).clamp(min=-100)


def part_loss_torch(cls_preds, part_preds, labels, part_labels, alpha, gamma, cls_weight, part_weight):
    """get_cls_layer_loss + get_part_layer_loss (point_head_template.py:131-173) in the dtype of the predictions, with
    SigmoidFocalClassificationLoss spelled out (loss_utils.py:9-72) and the positive count kept on the device"""
    C = cls_preds.shape[1]
    positives = labels > 0
    pos = positives.sum().to(cls_preds.dtype)
    norm = torch.clamp(pos, min=1.0)
    cls_weights = ((labels == 0) * 1.0 + 1.0 * positives).to(cls_preds.dtype) / norm
    one_hot =(torch.arange(C + 1, device=labels.device)[None, :] == (labels * (labels >= 0).long())[:, None]).to(cls_preds.dtype)
    target = one_hot[:, 1:]
    p = torch.sigmoid(cls_preds)
    alpha_w = target * alpha + (1 - target) * (1 - alpha)
    pt = target * (1.0 - p) + (1.0 - target) * p
    bce = torch.clamp(cls_preds, min=0) - cls_preds * target + torch.log1p(torch.exp(-torch.abs(cls_preds)))
    loss_cls = (alpha_w * torch.pow(pt, gamma) * bce * cls_weights[:, None]).sum() * cls_weight
    src = binary_cross_entropy(torch.sigmoid(part_preds), part_labels.to(part_preds.dtype))
    loss_part = (src.sum(dim=-1) * positives.to(src.dtype)).sum() / (3 * norm) * part_weight
    return loss_cls, loss_part, pos


class _PartLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cls_preds, part_preds, labels, part_labels, alpha, gamma, cls_weight, part_weight):
        c, p = cls_preds.contiguous(), part_preds.contiguous()
        n, C = (int(v) for v in c.shape)
        dev = c.device
        out = torch.empty((3,), dtype=torch.float64, device=dev)
        d_cls, d_part = torch.empty_like(c), torch.empty_like(p)
        wsb = int(lib.crb_part_loss_workspace_bytes(n))
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        check(lib.crb_part_loss_forward(ptr(c), ptr(p), ptr(labels.contiguous()), ptr(part_labels.contiguous()), n, C, alpha, gamma,
                                        cls_weight, part_weight, ptr(out), ptr(d_cls), ptr(d_part), ptr(ws), wsb, cur_stream(dev)),
              'crb_part_loss_forward')
        ctx.save_for_backward(d_cls, d_part)
        loss_cls, loss_part, pos = out[0], out[1], out[2]
        ctx.mark_non_differentiable(pos)
        return loss_cls, loss_part, pos

    @staticmethod
    def backward(ctx, g_cls, g_part, _g_pos):
        d_cls, d_part = ctx.saved_tensors
        n, C = (int(v) for v in d_cls.shape)
        g = torch.stack([g_cls.detach().float().reshape(()), g_part.detach().float().reshape(())])
        o_cls, o_part = torch.empty_like(d_cls), torch.empty_like(d_part)
        check(lib.crb_part_loss_backward(ptr(d_cls), ptr(d_part), ptr(g), n, C, ptr(o_cls), ptr(o_part), cur_stream(d_cls.device)),
              'crb_part_loss_backward')
        return o_cls, o_part, None, None, None, None, None, None


def part_loss(cls_preds, part_preds, labels, part_labels, alpha=0.25, gamma=2.0, cls_weight=1.0, part_weight=1.0):
    """cls_preds (N,C) logits, part_preds (N,3) logits, labels (N) i64, part_labels (N,3)
    -> (point_loss_cls, point_loss_part, positives), 0-dim, the two losses weighted"""
    assert cls_preds.dim() == 2 and part_preds.dim() == 2 and part_preds.shape[1] == 3 and cls_preds.shape[0] == part_preds.shape[0] \
        and labels.shape == (cls_preds.shape[0],) and part_labels.shape == part_preds.shape and labels.dtype == torch.int64
    if not _fused_ok(cls_preds, part_preds, labels, part_labels):
        return part_loss_torch(cls_preds, part_preds, labels, part_labels, alpha, gamma, cls_weight, part_weight)
    return _PartLoss.apply(cls_preds, part_preds, labels, part_labels, float(alpha), float(gamma), float(cls_weight), float(part_weight))
