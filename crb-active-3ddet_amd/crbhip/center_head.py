"""The anchor-free centre head of CenterPoint: target assignment, losses and box decoding (csrc/center_head.hip).

Host mirror of CenterHead.assign_targets / get_loss / generate_predicted_boxes (pcdet/models/dense_heads/center_head.py:103-304) with
centernet_utils (gaussian_radius, draw_gaussian_to_heatmap, decode_bbox_from_heatmap) and FocalLossCenterNet / RegLossCenterNet
(pcdet/utils/loss_utils.py:264-386). Three entry points, each with two routes:
  * fused (FUSED, device f32 tensors): the kernels - no host round trip, no copy of a whole map, bit-reproducible;
  * torch route (`*_torch`; CRB_CENTER_FUSED=0, host tensors, f64): the reference's formulas step by step. The CPU path, the f64 path
    and the comparison side of the A/B (tools/time_centerpoint.py).
assign_targets -> per head (heatmap (B,C_h,H,W), target_boxes (B,NMAX,8+E), inds (B,NMAX) i64, masks (B,NMAX) i64)
center_loss    -> (2) = {hm_loss * cls_weight, loc_loss * loc_weight} of one head (f64 on the fused route)
decode         -> boxes (B,K,7+vel), scores (B,K), labels (B,K) i64 class-in-head, keep (B,K) bool"""
import ctypes
import os
import warnings

import numpy as np
import torch

from ._lib import lib, check, ptr, cur_stream, CrbHipError

FUSED = os.environ.get('CRB_CENTER_FUSED', '1') == '1'
MAX_MAPS, MAX_CODE, MAX_SLOTS = 8, 16, 4096


class CenterMaps(ctypes.Structure):
    """CrbCenterMaps of include/crb_hip.h"""
    _fields_ = [('ptr', ctypes.c_void_p * MAX_MAPS), ('grad', ctypes.c_void_p * MAX_MAPS), ('stride_c', ctypes.c_int64 * MAX_MAPS),
                ('stride_p', ctypes.c_int64 * MAX_MAPS), ('channels', ctypes.c_int32 * MAX_MAPS), ('num_maps', ctypes.c_int32)]


class CenterLossCfg(ctypes.Structure):
    """CrbCenterLossCfg of include/crb_hip.h"""
    _fields_ = [('code_weights', ctypes.c_float * MAX_CODE), ('cls_weight', ctypes.c_float), ('loc_weight', ctypes.c_float)]


def class_tables(class_names, class_names_each_head):
    """-> (class_head, class_local, head_channels): for class c (0-based, the detector's order) the head that names it (-1: none) and
    its index there; the number of classes of every head"""
    heads = [[n for n in names if n in class_names] for names in class_names_each_head]
    class_head, class_local = [-1] * len(class_names), [0] * len(class_names)
    for h, names in enumerate(heads):
        for k, n in enumerate(names):
            class_head[class_names.index(n)], class_local[class_names.index(n)] = h, k
    return class_head, class_local, [len(n) for n in heads]


def _why_torch(*tensors):
    """None: the kernels take these tensors; else the reason for the torch route"""
    if not FUSED:
        return 'CRB_CENTER_FUSED=0'
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            return 'host tensors'
        if t.is_floating_point() and t.dtype != torch.float32:
            return 'tensors are not float32'
    return None


def _route(what, *tensors):
    why = _why_torch(*tensors)
    if why is not None and FUSED:
        warnings.warn('%s: torch route (%s)' % (what, why))
    return why is None


def _layout(t):
    """a (B,C,H,W) map as the kernels address it -> (tensor, stride_c, stride_p); NCHW and channels_last memory are taken as they
    are, anything else is made contiguous"""
    B, C, H, W = t.shape
    if t.is_contiguous():
        return t, H * W, 1
    if t.is_contiguous(memory_format=torch.channels_last):
        return t, 1, C
    return t.contiguous(), H * W, 1


def _data_ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _maps(tensors, grads=None):
    if len(tensors) > MAX_MAPS or sum(int(t.shape[1]) for t in tensors) > MAX_CODE:
        raise CrbHipError('crb_center: CRB_ERR_UNSUPPORTED (at most %d regression maps with %d channels in all)' % (MAX_MAPS, MAX_CODE))
    m = CenterMaps()
    keep = []
    for i, t in enumerate(tensors):
        t, sc, sp = _layout(t)
        keep.append(t)
        m.ptr[i], m.stride_c[i], m.stride_p[i], m.channels[i] = t.data_ptr(), sc, sp, int(t.shape[1])
        if grads is not None:
            m.grad[i] = grads[i].data_ptr()
    m.num_maps = len(tensors)
    return m, keep


def _f32(v, n):
    return (ctypes.c_float * n)(*[float(x) for x in v[:n]])


def _i32(v):
    return (ctypes.c_int32 * len(v))(*[int(x) for x in v])


# ---- target assignment ------------------------------------------------------------------------------------------------------
def gaussian_radius(height, width, min_overlap):
    """centernet_utils.gaussian_radius (:9-35), tensors of any float dtype"""
    b1 = height + width
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + (b1 ** 2 - 4 * c1).sqrt()) / 2
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + (b2 ** 2 - 16 * c2).sqrt()) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + (b3 ** 2 - 4 * a3 * c3).sqrt()) / 2
    return torch.min(torch.min(r1, r2), r3)


def assign_targets_torch(gt_boxes, class_head, class_local, head_channels, H, W, pc_range, voxel_size, stride, num_max_objs,
                         gaussian_overlap, min_radius):
    """the reference's assignment on the host, box by box (center_head.py:103-219), without its write into gt_boxes: an object goes to
    the head that names its class, with the class index of that head"""
    dev, dtype = gt_boxes.device, gt_boxes.dtype
    gt = gt_boxes.detach().cpu()
    B, E = gt.shape[0], gt.shape[2] - 8
    cls = gt[:, :, -1]
    cls = torch.where((cls >= 1) & (cls <= len(class_head)), cls, torch.zeros_like(cls)).long()
    out = []
    for h, C in enumerate(head_channels):
        heat = torch.zeros((B, C, H, W), dtype=dtype)
        tb = torch.zeros((B, num_max_objs, 8 + E), dtype=dtype)
        inds = torch.zeros((B, num_max_objs), dtype=torch.int64)
        masks = torch.zeros((B, num_max_objs), dtype=torch.int64)
        for b in range(B):
            pick = [i for i in range(gt.shape[1]) if cls[b, i] > 0 and class_head[int(cls[b, i]) - 1] == h][:num_max_objs]
            if not pick:
                continue
            g = gt[b, pick]
            local = [class_local[int(cls[b, i]) - 1] for i in pick]
            cx = torch.clamp((g[:, 0] - pc_range[0]) / voxel_size[0] / stride, min=0, max=W - 0.5)
            cy = torch.clamp((g[:, 1] - pc_range[1]) / voxel_size[1] / stride, min=0, max=H - 0.5)
            xi, yi = cx.int(), cy.int()
            dx, dy = g[:, 3] / voxel_size[0] / stride, g[:, 4] / voxel_size[1] / stride
            radius = torch.clamp_min(gaussian_radius(dx, dy, gaussian_overlap).int(), min=min_radius)
            for k in range(len(pick)):
                if dx[k] <= 0 or dy[k] <= 0 or not (cx[k] >= 0 and cy[k] >= 0):
                    continue
                r, x, y = int(radius[k]), int(xi[k]), int(yi[k])
                # draw_gaussian_to_heatmap (centernet_utils.py:38-69): the f64 window, cast to the map's dtype; its eps cut never
                # triggers at sigma = diameter / 6
                n = np.arange(-r, r + 1, dtype=np.float64)
                sigma = (2 * r + 1) / 6
                gauss = np.exp(-(n[None, :] * n[None, :] + n[:, None] * n[:, None]) / (2 * sigma * sigma))
                left, right, top, bottom = min(x, r), min(W - x, r + 1), min(y, r), min(H - y, r + 1)
                win = torch.from_numpy(gauss[r - top:r + bottom, r - left:r + right]).to(dtype)
                view = heat[b, local[k], y - top:y + bottom, x - left:x + right]
                torch.max(view, win, out=view)
                inds[b, k] = y * W + x
                masks[b, k] = 1
                tb[b, k, 0], tb[b, k, 1], tb[b, k, 2] = cx[k] - xi[k].to(dtype), cy[k] - yi[k].to(dtype), g[k, 2]
                tb[b, k, 3:6] = g[k, 3:6].log()
                tb[b, k, 6], tb[b, k, 7] = torch.cos(g[k, 6]), torch.sin(g[k, 6])
                if E > 0:
                    tb[b, k, 8:] = g[k, 7:-1]
        out.append((heat.to(dev), tb.to(dev), inds.to(dev), masks.to(dev)))
    return out


@torch.no_grad()
def assign_targets(gt_boxes, class_head, class_local, head_channels, H, W, pc_range, voxel_size, stride, num_max_objs,
                   gaussian_overlap, min_radius):
    """gt_boxes (B, M, 7 + E + 1), class in the last column (1-based, the detector's order) -> per head (heatmap, target_boxes, inds,
    masks). One launch sequence for all frames and heads; gt_boxes is not written."""
    args = (class_head, class_local, head_channels, int(H), int(W), [float(v) for v in pc_range], [float(v) for v in voxel_size],
            int(stride), int(num_max_objs), float(gaussian_overlap), int(min_radius))
    if not _route('center_head.assign_targets', gt_boxes):
        return assign_targets_torch(gt_boxes, *args)
    gt = gt_boxes.detach().contiguous()
    B, M, bd = (int(v) for v in gt.shape)
    if bd < 8:
        raise CrbHipError('crb_center_assign_targets: gt_boxes (B, M, 7 + E + 1) expected, got %s' % (tuple(gt.shape),))
    dev, nh, E, nmax = gt.device, len(head_channels), bd - 8, int(num_max_objs)
    sizes = [B * int(c) * H * W for c in head_channels]
    heat = torch.empty((sum(sizes),), dtype=torch.float32, device=dev)
    tb = torch.empty((nh, B, nmax, 8 + E), dtype=torch.float32, device=dev)
    inds = torch.empty((nh, B, nmax), dtype=torch.int64, device=dev)
    masks = torch.empty((nh, B, nmax), dtype=torch.int64, device=dev)
    wsb = int(lib.crb_center_assign_workspace_bytes(nh, B, nmax))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib.crb_center_assign_targets(ptr(gt), B, M, bd, len(class_head), _i32(class_head), _i32(class_local), nh, _i32(head_channels),
                                        int(H), int(W), _f32(pc_range, 2), _f32(voxel_size, 2), int(stride), nmax,
                                        float(gaussian_overlap), int(min_radius), ptr(heat), ptr(tb), ptr(inds), ptr(masks), ptr(ws),
                                        wsb, cur_stream(dev)), 'crb_center_assign_targets')
    out, off = [], 0
    for h, n in enumerate(sizes):
        out.append((heat[off:off + n].view(B, int(head_channels[h]), H, W), tb[h], inds[h], masks[h]))
        off += n
    return out


# ---- losses -----------------------------------------------------------------------------------------------------------------
def gather_at(maps, inds):
    """maps: list of (B,c,H,W) -> (B,NMAX,sum c) rows at the cells `inds` (reads the cells only, whatever the memory layout)"""
    cols = [m.flatten(2).gather(2, inds[:, None, :].expand(-1, m.shape[1], -1)) for m in maps]
    return torch.cat(cols, 1).transpose(1, 2)


def center_loss_torch(hm, heatmap, reg_maps, target_boxes, inds, masks, code_weights, cls_weight, loc_weight):
    """CenterHead.get_loss for one head (center_head.py:232-244) in the dtype of `hm` -> (2) = {hm_loss, loc_loss}, weighted"""
    pred = torch.clamp(hm.sigmoid(), min=1e-4, max=1 - 1e-4)
    gt = heatmap.to(pred.dtype)
    pos_inds, neg_inds = gt.eq(1).to(pred.dtype), gt.lt(1).to(pred.dtype)
    pos_loss = (torch.log(pred) * torch.pow(1 - pred, 2) * pos_inds).sum()
    neg_loss = (torch.log(1 - pred) * torch.pow(pred, 2) * torch.pow(1 - gt, 4) * neg_inds).sum()
    num_pos = pos_inds.sum()
    hm_loss = torch.where(num_pos == 0, -neg_loss, -(pos_loss + neg_loss) / num_pos.clamp(min=1))
    regr = gather_at(reg_maps, inds)
    tgt = target_boxes.to(regr.dtype)
    m = masks[:, :, None].to(regr.dtype) * (~torch.isnan(tgt)).to(regr.dtype)
    per_col = torch.abs(regr * m - torch.nan_to_num(tgt) * m).transpose(2, 0).sum(2).sum(1) / torch.clamp_min(masks.to(regr.dtype).sum(), 1.0)
    loc_loss = (per_col * per_col.new_tensor([float(w) for w in code_weights][:per_col.shape[0]])).sum()
    return torch.stack([hm_loss * cls_weight, loc_loss * loc_weight])


class _CenterLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hm, heatmap, target_boxes, inds, masks, cfg, *reg_maps):
        B, C, H, W = (int(v) for v in hm.shape)
        dev = hm.device
        hm, sc, sp = _layout(hm)
        maps, keep = _maps(reg_maps)
        loss = torch.empty((2,), dtype=torch.float64, device=dev)
        stats = torch.empty((2,), dtype=torch.float64, device=dev)
        wsb = int(lib.crb_center_loss_workspace_bytes(B, H, W))
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        check(lib.crb_center_loss_forward(_data_ptr(hm), sc, sp, ptr(heatmap), B, C, H, W, ctypes.byref(maps), ptr(target_boxes), ptr(inds),
                                          ptr(masks), int(inds.shape[1]), ctypes.byref(cfg), ptr(loss), ptr(stats), ptr(ws), wsb,
                                          cur_stream(dev)), 'crb_center_loss_forward')
        ctx.save_for_backward(hm, heatmap, target_boxes, inds, masks, stats, *keep)
        ctx.cfg, ctx.layout = cfg, (sc, sp)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        hm, heatmap, target_boxes, inds, masks, stats = ctx.saved_tensors[:6]
        reg_maps = ctx.saved_tensors[6:]
        B, C, H, W = (int(v) for v in hm.shape)
        dev = hm.device
        g = grad_loss.detach().float().contiguous()
        d_hm = torch.empty_like(hm)                                   # (preserves NCHW / channels_last memory)
        grads = [torch.empty_like(m) for m in reg_maps]
        maps, keep = _maps(reg_maps, grads)
        check(lib.crb_center_loss_backward(_data_ptr(hm), ctx.layout[0], ctx.layout[1], ptr(heatmap), B, C, H, W, ctypes.byref(maps),
                                           ptr(target_boxes), ptr(inds), ptr(masks), int(inds.shape[1]), ctypes.byref(ctx.cfg), ptr(stats),
                                           ptr(g), _data_ptr(d_hm), cur_stream(dev)), 'crb_center_loss_backward')
        del keep
        return (d_hm, None, None, None, None, None) + tuple(grads)


def center_loss(hm, heatmap, reg_maps, target_boxes, inds, masks, code_weights, cls_weight, loc_weight):
    """hm (B,C,H,W) logits, heatmap (B,C,H,W), reg_maps: the HEAD_ORDER maps (B,c,H,W) in NCHW or channels_last memory, target_boxes
    (B,NMAX,sum c), inds / masks (B,NMAX) i64 -> (2) = {hm_loss * cls_weight, loc_loss * loc_weight}; differentiable in hm and reg_maps"""
    reg_maps = list(reg_maps)
    if sum(int(m.shape[1]) for m in reg_maps) != int(target_boxes.shape[2]) or len(code_weights) < int(target_boxes.shape[2]):
        raise CrbHipError('crb_center_loss: %d regression channels, %d target columns, %d code weights'
                          % (sum(int(m.shape[1]) for m in reg_maps), int(target_boxes.shape[2]), len(code_weights)))
    if FUSED and int(inds.shape[1]) > MAX_SLOTS and hm.is_cuda and hm.dtype == torch.float32:
        warnings.warn('center_head.center_loss: torch route (NUM_MAX_OBJS %d above the kernels\' %d)' % (int(inds.shape[1]), MAX_SLOTS))
        return center_loss_torch(hm, heatmap, reg_maps, target_boxes, inds, masks, code_weights, cls_weight, loc_weight)
    if not _route('center_head.center_loss', hm, heatmap, target_boxes, inds, *reg_maps):
        return center_loss_torch(hm, heatmap, reg_maps, target_boxes, inds, masks, code_weights, cls_weight, loc_weight)
    cw = [float(w) for w in code_weights][:MAX_CODE]
    cfg = CenterLossCfg((ctypes.c_float * MAX_CODE)(*(cw + [0.0] * (MAX_CODE - len(cw)))), float(cls_weight), float(loc_weight))
    return _CenterLoss.apply(hm, heatmap.contiguous(), target_boxes.contiguous(), inds.contiguous(), masks.to(torch.int64).contiguous(),
                             cfg, *reg_maps)


# ---- decoding ---------------------------------------------------------------------------------------------------------------
def top_cells(hm, K):
    """the K largest logits of every frame over all classes and cells -> (values (B,K), flat indices (B,K), channels_last order?).
    The same set as the reference's two-stage top-K (centernet_utils._topk), ties aside. A channels_last map is flattened as it lies in
    memory (index = cell * C + c), a NCHW map likewise (c * H*W + cell): no copy."""
    cl = (not hm.is_contiguous()) and hm.is_contiguous(memory_format=torch.channels_last)
    flat = hm.permute(0, 2, 3, 1).flatten(1) if cl else hm.flatten(1)
    val, idx = torch.topk(flat, min(int(K), flat.shape[1]), dim=1)
    return val, idx, cl


def decode_torch(hm, reg_maps, K, pc_range, voxel_size, stride, limit_range, score_thresh, top=None):
    """decode_bbox_from_heatmap (centernet_utils.py:154-192) behind a one-stage top-K, in the dtype of `hm`"""
    B, C, H, W = hm.shape
    val, idx, cl = top if top is not None else top_cells(hm, K)
    cls, cell = (idx % C, idx // C) if cl else (idx // (H * W), idx % (H * W))
    rows = gather_at(reg_maps, cell)
    ys, xs = (cell // W).to(hm.dtype), (cell % W).to(hm.dtype)
    x = (xs + rows[..., 0]) * stride * voxel_size[0] + pc_range[0]
    y = (ys + rows[..., 1]) * stride * voxel_size[1] + pc_range[1]
    parts = [x[..., None], y[..., None], rows[..., 2:3], rows[..., 3:6].exp(), torch.atan2(rows[..., 7:8], rows[..., 6:7]), rows[..., 8:]]
    boxes = torch.cat(parts, -1)
    scores = val.sigmoid()
    lim = boxes.new_tensor([float(v) for v in limit_range])
    keep = (boxes[..., :3] >= lim[:3]).all(2) & (boxes[..., :3] <= lim[3:]).all(2)
    if score_thresh is not None:
        keep = keep & (scores > score_thresh)
    return boxes, scores, cls, keep


@torch.no_grad()
def decode(hm, reg_maps, K, pc_range, voxel_size, stride, limit_range, score_thresh, top=None):
    """hm (B,C,H,W) logits of one head, reg_maps = [center, center_z, dim, rot (, vel)] -> boxes (B,K,7 + vel), scores (B,K) = sigmoid,
    labels (B,K) i64 class in head, keep (B,K) bool: inside POST_CENTER_LIMIT_RANGE and score > SCORE_THRESH. top: top_cells(hm, K) when the caller already has it"""
    reg_maps = list(reg_maps)
    if not _route('center_head.decode', hm, *reg_maps):
        return decode_torch(hm, reg_maps, K, pc_range, voxel_size, stride, limit_range, score_thresh, top)
    B, C, H, W = (int(v) for v in hm.shape)
    dev = hm.device
    val, idx, cl = top if top is not None else top_cells(hm.detach(), K)
    val, idx = val.contiguous(), idx.contiguous()
    K = int(val.shape[1])
    maps, keep_alive = _maps([m.detach() for m in reg_maps])
    nbox = 7 + (int(reg_maps[4].shape[1]) if len(reg_maps) > 4 else 0)
    boxes = torch.empty((B, K, nbox), dtype=torch.float32, device=dev)
    scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    labels = torch.empty((B, K), dtype=torch.int64, device=dev)
    keep = torch.empty((B, K), dtype=torch.uint8, device=dev)
    thresh = -1.0 if score_thresh is None else float(score_thresh)    # (scores are > 0)
    check(lib.crb_center_decode(ptr(val), ptr(idx), B, K, C, H, W, int(cl), ctypes.byref(maps), _f32(pc_range, 2), _f32(voxel_size, 2),
                                int(stride), _f32(limit_range, 6), thresh, ptr(boxes), ptr(scores), ptr(labels), ptr(keep),
                                cur_stream(dev)), 'crb_center_decode')
    del keep_alive
    return boxes, scores, labels, keep.bool()
