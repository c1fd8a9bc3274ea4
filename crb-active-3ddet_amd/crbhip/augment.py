"""Host side of the fused world augmentation + range mask (C-ABI: crb_augment_mask_points, crb_augment_boxes)."""
import ctypes

import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError


def _range6(point_cloud_range):
    if point_cloud_range is None:
        return None
    return (ctypes.c_float * 6)(*[float(v) for v in point_cloud_range])


def _params(params, B):
    if params.dtype != torch.float32 or tuple(params.shape) != (B, 8):
        raise CrbHipError('augmentation parameters must be (B, 8) f32: [flip_x, flip_y, c, s, scale, tx, ty, tz] per frame')
    params = params.contiguous()
    if params.data_ptr() % 16:
        params = params.clone()
    return params


def augment_mask_points(points, frame_offsets, params, point_cloud_range=None, mask=True, xyz_col=0, num_features=None,
                        frame_col=False, lazy=False):
    """points (n, row) f32 cuda (rows may be strided: only stride(1) == 1 is needed), xyz at column xyz_col followed by
    num_features - 3 feature columns (default: the rest of the row); frame_offsets (B+1) i32 cuda; params (B, 8) f32 cuda.
    -> (out, new_offsets): the transformed rows that pass the x/y range test (all rows when mask=False), original order, as
    (n_kept, frame_col + num_features) f32, and the new (B+1) i32 offsets.
    One host read-back of the total; lazy=True skips it and returns out at its capacity of n rows."""
    require_cuda(points, frame_offsets, params)
    if points.dtype != torch.float32 or points.dim() != 2 or frame_offsets.dtype != torch.int32:
        raise CrbHipError('augment_mask_points: points (n, row) f32 and frame_offsets (B+1) i32')
    n = points.shape[0]
    if n > 1 and points.stride(1) != 1:
        points = points.contiguous()
    row_stride = points.stride(0) if n > 1 else points.shape[1]
    C = points.shape[1] - xyz_col if num_features is None else int(num_features)
    if C < 3 or xyz_col + C > points.shape[1]:
        raise CrbHipError('augment_mask_points: xyz_col + num_features exceeds the row')
    frame_offsets = frame_offsets.contiguous()
    B = frame_offsets.numel() - 1
    params = _params(params, B)
    if mask and point_cloud_range is None:
        raise CrbHipError('augment_mask_points: mask=True needs point_cloud_range')
    dev = points.device
    out = torch.empty((n, C + int(bool(frame_col))), dtype=torch.float32, device=dev)
    new_off = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    ws_bytes = lib.crb_augment_mask_points_workspace_bytes(n, B)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    rc = lib.crb_augment_mask_points(ctypes.c_void_p(points.data_ptr()) if n else None, n, row_stride, int(xyz_col), C,
                                     ptr(frame_offsets), B, ptr(params), _range6(point_cloud_range), int(bool(mask)),
                                     ptr(out), int(bool(frame_col)), ptr(new_off), ptr(ws), ws_bytes, cur_stream(dev))
    _hold = points                                         # (a strided view: its address went in without ptr())
    check(rc, 'crb_augment_mask_points')
    del _hold
    if lazy:
        return out, new_off
    return out[:int(new_off[-1])], new_off                 # the one sync


def augment_boxes(gt_boxes, counts, params, angles=None, point_cloud_range=None, mask=False, min_num_corners=1):
    """gt_boxes (B, G, W) f32 cuda, W = 8 or 10 (box coordinates + class); counts (B) i32 cuda valid rows per frame; params (B, 8)
    and angles (B) f32 cuda (the f32 of each frame's drawn rotation angle, None = no rotation).
    -> (out (B, G, W): transformed, heading limited to [-pi, pi), kept rows compacted in order, the rest zero; new counts (B) i32)"""
    require_cuda(gt_boxes, counts, params, angles)
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or counts.dtype != torch.int32:
        raise CrbHipError('augment_boxes: gt_boxes (B, G, W) f32 and counts (B) i32')
    B, G, W = gt_boxes.shape
    if W not in (8, 10):
        raise CrbHipError('augment_boxes: rows of 7 or 9 box coordinates plus the class column (W = 8 or 10), got W = %d' % W)
    if counts.numel() != B or (angles is not None and (angles.numel() != B or angles.dtype != torch.float32)):
        raise CrbHipError('augment_boxes: counts (B) i32, angles (B) f32')
    if mask and point_cloud_range is None:
        raise CrbHipError('augment_boxes: mask=True needs point_cloud_range')
    gt_boxes = gt_boxes.contiguous()
    params = _params(params, B)
    out = torch.empty_like(gt_boxes)
    new_counts = torch.empty((B,), dtype=torch.int32, device=gt_boxes.device)
    rc = lib.crb_augment_boxes(ptr(gt_boxes), ptr(counts.contiguous()), B, G, W, ptr(params),
                               ptr(angles.contiguous()) if angles is not None else None, _range6(point_cloud_range),
                               int(bool(mask)), int(min_num_corners), ptr(out), ptr(new_counts), cur_stream(gt_boxes.device))
    check(rc, 'crb_augment_boxes')
    return out, new_counts
