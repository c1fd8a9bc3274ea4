"""Host side of gt_sampling on the device (C-ABI: crb_gt_sample_select, crb_gt_sample_paste)."""
import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

CAND_WIDTH = 20
MAX_CANDIDATES = 256
MAX_BOXES = 512


def _candidates(cand, cand_obj, B):
    if cand.dtype != torch.float32 or cand.dim() != 3 or cand.shape[0] != B or cand.shape[2] != CAND_WIDTH:
        raise CrbHipError('gt_sampling: cand (B, S, %d) f32 candidate records' % CAND_WIDTH)
    S = cand.shape[1]
    if cand_obj.dtype != torch.int32 or tuple(cand_obj.shape) != (B, S):
        raise CrbHipError('gt_sampling: cand_obj (B, S) i32')
    return S


def _database(db, C=None):
    if db['points'].dtype != torch.float32 or db['points'].dim() != 2 or db['obj_offsets'].dtype != torch.int32:
        raise CrbHipError('gt_sampling: database points (P, C) f32 and obj_offsets (N + 1) i32')
    if C is not None and db['points'].shape[1] != C:
        raise CrbHipError('gt_sampling: the database holds %d point features, the frames %d' % (db['points'].shape[1], C))
    return db['obj_offsets'].numel() - 1


def select(gt_boxes, gt_counts, cand, cand_obj, group_offsets, db):
    """gt_boxes (B, G, 8) f32 cuda with gt_counts (B) i32 valid rows; cand (B, S, 20) f32, cand_obj (B, S) i32, group_offsets
    (B, K + 1) i32 (DeviceDataAugmentor.draw_batch); db = DeviceGtDatabase.device_tensors(device).
    -> valid (B, S) u8, out_boxes (B, G + S, 8) f32, new_counts (B) i32, cand_rows (B, S) i32, paste_counts (B) i32
    (see include/crb_hip.h). No host synchronisation."""
    require_cuda(gt_boxes, gt_counts, cand, cand_obj, group_offsets, db['points'], db['obj_offsets'])
    if gt_boxes.dtype != torch.float32 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 8:
        raise CrbHipError('gt_sample_select: gt_boxes (B, G, 8) f32 (7 box coordinates + class: the database carries no velocities)')
    B, G, _ = gt_boxes.shape
    S = _candidates(cand, cand_obj, B)
    if gt_counts.dtype != torch.int32 or gt_counts.numel() != B:
        raise CrbHipError('gt_sample_select: gt_counts (B) i32')
    if group_offsets.dtype != torch.int32 or group_offsets.dim() != 2 or group_offsets.shape[0] != B or group_offsets.shape[1] < 1:
        raise CrbHipError('gt_sample_select: group_offsets (B, K + 1) i32')
    K = group_offsets.shape[1] - 1
    N = _database(db)
    dev = gt_boxes.device
    valid = torch.empty((B, S), dtype=torch.uint8, device=dev)
    out_boxes = torch.empty((B, G + S, 8), dtype=torch.float32, device=dev)
    new_counts = torch.empty((B,), dtype=torch.int32, device=dev)
    cand_rows = torch.empty((B, S), dtype=torch.int32, device=dev)
    paste_counts = torch.empty((B,), dtype=torch.int32, device=dev)
    rc = lib.crb_gt_sample_select(ptr(gt_boxes.contiguous()), ptr(gt_counts.contiguous()), B, G, ptr(cand.contiguous()),
                                  ptr(cand_obj.contiguous()), ptr(group_offsets.contiguous()), S, K, ptr(db['obj_offsets']), N,
                                  ptr(valid), ptr(out_boxes), ptr(new_counts), ptr(cand_rows), ptr(paste_counts), cur_stream(dev))
    check(rc, 'crb_gt_sample_select')
    return valid, out_boxes, new_counts, cand_rows, paste_counts


def paste(points, frame_offsets, cand, cand_obj, valid, cand_rows, paste_counts, db, capacity, lazy=False):
    """points (n, C) f32 cuda dense rows, frame_offsets (B + 1) i32; the candidates and select()'s outputs; capacity >= n + the
    point count of all candidates (host arithmetic).
    -> (out, new_offsets (B + 2) i32): per frame the valid candidates' points, then the frame's own points outside every valid
    candidate's removal box; new_offsets[B] = total rows, [B + 1] = capacity.
    lazy=True returns out at its capacity (rows past the total untouched) and reads nothing back; otherwise one read-back of the
    total, out cut to it and new_offsets to its first B + 1 entries."""
    require_cuda(points, frame_offsets, cand, cand_obj, valid, cand_rows, paste_counts, db['points'], db['obj_offsets'])
    if points.dtype != torch.float32 or points.dim() != 2 or frame_offsets.dtype != torch.int32 or points.shape[1] < 3:
        raise CrbHipError('gt_sample_paste: points (n, C) f32 and frame_offsets (B + 1) i32')
    n, C = points.shape
    B = frame_offsets.numel() - 1
    S = _candidates(cand, cand_obj, B)
    N = _database(db, C)
    if valid.dtype != torch.uint8 or tuple(valid.shape) != (B, S) or cand_rows.dtype != torch.int32 or \
            tuple(cand_rows.shape) != (B, S) or paste_counts.dtype != torch.int32 or paste_counts.numel() != B:
        raise CrbHipError('gt_sample_paste: valid (B, S) u8, cand_rows (B, S) i32, paste_counts (B) i32')
    capacity = int(capacity)
    if capacity < n:
        raise CrbHipError('gt_sample_paste: capacity below the number of scene points')
    dev = points.device
    out = torch.empty((capacity, C), dtype=torch.float32, device=dev)
    new_off = torch.empty((B + 2,), dtype=torch.int32, device=dev)
    ws_bytes = lib.crb_gt_sample_paste_workspace_bytes(n, B)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    rc = lib.crb_gt_sample_paste(ptr(points.contiguous()), n, C, ptr(frame_offsets.contiguous()), B, ptr(cand.contiguous()),
                                 ptr(cand_obj.contiguous()), S, ptr(valid.contiguous()), ptr(cand_rows.contiguous()),
                                 ptr(paste_counts.contiguous()), ptr(db['points']), ptr(db['obj_offsets']), N, capacity,
                                 ptr(out), ptr(new_off), ptr(ws), ws_bytes, cur_stream(dev))
    check(rc, 'crb_gt_sample_paste')
    if lazy:
        return out, new_off
    return out[:int(new_off[B])], new_off[:B + 1]              # the one sync
