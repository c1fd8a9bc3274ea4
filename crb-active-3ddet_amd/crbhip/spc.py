"""Sectorized proposal-centric keypoint sampling (csrc/spc_sampling.hip): what sample_points_with_roi, sector_fps and the per-frame
loop of VoxelSetAbstraction.get_sampled_points of the reference compute, for all frames of a batch at once.

roi_proximity_mask   per point: is it within |dims / 2| + radius of its nearest RoI centre (one launch, no (N, R) tensor)
spc_plan             sectors, (frame, sector) segments in input order, per-segment quotas, keypoint counts (no read-back)
fps_segments         farthest-point sampling of every segment in one launch (the reference's stack kernel: 1024-thread tie rule)
spc_sample           the three in a row and ONE read-back (the header: segment / keypoint counts) -> keypoints (sum M_b, 4)
stack_fps            the reference's stack_farthest_point_sample: global indices into the stacked array

`points` is an (N, C) f32 matrix with x, y, z in columns col .. col + 2, rows stacked frame by frame; frame_offsets (B + 1) i32 on
the device."""
import ctypes
import math

import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

SEG_ROW = 8            # i32 per segment-table row: {first row, n, m, first output row, frame, 0, 0, 0}
REG_ROWS = 20480       # crb_fps_segments needs the distance array above this many rows


def frame_offsets(counts):
    """(B) per-frame row counts on the device -> (B + 1) i32 offsets, no read-back"""
    B = counts.shape[0]
    before = torch.ones((B + 1, B), dtype=torch.int32, device=counts.device).tril(-1)       # row b: frames 0 .. b - 1
    return (before * counts.to(torch.int32)[None, :]).sum(1, dtype=torch.int32)            # (an integer sum: no cumsum launch, which torch
    #                                                                                          refuses under use_deterministic_algorithms)


def _xyz_ptr(points, col):
    require_cuda(points)
    if points.dim() != 2 or points.dtype != torch.float32 or not points.is_contiguous() or col < 0 or col + 3 > points.shape[1]:
        raise CrbHipError('crb_spc: points (N, C) contiguous f32 with x, y, z in columns col .. col + 2 expected')
    ptr(points)                                            # (kept alive until check())
    return ctypes.c_void_p(points.data_ptr() + 4 * col) if points.shape[0] else None


def _check_offsets(off, B):
    require_cuda(off)
    if off.dtype != torch.int32 or off.dim() != 1 or off.shape[0] != B + 1 or not off.is_contiguous():
        raise CrbHipError('crb_spc: frame_offsets (B + 1) i32 expected')


@torch.no_grad()
def roi_proximity_mask(points, col, off, rois, radius, want_nearest=False):
    """rois (B, R, 7+) -> mask (N) bool [, nearest (N) i32]"""
    require_cuda(rois)
    if rois.dim() != 3 or rois.dtype != torch.float32 or (rois.shape[1] > 0 and rois.shape[2] < 6):
        raise CrbHipError('crb_roi_proximity_mask: rois (B, R, 7+) f32 expected')
    rois = rois.contiguous()
    B, R = int(rois.shape[0]), int(rois.shape[1])
    _check_offsets(off, B)
    N = int(points.shape[0])
    mask = torch.empty((N,), dtype=torch.uint8, device=points.device)
    nearest = torch.empty((N,), dtype=torch.int32, device=points.device) if want_nearest else None
    check(lib.crb_roi_proximity_mask(_xyz_ptr(points, col), N, int(points.shape[1]), ptr(off), B, ptr(rois), R, int(rois.shape[2]),
                                     float(radius), ptr(mask), ptr(nearest), cur_stream(points.device)), 'crb_roi_proximity_mask')
    mask = mask.view(torch.bool)
    return (mask, nearest) if want_nearest else mask


def inv_sector_size(num_sectors):
    """1.f / (float)(2 pi / S): the f32 reciprocal torch's device division by a host scalar multiplies with"""
    size = torch.tensor(math.pi * 2 / num_sectors, dtype=torch.float32)
    return float(torch.tensor(1.0, dtype=torch.float32) / size)


@torch.no_grad()
def spc_plan(points, col, off, mask, num_sectors, num_keypoints):
    """-> dict(sector (N) u8, xyz (N, 3) compacted segment points, src (N) i32 their rows, seg (B * S, 8) i32, header (3 + B) i32);
    the valid lengths are in the header: [segments, compacted rows, keypoints, keypoints per frame]"""
    B, S, K = int(off.shape[0]) - 1, int(num_sectors), int(num_keypoints)
    _check_offsets(off, B)
    require_cuda(mask)
    N, dev = int(points.shape[0]), points.device
    if mask.shape != (N,) or mask.dtype not in (torch.bool, torch.uint8):
        raise CrbHipError('crb_spc_plan: mask (N) bool expected')
    mask = mask.contiguous().view(torch.uint8)
    out = {'sector': torch.empty((N,), dtype=torch.uint8, device=dev), 'xyz': torch.empty((N, 3), dtype=torch.float32, device=dev),
           'src': torch.empty((N,), dtype=torch.int32, device=dev), 'seg': torch.zeros((max(B * S, 1), SEG_ROW), dtype=torch.int32, device=dev),
           'header': torch.empty((3 + B,), dtype=torch.int32, device=dev)}
    nbytes = int(lib.crb_spc_plan_workspace_bytes(B, S))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    check(lib.crb_spc_plan(_xyz_ptr(points, col), N, int(points.shape[1]), ptr(off), B, ptr(mask), S, K, inv_sector_size(S),
                           ptr(out['sector']), ptr(out['xyz']), ptr(out['src']), ptr(out['seg']), ptr(out['header']), ptr(ws), nbytes,
                           cur_stream(dev)), 'crb_spc_plan')
    return out


@torch.no_grad()
def fps_segments(xyz, seg, num_segments, out_capacity, want_idx=True, want_keypoints=False):
    """xyz (rows, 3) f32; seg (max_segments, 8) i32 table; num_segments: device i32 scalar tensor or None (all rows of seg).
    -> (idx (out_capacity) i32 or None, keypoints (out_capacity, 4) or None); rows no segment writes stay as allocated (zero)"""
    require_cuda(xyz, seg, num_segments)
    if xyz.dim() != 2 or xyz.shape[1] != 3 or xyz.dtype != torch.float32 or seg.dtype != torch.int32 or seg.dim() != 2 or seg.shape[1] != SEG_ROW:
        raise CrbHipError('crb_fps_segments: xyz (rows, 3) f32 and seg (segments, 8) i32 expected')
    xyz, seg = xyz.contiguous(), seg.contiguous()
    rows, dev = int(xyz.shape[0]), xyz.device
    idx = torch.zeros((out_capacity,), dtype=torch.int32, device=dev) if want_idx else None
    kp = torch.zeros((out_capacity, 4), dtype=torch.float32, device=dev) if want_keypoints else None
    temp = torch.empty((rows,), dtype=torch.float32, device=dev) if rows > REG_ROWS else None
    check(lib.crb_fps_segments(ptr(xyz), rows, ptr(seg), ptr(num_segments), int(seg.shape[0]), int(out_capacity), ptr(temp), ptr(idx),
                               ptr(kp), cur_stream(dev)), 'crb_fps_segments')
    return idx, kp


@torch.no_grad()
def spc_sample(points, col, off, rois, radius, num_sectors, num_keypoints):
    """-> (keypoints (sum M_b, 4) [frame, x, y, z], per-frame keypoint counts (list)); frames in order, sectors ascending inside a
    frame, picks in pick order inside a sector. One read-back."""
    B, S, K = int(off.shape[0]) - 1, int(num_sectors), int(num_keypoints)
    mask = roi_proximity_mask(points, col, off, rois, radius)
    plan = spc_plan(points, col, off, mask, S, K)
    _, kp = fps_segments(plan['xyz'], plan['seg'], plan['header'][0:1], B * (K + S), want_idx=False, want_keypoints=True)
    header = plan['header'].cpu().tolist()                  # the one read-back of the sampling
    return kp[:header[2]], header[3:]


@torch.no_grad()
def stack_fps(xyz, xyz_batch_cnt, num_sampled_points):
    """stacked xyz (N, 3), per-segment counts and quotas (lists, or tensors anywhere) -> (sum m) i32 GLOBAL row indices, the
    reference's stack_farthest_point_sample (m is clamped to n)"""
    dev = xyz.device
    n = torch.as_tensor(xyz_batch_cnt, dtype=torch.int32).to(dev).view(-1)
    m = torch.minimum(torch.as_tensor(num_sampled_points, dtype=torch.int32).to(dev).view(-1), n)
    total = int(sum(min(int(a), int(b)) for a, b in zip(_host_list(num_sampled_points), _host_list(xyz_batch_cnt))))
    seg = torch.zeros((n.shape[0], SEG_ROW), dtype=torch.int32, device=dev)
    seg[:, 0] = frame_offsets(n)[:-1]
    seg[:, 1] = n
    seg[:, 2] = m
    seg[:, 3] = frame_offsets(m)[:-1]
    idx, _ = fps_segments(xyz, seg, None, total)
    return idx


def _host_list(v):
    return [int(x) for x in (v.tolist() if isinstance(v, torch.Tensor) else v)]
