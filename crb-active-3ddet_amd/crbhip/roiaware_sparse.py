"""RoI-aware pooling of all frames straight into the rows of the sparse RoI-grid tensor (csrc/roiaware_sparse.hip).

forward(rois, pts, frame_offsets, part, feat, out_size, max_pts) -> SparsePool or None
    rois (B, R, 7), pts (N, 3) stacked frame after frame, frame_offsets (B + 1) i32, part (N, 4) avg-pooled, feat (N, C)
    max-pooled. Launch sequence: count -> scan over the RoIs -> ONE read-back {rows, kept hits, flag} -> fill -> pool. The
    launch count does not depend on B. None when the device flag says that the result would follow another rule than the
    dense route's (a negative part feature inside a RoI): the caller takes the dense route for that call.
backward(sp, n_points, g_part, g_feat) -> grad_part (N, 4), grad_feat (N, C): fixed summation order, no read-back.

supported(out_size): the per-wave LDS histogram bounds out_x * out_y * out_z; larger grids belong to the dense route."""
import os
from collections import namedtuple

import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda

ENABLED = os.environ.get('CRB_ROIAWARE_SPARSE', '1') == '1'

FLAG_NEGATIVE = 1

SparsePool = namedtuple('SparsePool', 'coords part feat argmax row_ptr hit_pt hit_row')


def out_xyz(out_size):
    if isinstance(out_size, int):
        return out_size, out_size, out_size
    ox, oy, oz = [int(v) for v in out_size]
    return ox, oy, oz


def supported(out_size):
    ox, oy, oz = out_xyz(out_size)
    return ox * oy * oz <= lib.crb_roiaware_sparse_max_cells()


def forward(rois, pts, frame_offsets, part, feat, out_size, max_pts, extra_flags=None, buffers=None):
    """The stacked points must be grouped by frame (frame_offsets). A caller that cannot know whether they are hands its own device
    flag in as extra_flags, reads it from the same read-back, sorts and calls again: PartA2FCHead does so, which costs rows that are
    NOT grouped a second read-back (the first call then ran in bounds on offsets that mean nothing and its result is discarded).
    extra_flags: optional (k) i32 device tensor that rides in the same read-back (returned as ints after the SparsePool).
    buffers: optional callable (shape, dtype) -> tensor that supplies every output and workspace (tests hand in garbage)."""
    require_cuda(rois, pts, frame_offsets, part, feat)
    B, R = rois.shape[0], rois.shape[1]
    assert B >= 1 and R >= 1, 'no RoIs: nothing to pool (the caller takes the dense route)'
    assert rois.shape[2] == 7 and pts.shape[1] == 3 and part.shape[1] == 4 and frame_offsets.numel() == B + 1
    N, C = pts.shape[0], feat.shape[1]
    assert part.shape[0] == N and feat.shape[0] == N
    ox, oy, oz = out_xyz(out_size)
    dev = rois.device
    new = buffers or (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
    rois = rois.reshape(B * R, 7).contiguous().float()
    pts, part, feat = pts.contiguous().float(), part.contiguous().float(), feat.contiguous().float()
    off = frame_offsets.contiguous().to(torch.int32)
    st = cur_stream(dev)
    counts = new((B * R, 2), torch.int32)
    flag = new((1,), torch.int32)
    check(lib.crb_roiaware_sparse_count(B * R, R, B, N, max_pts, ox, oy, oz, ptr(rois), ptr(pts), ptr(off), ptr(part),
                                        ptr(counts), ptr(flag), st), 'crb_roiaware_sparse_count')
    ends = torch.cumsum(counts, 0, dtype=torch.int32)
    starts = (ends - counts).contiguous()
    tail = [ends[-1], flag]
    if extra_flags is not None:
        tail.append(extra_flags.to(torch.int32).view(-1))
    host = torch.cat(tail).tolist()                                  # the one read-back
    T, H, fl, extra = host[0], host[1], host[2], host[3:]
    if fl & FLAG_NEGATIVE:
        return (None, *extra) if extra_flags is not None else None
    coords = new((T, 4), torch.int32)
    row_ptr = new((T + 1,), torch.int32)
    hit_pt = new((H,), torch.int32)
    hit_row = new((H,), torch.int32)
    o_part = new((T, 4), torch.float32)
    o_feat = new((T, C), torch.float32)
    argmax = new((T, C), torch.int32)
    check(lib.crb_roiaware_sparse_fill(B * R, R, B, N, max_pts, ox, oy, oz, ptr(rois), ptr(pts), ptr(off), ptr(part),
                                       ptr(starts), T, H, ptr(coords), ptr(row_ptr), ptr(hit_pt), ptr(hit_row), st),
          'crb_roiaware_sparse_fill')
    check(lib.crb_roiaware_sparse_pool(T, C, ptr(row_ptr), ptr(hit_pt), ptr(part), ptr(feat), ptr(o_part), ptr(o_feat),
                                       ptr(argmax), st), 'crb_roiaware_sparse_pool')
    sp = SparsePool(coords, o_part, o_feat, argmax, row_ptr, hit_pt, hit_row)
    return (sp, *extra) if extra_flags is not None else sp


def backward(sp, n_points, g_part, g_feat, buffers=None):
    dev = g_part.device
    new = buffers or (lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev))
    T, C, H = sp.coords.shape[0], sp.feat.shape[1], sp.hit_pt.shape[0]
    g_part, g_feat = g_part.contiguous().float(), g_feat.contiguous().float()
    grad_part = new((n_points, 4), torch.float32)
    grad_feat = new((n_points, C), torch.float32)
    nbytes = lib.crb_roiaware_sparse_backward_workspace_bytes(n_points, H)
    ws = new((nbytes,), torch.uint8)
    check(lib.crb_roiaware_sparse_backward(n_points, T, H, C, ptr(sp.row_ptr), ptr(sp.hit_pt), ptr(sp.hit_row),
                                           ptr(sp.argmax), ptr(g_part), ptr(g_feat), ptr(grad_part), ptr(grad_feat), ptr(ws),
                                           nbytes, cur_stream(dev)), 'crb_roiaware_sparse_backward')
    return grad_part, grad_feat
