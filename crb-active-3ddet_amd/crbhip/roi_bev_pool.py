"""Rotated grid pooling of the NHWC BEV map under the first-stage proposals, all frames in one HIP launch (csrc/roi_bev_pool.hip).

Host mirror of SECONDHead.roi_grid_pool (pcdet/models/roi_heads/second_head.py:53-110). No backward: the reference detaches the map
and the RoIs before it pools."""
import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError


@torch.no_grad()
def roi_bev_pool(bev, rois, grid_size, x_min, y_min, cell_x, cell_y):
    """bev (B,H,W,C) f32 NHWC contiguous, rois (B,R,7+) -> (B*R, G*G, C) rows, grid point j * G + i (row j, column i) of RoI n in
    row (n, j * G + i); `as_nchw` turns them into the reference's (B*R, C, G, G) view"""
    require_cuda(bev, rois)
    if bev.dim() != 4 or rois.dim() != 3 or rois.shape[0] != bev.shape[0] or bev.dtype != torch.float32:
        raise CrbHipError('crb_roi_bev_pool: bev (B,H,W,C) f32 and rois (B,R,7+) of the same B expected')
    bev = bev.detach()
    if not bev.is_contiguous():
        raise CrbHipError('crb_roi_bev_pool: the map must be NHWC-contiguous (it is never copied or transposed here)')
    rois = rois.detach().contiguous().float()
    B, H, W, C = (int(v) for v in bev.shape)
    R, G = int(rois.shape[1]), int(grid_size)
    out = torch.empty((B * R, max(G, 0) ** 2, C), dtype=torch.float32, device=bev.device)
    check(lib.crb_roi_bev_pool(ptr(bev), B, H, W, C, ptr(rois), int(rois.shape[-1]), R, G, float(x_min), float(y_min), float(cell_x),
                               float(cell_y), ptr(out), cur_stream(bev.device)), 'crb_roi_bev_pool')
    return out


def as_nchw(rows, grid_size):
    """(N, G*G, C) rows -> the logical (N, C, G, G) tensor of the reference as a permuted view (no copy)"""
    n, _, c = rows.shape
    return rows.view(n, grid_size, grid_size, c).permute(0, 3, 1, 2)
