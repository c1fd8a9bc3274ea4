"""Dynamic voxelization and the segmented mean (csrc/dyn_voxelize.hip): what DynamicPillarVFE and DynamicMeanVFE of the reference
take from torch.unique and torch_scatter.

dyn_voxelize groups the rows of `points` (N, 1 + C) [b, x, y, z, ...] by cell, with no cap on points per voxel or on voxels: voxels in
ascending key order (torch.unique's order), points of a voxel in input order. One read-back of (M, Nk) sizes the outputs.
dyn_mean reduces the point features over those variable-length segments; there is no gradient (the reference's forward is no_grad).
dyn_canonical_order re-orders the points inside every voxel by content, for sums that must not depend on the order of the input."""
import ctypes

import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, host_f32x3, host_i32x3, CrbHipError
from .pillar_vfe import batch_stats, param_grads

PILLAR, VOXEL = 0, 1                       # CRB_DYN_PILLAR, CRB_DYN_VOXEL


def _check_points(points):
    require_cuda(points)
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < 4:
        raise CrbHipError('crb_dyn_voxelize: points (N, 1 + C) f32 rows [b, x, y, z, ...] expected')


@torch.no_grad()
def dyn_voxelize(points, batch_size, point_cloud_range, voxel_size, grid_size, mode):
    """points (N, 1 + C) f32 on the device; mode PILLAR (x, y masked; coords [b, 0, cy, cx]) or VOXEL (x, y, z masked; coords
    [b, cz, cy, cx]) -> dict(perm (Nk) i32: point rows voxel by voxel, seg_offsets (M + 1) i32, coords (M, 4) i32, M, Nk)"""
    _check_points(points)
    if mode not in (PILLAR, VOXEL):
        raise CrbHipError('crb_dyn_voxelize: mode PILLAR or VOXEL expected')
    points = points.contiguous()
    N, dev = int(points.shape[0]), points.device
    grid = [int(g) for g in grid_size]
    cells = int(batch_size) * grid[0] * grid[1] * (grid[2] if mode == VOXEL else 1)
    cap = max(min(N, cells), 0)
    perm = torch.empty((N,), dtype=torch.int32, device=dev)
    seg = torch.empty((cap + 1,), dtype=torch.int32, device=dev)
    coords = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    counts = torch.empty((2,), dtype=torch.int32, device=dev)
    nbytes = int(lib.crb_dyn_voxelize_workspace_bytes(N))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    check(lib.crb_dyn_voxelize(ptr(points), N, int(points.shape[1]), int(batch_size), int(mode), host_f32x3(point_cloud_range[:3]),
                               host_f32x3(voxel_size), host_i32x3(grid), cap, ptr(perm), ptr(seg), ptr(coords), ptr(counts), ptr(ws),
                               nbytes, cur_stream(dev)), 'crb_dyn_voxelize')
    M, Nk = (int(v) for v in counts.cpu())                  # the one read-back of the forward pass
    return {'perm': perm[:Nk], 'seg_offsets': seg[:M + 1], 'coords': coords[:M], 'M': M, 'Nk': Nk}


@torch.no_grad()
def dyn_mean(points, perm, seg_offsets):
    """(M, C) f32 means of columns 1 .. C of `points` over the segments of dyn_voxelize (f64 sums in segment order, rounded once)"""
    _check_points(points)
    require_cuda(perm, seg_offsets)
    if perm.dtype != torch.int32 or seg_offsets.dtype != torch.int32 or seg_offsets.dim() != 1 or seg_offsets.shape[0] < 1:
        raise CrbHipError('crb_dyn_mean_vfe: perm (Nk) i32, seg_offsets (M + 1) i32 expected')
    points, perm, seg_offsets = points.contiguous(), perm.contiguous(), seg_offsets.contiguous()
    M, C = int(seg_offsets.shape[0]) - 1, int(points.shape[1]) - 1
    out = torch.empty((M, C), dtype=torch.float32, device=points.device)
    if M > 0:
        check(lib.crb_dyn_mean_vfe(ptr(points), int(points.shape[0]), C + 1, C, ptr(perm), ptr(seg_offsets), M, ptr(out),
                                   cur_stream(points.device)), 'crb_dyn_mean_vfe')
    return out


@torch.no_grad()
def dyn_canonical_order(points, seg):
    """seg of dyn_voxelize -> the same segments with the points of every voxel ordered by content (the bit patterns of columns 1 .. C,
    column 1 most significant) instead of input order: what a sum in segment order then gives is a function of the set of rows alone"""
    _check_points(points)
    points, perm = points.contiguous(), seg['perm'].contiguous()
    Nk, M, dev = int(seg['Nk']), int(seg['M']), points.device
    out = torch.empty_like(perm)
    if Nk > 0:
        nbytes = int(lib.crb_dyn_canonical_order_workspace_bytes(Nk))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        check(lib.crb_dyn_canonical_order(ptr(points), int(points.shape[0]), int(points.shape[1]), int(points.shape[1]) - 1, ptr(perm), Nk,
                                          ptr(seg['seg_offsets']), M, ptr(out), ptr(ws), nbytes, cur_stream(dev)), 'crb_dyn_canonical_order')
    return dict(seg, perm=out)


# ---- the fused two-layer pillar net of DynamicPillarVFE (csrc/dyn_pillar_vfe.hip) -------------------------------------------------
# Layer 1 is the single-layer algebra of crbhip/pillar_vfe.py with n = Nk (no padded slots): batch statistics from the moments S1, S2,
# folded affine A1, b1, and dW1 / dgamma1 / dbeta1 in closed form from G1 = sum dy1 f^T, G0 = sum dy1. Layer 2's statistics are not
# linear in f: y = W2 [x1; x_max] is summed by a pass of its own (sum y, sum y^2), and its backward is BatchNorm through the batch
# statistics as usual: dbeta2 = sum dy2, dgamma2 = sum dy2 yhat2 (pass A, over the selected points), dx2 = scale2 (dy2 - dbeta2 / n -
# yhat2 dgamma2 / n) over all points (pass B), dW2 = sum dx2 [x1; x_max]^T. All algebra here is f64 element-wise products and
# torch.sum on the device: bit-reproducible. Every kernel sums in segment order, and dyn_pillar_net puts the points of a pillar into
# canonical order first (dyn_canonical_order), so a permutation of the input rows changes no bit of any output, gradient or statistic.
H1, COUT = 32, 64
_KS = 12


class _Args(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ('points', 'perm', 'seg_offsets', 'coords', 'pillar_mean', 'A1', 'b1', 'W2', 'scale2', 'shift2',
                                               'mean2', 'inv_sigma2', 'k1', 'k2')] + \
               [('n_points', ctypes.c_int64), ('M', ctypes.c_int64), ('row_stride', ctypes.c_int32), ('C', ctypes.c_int32),
                ('voxel_xy', ctypes.c_float * 2), ('offsets', ctypes.c_float * 3)]


def pillar_supported(C, num_filters):
    """the configurations the kernels take (crb_dyn_pillar_vfe_supported): C in {4, 5}, NUM_FILTERS [64, 64]"""
    nf = [int(v) for v in num_filters]
    return bool(lib.crb_dyn_pillar_vfe_supported(int(C), len(nf), nf[0] if nf else 0, nf[1] if len(nf) > 1 else 0))


def _args(points, seg, pmean, voxel_size, offsets, **tensors):
    a = _Args()
    keep = [points, seg['perm'], seg['seg_offsets'], seg['coords'], pmean]
    a.points, a.perm, a.seg_offsets, a.coords, a.pillar_mean = (t.data_ptr() for t in keep)
    for k, t in tensors.items():
        t = t.contiguous()
        keep.append(t)
        setattr(a, k, t.data_ptr())
    a.n_points, a.M, a.row_stride, a.C = int(points.shape[0]), int(seg['M']), int(points.shape[1]), int(points.shape[1]) - 1
    a.voxel_xy = (ctypes.c_float * 2)(float(voxel_size[0]), float(voxel_size[1]))
    a.offsets = (ctypes.c_float * 3)(*[float(v) for v in offsets])
    return a, keep


def _workspace(M, dev):
    nbytes = int(lib.crb_dyn_pillar_workspace_bytes(int(M)))
    return torch.empty((nbytes // 8,), dtype=torch.float64, device=dev), nbytes


@torch.no_grad()
def pillar_moments(points, seg, pmean, voxel_size, offsets):
    """-> (S1 (K), S2 (K, K)) f64: sum f and sum f f^T over all kept points"""
    K, dev = int(points.shape[1]) + 5, points.device
    nm = int(lib.crb_dyn_pillar_num_moments(K - 6))
    sums = torch.empty((nm,), dtype=torch.float64, device=dev)
    ws, nbytes = _workspace(seg['M'], dev)
    a, keep = _args(points, seg, pmean, voxel_size, offsets)
    check(lib.crb_dyn_pillar_moments(ctypes.byref(a), ptr(sums), ptr(ws), nbytes, cur_stream(dev)), 'crb_dyn_pillar_moments')
    iu = torch.triu_indices(K + 1, K + 1, device=dev)[:, :nm]
    G = torch.zeros((K + 1, K + 1), dtype=torch.float64, device=dev)
    G[iu[0], iu[1]] = sums
    G[iu[1], iu[0]] = sums
    return G[:K, K].clone(), G[:K, :K].clone()


class _DynPillarNet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W1, g1, be1, W2, g2, be2, points, seg, pmean, rm1, rv1, rm2, rv2, training, momentum, eps, voxel_size, offsets):
        dev, M, n = points.device, int(seg['M']), float(seg['Nk'])
        W1d, W2f = W1.detach().double(), W2.detach().float().contiguous()
        ws, nbytes = _workspace(M, dev)
        if training:
            S1, S2 = pillar_moments(points, seg, pmean, voxel_size, offsets)
            mean1, var1, WS2 = batch_stats(W1d, S1, S2, n)
        else:
            S1 = WS2 = None
            mean1, var1 = rm1.detach().double(), rv1.detach().double()
        sigma1 = torch.sqrt(var1 + eps)
        scale1 = g1.detach().double() / sigma1
        A1 = (scale1[:, None] * W1d).float().contiguous()
        b1 = (be1.detach().double() - mean1 * scale1).float().contiguous()
        if training:
            sums = torch.empty((2 * COUT,), dtype=torch.float64, device=dev)
            a, keep = _args(points, seg, pmean, voxel_size, offsets, A1=A1, b1=b1, W2=W2f)
            check(lib.crb_dyn_pillar_stats2(ctypes.byref(a), ptr(sums), ptr(ws), nbytes, cur_stream(dev)), 'crb_dyn_pillar_stats2')
            mean2 = sums[:COUT] / n
            var2 = (sums[COUT:] / n - mean2 * mean2).clamp(min=0)
            with torch.no_grad():
                unb = n / max(n - 1, 1)
                for rm, rv, mean, var in ((rm1, rv1, mean1, var1), (rm2, rv2, mean2, var2)):
                    if rm is not None:
                        rm.copy_((1 - momentum) * rm.double() + momentum * mean)
                        rv.copy_((1 - momentum) * rv.double() + momentum * var * unb)
        else:
            mean2, var2 = rm2.detach().double(), rv2.detach().double()
        sigma2 = torch.sqrt(var2 + eps)
        scale2 = g2.detach().double() / sigma2
        shift2 = be2.detach().double() - mean2 * scale2
        dev_f = dict(A1=A1, b1=b1, W2=W2f, scale2=scale2.float(), shift2=shift2.float())
        out = torch.empty((M, COUT), dtype=torch.float32, device=dev)
        a, keep = _args(points, seg, pmean, voxel_size, offsets, **dev_f)
        check(lib.crb_dyn_pillar_forward(ctypes.byref(a), ptr(out), cur_stream(dev)), 'crb_dyn_pillar_forward')
        ctx.save_for_backward(points, seg['perm'], seg['seg_offsets'], seg['coords'], pmean, A1, b1, W2f, dev_f['scale2'], dev_f['shift2'],
                              W1d, mean1, sigma1, scale1, S1, WS2, mean2, sigma2, scale2)
        ctx.meta = (training, n, M, int(seg['Nk']), tuple(voxel_size), tuple(offsets))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (points, perm, seg_offsets, coords, pmean, A1, b1, W2f, scale2f, shift2f, W1d, mean1, sigma1, scale1, S1, WS2, mean2, sigma2,
         scale2) = ctx.saved_tensors
        training, n, M, Nk, voxel_size, offsets = ctx.meta
        dev = points.device
        seg = {'perm': perm, 'seg_offsets': seg_offsets, 'coords': coords, 'M': M, 'Nk': Nk}
        g = grad_out.contiguous().float()
        ws, nbytes = _workspace(M, dev)
        dev_f = dict(A1=A1, b1=b1, W2=W2f, scale2=scale2f, shift2=shift2f, mean2=mean2.float(), inv_sigma2=(1.0 / sigma2).float())
        arg2 = torch.empty((M, COUT), dtype=torch.int32, device=dev)
        sums = torch.empty((2 * COUT,), dtype=torch.float64, device=dev)
        a, keep = _args(points, seg, pmean, voxel_size, offsets, **dev_f)
        check(lib.crb_dyn_pillar_backward_a(ctypes.byref(a), ptr(g), ptr(arg2), ptr(sums), ptr(ws), nbytes, cur_stream(dev)),
              'crb_dyn_pillar_backward_a')
        dbeta2, dgamma2 = sums[:COUT], sums[COUT:]
        zero = torch.zeros_like(dbeta2)
        dev_f['k1'] = ((dbeta2 / n) if training else zero).float()
        dev_f['k2'] = ((dgamma2 / n) if training else zero).float()
        d = torch.empty((COUT * COUT + H1 * _KS,), dtype=torch.float64, device=dev)
        a, keep = _args(points, seg, pmean, voxel_size, offsets, **dev_f)
        check(lib.crb_dyn_pillar_backward_b(ctypes.byref(a), ptr(g), ptr(arg2), ptr(d), ptr(ws), nbytes, cur_stream(dev)),
              'crb_dyn_pillar_backward_b')
        K = int(points.shape[1]) + 5
        dW2 = d[:COUT * COUT].view(COUT, COUT)
        G = d[COUT * COUT:].view(H1, _KS)
        dW1, dgamma1, dbeta1 = param_grads(W1d, mean1, sigma1, scale1, G[:, :K], G[:, K], n, S1 if training else None, WS2)
        return (dW1.float(), dgamma1.float(), dbeta1.float(), dW2.float(), dgamma2.float(), dbeta2.float()) + (None,) * 12


def dyn_pillar_net(points, seg, weight1, gamma1, beta1, weight2, gamma2, beta2, running1, running2, training, momentum, eps, voxel_size,
                   offsets):
    """points (N, 1 + C) f32; seg = dyn_voxelize(..., PILLAR); weight1 (32, C + 6), weight2 (64, 64), gamma / beta of the two BatchNorm1d
    (differentiable); running1 / running2 = (running_mean, running_var) of each, updated in place when training (unbiased variance,
    n = Nk), the statistics used otherwise -> (M, 64). There is no gradient to the points."""
    _check_points(points)
    C = int(points.shape[1]) - 1
    if tuple(weight1.shape) != (H1, C + 6) or tuple(weight2.shape) != (COUT, COUT) or not pillar_supported(C, [COUT, COUT]):
        raise CrbHipError('crb_dyn_pillar_vfe: CRB_ERR_UNSUPPORTED (C in {4, 5}, weights (32, C + 6) and (64, 64); got C=%d, %s, %s)'
                          % (C, tuple(weight1.shape), tuple(weight2.shape)))
    require_cuda(weight1, gamma1, beta1, weight2, gamma2, beta2, *running1, *running2)          # (a None is passed over)
    if not training and any(t is None for t in tuple(running1) + tuple(running2)):
        raise CrbHipError('crb_dyn_pillar_vfe: eval mode needs the running statistics')
    if training and seg['Nk'] == 1:
        raise ValueError('Expected more than 1 value per channel when training, got input size torch.Size([1, %d])' % H1)
    if seg['M'] == 0:
        return torch.zeros((0, COUT), dtype=torch.float32, device=points.device) + 0 * (weight1.sum() + weight2.sum())
    points = points.detach().contiguous()
    seg = dyn_canonical_order(points, seg)
    pmean = dyn_mean(points, seg['perm'], seg['seg_offsets'])
    return _DynPillarNet.apply(weight1, gamma1, beta1, weight2, gamma2, beta2, points, seg, pmean, running1[0], running1[1], running2[0],
                               running2[1], bool(training), float(momentum), float(eps), [float(v) for v in voxel_size],
                               [float(v) for v in offsets])
