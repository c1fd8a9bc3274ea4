"""The fused pillar feature net of PointPillars (csrc/pillar_vfe.hip): PillarVFE with one PFNLayer, i.e. Linear(K -> 64, no bias) +
BatchNorm1d + ReLU + max over the T slots of a pillar, without any (M, T, .) tensor in either direction.

The kernels sum; the small algebra around them (K = C + 6 <= 11, 64 channels) runs here in f64 torch ops on the device, element-wise
products and torch.sum only, so every result is bit-reproducible from call to call.

With x = w_c . f (no bias), n = M * T entries per channel (padded slots are exact zeros that count in n) and the moments
S1 = sum f, S2 = sum f f^T over the valid slots:
    mean_c = w_c . S1 / n,   E[x^2]_c = w_c^T S2 w_c / n,   var_c = E[x^2]_c - mean_c^2,   sigma_c = sqrt(var_c + eps)
    scale_c = gamma_c / sigma_c,   A = diag(scale) W,   b = beta - mean * scale,   out = max_t relu(A f_t + b)
Backward, with dy the gradient at the BatchNorm output (grad_out at the selected slot), G1 = sum dy f^T, G0 = sum dy:
    dbeta = G0,   dgamma_c = sum dy xhat = (w_c . G1_c - mean_c G0_c) / sigma_c          (xhat = (w_c . f - mean_c) / sigma_c is linear in f)
    dx = scale (dy - G0 / n - xhat dgamma / n)                                           (BatchNorm through its batch statistics)
    dW_c = sum_rows dx f^T = scale_c [G1_c - (G0_c / n) S1^T - (dgamma_c / n) sum xhat f^T],   sum xhat f^T = (w_c^T S2 - mean_c S1^T) / sigma_c
In eval mode the statistics are constants: dW = scale G1, dgamma = (w . G1 - running_mean G0) / sigma, dbeta = G0."""
import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, host_f32x3, CrbHipError

COUT = 64


def supported(C, T, Cout=COUT):
    """the shapes the kernels take (crb_pillar_vfe_supported): C in {4, 5}, 1 <= T <= 32, Cout == 64"""
    return bool(lib.crb_pillar_vfe_supported(int(C), int(T), int(Cout)))


def _check_inputs(voxels, num_points, coords):
    require_cuda(voxels, num_points, coords)
    if voxels.dim() != 3 or voxels.dtype != torch.float32 or num_points.dtype != torch.int32 or coords.dtype != torch.int32 or \
            coords.dim() != 2 or coords.shape[1] != 4 or coords.shape[0] != voxels.shape[0] or num_points.shape[0] != voxels.shape[0]:
        raise CrbHipError('crb_pillar_vfe: voxels (M,T,C) f32, num_points (M) int32, coords (M,4) int32 [b,z,y,x] expected')
    if voxels.shape[0] < 1:
        raise CrbHipError('crb_pillar_vfe: no pillars')


@torch.no_grad()
def moments(voxels, num_points, coords, voxel_size, offsets):
    """-> (S1 (K), S2 (K,K)) f64: sum f and sum f f^T over the valid slots of all pillars"""
    _check_inputs(voxels, num_points, coords)
    voxels, num_points, coords = voxels.contiguous(), num_points.contiguous(), coords.contiguous()
    M, T, C = (int(v) for v in voxels.shape)
    K, dev = C + 6, voxels.device
    nm = int(lib.crb_pillar_vfe_num_moments(C))
    sums = torch.empty((nm,), dtype=torch.float64, device=dev)
    nbytes = int(lib.crb_pillar_vfe_moments_workspace_bytes(M, C))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    check(lib.crb_pillar_vfe_moments(ptr(voxels), ptr(num_points), ptr(coords), M, T, C, host_f32x3(voxel_size), host_f32x3(offsets),
                                     ptr(sums), ptr(ws), nbytes, cur_stream(dev)), 'crb_pillar_vfe_moments')
    iu = torch.triu_indices(K + 1, K + 1, device=dev)[:, :nm]          # row-major upper triangle; the (K, K) corner is the last entry
    G = torch.zeros((K + 1, K + 1), dtype=torch.float64, device=dev)
    G[iu[0], iu[1]] = sums
    G[iu[1], iu[0]] = sums
    return G[:K, K].clone(), G[:K, :K].clone()


def _rowdot(a, b):
    return (a * b).sum(1)


def batch_stats(W, S1, S2, n):
    """W (64,K), S1 (K), S2 (K,K) f64 -> mean (64), biased var (64), WS2 (64,K) = rows w_c^T S2 (plain tensor algebra, any device)"""
    mean = (W * S1[None, :]).sum(1) / n
    WS2 = (W[:, :, None] * S2[None, :, :]).sum(1)
    return mean, (_rowdot(WS2, W) / n - mean * mean).clamp(min=0), WS2


def param_grads(W, mean, sigma, scale, G1, G0, n=None, S1=None, WS2=None):
    """the closed form of the module docstring, f64 -> dW (64,K), dgamma (64), dbeta (64). With S1 / WS2 (training): through the batch
    statistics; without: the statistics are constants (eval mode)."""
    dgamma = (_rowdot(W, G1) - mean * G0) / sigma
    if S1 is None:
        return scale[:, None] * G1, dgamma, G0
    Sxf = (WS2 - mean[:, None] * S1[None, :]) / sigma[:, None]
    return scale[:, None] * (G1 - (G0 / n)[:, None] * S1[None, :] - (dgamma / n)[:, None] * Sxf), dgamma, G0


class _PillarVFE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, gamma, beta, voxels, num_points, coords, running_mean, running_var, training, momentum, eps, voxel_size,
                offsets):
        M, T, C = (int(v) for v in voxels.shape)
        dev = voxels.device
        W = weight.detach().double()
        n = float(M * T)
        if training:
            S1, S2 = moments(voxels, num_points, coords, voxel_size, offsets)
            mean, var, WS2 = batch_stats(W, S1, S2, n)
            if running_mean is not None:
                with torch.no_grad():
                    running_mean.copy_((1 - momentum) * running_mean.double() + momentum * mean)
                    running_var.copy_((1 - momentum) * running_var.double() + momentum * var * (n / max(n - 1, 1)))
        else:
            S1 = S2 = WS2 = None
            mean, var = running_mean.detach().double(), running_var.detach().double()
        sigma = torch.sqrt(var + eps)
        scale = gamma.detach().double() / sigma
        A = (scale[:, None] * W).float().contiguous()
        b = (beta.detach().double() - mean * scale).float().contiguous()
        out = torch.empty((M, COUT), dtype=torch.float32, device=dev)
        vs, of = host_f32x3(voxel_size), host_f32x3(offsets)
        check(lib.crb_pillar_vfe_forward(ptr(voxels), ptr(num_points), ptr(coords), M, T, C, vs, of, ptr(A), ptr(b), COUT, ptr(out),
                                         cur_stream(dev)), 'crb_pillar_vfe_forward')
        ctx.save_for_backward(voxels, num_points, coords, A, b, W, mean, sigma, scale, S1, WS2)
        ctx.meta = (training, n, tuple(voxel_size), tuple(offsets))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        voxels, num_points, coords, A, b, W, mean, sigma, scale, S1, WS2 = ctx.saved_tensors
        training, n, voxel_size, offsets = ctx.meta
        M, T, C = (int(v) for v in voxels.shape)
        K, dev = C + 6, voxels.device
        g = grad_out.contiguous().float()
        d = torch.empty((COUT, K + 1), dtype=torch.float64, device=dev)
        nbytes = int(lib.crb_pillar_vfe_backward_workspace_bytes(M, C, COUT))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        check(lib.crb_pillar_vfe_backward(ptr(g), ptr(voxels), ptr(num_points), ptr(coords), M, T, C, host_f32x3(voxel_size),
                                          host_f32x3(offsets), ptr(A), ptr(b), COUT, ptr(d), ptr(ws), nbytes, cur_stream(dev)),
              'crb_pillar_vfe_backward')
        dW, dgamma, dbeta = param_grads(W, mean, sigma, scale, d[:, :K], d[:, K], n, S1 if training else None, WS2)
        return (dW.float(), dgamma.float(), dbeta.float()) + (None,) * 10


def pillar_vfe(voxels, num_points, coords, weight, gamma, beta, running_mean, running_var, training, momentum, eps, voxel_size, offsets):
    """voxels (M,T,C), num_points (M) i32, coords (M,4) i32 [b,z,y,x]; weight (64,K), gamma / beta (64) (differentiable);
    running_mean / running_var (64): updated in place when training (unbiased variance, `momentum`), the statistics used otherwise
    -> (M,64). There is no gradient to the points."""
    _check_inputs(voxels, num_points, coords)
    require_cuda(weight, gamma, beta, running_mean, running_var)
    M, T, C = (int(v) for v in voxels.shape)
    if tuple(weight.shape) != (COUT, C + 6) or not supported(C, T, weight.shape[0]):
        raise CrbHipError('crb_pillar_vfe: CRB_ERR_UNSUPPORTED (C in {4, 5}, 1 <= T <= 32, weight (64, C + 6); got C=%d T=%d weight %s)'
                          % (C, T, tuple(weight.shape)))
    if not training and (running_mean is None or running_var is None):
        raise CrbHipError('crb_pillar_vfe: eval mode needs the running statistics')
    return _PillarVFE.apply(weight, gamma, beta, voxels.detach().contiguous(), num_points.contiguous(), coords.contiguous(),
                            running_mean, running_var, bool(training), float(momentum), float(eps),
                            [float(v) for v in voxel_size], [float(v) for v in offsets])
