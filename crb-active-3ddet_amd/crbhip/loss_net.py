"""LLAL loss-prediction module (LossNet) as two HIP launches forward and two backward (csrc/loss_net.hip).

Host side of LossNet.forward (pcdet/models/roi_heads/loss_net.py:54-70) and its autograd for f32 device tensors: the latents are the
post-ReLU outputs of the RoI head's shared FC layers, (frames * rows_per_frame, C_k[, 1]); the result is the (frames, 1) loss
prediction. Train mode updates the BatchNorm running statistics and num_batches_tracked in place, as torch does."""
import ctypes

import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

MAX_LAYERS = 4


class LossNetArgs(ctypes.Structure):
    """CrbLossNetArgs of include/crb_hip.h"""
    _fields_ = [('x', ctypes.c_void_p * MAX_LAYERS), ('w', ctypes.c_void_p * MAX_LAYERS), ('gamma', ctypes.c_void_p * MAX_LAYERS),
                ('beta', ctypes.c_void_p * MAX_LAYERS), ('running_mean', ctypes.c_void_p * MAX_LAYERS),
                ('running_var', ctypes.c_void_p * MAX_LAYERS), ('num_batches_tracked', ctypes.c_void_p * MAX_LAYERS),
                ('channels', ctypes.c_int32 * MAX_LAYERS), ('num_layer', ctypes.c_int32), ('rows_per_frame', ctypes.c_int32),
                ('frames', ctypes.c_int32), ('training', ctypes.c_int32), ('momentum', ctypes.c_float), ('eps', ctypes.c_float)]


class LossNetGrads(ctypes.Structure):
    """CrbLossNetGrads of include/crb_hip.h"""
    _fields_ = [('d_x', ctypes.c_void_p * MAX_LAYERS), ('d_w', ctypes.c_void_p * MAX_LAYERS), ('d_gamma_beta', ctypes.c_void_p),
                ('d_lin_w', ctypes.c_void_p), ('d_lin_b', ctypes.c_void_p)]


def _addr(t):
    return None if t is None else t.data_ptr()


def _args(xs, ws, gammas, betas, bufs, frames, rows_per_frame, training, momentum, eps):
    a = LossNetArgs()
    for k, (x, w, g, b, (rm, rv, nbt)) in enumerate(zip(xs, ws, gammas, betas, bufs)):
        a.x[k], a.w[k], a.gamma[k], a.beta[k] = _addr(x), _addr(w), _addr(g), _addr(b)
        a.running_mean[k], a.running_var[k], a.num_batches_tracked[k] = _addr(rm), _addr(rv), _addr(nbt)
        a.channels[k] = int(w.numel())
    a.num_layer, a.rows_per_frame, a.frames, a.training = len(xs), int(rows_per_frame), int(frames), 1 if training else 0
    a.momentum, a.eps = float(momentum), float(eps)
    return a


class _LossNet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, meta, *tensors):
        L, frames, P, training, momentum, eps, bufs = meta
        xs, ws, gammas, betas = tensors[:L], tensors[L:2 * L], tensors[2 * L:3 * L], tensors[3 * L:4 * L]
        lin_w, lin_b = tensors[4 * L], tensors[4 * L + 1]
        dev = xs[0].device
        args = _args(xs, ws, gammas, betas, bufs, frames, P, training, momentum, eps)
        wsb = lib.crb_lossnet_workspace_bytes(L, frames * P)
        work = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        out = torch.empty((frames, 1), dtype=torch.float32, device=dev)
        check(lib.crb_lossnet_forward(ctypes.byref(args), ptr(lin_w), ptr(lin_b), ptr(out), ptr(work), wsb, cur_stream(dev)),
              'crb_lossnet_forward')
        ctx.meta = meta
        ctx.save_for_backward(*xs, *ws, *gammas, *betas, lin_w, work)
        return out

    @staticmethod
    def backward(ctx, d_out):
        L, frames, P, training, momentum, eps, bufs = ctx.meta
        saved = ctx.saved_tensors
        xs, ws, gammas, betas = saved[:L], saved[L:2 * L], saved[2 * L:3 * L], saved[3 * L:4 * L]
        lin_w, work = saved[4 * L], saved[4 * L + 1]
        dev = xs[0].device
        args = _args(xs, ws, gammas, betas, bufs, frames, P, training, momentum, eps)
        g = d_out.contiguous().float()
        dxs = [torch.empty_like(x) if ctx.needs_input_grad[1 + k] else None for k, x in enumerate(xs)]
        dws = [torch.empty_like(w) for w in ws]
        dgb = torch.empty((2 * L,), dtype=torch.float32, device=dev)
        dlw = torch.empty_like(lin_w)
        dlb = torch.empty((1,), dtype=torch.float32, device=dev)
        gr = LossNetGrads()
        for k in range(L):
            gr.d_x[k], gr.d_w[k] = _addr(dxs[k]), _addr(dws[k])
        gr.d_gamma_beta, gr.d_lin_w, gr.d_lin_b = _addr(dgb), _addr(dlw), _addr(dlb)
        check(lib.crb_lossnet_backward(ctypes.byref(args), ptr(lin_w), ptr(g), ptr(work), int(work.numel()), ctypes.byref(gr),
                                       cur_stream(dev)), 'crb_lossnet_backward')
        d_gamma = [dgb[2 * k:2 * k + 1] for k in range(L)]
        d_beta = [dgb[2 * k + 1:2 * k + 2] for k in range(L)]
        return (None, *dxs, *dws, *d_gamma, *d_beta, dlw.view_as(lin_w), dlb)


def loss_net(module, features, batch_size):
    """LossNet `module` (pcdet/models/roi_heads/loss_net.py) on device latents `features` (one per layer) -> (batch_size, 1)"""
    L = module.num_layer
    if len(features) != L:
        raise CrbHipError('LossNet: %d latent tensors for %d layers' % (len(features), L))
    require_cuda(*features)
    rows = int(features[0].shape[0])
    P = module.rows_per_frame
    if rows != batch_size * P:
        raise CrbHipError('LossNet: %d RoI rows for %d frames, the linear layer needs %d rows per frame' % (rows, batch_size, P))
    if L > MAX_LAYERS:
        raise CrbHipError('LossNet: at most %d layers, got %d' % (MAX_LAYERS, L))
    xs, ws, gammas, betas, bufs = [], [], [], [], []
    momentum = eps = None
    for k in range(L):
        conv, bn = getattr(module, 'conv_%d' % k), getattr(module, 'bn_%d' % k)
        x = features[k]
        if x.dtype != torch.float32 or conv.weight.dtype != torch.float32:
            raise CrbHipError('LossNet: the HIP path takes f32 tensors')
        if x.shape[0] != rows or x.numel() != rows * conv.in_channels:
            raise CrbHipError('LossNet: latent %d has shape %s, expected (%d, %d[, 1])' % (k, tuple(x.shape), rows, conv.in_channels))
        if bn.momentum is None or not bn.track_running_stats or not bn.affine:
            raise CrbHipError('LossNet: the HIP path implements BatchNorm1d with momentum, running statistics and affine parameters')
        if momentum is not None and (bn.momentum != momentum or bn.eps != eps):
            raise CrbHipError('LossNet: all bn_k must share momentum and eps')
        momentum, eps = bn.momentum, bn.eps
        xs.append(x.contiguous())
        ws.append(conv.weight)
        gammas.append(bn.weight)
        betas.append(bn.bias)
        bufs.append((bn.running_mean, bn.running_var, bn.num_batches_tracked))
    lin = module.linear
    if lin.weight.numel() != L * P:
        raise CrbHipError('LossNet: linear layer has %d inputs, expected %d' % (lin.weight.numel(), L * P))
    modes = {getattr(module, 'bn_%d' % k).training for k in range(L)}
    if len(modes) != 1:
        raise CrbHipError('LossNet: the HIP path runs every bn_k in one mode, got some in train and some in eval mode')
    training = modes.pop()
    meta = (L, int(batch_size), P, training, momentum, eps, bufs)
    return _LossNet.apply(meta, *xs, *ws, *gammas, *betas, lin.weight, lin.bias)
