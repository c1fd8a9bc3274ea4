"""The up-sampling branches of the BEV backbone - transposed convolutions with kernel = stride (1 or 2), no padding, no bias - as row
GEMMs on the bf16 matrix pipe (csrc/rows_gemm4.hip): a channels_last map is the row matrix (pixels x channels), the layer is
X[N H W x Cin] . W[Cin x s s Cout] with the s * s result blocks of a row scattered to their output pixels. f32 in, f32 out; operands are
split exactly into three bf16 pieces and every product runs as six bf16 MFMA passes with f32 accumulation (the arithmetic of the
split-bf16 Winograd kernels). No atomics in any direction: two calls give the same bits.

CRB_ROWS_GEMM_KERNEL: 'x6' (default) = these kernels wherever they have an instance and their launch is switched on (LAUNCHES);
'vendor' = the path the layers took before (`up_conv` answers None and the caller runs MIOpen / CK / hipBLASLt): the A/B stand-in
and the tests' reference.
CRB_ROWS_GEMM_LAUNCHES: which of the six launches run on the new kernels, a comma list of <stride><direction> with direction
f = forward, i = input gradient, w = weight gradient; the default is the set that measured faster than what it replaces
(DESIGN.md section 6). A launch that is switched off or has no instance runs on the vendor kernel of that direction."""
import os

import numpy as np
import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

KERNEL = os.environ.get('CRB_ROWS_GEMM_KERNEL', 'x6')
DEFAULT_LAUNCHES = '1i,2f,2i,2w'
LAUNCHES = set(v.strip() for v in os.environ.get('CRB_ROWS_GEMM_LAUNCHES', DEFAULT_LAUNCHES).split(',') if v.strip())
FORWARD, INPUT_GRAD, WGRAD = 0, 1, 2
_DIR = 'fiw'


def supported(cin, cout, stride, direction):
    """has csrc/rows_gemm4.hip an instance for this layer and direction"""
    return bool(lib.crb_rows_gemm4_supported(int(cin), int(cout), int(stride), int(direction)))


def use(cin, cout, stride, direction):
    """does this launch run on the new kernel: the switch, the per-launch default and the instance"""
    return KERNEL == 'x6' and ('%d%s' % (stride, _DIR[direction])) in LAUNCHES and supported(cin, cout, stride, direction)


def _geometry(conv):
    """(cin, cout, stride, transposed) of a module `up_conv` can take, else None"""
    import torch.nn as nn
    if not isinstance(conv, (nn.Conv2d, nn.ConvTranspose2d)) or conv.bias is not None or conv.groups != 1:
        return None
    if conv.dilation != (1, 1) or conv.padding != (0, 0) or getattr(conv, 'padding_mode', 'zeros') != 'zeros':
        return None
    k, s = conv.kernel_size, conv.stride
    if k[0] != k[1] or s[0] != s[1] or k[0] != s[0] or s[0] not in (1, 2):
        return None
    transposed = isinstance(conv, nn.ConvTranspose2d)
    if transposed and conv.output_padding != (0, 0):
        return None
    if not transposed and s[0] != 1:               # a Conv2d with kernel = stride = 2 is a down-sampling layer: not this GEMM
        return None
    return conv.in_channels, conv.out_channels, s[0], transposed


def dispatch(conv, x):
    """which path `up_conv(conv, x)` takes and why: ('x6', launches on the new kernels) or ('vendor', reason)"""
    g = _geometry(conv)
    if KERNEL != 'x6':
        return 'vendor', 'CRB_ROWS_GEMM_KERNEL=%s' % KERNEL
    if g is None:
        return 'vendor', 'not a bias-free kernel = stride convolution with stride 1 or 2'
    if not (x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)):
        return 'vendor', 'input is not an f32 channels_last device map'
    cin, cout, s, _ = g
    on = [d for d in range(3) if use(cin, cout, s, d)]
    if not on:
        return 'vendor', 'no launch of %d -> %d stride %d is switched on with an instance' % (cin, cout, s)
    return 'x6', ''.join(_DIR[d] for d in on)


def _strides(weight, transposed):
    """element strides (s_ci, s_co, s_a, s_b) of a ConvTranspose2d weight (Cin,Cout,k,k) or a Conv2d 1x1 weight (Cout,Cin,1,1)"""
    st = weight.stride()
    return (st[0], st[1], st[2], st[3]) if transposed else (st[1], st[0], st[2], st[3])


# weight images: (weight memory, direction) -> (version, shape, strides, image, weight). An optimizer step bumps the version and the
# next call makes a new image; in a scoring pass over many frames the weight keeps its version and the image is made once
_IMAGES = {}


def weights(weight, cin, cout, stride, direction, transposed=True):
    """the split-bf16 image of `weight` for the forward (0) / input-gradient (1) kernel (crb_rows_gemm4_weights), cached per weight
    memory and version"""
    require_cuda(weight)
    w = weight.detach()
    key = (w.data_ptr(), w.device.index, int(direction))
    tag = (w._version, tuple(w.shape), tuple(w.stride()), cin, cout, stride, transposed)
    hit = _IMAGES.get(key)
    if hit is not None and hit[0] == tag:
        return hit[1]
    if w.dtype != torch.float32:
        raise CrbHipError('crb_rows_gemm4_weights takes f32 weights')
    img = torch.empty((int(lib.crb_rows_gemm4_weights_bytes(cin, cout, stride)),), dtype=torch.uint8, device=w.device)
    s_ci, s_co, s_a, s_b = _strides(w, transposed)
    check(lib.crb_rows_gemm4_weights(w.data_ptr(), s_ci, s_co, s_a, s_b, ptr(img), cin, cout, stride, int(direction),
                                     cur_stream(w.device)), 'crb_rows_gemm4_weights')
    if len(_IMAGES) > 64:
        _IMAGES.clear()
    _IMAGES[key] = (tag, img, w)               # (w keeps the storage alive: no other tensor can take the key's address meanwhile)
    return img


def weight_image_reference(w, stride, direction):
    """numpy restatement of the image layout: w (Cin,Cout,s,s) f32 array -> uint16 array [n / 32][K / 16][piece 3][lane 64][8] of the
    bf16 bit patterns. Wm[k][n]: forward k = ci, n = t Cout + co; input gradient k = t Cout + co, n = ci (t = a s + b); lane (r, h),
    element j of k step 2 c + u holds k = 32 c + 16 h + 8 u + j, n = 32 nb + r; pieces: x1 = high half of x, x2 = high half of
    x - x1, x3 = high half of x - x1 - x2 (both differences exact)."""
    w = np.asarray(w, dtype=np.float32)
    cin, cout, s = w.shape[0], w.shape[1], int(stride)
    T = s * s
    wm = w.reshape(cin, cout, T).transpose(0, 2, 1).reshape(cin, T * cout)          # [ci][t cout + co]
    if direction == INPUT_GRAD:
        wm = wm.T
    K, N = wm.shape
    ks, lane, j = np.meshgrid(np.arange(K // 16), np.arange(64), np.arange(8), indexing='ij')
    k = 32 * (ks >> 1) + 16 * (lane >> 5) + 8 * (ks & 1) + j
    r = lane & 31
    out = np.empty((N // 32, K // 16, 3, 64, 8), dtype=np.uint16)
    for nb in range(N // 32):
        v = np.ascontiguousarray(wm[k, 32 * nb + r])
        for p in range(3):
            hi = v.view(np.uint32) & np.uint32(0xffff0000)
            out[nb, :, p] = (hi >> np.uint32(16)).astype(np.uint16)
            v = v - hi.view(np.float32)
    return out


def _nhwc(x):
    if not x.is_contiguous(memory_format=torch.channels_last):
        x = x.contiguous(memory_format=torch.channels_last)
    return x.permute(0, 2, 3, 1)


def forward_x6(x, weight, cin, cout, s, transposed=True):
    """x (N,Cin,H,W) f32 channels_last -> y (N,Cout,sH,sW) channels_last (crb_rows_gemm4_forward)"""
    require_cuda(x, weight)
    xv = _nhwc(x)
    N, H, W, _ = xv.shape
    img = weights(weight, cin, cout, s, FORWARD, transposed)
    y = torch.empty((N, cout, s * H, s * W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    check(lib.crb_rows_gemm4_forward(xv.data_ptr(), ptr(img), y.data_ptr(), N, H, W, cin, cout, s, cur_stream(x.device)),
          'crb_rows_gemm4_forward')
    return y


def input_grad_x6(dy, weight, cin, cout, s, transposed=True):
    """dy (N,Cout,sH,sW) f32 channels_last -> dx (N,Cin,H,W) channels_last (crb_rows_gemm4_input_grad)"""
    require_cuda(dy, weight)
    gv = _nhwc(dy)
    N, Hs, Ws, _ = gv.shape
    H, W = Hs // s, Ws // s
    img = weights(weight, cin, cout, s, INPUT_GRAD, transposed)
    dx = torch.empty((N, cin, H, W), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last)
    check(lib.crb_rows_gemm4_input_grad(gv.data_ptr(), ptr(img), dx.data_ptr(), N, H, W, cin, cout, s, cur_stream(dy.device)),
          'crb_rows_gemm4_input_grad')
    return dx


_WGRAD_WS = {}


def wgrad_x6(x, dy, like, cin, cout, s, transposed=True):
    """x (N,Cin,H,W), dy (N,Cout,sH,sW) f32 channels_last -> gradient of the weight in the memory layout of `like`
    (crb_rows_gemm4_wgrad: partials per range of rows, added in range order in double)"""
    require_cuda(x, dy)
    xv, gv = _nhwc(x), _nhwc(dy)
    N, H, W, _ = xv.shape
    if tuple(gv.shape) != (N, s * H, s * W, cout):
        raise CrbHipError('rows_gemm wgrad: dy does not belong to x')
    dw = torch.empty_like(like, dtype=torch.float32)
    nbytes = int(lib.crb_rows_gemm4_wgrad_workspace_bytes(cin, cout, s))
    key = (x.device, torch.cuda.current_stream(x.device).cuda_stream)
    ws = _WGRAD_WS.get(key)                      # one per (device, stream): every call on a stream is ordered behind the last
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _WGRAD_WS[key] = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
    s_ci, s_co, s_a, s_b = _strides(dw, transposed)
    check(lib.crb_rows_gemm4_wgrad(xv.data_ptr(), gv.data_ptr(), dw.data_ptr(), s_ci, s_co, s_a, s_b, N, H, W, cin, cout, s, ptr(ws),
                                   ws.numel() * 4, cur_stream(x.device)), 'crb_rows_gemm4_wgrad')
    return dw


def _vendor_forward(x, weight, s, transposed):
    if s == 1:                                   # the row GEMM the layer ran as before (LinearRows)
        from pcdet.utils.linear_rows import rows_view, rows_to_nchw
        w2d = weight[:, :, 0, 0]
        w2d = w2d.t() if transposed else w2d     # (Cout, Cin)
        n, _, h, w_ = x.shape
        return rows_to_nchw(rows_view(x) @ w2d.t(), n, h, w_)
    return torch.nn.functional.conv_transpose2d(x, weight, None, s, 0)


class _UpConv(torch.autograd.Function):
    """y = conv_transpose2d(x, weight, stride = kernel = s) (or the 1x1 Conv2d): every direction on the new kernel where `use` says so,
    otherwise on the vendor kernel of that direction"""

    @staticmethod
    def forward(ctx, x, weight, cin, cout, s, transposed, det_wgrad=False):
        ctx.save_for_backward(x, weight)
        ctx.geo = (cin, cout, s, transposed)
        ctx.det_wgrad = det_wgrad
        if use(cin, cout, s, FORWARD):
            return forward_x6(x, weight, cin, cout, s, transposed)
        return _vendor_forward(x, weight, s, transposed)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        cin, cout, s, transposed = ctx.geo
        dy = dy.contiguous(memory_format=torch.channels_last)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            if use(cin, cout, s, INPUT_GRAD):
                dx = input_grad_x6(dy, weight, cin, cout, s, transposed)
            elif s == 1:
                from pcdet.utils.linear_rows import rows_view, rows_to_nchw
                w2d = weight[:, :, 0, 0]
                w2d = w2d.t() if transposed else w2d
                n, _, h, w_ = x.shape
                dx = rows_to_nchw(rows_view(dy) @ w2d, n, h, w_)
            else:
                dx = torch.ops.aten.convolution_backward(dy, x, weight, None, [s, s], [0, 0], [1, 1], True, [0, 0], 1,
                                                         [True, False, False])[0]
        if ctx.needs_input_grad[1]:
            if ctx.det_wgrad:                    # the deterministic mode's weight gradient of the strided branch keeps its kernel
                from . import dense_strided
                dw = dense_strided.weight_grad('deconv', x, dy, s, s, s, 0)
            elif use(cin, cout, s, WGRAD):
                dw = wgrad_x6(x, dy, weight, cin, cout, s, transposed)
            elif s == 1:
                from pcdet.utils.linear_rows import rows_view, tall_t_matmul
                d2 = tall_t_matmul(rows_view(dy), rows_view(x))                      # (Cout, Cin)
                dw = (d2.t() if transposed else d2).reshape(weight.shape)
            else:
                dw = torch.ops.aten.convolution_backward(dy, x, weight, None, [s, s], [0, 0], [1, 1], True, [0, 0], 1,
                                                         [False, True, False])[1]
        return dx, dw, None, None, None, None, None


def up_conv(conv, x):
    """conv(x) for the first module of an up-sampling branch on the row-GEMM kernels, or None when `dispatch` says vendor (the caller
    then runs the path it had).
    Deterministic mode (torch.use_deterministic_algorithms, grad enabled), stride-2 branch: the mode promises the default mode's
    gradients up to summation order, so forward and input gradient run on the same kernels as in the default mode (they are
    bit-reproducible) and only the weight gradient keeps the mode's own kernel (dense_strided.weight_grad). Where forward and input
    gradient are not both on the new kernels the answer is None and the caller keeps its dense_strided route whole."""
    path, _ = dispatch(conv, x)
    if path != 'x6':
        return None
    cin, cout, s, transposed = _geometry(conv)
    det_wgrad = False
    if s != 1 and torch.are_deterministic_algorithms_enabled() and torch.is_grad_enabled():
        from . import dense_strided
        if not (use(cin, cout, s, FORWARD) and use(cin, cout, s, INPUT_GRAD) and transposed and dense_strided.supported(conv, x)):
            return None
        det_wgrad = True
    return _UpConv.apply(x, conv.weight, cin, cout, s, transposed, det_wgrad)
