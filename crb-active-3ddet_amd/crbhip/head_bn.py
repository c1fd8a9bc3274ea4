"""The anchor head's backward inside the backward of the concatenated up-sampling BatchNorm (csrc/head_bn.hip).

The head out = z W^T + b reads the concatenated map z = relu(bn_i(x_i)) (n, sum C_i) that `bnrelu.bn_relu_concat` wrote. Its input
gradient dz = dOut W has rank K (72 at the KITTI head) and BatchNorm backward is linear in it, so the head's weight gradient, the
BatchNorm parameter gradients and the branch input gradients all follow from dOut, the branch inputs and W: dz is never written and z
is not kept for backward. `bn_relu_concat` notes on the map what that takes (`_crb_head_bn`, the pattern of `_crb_bn_slabs`);
`linear(rows, w, b)` runs one autograd function over the map, W, b, the branch inputs and their gamma / beta, whose backward returns
None for the map and the fused gradients for everything else.

CRB_HEAD_BN: '1' (default) = the fused backward wherever `dispatch` finds an instance; '0' = the path the head took before
(`linear` answers None and the caller runs LinearRows): the A/B stand-in and the tests' reference.
CRB_HEAD_BN_LAUNCHES: which of the two streaming launches run on the new kernels, a comma list of 'sums' (P2 / P3 sums + finalize:
dW, db, dgamma, dbeta) and 'apply' (dx). A launch that is switched off runs on the kernels it replaces (the vendor GEMMs and
crb_bn_relu_backward); with 'sums' off the function keeps the map for the weight gradient as LinearRows does."""
import os

import torch

from ._lib import lib, check, ptr, cur_stream

ENABLED = os.environ.get('CRB_HEAD_BN', '1') == '1'
DEFAULT_LAUNCHES = 'sums,apply'
LAUNCHES = set(v.strip() for v in os.environ.get('CRB_HEAD_BN_LAUNCHES', DEFAULT_LAUNCHES).split(',') if v.strip())

# When set to a list, every fused backward appends what it launched ('sums', 'apply', 'vendor_sums', 'vendor_apply'): the tests read it
TRACE = None


def supported(widths, K):
    """has csrc/head_bn.hip an instance for branches of these widths and a head with K outputs"""
    widths = [int(v) for v in widths]
    return len(widths) > 0 and len(set(widths)) == 1 and bool(lib.crb_head_bn_supported(len(widths), widths[0], int(K)))


class Record(object):
    """what `bn_relu_concat` notes on the map it wrote: the tensors given to it (graph inputs), the contiguous branch inputs with
    their statistics and parameters as the kernels read them, and the map's address and shape"""

    def __init__(self, rows, inputs, saved, relu):
        self.rows_ptr, self.rows_shape = rows.data_ptr(), tuple(rows.shape)     # the (n, sum C_i) map (no reference: no cycle)
        self.inputs = inputs                # [(x_i, gamma_i, beta_i)] as given: the tensors the gradients belong to
        self.saved = saved                  # [(x_i contiguous, mean_i, invstd_i, gamma_i f32, beta_i f32)]
        self.relu = bool(relu)

    @property
    def widths(self):
        return [s[0].shape[1] for s in self.saved]


def dispatch(rows, record, K):
    """which path `linear` takes and why: ('fused', launches on the new kernels) or ('vendor', reason)"""
    if not ENABLED:
        return 'vendor', 'CRB_HEAD_BN=0'
    if record is None:
        return 'vendor', 'the map carries no BatchNorm record (eval mode, grad mode off, frame_groups or another producer)'
    if not torch.is_grad_enabled():
        return 'vendor', 'grad mode is off'
    if not (rows.is_cuda and rows.dim() == 2 and rows.dtype == torch.float32 and rows.is_contiguous()):
        return 'vendor', 'the map is not a contiguous f32 device row matrix'
    if rows.data_ptr() != record.rows_ptr or tuple(rows.shape) != record.rows_shape:
        return 'vendor', 'the record belongs to another map'
    if not record.relu:
        return 'vendor', 'BatchNorm without ReLU'
    if not supported(record.widths, K):
        return 'vendor', 'no instance for widths %s with K = %d' % (record.widths, K)
    return 'fused', ','.join(sorted(LAUNCHES & {'sums', 'apply'}))


_WS = {}


def _workspace(dev, nbytes):
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _WS.get(key)                         # one per (device, stream): every call on a stream is ordered behind the last
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def params(saved):
    """(4, Ct) f32: mean | invstd | gamma | beta of the concatenated channels"""
    return torch.cat([torch.stack([s[1], s[2], s[3], s[4]]) for s in saved], 1).contiguous()


def sums(xs, par, dout, K):
    """crb_head_bn_sums: f64 (2 K Ct + K) = P2 | P3 | column sums of dOut"""
    n, width, nb = xs[0].shape[0], xs[0].shape[1], len(xs)
    out = torch.empty((int(lib.crb_head_bn_sums_count(nb, width, K)),), dtype=torch.float64, device=dout.device)
    nbytes = int(lib.crb_head_bn_workspace_bytes(nb, width, K))
    ws = _workspace(dout.device, nbytes)
    check(lib.crb_head_bn_sums(ptr(xs[0]), ptr(xs[1]), ptr(par), ptr(dout), n, nb, width, K, ptr(out), ptr(ws), ws.numel(),
                               cur_stream(dout.device)), 'crb_head_bn_sums')
    return out


def finalize(s, w, par, nb, width, K, want_bias=True):
    """crb_head_bn_finalize: -> dgb (2, Ct) = dbeta | dgamma, dw (K, Ct), dbias (K) or None"""
    Ct = nb * width
    dgb = torch.empty((2, Ct), dtype=torch.float32, device=w.device)
    dw = torch.empty((K, Ct), dtype=torch.float32, device=w.device)
    db = torch.empty((K,), dtype=torch.float32, device=w.device) if want_bias else None
    check(lib.crb_head_bn_finalize(ptr(s), ptr(w), ptr(par), nb, width, K, ptr(dgb), ptr(dw), ptr(db), cur_stream(w.device)),
          'crb_head_bn_finalize')
    return dgb, dw, db


def apply(xs, par, dgb, dout, w, K):
    """crb_head_bn_weights + crb_head_bn_apply: -> [dx_i (n, width)]"""
    n, width, nb = xs[0].shape[0], xs[0].shape[1], len(xs)
    img = torch.empty((int(lib.crb_head_bn_weights_bytes(nb, width, K)),), dtype=torch.uint8, device=w.device)
    check(lib.crb_head_bn_weights(ptr(w), ptr(img), nb, width, K, cur_stream(w.device)), 'crb_head_bn_weights')
    dxs = [torch.empty_like(x) for x in xs]
    check(lib.crb_head_bn_apply(ptr(xs[0]), ptr(xs[1]), ptr(par), ptr(dgb), ptr(dout), ptr(img), n, nb, width, K, ptr(dxs[0]),
                                ptr(dxs[1]), cur_stream(w.device)), 'crb_head_bn_apply')
    return dxs


def _note(what):
    if TRACE is not None:
        TRACE.append(what)


class _HeadBN(torch.autograd.Function):
    """out = rows w^T + b on the vendor GEMM; backward: None for the map, the fused gradients for w, b and per branch x, gamma, beta.
    Arguments: rows, w (K, Ct), b (K), record, then (x, gamma, beta) per branch - the tensors `bn_relu_concat` was given."""

    @staticmethod
    def forward(ctx, rows, w, b, record, *branch):
        ctx.set_materialize_grads(False)
        ctx.nb = len(record.saved)
        ctx.launches = set(LAUNCHES)             # as switched at the forward: with 'sums' off the map is kept for the weight gradient
        flat = [t for s in record.saved for t in s]
        ctx.save_for_backward(w, *(flat + ([rows] if 'sums' not in ctx.launches else [])))
        return torch.addmm(b, rows, w.t())

    @staticmethod
    def backward(ctx, dy):
        nb = ctx.nb
        none = (None,) * (4 + 3 * nb)
        if dy is None:
            return none
        t = ctx.saved_tensors
        w = t[0].contiguous()
        saved = [t[1 + 5 * i:6 + 5 * i] for i in range(nb)]
        xs = [s[0] for s in saved]
        need = ctx.needs_input_grad
        need_x = any(need[4 + 3 * i] for i in range(nb))
        need_gb = any(need[5 + 3 * i] or need[6 + 3 * i] for i in range(nb))
        dy = dy.contiguous().float()
        K, width = w.shape[0], xs[0].shape[1]
        dw = db = dgb = None
        dxs = [None] * nb
        dz = None
        if need[1] or need_gb or need_x:
            par = params(saved)
            if 'sums' in ctx.launches:
                _note('sums')
                dgb, dw, db = finalize(sums(xs, par, dy, K), w, par, nb, width, K, want_bias=need[2])
            else:
                # the launches the sums replace: dz = dOut W, one reduce pass per branch, the sliced weight-gradient GEMM, the column sum
                from pcdet.utils.linear_rows import tall_t_matmul
                from . import bnrelu
                _note('vendor_sums')
                dz = dy @ w
                dgb = torch.empty((2, nb * width), dtype=torch.float32, device=dy.device)
                for i, (x, mean, invstd, g, be) in enumerate(saved):
                    dgb[:, i * width:(i + 1) * width] = torch.stack(bnrelu.concat_reduce(x, dz, i * width, mean, invstd, g, be))
                dw = tall_t_matmul(dy, t[-1]) if need[1] else None
            if need_x:
                if 'apply' in ctx.launches:
                    _note('apply')
                    dxs = apply(xs, par, dgb, dy, w, K)
                else:
                    # the launches the apply replaces: dz = dOut W and crb_bn_relu_backward per branch (its own reduce pass included)
                    from . import bnrelu
                    _note('vendor_apply')
                    dz = dy @ w if dz is None else dz
                    dxs = [bnrelu.concat_backward(x, dz, i * width, mean, invstd, g, be)[0]
                           for i, (x, mean, invstd, g, be) in enumerate(saved)]
        if need[2] and db is None:
            db = dy.sum(0)
        grads = [None, dw if need[1] else None, db if need[2] else None, None]
        for i in range(nb):
            sl = slice(i * width, (i + 1) * width)
            grads += [dxs[i] if need[4 + 3 * i] else None,
                      dgb[1, sl] if (dgb is not None and need[5 + 3 * i]) else None,
                      dgb[0, sl] if (dgb is not None and need[6 + 3 * i]) else None]
        return tuple(grads)


def linear(rows, w, b, record):
    """rows w^T + b with the fused backward, or None when `dispatch` says vendor (the caller then runs the path it had)"""
    path, _ = dispatch(rows, record, w.shape[0])
    if path != 'fused':
        return None
    if b is None or w.dim() != 2 or w.dtype != torch.float32 or w.shape[1] != rows.shape[1]:
        return None
    branch = [t for trio in record.inputs for t in trio]
    return _HeadBN.apply(rows, w, b, record, *branch)
