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
crb_bn_relu_backward); with 'sums' off the function keeps the map for the weight gradient as LinearRows does.
CRB_HEAD_BN_FORWARD: '1' (default) = the forward of the same region without the map, a switch of its own beside the two above:
`bnrelu.bn_relu_concat(defer=True)` runs the statistics launches only and returns a Record that carries no map,
`linear_deferred(record, w, b)` forms relu(bn(x)) in registers and multiplies it into the head's outputs (head_bn_forward_kernel), and
its backward is the backward above as CRB_HEAD_BN and CRB_HEAD_BN_LAUNCHES switch it (with CRB_HEAD_BN=0 the launches the head took
before, on a map that the apply launches write again for the weight gradient: an extra pass the old path did not have, so a
timing A/B of the backward switches CRB_HEAD_BN_FORWARD off in both runs). `dispatch_forward` says which way a pending record
goes; with '0', with 'sums' switched off or on a rejected shape the caller calls `record.materialize()` and takes the path above."""
import os

import torch

from ._lib import lib, check, ptr, cur_stream

ENABLED = os.environ.get('CRB_HEAD_BN', '1') == '1'
DEFAULT_LAUNCHES = 'sums,apply'
LAUNCHES = set(v.strip() for v in os.environ.get('CRB_HEAD_BN_LAUNCHES', DEFAULT_LAUNCHES).split(',') if v.strip())
FORWARD = os.environ.get('CRB_HEAD_BN_FORWARD', '1') == '1'

# When set to a list, every fused backward appends what it launched ('sums', 'apply', 'vendor_sums', 'vendor_apply'): the tests read it
TRACE = None
# When set to a list, every fused forward on a pending record appends 'forward'
TRACE_FORWARD = None


def supported(widths, K):
    """has csrc/head_bn.hip an instance for branches of these widths and a head with K outputs"""
    widths = [int(v) for v in widths]
    return len(widths) > 0 and len(set(widths)) == 1 and bool(lib.crb_head_bn_supported(len(widths), widths[0], int(K)))


class Record(object):
    """what `bn_relu_concat` notes on the map it wrote: the tensors given to it (graph inputs), the contiguous branch inputs with
    their statistics and parameters as the kernels read them, and the map's address and shape. A pending record
    (`bn_relu_concat(defer=True)`) has no map yet: `rows_ptr` is None, `rows_shape` is the shape the map would have, and
    `materialize()` writes it."""

    def __init__(self, rows, inputs, saved, relu):
        if rows is None:
            self.rows_ptr, self.rows_shape = None, (saved[0][0].shape[0], sum(s[0].shape[1] for s in saved))
        else:
            self.rows_ptr, self.rows_shape = rows.data_ptr(), tuple(rows.shape)     # the (n, sum C_i) map (no reference: no cycle)
        self.inputs = inputs                # [(x_i, gamma_i, beta_i)] as given: the tensors the gradients belong to
        self.saved = saved                  # [(x_i contiguous, mean_i, invstd_i, gamma_i f32, beta_i f32)]
        self.relu = bool(relu)
        self.nhw = None                     # (N, H, W) of the map as an image, noted by the backbone on a pending record

    @property
    def widths(self):
        return [s[0].shape[1] for s in self.saved]

    @property
    def pending(self):
        return self.rows_ptr is None

    @property
    def n(self):
        return self.rows_shape[0]

    def materialize(self):
        """the map of a pending record, written by the apply launches from the stored statistics (the running statistics are not
        advanced again): the tensor `bn_relu_concat(defer=False)` returns - same values, same backward, same `_crb_head_bn` note"""
        from . import bnrelu
        return bnrelu.materialize_concat(self)


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


def dispatch_forward(record, K):
    """which way a pending record goes and why: ('fused', what runs on the new kernels) = `linear_deferred`, or ('vendor', reason) =
    `record.materialize()` and the path `dispatch` picks for the map"""
    if not FORWARD:
        return 'vendor', 'CRB_HEAD_BN_FORWARD=0'
    if record is None or not record.pending:
        return 'vendor', 'no pending record (the map is written)'
    if ENABLED and 'sums' not in LAUNCHES:
        return 'vendor', "'sums' is not in CRB_HEAD_BN_LAUNCHES: the weight gradient reads the map"
    if not torch.is_grad_enabled():
        return 'vendor', 'grad mode is off'
    if not record.relu:
        return 'vendor', 'BatchNorm without ReLU'
    if not supported(record.widths, K):
        return 'vendor', 'no instance for widths %s with K = %d' % (record.widths, K)
    return 'fused', ','.join(['forward'] + (sorted(LAUNCHES & {'sums', 'apply'}) if ENABLED else []))


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


def forward(xs, par, w, b, K):
    """crb_bn_head_forward_weights + crb_bn_head_forward: -> out (n, K) = relu(bn(x)) w^T + b"""
    n, width, nb = xs[0].shape[0], xs[0].shape[1], len(xs)
    img = torch.empty((int(lib.crb_bn_head_forward_weights_bytes(nb, width, K)),), dtype=torch.uint8, device=w.device)
    check(lib.crb_bn_head_forward_weights(ptr(w), ptr(img), nb, width, K, cur_stream(w.device)), 'crb_bn_head_forward_weights')
    out = torch.empty((n, K), dtype=torch.float32, device=w.device)
    check(lib.crb_bn_head_forward(ptr(xs[0]), ptr(xs[1]), ptr(par), ptr(img), ptr(b), n, nb, width, K, ptr(out),
                                  cur_stream(w.device)), 'crb_bn_head_forward')
    return out


def _note(what, quiet=False):
    if TRACE is not None and not quiet:
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
        if dy is None:
            return (None,) * (4 + 3 * ctx.nb)
        t = ctx.saved_tensors
        need = ctx.needs_input_grad
        rows = t[-1] if 'sums' not in ctx.launches else None
        return (None,) + _backward(ctx, dy, t[0], t[1:1 + 5 * ctx.nb], rows, need[1], need[2], need[4:])


def _backward(ctx, dy, w, flat, rows, need_w, need_b, need_branch):
    """the fused backward both functions share -> (dw, db, None for the record, then dx, dgamma, dbeta per branch). `flat`: the
    record's saved tensors, `rows`: the map when 'sums' is off, `need_branch`: needs_input_grad of (x, gamma, beta) per branch"""
    nb, quiet = ctx.nb, getattr(ctx, 'quiet', False)       # quiet: CRB_HEAD_BN=0 under the deferred forward, nothing fused to note
    w = w.contiguous()
    saved = [flat[5 * i:5 + 5 * i] for i in range(nb)]
    xs = [s[0] for s in saved]
    need_x = any(need_branch[3 * i] for i in range(nb))
    need_gb = any(need_branch[1 + 3 * i] or need_branch[2 + 3 * i] for i in range(nb))
    dy = dy.contiguous().float()
    K, width = w.shape[0], xs[0].shape[1]
    dw = db = dgb = None
    dxs = [None] * nb
    dz = None
    if need_w or need_gb or need_x:
        par = params(saved)
        if 'sums' in ctx.launches:
            _note('sums', quiet)
            dgb, dw, db = finalize(sums(xs, par, dy, K), w, par, nb, width, K, want_bias=need_b)
        else:
            # the launches the sums replace: dz = dOut W, one reduce pass per branch, the sliced weight-gradient GEMM, the column sum
            from pcdet.utils.linear_rows import tall_t_matmul
            from . import bnrelu
            _note('vendor_sums', quiet)
            dz = dy @ w
            dgb = torch.empty((2, nb * width), dtype=torch.float32, device=dy.device)
            for i, (x, mean, invstd, g, be) in enumerate(saved):
                dgb[:, i * width:(i + 1) * width] = torch.stack(bnrelu.concat_reduce(x, dz, i * width, mean, invstd, g, be))
            dw = tall_t_matmul(dy, rows) if need_w else None
        if need_x:
            if 'apply' in ctx.launches:
                _note('apply', quiet)
                dxs = apply(xs, par, dgb, dy, w, K)
            else:
                # the launches the apply replaces: dz = dOut W and crb_bn_relu_backward per branch (its own reduce pass included)
                from . import bnrelu
                _note('vendor_apply', quiet)
                dz = dy @ w if dz is None else dz
                dxs = [bnrelu.concat_backward(x, dz, i * width, mean, invstd, g, be)[0]
                       for i, (x, mean, invstd, g, be) in enumerate(saved)]
    if need_b and db is None:
        db = dy.sum(0)
    grads = [dw if need_w else None, db if need_b else None, None]
    for i in range(nb):
        sl = slice(i * width, (i + 1) * width)
        grads += [dxs[i] if need_branch[3 * i] else None,
                  dgb[1, sl] if (dgb is not None and need_branch[1 + 3 * i]) else None,
                  dgb[0, sl] if (dgb is not None and need_branch[2 + 3 * i]) else None]
    return tuple(grads)


class _HeadBNDeferred(torch.autograd.Function):
    """out = relu(bn(x)) w^T + b from the branch inputs of a pending record (head_bn_forward_kernel: the map is never written);
    backward: `_HeadBN`'s, or with CRB_HEAD_BN=0 the launches it replaces - the map their weight gradient reads is written again by
    the apply launches and dropped. Arguments: w (K, Ct), b (K), record, then (x, gamma, beta) per branch."""

    @staticmethod
    def forward(ctx, w, b, record, *branch):
        ctx.set_materialize_grads(False)
        ctx.nb = len(record.saved)
        ctx.launches = set(LAUNCHES) if ENABLED else set()
        ctx.quiet = not ENABLED
        flat = [t for s in record.saved for t in s]
        ctx.save_for_backward(w, *flat)
        if TRACE_FORWARD is not None:
            TRACE_FORWARD.append('forward')
        return forward([s[0] for s in record.saved], params(record.saved), w.contiguous(), b.contiguous().float(), w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        if dy is None:
            return (None,) * (3 + 3 * ctx.nb)
        t = ctx.saved_tensors
        need = ctx.needs_input_grad
        rows = None
        if 'sums' not in ctx.launches and need[0]:
            from . import bnrelu
            rows = bnrelu.concat_apply([t[1 + 5 * i:6 + 5 * i] for i in range(ctx.nb)], True)
        return _backward(ctx, dy, t[0], t[1:], rows, need[0], need[1], need[3:])


def linear_deferred(record, w, b):
    """relu(bn(x)) w^T + b of a pending record without its map, or None when `dispatch_forward` says vendor or the head is not a plain
    f32 (K, Ct) matrix with a bias (the caller then materializes the record and runs the path it had)"""
    path, _ = dispatch_forward(record, w.shape[0])
    if path != 'fused':
        return None
    if b is None or w.dim() != 2 or w.dtype != torch.float32 or w.shape[1] != record.rows_shape[1]:
        return None
    branch = [t for trio in record.inputs for t in trio]
    return _HeadBNDeferred.apply(w, b, record, *branch)


def linear(rows, w, b, record):
    """rows w^T + b with the fused backward, or None when `dispatch` says vendor (the caller then runs the path it had)"""
    path, _ = dispatch(rows, record, w.shape[0])
    if path != 'fused':
        return None
    if b is None or w.dim() != 2 or w.dtype != torch.float32 or w.shape[1] != rows.shape[1]:
        return None
    branch = [t for trio in record.inputs for t in trio]
    return _HeadBN.apply(rows, w, b, record, *branch)
