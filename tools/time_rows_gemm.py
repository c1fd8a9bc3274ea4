"""The six launches of the BEV up-sampling branches (two layers x forward / input gradient / weight gradient) on the split-bf16 row-GEMM
kernels (csrc/rows_gemm4.hip) against the vendor kernels they replace, alternated in one process, with medians; and each side's
distance from an f64 evaluation on the same inputs.
  python tools/time_rows_gemm.py [--pairs 15] [--batch 16] [--out profiles/time_rows_gemm4_X.txt] [--no-errors]
Every timed call works on one of three buffer sets in rotation (1.4 - 2.2 GB in total: more than the 256 MB of last-level cache), as in
the training step, where the operands were written by other kernels a while ago."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))

from crbhip import rows_gemm  # noqa: E402
from pcdet.utils.linear_rows import rows_view, tall_t_matmul  # noqa: E402

LAYERS = (('k1s1', 128, 256, 1, 200, 176), ('k2s2', 256, 256, 2, 100, 88))


def f64_all(x, w, dy, s):
    """(y, dx, dw) of conv_transpose2d(x, w, stride = kernel = s) in f64, as GEMMs on the row matrices"""
    N, cin, H, W = x.shape
    cout = w.shape[1]
    xr = x.permute(0, 2, 3, 1).reshape(-1, cin).double()
    wm = w.double().permute(0, 2, 3, 1).reshape(cin, s * s * cout)                       # [ci][(a, b, co)]
    y = (xr @ wm).view(N, H, W, s, s, cout).permute(0, 1, 3, 2, 4, 5).reshape(N, s * H, s * W, cout)
    dyr = dy.permute(0, 2, 3, 1).double().reshape(N, H, s, W, s, cout).permute(0, 1, 3, 2, 4, 5).reshape(-1, s * s * cout)
    dx = (dyr @ wm.t()).view(N, H, W, cin)
    dw = (xr.t() @ dyr).view(cin, s, s, cout).permute(0, 3, 1, 2)
    return y.permute(0, 3, 1, 2), dx.permute(0, 3, 1, 2), dw


def rel_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def calls(x, w, dy, cin, cout, s):
    """direction -> (new, vendor) callables"""
    def v_f():
        return rows_gemm._vendor_forward(x, w, s, True)

    def v_i():
        if s == 1:
            return rows_view(dy) @ w[:, :, 0, 0].t()
        return torch.ops.aten.convolution_backward(dy, x, w, None, [s, s], [0, 0], [1, 1], True, [0, 0], 1, [True, False, False])[0]

    def v_w():
        if s == 1:
            return tall_t_matmul(rows_view(dy), rows_view(x))
        return torch.ops.aten.convolution_backward(dy, x, w, None, [s, s], [0, 0], [1, 1], True, [0, 0], 1, [False, True, False])[1]
    return {'f': (lambda: rows_gemm.forward_x6(x, w, cin, cout, s), v_f),
            'i': (lambda: rows_gemm.input_grad_x6(dy, w, cin, cout, s), v_i),
            'w': (lambda: rows_gemm.wgrad_x6(x, dy, w, cin, cout, s), v_w)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=15)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-errors', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = ['rows_gemm4 against the vendor kernels, batch %d, %d alternated pairs, medians in us (min .. max)' % (args.batch, args.pairs)]
    for name, cin, cout, s, H, W in LAYERS:
        g = torch.Generator(device='cuda').manual_seed(7)
        sets = []
        for _ in range(3):
            x = torch.randn((args.batch, cin, H, W), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
            dy = torch.randn((args.batch, cout, s * H, s * W), device=dev, generator=g).contiguous(memory_format=torch.channels_last)
            w = torch.randn((cin, cout, s, s), device=dev, generator=g) * (1.0 / cin ** 0.5)
            sets.append((x, w, dy))
        if not args.no_errors:
            x, w, dy = sets[0]
            refs = dict(zip('fiw', f64_all(x, w, dy, s)))
            c = calls(x, w, dy, cin, cout, s)
            for d in 'fiw':
                if not rows_gemm.supported(cin, cout, s, 'fiw'.index(d)):
                    lines.append('%s %s: no instance' % (name, d))
                    continue
                new, ven = c[d][0](), c[d][1]()
                if d == 'w' and s == 1:
                    ven = ven.t().reshape(cin, cout, 1, 1)
                if d == 'i' and s == 1:
                    ven = ven.view(args.batch, H, W, cin).permute(0, 3, 1, 2)
                lines.append('%s %s: max error over the largest entry against f64: new %.3e  vendor %.3e'
                             % (name, d, rel_err(new, refs[d]), rel_err(ven, refs[d])))
                print(lines[-1], flush=True)
            del refs
        cs = [calls(x, w, dy, cin, cout, s) for x, w, dy in sets]
        for d in 'fiw':
            if not rows_gemm.supported(cin, cout, s, 'fiw'.index(d)):
                continue
            for k in range(3):
                cs[k][d][0](), cs[k][d][1]()
            torch.cuda.synchronize()
            tn, tv = [], []
            for p in range(args.pairs):
                tn.append(timed(cs[p % 3][d][0]))
                tv.append(timed(cs[(p + 1) % 3][d][1]))
            lines.append('%s %s %3d -> %3d: new %7.1f (%7.1f .. %7.1f)   vendor %7.1f (%7.1f .. %7.1f)   ratio %.2f'
                         % (name, d, cin, cout, statistics.median(tn), min(tn), max(tn), statistics.median(tv), min(tv), max(tv),
                            statistics.median(tv) / statistics.median(tn)))
            print(lines[-1], flush=True)
        del sets, cs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
