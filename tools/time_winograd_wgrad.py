#!/usr/bin/env python
"""Winograd-domain weight gradient against MIOpen's wrw on the stride-1 3x3 shapes of the BEV backbone, the split-bf16 kernel
(csrc/winograd_wgrad4.hip, crb_winograd4_wgrad) against the f32-MFMA kernel (csrc/winograd_wgrad.hip, crb_winograd2_wgrad) in
alternated runs: error against an f64 weight gradient, run-to-run bit equality, time per call, skip-work builds of both.
usage: python tools/time_winograd_wgrad.py [--quick]      (--quick: no MIOpen timing, fewer iterations)"""
import os
os.environ.setdefault('CRB_MEASURE_LIB', '1')
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timeit(fn, it=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(it):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def wgrad_miopen(x, dy, w):
    return torch.ops.aten.convolution_backward(dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])[1]


if __name__ == '__main__':
    from crbhip import winograd, lib
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    small = ((2, 64, 64, 9, 11), (1, 128, 64, 40, 31), (3, 64, 192, 7, 5), (2, 128, 128, 37, 29))
    big = ((16, 128, 128, 200, 176), (16, 256, 256, 100, 88), (16, 256, 128, 200, 176))
    quick = '--quick' in sys.argv

    def run(kernel, x, dy, w):
        winograd.WGRAD_KERNEL = kernel
        try:
            return winograd.conv3x3_wgrad(x, dy, w)
        finally:
            winograd.WGRAD_KERNEL = 'x6'

    for (N, C, K, H, W) in small + big:
        x = torch.randn(N, C, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        w = (torch.randn(K, C, 3, 3, device=dev) / np.sqrt(9 * C)).contiguous(memory_format=torch.channels_last)
        dy = torch.randn(N, K, H, W, device=dev).contiguous(memory_format=torch.channels_last)
        ref = wgrad_miopen(x, dy, w)
        got = run('x6', x, dy, w)
        again = run('x6', x, dy, w)
        got_c = run('x6', x, dy, w.contiguous())
        old = run('f32', x, dy, w)
        f64 = N * H * W <= 40000 or (N, C, K, H, W) in big
        if f64:
            r64 = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), padding=1)
        else:
            r64 = ref.double()
        sc = float(r64.abs().max())
        four = bool(lib.crb_winograd4_wgrad_supported(C, K, H, W))
        print('%dx%d->%d @%dx%d (%s): weight gradient error / largest entry: split-bf16 path %.2e, f32-MFMA kernel %.2e, MIOpen %.2e '
              '(reference: %s); bit-equal rerun %s; contiguous weight layout equal %s'
              % (N, C, K, H, W, 'crb_winograd4_wgrad' if four else 'no split-bf16 instance: crb_winograd2_wgrad both times',
                 float((got.double() - r64).abs().max()) / sc, float((old.double() - r64).abs().max()) / sc,
                 float((ref.double() - r64).abs().max()) / sc, 'f64' if f64 else 'MIOpen',
                 bool(torch.equal(got, again)), bool(torch.equal(got_c, got))), flush=True)
        if (N, C, K, H, W) not in big:
            continue
        flops = 2.0 * N * H * W * 9 * C * K
        it, warm = (8, 3) if quick else (20, 5)
        t_m = float('nan') if quick else timeit(lambda: wgrad_miopen(x, dy, w))[0]
        t_old, t_new = [], []
        for _ in range(3):                    # alternated: old, new, old, new, ...
            t_old.append(timeit(lambda: run('f32', x, dy, w), it=it, warm=warm))
            t_new.append(timeit(lambda: run('x6', x, dy, w), it=it, warm=warm))
        tm2, tm4 = [], []
        for mode in (1, 2, 3):
            lib.crb_winograd2_wgrad_set_mode(mode)
            tm2.append(timeit(lambda: run('f32', x, dy, w), it=8, warm=3)[0])
            lib.crb_winograd2_wgrad_set_mode(0)
            lib.crb_winograd4_wgrad_set_mode(mode)
            tm4.append(timeit(lambda: run('x6', x, dy, w), it=8, warm=3)[0])
            lib.crb_winograd4_wgrad_set_mode(0)
        t_ab = []                                         # A/B builds with correct results (include/crb_hip_measure.h)
        for mode in (4, 5, 6):
            lib.crb_winograd4_wgrad_set_mode(mode)
            t_ab.append(timeit(lambda: run('x6', x, dy, w), it=it, warm=warm)[0])
            lib.crb_winograd4_wgrad_set_mode(0)
        med_o, med_n = float(np.median([t[0] for t in t_old])), float(np.median([t[0] for t in t_new]))
        print('   MIOpen %.0f us | f32-MFMA kernel: medians %s us (min %.0f) | split-bf16 kernel: medians %s us (min %.0f): %.2fx, '
              '%.0f TF direct-equivalent, %.0f TF of bf16 MFMA work issued'
              % (t_m, ' / '.join('%.0f' % t[0] for t in t_old), min(t[1] for t in t_old),
                 ' / '.join('%.0f' % t[0] for t in t_new), min(t[1] for t in t_new), med_o / med_n, flops / med_n / 1e6,
                 6 * flops / 2.25 / med_n / 1e6), flush=True)
        print('   skip-work builds (no MFMAs / no transforms / no loads): f32-MFMA kernel %.0f / %.0f / %.0f us | split-bf16 kernel '
              '%.0f / %.0f / %.0f us; split-bf16 kernel with prefetch touches %.0f us, with 2 / 5 loads per MFMA gap instead of 1.5 %.0f / %.0f us'
              % (tm2[0], tm2[1], tm2[2], tm4[0], tm4[1], tm4[2], t_ab[0], t_ab[1], t_ab[2]), flush=True)
