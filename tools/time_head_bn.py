"""The anchor head's backward inside the concat BatchNorm backward (csrc/head_bn.hip) against the launches it replaces, at the bench
shape (16 x 200 x 176 = 563,200 rows, 2 x 256 channels, K = 72), alternated in one process, with medians; and both paths' distances from
an f64 evaluation at that size (64-bit row offsets, full-length ranges).
  python tools/time_head_bn.py [--pairs 15] [--rows 563200] [--out profiles/time_head_bn_X.txt] [--no-errors]
    A  sums + finalize        against  head weight gradient (256-slice batched GEMM + sum) + column sum of dOut + 2 reduce passes
    B  weight image + apply   against  head input gradient dz = dOut W + 2 apply passes
The old apply pass has no entry point of its own: crb_bn_relu_backward (reduce + apply) is timed and the separately timed reduce passes
are subtracted. Every timed call works on one of three buffer sets in rotation (more than the 256 MB of last-level cache)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))

from crbhip import bnrelu, head_bn  # noqa: E402
from pcdet.utils.linear_rows import tall_t_matmul  # noqa: E402

EPS = 1e-3


class Set(object):
    def __init__(self, n, C, K, g, dev):
        self.n, self.C, self.K = n, C, K
        self.xs = [torch.randn(n, C, device=dev, generator=g) for _ in range(2)]
        self.dout = torch.randn(n, K, device=dev, generator=g)
        self.w = torch.randn(K, 2 * C, device=dev, generator=g) / (2 * C) ** 0.5
        self.saved = []
        for x in self.xs:
            gamma = torch.rand(C, device=dev, generator=g) + 0.5
            beta = torch.rand(C, device=dev, generator=g) - 0.5
            self.saved.append((x, x.mean(0), (x.var(0, unbiased=False) + EPS).rsqrt(), gamma, beta))
        self.par = head_bn.params(self.saved)
        self.z = torch.cat([torch.relu(g_ * ((x - m) * i) + b_) for x, m, i, g_, b_ in self.saved], 1)
        self.dz = self.dout @ self.w
        self.dgb = None

    # new
    def new_a(self):
        return head_bn.finalize(head_bn.sums(self.xs, self.par, self.dout, self.K), self.w, self.par, 2, self.C, self.K)

    def new_b(self):
        return head_bn.apply(self.xs, self.par, self.dgb, self.dout, self.w, self.K)

    # today
    def old_reduce(self):
        return [bnrelu.concat_reduce(s[0], self.dz, i * self.C, *s[1:]) for i, s in enumerate(self.saved)]

    def old_a(self):
        return tall_t_matmul(self.dout, self.z), self.dout.sum(0), self.old_reduce()

    def old_b_with_reduce(self):
        dz = self.dout @ self.w
        return [bnrelu.concat_backward(s[0], dz, i * self.C, *s[1:]) for i, s in enumerate(self.saved)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def rel_err(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def errors(s, lines):
    n, C = s.n, s.C
    dgb, dw, db = s.new_a()
    s.dgb = dgb
    dxs = s.new_b()
    dw_old, db_old, red_old = s.old_a()
    back_old = s.old_b_with_reduce()
    dout, W = s.dout.double(), s.w.double()
    zi = []
    for i, (x, _, _, g, b) in enumerate(s.saved):
        x64, g64, b64 = x.double(), g.double(), b.double()
        invstd = (x64.var(0, unbiased=False) + EPS).rsqrt()
        xh = (x64 - x64.mean(0)) * invstd
        del x64
        mask = (s.z[:, i * C:(i + 1) * C] > 0).double()
        d = mask * (dout @ W[:, i * C:(i + 1) * C])
        dbeta, dgamma = d.sum(0), (d * xh).sum(0)
        dx = g64 * invstd * (d - dbeta / n - xh * dgamma / n)
        zi.append(mask * (g64 * xh + b64))
        sl = slice(i * C, (i + 1) * C)
        for name, new, old, ref in (('dx%d' % i, dxs[i], back_old[i][0], dx), ('dgamma%d' % i, dgb[1, sl], red_old[i][1], dgamma),
                                    ('dbeta%d' % i, dgb[0, sl], red_old[i][0], dbeta)):
            lines.append('%s: max error over the largest entry against f64: new %.3e  today %.3e' % (name, rel_err(new, ref), rel_err(old, ref)))
            print(lines[-1], flush=True)
        del d, dx, xh, mask
    dw64 = dout.t() @ torch.cat(zi, 1)
    for name, new, old, ref in (('dW', dw, dw_old, dw64), ('db', db, db_old, dout.sum(0))):
        lines.append('%s: max error over the largest entry against f64: new %.3e  today %.3e' % (name, rel_err(new, ref), rel_err(old, ref)))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=15)
    ap.add_argument('--rows', type=int, default=16 * 200 * 176)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-errors', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda')
    C, K = 256, 72
    g = torch.Generator(device='cuda').manual_seed(7)
    sets = [Set(args.rows, C, K, g, dev) for _ in range(3)]
    lines = ['head_bn against the launches it replaces, %d rows, 2 x %d channels, K = %d, %d alternated pairs, medians in us (min .. max)'
             % (args.rows, C, K, args.pairs)]
    if not args.no_errors:
        errors(sets[0], lines)
        torch.cuda.empty_cache()
    for s in sets:
        s.dgb = s.new_a()[0]
        s.new_b(), s.old_a(), s.old_b_with_reduce()
    torch.cuda.synchronize()
    t = {k: [] for k in ('new_a', 'old_a', 'new_b', 'old_b_with_reduce', 'old_reduce')}
    for p in range(args.pairs):
        for j, k in enumerate(t):
            t[k].append(timed(getattr(sets[(p + j) % 3], k)))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, v in t.items():
        lines.append('%-18s %7.1f (%7.1f .. %7.1f)' % (k, med[k], min(v), max(v)))
    old_b = med['old_b_with_reduce'] - med['old_reduce']
    lines.append('A: sums + finalize %.1f against weight gradient + column sum + 2 reduce passes %.1f: ratio %.2f'
                 % (med['new_a'], med['old_a'], med['old_a'] / med['new_a']))
    lines.append('B: image + apply %.1f against dz GEMM + 2 apply passes %.1f (= %.1f with the reduce passes - %.1f): ratio %.2f'
                 % (med['new_b'], old_b, med['old_b_with_reduce'], med['old_reduce'], old_b / med['new_b']))
    lines.append('both: %.1f against %.1f' % (med['new_a'] + med['new_b'], med['old_a'] + old_b))
    print('\n'.join(lines[-8:]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
