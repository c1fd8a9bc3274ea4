"""The anchor head's forward inside the concat BatchNorm apply (csrc/head_bn.hip: head_bn_forward_kernel) against the launches it
replaces, at the bench shape (16 x 200 x 176 = 563,200 rows, 2 x 256 channels, K = 72), alternated in one process on three rotating
buffer sets (more than the 256 MB of last-level cache); median, p10 and p90 of the samples, and both paths' distances from an f64
evaluation at that size (64-bit row offsets).
  python tools/time_head_bn_forward.py [--samples 15] [--rows 563200] [--out profiles/time_head_bn_forward_X.txt] [--no-errors]
    new  weight image + fused forward          against   old  two apply passes (the map is written) + addmm (the map is read)
The statistics launches run on both paths and are not timed."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))

from crbhip import bnrelu, head_bn  # noqa: E402

EPS = 1e-3


class Set(object):
    def __init__(self, n, C, K, g, dev):
        self.n, self.C, self.K = n, C, K
        xs = [torch.randn(n, C, device=dev, generator=g) for _ in range(2)]
        self.w = torch.randn(K, 2 * C, device=dev, generator=g) / (2 * C) ** 0.5
        self.b = torch.randn(K, device=dev, generator=g)
        self.saved = []
        for x in xs:
            gamma = torch.rand(C, device=dev, generator=g) + 0.5
            beta = torch.rand(C, device=dev, generator=g) - 0.5
            self.saved.append((x, x.mean(0), (x.var(0, unbiased=False) + EPS).rsqrt(), gamma, beta))
        self.par = head_bn.params(self.saved)
        self.record = head_bn.Record(None, [(s[0], s[3], s[4]) for s in self.saved], self.saved, True)

    def new(self):
        return head_bn.forward([s[0] for s in self.saved], self.par, self.w, self.b, self.K)

    def old(self):
        with torch.no_grad():
            return torch.addmm(self.b, bnrelu.materialize_concat(self.record), self.w.t())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    del out
    return e0.elapsed_time(e1) * 1e3


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, max(0, int(round(q * (len(s) - 1)))))]


def errors(s, lines):
    new, old = s.new(), s.old()
    want = torch.empty((s.n, s.K), dtype=torch.float64, device=new.device)
    step = 1 << 16
    for r0 in range(0, s.n, step):
        z = torch.cat([torch.relu(g.double() * ((x[r0:r0 + step].double() - m.double()) * i.double()) + b.double())
                       for x, m, i, g, b in s.saved], 1)
        want[r0:r0 + step] = z @ s.w.double().t() + s.b.double()
    top = float(want.abs().max())
    lines.append('out: max error over the largest entry against f64: new %.3e  today %.3e'
                 % (float((new.double() - want).abs().max()) / top, float((old.double() - want).abs().max()) / top))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--samples', type=int, default=15)
    ap.add_argument('--rows', type=int, default=16 * 200 * 176)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-errors', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda')
    C, K = 256, 72
    g = torch.Generator(device='cuda').manual_seed(7)
    sets = [Set(args.rows, C, K, g, dev) for _ in range(3)]
    lines = ['head_bn forward against the launches it replaces, %d rows, 2 x %d channels, K = %d, %d alternated samples, us'
             % (args.rows, C, K, args.samples)]
    if not args.no_errors:
        errors(sets[0], lines)
        torch.cuda.empty_cache()
    for s in sets:
        s.new(), s.old()
    torch.cuda.synchronize()
    t = {'new': [], 'old': []}
    for p in range(args.samples):
        for j, k in enumerate(t):
            t[k].append(timed(getattr(sets[(p + j) % 3], k)))
    for k, v in t.items():
        lines.append('%-4s median %7.1f  p10 %7.1f  p90 %7.1f' % (k, statistics.median(v), pct(v, 0.1), pct(v, 0.9)))
    mn, mo = statistics.median(t['new']), statistics.median(t['old'])
    lines.append('image + fused forward %.1f against two apply passes + addmm %.1f: ratio %.2f; new median %s old p10 (%.1f)'
                 % (mn, mo, mo / mn, 'below' if mn < pct(t['old'], 0.1) else 'NOT below', pct(t['old'], 0.1)))
    print('\n'.join(lines[-3:]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
