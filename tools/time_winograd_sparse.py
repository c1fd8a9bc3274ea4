"""Per-launch timing of the first 3x3 BEV layer (256 -> 128 at B x 200 x 176) with and without the block lists of its sparse input
(crbhip.bev_blocks, CRB_WINOGRAD_SPARSE), on the real maps of the two batches bench.py keeps resident.

Runs the SECOND model's sparse backbone once per batch, takes the indices HeightCompression scatters, and prints
  * the three list counts over their totals,
  * median and p10 of the dense and the listed launch of each direction (forward with statistics, input gradient, weight gradient),
    alternated launch by launch (HIP events around each launch; the listed time includes its fill launch),
  * the time of the list build.
A direction belongs in the default set of CRB_WINOGRAD_SPARSE only if its listed median is below the dense launch's p10.

    python tools/time_winograd_sparse.py [--batch 16] [--iters 40]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'crb-active-3ddet_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def alternate(fns, iters, warm=5):
    """{name: fn} -> {name: sorted times in us}, the launches interleaved a, b, a, b .."""
    for _ in range(warm):
        for f in fns.values():
            f()
    ev = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            ev[k].append(timed(f, 1))
    torch.cuda.synchronize()
    return {k: np.array(sorted(1e3 * a.elapsed_time(b) for a, b in v)) for k, v in ev.items()}


def stat(xs):
    return 'median %7.1f us  p10 %7.1f us' % (float(np.median(xs)), float(np.percentile(xs, 10)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--iters', type=int, default=40)
    args = ap.parse_args()
    from crbhip import bev_blocks, winograd
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = build_network(second_cfg('kitti').MODEL, 3, SyntheticDataset(num_frames=args.batch)).to(dev).train()
    conv = [m for m in model.backbone_2d.blocks[0] if isinstance(m, torch.nn.Conv2d)][0]
    w = conv.weight.detach()
    cout, cin = w.shape[0], w.shape[1]
    winograd.SPARSE = {'f', 'i', 'w'}
    seen = {}
    hook = model.map_to_bev_module.register_forward_hook(
        lambda m, i, o: seen.update(x=o['spatial_features'].detach(), sp=o['encoded_spconv_tensor']))
    verdict = {}
    for k in range(2):
        first = k * args.batch
        pts, off, gt = kitti_batch(first, args.batch, args.points)
        bidx = np.repeat(np.arange(args.batch, dtype=np.float32), np.diff(off))[:, None]
        batch = {'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                 'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': args.batch}
        model(batch)
        x, sp = seen['x'], seen['sp']
        N, _, H, W = x.shape
        idx = sp.indices
        bl = bev_blocks.build(idx, N, H, W)
        c = bl.counts.cpu().tolist()
        g = bl.geom
        active = int((x != 0).any(1).sum())
        print('batch %d (frames %d..%d): map %d x %d x %d x %d, %d index rows, %.1f %% of the pixels nonzero' %
              (k, first, first + args.batch - 1, N, cin, H, W, idx.shape[0], 100.0 * active / (N * H * W)))
        print('  conv-in  list %5d / %5d blocks (%.1f %% skipped)' % (c[0], g['nblocks'], 100.0 * (1 - c[0] / g['nblocks'])))
        print('  conv-out list %5d / %5d blocks (%.1f %% skipped)' % (c[1], g['nblocks'], 100.0 * (1 - c[1] / g['nblocks'])))
        print('  wgrad    list %5d / %5d chunks (%.1f %% skipped)' % (c[2], g['nchunks'], 100.0 * (1 - c[2] / g['nchunks'])))
        xs = x.view_as(x)
        xs._crb_bev_blocks = bl
        dy = torch.randn((N, cout, H, W), device=dev).contiguous(memory_format=torch.channels_last)
        dyo = dy.view_as(dy)
        dyo._crb_bev_blocks_out = bl
        Uf, Ui = winograd.weights_forward2(w), winograd.weights_input_grad2(w)
        t = alternate({'dense': lambda: winograd.conv3x3_stats_U4(x, Uf), 'listed': lambda: winograd.conv3x3_stats_U4(xs, Uf)}, args.iters)
        print('  forward (+ slab sums)  dense  %s | listed %s' % (stat(t['dense']), stat(t['listed'])))
        verdict.setdefault('f', []).append(float(np.median(t['listed'])) < float(np.percentile(t['dense'], 10)))
        t = alternate({'dense': lambda: winograd.conv3x3_U2(dy, Ui), 'listed': lambda: winograd.conv3x3_U2(dyo, Ui)}, args.iters)
        print('  input gradient         dense  %s | listed %s' % (stat(t['dense']), stat(t['listed'])))
        verdict.setdefault('i', []).append(float(np.median(t['listed'])) < float(np.percentile(t['dense'], 10)))
        t = alternate({'dense': lambda: winograd.conv3x3_wgrad(x, dy, w), 'listed': lambda: winograd.conv3x3_wgrad(xs, dy, w)}, args.iters)
        print('  weight gradient        dense  %s | listed %s' % (stat(t['dense']), stat(t['listed'])))
        verdict.setdefault('w', []).append(float(np.median(t['listed'])) < float(np.percentile(t['dense'], 10)))
        t = alternate({'build': lambda: bev_blocks.build(idx, N, H, W)}, args.iters)
        print('  list build (2 clears + mark + compact)   %s' % stat(t['build']))
        # the fills alone: a listed launch with an EMPTY list is its fill over every block (+ a kernel that returns at once)
        empty = bev_blocks.build(idx[:0], N, H, W)
        xe, dye = x.view_as(x), dy.view_as(dy)
        xe._crb_bev_blocks, dye._crb_bev_blocks_out = empty, empty
        t = alternate({'f': lambda: winograd.conv3x3_stats_U4(xe, Uf), 'i': lambda: winograd.conv3x3_U2(dye, Ui)}, args.iters)
        print('  fill of EVERY block: forward y %s | input gradient %s (a real fill covers the skipped share)' % (stat(t['f']), stat(t['i'])))
    hook.remove()
    print('listed median below dense p10 on both batches: ' + ', '.join('%s=%s' % (k, all(v)) for k, v in verdict.items()))


if __name__ == '__main__':
    main()
