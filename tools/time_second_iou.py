#!/usr/bin/env python
"""SECOND-IoU timings on one MI355X:
  pool  : crb_roi_bev_pool alone on a random (batch, 200, 176, 512) NHWC map, 128 RoIs per frame (training) and 100 (test), G = 7,
          next to the reference's route on the device: the NHWC -> NCHW layout copy + per-frame affine_grid / grid_sample
          (roi_grid_pool_torch of second_head.py). Device time between two events, one call per sample.
  step  : a full fwd + bwd + grad-clip + fused AdamW step of SECONDNetIoU at --batch frames of --points points, next to SECONDNet's
          step in the same process (the sparse prologue of the next batch enqueued before the backward pass, as bench.py does).
          Device time between events at the step boundaries.
Per figure: median, p10 and p90 over --steps samples after --warmup. Each route runs in a child process of its own under a time
limit; a route that fails or runs out of time ends the run.
Usage: python tools/time_second_iou.py [--batch 16] [--points 20000] [--steps 20] [--warmup 5] [--routes pool,step]
Prints one JSON line per route."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
CHILD_TIME_LIMIT_S = 420


def _stats(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {'median_ms': q(0.5), 'p10_ms': q(0.1), 'p90_ms': q(0.9), 'samples': len(ms)}


def _timed(fn, steps, warmup):
    import torch
    out = []
    for i in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return _stats(out)


def run_pool(args):
    import torch
    from crbhip import roi_bev_pool
    from pcdet.models.roi_heads.second_head import roi_grid_pool_torch
    dev = torch.device('cuda', 0)
    B, H, W, C, G = args.batch, 200, 176, 512, 7
    g = torch.Generator(device=dev).manual_seed(0)
    bev = torch.randn((B, H, W, C), device=dev, generator=g)
    geo = (0.0, -40.0, 0.4, 0.4)
    out = {'route': 'pool', 'map': [B, H, W, C], 'grid': G}
    for name, R in (('train', 128), ('test', 100)):
        u = torch.rand((B, R, 7), device=dev, generator=g)
        rois = torch.stack([u[..., 0] * 70.4, u[..., 1] * 80 - 40, u[..., 2] - 1.5, 1.5 + 3 * u[..., 3], 0.6 + 1.4 * u[..., 4],
                            1.4 + 0.4 * u[..., 5], (u[..., 6] * 2 - 1) * 3.14159], -1).contiguous()
        k = _timed(lambda: roi_bev_pool.roi_bev_pool(bev, rois, G, *geo), args.steps, args.warmup)
        nchw_view = bev.permute(0, 3, 1, 2)
        t = _timed(lambda: roi_grid_pool_torch(nchw_view.contiguous(), rois, G, *geo), args.steps, args.warmup)
        t_nocopy_src = nchw_view.contiguous()
        s = _timed(lambda: roi_grid_pool_torch(t_nocopy_src, rois, G, *geo), args.steps, args.warmup)
        del t_nocopy_src
        out_bytes = 4 * B * R * G * G * C
        out[name] = {'rois_per_frame': R, 'kernel': k, 'grid_sample_route_with_layout_copy': t, 'grid_sample_route_on_a_resident_nchw_map': s,
                     'output_bytes': out_bytes, 'kernel_output_GBps': out_bytes / (k['median_ms'] * 1e-3) / 1e9}
    return out


def run_step(args):
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import second_cfg, second_iou_cfg
    from pcdet.models import build_network
    import numpy as np
    dev = torch.device('cuda', 0)
    out = {'route': 'step', 'batch': args.batch, 'points_per_frame': args.points}
    batches = []
    for k in range(2):
        pts, off, gt = kitti_batch(k * args.batch, args.batch, args.points)
        bidx = np.repeat(np.arange(args.batch, dtype=np.float32), np.diff(off))[:, None]
        batches.append({'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                        'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': args.batch})
    for name, cfg in (('second', second_cfg()), ('second_iou', second_iou_cfg())):
        torch.manual_seed(0)
        model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=args.batch, n_points=args.points)).to(dev)
        model.train()
        opt = torch.optim.AdamW(model.parameters(), lr=3e-3, weight_decay=0.01, betas=(0.9, 0.99), fused=True)
        ahead = {}
        state = {'i': 0}

        def step():
            i = state['i']
            b = ahead.pop(i, None) or dict(batches[i % 2])
            opt.zero_grad(set_to_none=True)
            ret, _, _ = model(b)
            ahead.clear()
            ahead[i + 1] = model.prefetch_sparse(dict(batches[(i + 1) % 2]))
            ret['loss'].backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
            opt.step()
            state['i'] = i + 1
        out[name] = _timed(step, args.steps, args.warmup)
        out[name]['frames_per_s'] = args.batch / (out[name]['median_ms'] * 1e-3)
        del model, opt
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='pool,step')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({'pool': run_pool, 'step': run_step}[a.child](a)), flush=True)
        return
    for route in a.routes.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', route, '--batch', str(a.batch), '--points', str(a.points),
               '--steps', str(a.steps), '--warmup', str(a.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_TIME_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                                                        # nothing more is started after a failed route
            print(json.dumps({'route': route, 'rc': rc}), flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
