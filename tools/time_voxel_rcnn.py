#!/usr/bin/env python
"""Voxel R-CNN timings on one MI355X:
  pool  : VoxelRCNNHead.roi_grid_pool (the three levels x_conv2 / x_conv3 / x_conv4 of voxel_rcnn_car.yaml, G = 6) forward + backward on
          the sparse feature levels of --batch synthetic frames, 128 random car-sized RoIs per frame, on the HIP route (site hash, fused
          pooling) and on the torch route (dense (B, Z, Y, X) index, materialised groups, Conv2d + BatchNorm2d), each in its own child
          process (the torch route is switched on with CRB_VOXEL_POOL_FUSED=0). Device time between two events, one call per sample.
  step  : a full fwd + bwd + grad-clip + fused AdamW step of VoxelRCNN at --batch frames of --points points (the sparse prologue of the
          next batch enqueued before the backward pass, as bench.py does). Device time between events at the step boundaries.
Per figure: median, p10 and p90 over --steps samples after --warmup. Each route runs in a child process of its own under a time
limit; a route that fails or runs out of time ends the run. No pass / fail time is set.
Usage: python tools/time_voxel_rcnn.py [--batch 16] [--points 20000] [--steps 20] [--warmup 5] [--routes pool,pool_torch,step]
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


def _model_and_batches(args, n_batches):
    import numpy as np
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import voxel_rcnn_cfg
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    cfg = voxel_rcnn_cfg()
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 1, SyntheticDataset(num_frames=args.batch, n_points=args.points, class_names=cfg.CLASS_NAMES)).to(dev)
    batches = []
    for k in range(n_batches):
        pts, off, gt = kitti_batch(k * args.batch, args.batch, args.points)
        gt = gt.copy()
        gt[..., 7] = (gt[..., 3] > 0)
        bidx = np.repeat(np.arange(args.batch, dtype=np.float32), np.diff(off))[:, None]
        batches.append({'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                        'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': args.batch})
    return dev, model, batches


def run_pool(args):
    """roi_grid_pool forward + backward on whichever route CRB_VOXEL_POOL_FUSED selects"""
    import warnings
    import torch
    from pcdet.ops.pointnet2.pointnet2_stack import voxel_pool_modules
    dev, model, batches = _model_and_batches(args, 1)
    model.train()
    bd = dict(batches[0])
    with torch.no_grad():
        for m in (model.vfe, model.backbone_3d):
            bd = m(bd)
    R = 128
    g = torch.Generator(device=dev).manual_seed(0)
    u = torch.rand((args.batch, R, 7), device=dev, generator=g)
    bd['rois'] = torch.stack([5 + u[..., 0] * 60, u[..., 1] * 70 - 35, u[..., 2] * 0.8 - 1.4, 3.2 + 1.2 * u[..., 3], 1.4 + 0.5 * u[..., 4],
                              1.4 + 0.4 * u[..., 5], (u[..., 6] * 2 - 1) * 3.14159], -1).contiguous()
    head = model.roi_head
    levels = {k: [int(v.features.shape[0]), int(v.features.shape[1])] + list(v.spatial_shape) for k, v in bd['multi_scale_3d_features'].items()
              if k in head.pool_cfg.FEATURES_SOURCE}
    for v in bd['multi_scale_3d_features'].values():
        v.features = v.features.detach().requires_grad_(True)

    def fwd_bwd():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            head.roi_grid_pool(bd).sum().backward()

    def fwd():
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            head.roi_grid_pool(bd)
    out = {'route': 'pool' if voxel_pool_modules.FUSED else 'pool_torch', 'fused': voxel_pool_modules.FUSED, 'batch': args.batch,
           'rois_per_frame': R, 'grid_points': args.batch * R * 216, 'levels_rows_channels_shape': levels}
    out['forward'] = _timed(fwd, args.steps, args.warmup)
    out['forward_backward'] = _timed(fwd_bwd, args.steps, args.warmup)
    out['peak_allocated_MB'] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    return out


def run_step(args):
    import torch
    dev, model, batches = _model_and_batches(args, 2)
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
    out = {'route': 'step', 'batch': args.batch, 'points_per_frame': args.points}
    out['voxel_rcnn'] = _timed(step, args.steps, args.warmup)
    out['voxel_rcnn']['frames_per_s'] = args.batch / (out['voxel_rcnn']['median_ms'] * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='pool,pool_torch,step')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps({'pool': run_pool, 'pool_torch': run_pool, 'step': run_step}[a.child](a)), flush=True)
        return
    for route in a.routes.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', route, '--batch', str(a.batch), '--points', str(a.points),
               '--steps', str(a.steps), '--warmup', str(a.warmup)]
        env = dict(os.environ, CRB_VOXEL_POOL_FUSED='0' if route == 'pool_torch' else '1')
        try:
            rc = subprocess.run(cmd, timeout=CHILD_TIME_LIMIT_S, env=env).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                                                        # nothing more is started after a failed route
            print(json.dumps({'route': route, 'rc': rc}), flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
