#!/usr/bin/env python
"""PointPillars timings on one MI355X:
  vfe        : PillarVFE on the pillars of --batch synthetic frames of --points points (voxelized once, outside the timed region), on
               the fused kernels (csrc/pillar_vfe.hip): training forward + backward, and the eval forward.
  vfe_torch  : the same module and pillars on the reference's formulation in torch ops on the same device (the (M, T, 10) and
               (M, T, 64) tensors): the yardstick - the parent commit cannot run this model at all.
  step       : a full fwd + bwd + grad-clip + fused AdamW step of PointPillar at --batch frames of raw points.
  eval       : the eval pass (post-processing included) on the same batches.
Device time between two events, one call per sample; per figure median, p10 and p90 over --steps samples after --warmup, and the peak
allocation of the process. Each route runs in a child process of its own under a time limit; a route that fails or runs out of
time ends the run. No pass / fail time is set.
Usage: python tools/time_pointpillar.py [--batch 16] [--points 20000] [--steps 20] [--warmup 5] [--routes vfe,vfe_torch,step,eval]
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
    from pcdet.model_cfgs import pointpillar_cfg, pointpillar_dataset_args
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    cfg = pointpillar_cfg()
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=args.batch, n_points=args.points, **pointpillar_dataset_args(cfg))).to(dev)
    batches = []
    for k in range(n_batches):
        pts, off, gt = kitti_batch(k * args.batch, args.batch, args.points)
        bidx = np.repeat(np.arange(args.batch, dtype=np.float32), np.diff(off))[:, None]
        batches.append({'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                        'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': args.batch})
    return dev, model, batches


def run_vfe(args, fused):
    import warnings
    import torch
    dev, model, batches = _model_and_batches(args, 1)
    vfe = model.vfe.train()
    bd = dict(batches[0])
    voxels = vfe._voxelize_on_device(bd)
    num_points, coords = bd['voxel_num_points'], bd['voxel_coords']
    M, T, C = voxels.shape
    g = torch.randn((M, 64), device=dev)
    route = (lambda: vfe._forward_fused(voxels, num_points, coords)) if fused else (lambda: vfe._forward_torch(voxels, num_points, coords))
    assert not fused or vfe.unsupported_reason(C, T) is None

    def fwd_bwd():
        vfe.zero_grad(set_to_none=True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            (route() * g).sum().backward()

    def fwd_eval():
        with torch.no_grad():
            route()
    out = {'route': 'vfe' if fused else 'vfe_torch', 'batch': args.batch, 'pillars': int(M), 'T': int(T), 'C': int(C),
           'valid_points': int(num_points.sum()), 'voxels_MB': voxels.numel() * 4 / 2 ** 20}
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out['train_forward_backward'] = _timed(fwd_bwd, args.steps, args.warmup)
    out['train_peak_over_inputs_MB'] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    vfe.eval()
    vfe.zero_grad(set_to_none=True)
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out['eval_forward'] = _timed(fwd_eval, args.steps, args.warmup)
    out['eval_peak_over_inputs_MB'] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    return out


def run_step(args):
    import torch
    dev, model, batches = _model_and_batches(args, 2)
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=3e-3, weight_decay=0.01, betas=(0.9, 0.99), fused=True)
    state = {'i': 0}

    def step():
        b = dict(batches[state['i'] % 2])
        opt.zero_grad(set_to_none=True)
        ret, _, _ = model(b)
        ret['loss'].backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        state['i'] += 1
    out = {'route': 'step', 'batch': args.batch, 'points_per_frame': args.points}
    out['pointpillar'] = _timed(step, args.steps, args.warmup)
    out['pointpillar']['frames_per_s'] = args.batch / (out['pointpillar']['median_ms'] * 1e-3)
    out['peak_allocated_MB'] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    return out


def run_eval(args):
    import torch
    dev, model, batches = _model_and_batches(args, 2)
    model.eval()
    state = {'i': 0}

    def go():
        with torch.no_grad():
            model(dict(batches[state['i'] % 2]))
        state['i'] += 1
    out = {'route': 'eval', 'batch': args.batch, 'points_per_frame': args.points}
    out['pointpillar'] = _timed(go, args.steps, args.warmup)
    out['pointpillar']['frames_per_s'] = args.batch / (out['pointpillar']['median_ms'] * 1e-3)
    out['peak_allocated_MB'] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='vfe,vfe_torch,step,eval')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        runs = {'vfe': lambda x: run_vfe(x, True), 'vfe_torch': lambda x: run_vfe(x, False), 'step': run_step, 'eval': run_eval}
        print(json.dumps(runs[a.child](a)), flush=True)
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
