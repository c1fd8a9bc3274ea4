#!/usr/bin/env python
"""Dynamic voxelization timings on one MI355X, on --batch synthetic Waymo-like frames of --points points:
  voxelize   : crb_dyn_voxelize alone, pillar mode on the 0.32 x 0.32 m pillar grid of the reference's centerpoint_dyn_pillar yaml
               (468 x 468) and voxel mode on the SECOND Waymo grid, one read-back of (M, Nk) included.
  mean       : DynMeanVFE on the device route (csrc/dyn_voxelize.hip: voxelization + segmented mean) and on the reference's
               formulation in torch ops on the same device tensors (floor / mask / torch.unique(return_inverse) / index_add_): the
               yardstick - the parent commit cannot run this module at all.
  pillar     : DynPillarVFE on the fused route (csrc/dyn_pillar_vfe.hip, voxelization included): training forward + backward, eval
               forward, peak allocation over the inputs.
  pillar_torch : the same module and points on the reference's formulation in torch ops on the same device (the (N, 64) tensors).
  step       : a full fwd + bwd + grad-clip + fused AdamW step of SECOND (Waymo shapes) behind DynMeanVFE, and behind MeanVFE (the
               capped generator) for comparison.
  det_step   : the same kind of step of CenterPoint behind DynPillarVFE (centerpoint_dyn_pillar_cfg, a 468 x 468 map at stride 1).
Device time between two events, one call per sample; per figure median, p10 and p90 over --steps samples after --warmup, and the peak
allocation over the inputs. Each route runs in a child process of its own under a time limit; a route that fails or runs out of
time ends the run. No pass / fail time is set.
Usage: python tools/time_dyn_pillar.py [--batch 16] [--points 180000] [--steps 20] [--warmup 5] [--routes voxelize,mean,pillar,pillar_torch,step,det_step]
Prints one JSON line per route."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
CHILD_TIME_LIMIT_S = 420
PILLAR_VOXEL = [0.32, 0.32, 6.0]
PILLAR_RANGE = [-74.88, -74.88, -2.0, 74.88, 74.88, 4.0]
PILLAR_GRID = [468, 468, 1]


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


def _with_peak(fn, args, dev):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    r = _timed(fn, args.steps, args.warmup)
    r['peak_over_inputs_MB'] = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    return r


def _batches(args, n_batches, dev):
    import numpy as np
    import torch
    from pcdet.datasets.synthetic import kitti_batch
    out = []
    for k in range(n_batches):
        pts, off, gt = kitti_batch(k * args.batch, args.batch, args.points, waymo=True)
        bidx = np.repeat(np.arange(args.batch, dtype=np.float32), np.diff(off))[:, None]
        out.append({'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                    'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': args.batch})
    return out


def run_voxelize(args):
    import torch
    from crbhip import dyn_vfe
    from pcdet.datasets import SyntheticDataset
    dev = torch.device('cuda', 0)
    pts = _batches(args, 1, dev)[0]['points']
    ds = SyntheticDataset(num_frames=1, kind='waymo')
    out = {'route': 'voxelize', 'batch': args.batch, 'points': int(pts.shape[0])}
    for name, mode, pcr, voxel, grid in (('pillar', dyn_vfe.PILLAR, PILLAR_RANGE, PILLAR_VOXEL, PILLAR_GRID),
                                         ('voxel', dyn_vfe.VOXEL, list(ds.point_cloud_range), ds.voxel_size, list(ds.grid_size))):
        r = dyn_vfe.dyn_voxelize(pts, args.batch, pcr, voxel, grid, mode)
        out[name] = dict(_with_peak(lambda: dyn_vfe.dyn_voxelize(pts, args.batch, pcr, voxel, grid, mode), args, dev),
                         voxels=r['M'], kept_points=r['Nk'], grid=[int(g) for g in grid])
    return out


def run_mean(args):
    import torch
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset
    from pcdet.models.backbones_3d.vfe import DynamicMeanVFE
    dev = torch.device('cuda', 0)
    pts = _batches(args, 1, dev)[0]['points']
    ds = SyntheticDataset(num_frames=1, kind='waymo')
    vfe = DynamicMeanVFE(EasyDict({'NAME': 'DynMeanVFE'}), pts.shape[1] - 1, ds.voxel_size, ds.grid_size, ds.point_cloud_range)
    out = {'route': 'mean', 'batch': args.batch, 'points': int(pts.shape[0])}
    with torch.no_grad():
        f_dev, c_dev = vfe._forward_fused(pts, args.batch)
        f_tor, c_tor = vfe._forward_torch(pts, args.batch)
        out['voxels'] = int(c_dev.shape[0])
        out['coords_equal'] = bool(c_dev.shape == c_tor.shape and (c_dev == c_tor).all())
        out['max_abs_difference_of_the_means'] = float((f_dev - f_tor).abs().max())
        del f_dev, c_dev, f_tor, c_tor
        out['device_route'] = _with_peak(lambda: vfe._forward_fused(pts, args.batch), args, dev)
        out['torch_route'] = _with_peak(lambda: vfe._forward_torch(pts, args.batch), args, dev)
    return out


def run_pillar(args, fused):
    import warnings
    import torch
    from pcdet.config import EasyDict
    from pcdet.models.backbones_3d.vfe import DynamicPillarVFE
    dev = torch.device('cuda', 0)
    pts = _batches(args, 1, dev)[0]['points']
    cfg = EasyDict({'NAME': 'DynPillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [64, 64]})
    torch.manual_seed(0)
    vfe = DynamicPillarVFE(cfg, pts.shape[1] - 1, PILLAR_VOXEL, PILLAR_GRID, PILLAR_RANGE).to(dev).train()
    assert not fused or vfe.unsupported_reason(pts.shape[1] - 1) is None
    route = (lambda: vfe._forward_fused(pts, args.batch)[0]) if fused else (lambda: vfe._forward_torch(pts, args.batch)[0])
    with torch.no_grad():
        M = int(route().shape[0])
    g = torch.randn((M, 64), device=dev)

    def fwd_bwd():
        vfe.zero_grad(set_to_none=True)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            (route() * g).sum().backward()

    def fwd_eval():
        with torch.no_grad():
            route()
    out = {'route': 'pillar' if fused else 'pillar_torch', 'batch': args.batch, 'points': int(pts.shape[0]), 'pillars': M,
           'one_N_by_64_f32_tensor_MB': pts.shape[0] * 64 * 4 / 2 ** 20}
    out['train_forward_backward'] = _with_peak(fwd_bwd, args, dev)
    vfe.eval()
    vfe.zero_grad(set_to_none=True)
    out['eval_forward'] = _with_peak(fwd_eval, args, dev)
    return out


def run_det_step(args):
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import centerpoint_dyn_pillar_cfg, centerpoint_dyn_pillar_dataset_args
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    batches = _batches(args, 2, dev)
    cfg = centerpoint_dyn_pillar_cfg()
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=args.batch, n_points=args.points,
                                                         **centerpoint_dyn_pillar_dataset_args(cfg))).to(dev).train()
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
    out = {'route': 'det_step', 'batch': args.batch, 'points_per_frame': args.points}
    out['centerpoint_dyn_pillar'] = _timed(step, args.steps, args.warmup)
    out['centerpoint_dyn_pillar']['frames_per_s'] = args.batch / (out['centerpoint_dyn_pillar']['median_ms'] * 1e-3)
    out['peak_allocated_MB'] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    return out


def run_step(args):
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    batches = _batches(args, 2, dev)
    out = {'route': 'step', 'batch': args.batch, 'points_per_frame': args.points}
    for name in ('DynMeanVFE', 'MeanVFE'):
        cfg = second_cfg('waymo')
        cfg.MODEL.VFE.NAME = name
        torch.manual_seed(0)
        model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=args.batch, kind='waymo', n_points=args.points)).to(dev).train()
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
        torch.cuda.reset_peak_memory_stats(dev)
        out[name] = _timed(step, args.steps, args.warmup)
        out[name]['frames_per_s'] = args.batch / (out[name]['median_ms'] * 1e-3)
        out[name]['peak_allocated_MB'] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
        del model, opt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=180000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='voxelize,mean,pillar,pillar_torch,step,det_step')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        runs = {'voxelize': run_voxelize, 'mean': run_mean, 'pillar': lambda x: run_pillar(x, True), 'pillar_torch': lambda x: run_pillar(x, False),
                'step': run_step, 'det_step': run_det_step}
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
