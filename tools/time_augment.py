#!/usr/bin/env python
"""World-augmentation timings on one MI355X: a batch of --batch frames of --points points through
  fused : DeviceDataProcessor.process_batch(..., augmentor=KITTI queue)   crb_augment_mask_points + crb_augment_boxes
  plain : the same process_batch without augmentation (torch comparisons, boolean index, repeat_interleave)
  host  : the host mirror (DataAugmentor + DataProcessor range masks) frame after frame on one core, no GPU involved
Per route: median and minimum wall time of a whole call (upload and the one size read-back included) after --warmup calls, and
for the two device routes the number of kernels and copies one call launches (torch profiler). Each route runs in a child process of its own under a time limit; a
route that fails or runs out of time ends the run.
Usage: python tools/time_augment.py [--batch 16] [--points 20000] [--steps 30] [--warmup 5] [--routes fused,plain,host]
Prints one JSON line per route."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
CHILD_TIME_LIMIT_S = 240

KITTI_QUEUE = [{'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']},
               {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]},
               {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}]
PCR = [0, -40, -3, 70.4, 40, 1]


def _setup(batch, points):
    import numpy as np
    from pcdet.config import EasyDict
    from pcdet.datasets.synthetic import kitti_frame
    frames, gts = zip(*[kitti_frame(500 + f, points) for f in range(batch)])
    cfgs = [EasyDict({'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}),
            EasyDict({'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': EasyDict({'train': False, 'test': False})})]
    np.random.seed(0)
    return list(frames), list(gts), cfgs, [EasyDict(c) for c in KITTI_QUEUE]


def _stats(times):
    times = sorted(times)
    return {'median_ms': 1e3 * times[len(times) // 2], 'min_ms': 1e3 * times[0], 'calls': len(times)}


def run_route(route, batch, points, steps, warmup):
    import numpy as np
    frames, gts, cfgs, queue = _setup(batch, points)
    out = {'route': route, 'batch': batch, 'points_per_frame': points}
    if route == 'host':
        import torch
        from pcdet.datasets.augmentor import DataAugmentor
        from pcdet.datasets.processor.data_processor import DataProcessor
        torch.set_num_threads(1)                                          # (the box corners go through torch on the host)
        aug = DataAugmentor(None, queue, ['Car', 'Pedestrian', 'Cyclist'])
        dp = DataProcessor(cfgs[:1], PCR, training=True, num_point_features=frames[0].shape[1])

        def call():
            for p, g in zip(frames, gts):
                d = aug.forward({'points': p.copy(), 'gt_boxes': g[:, :-1].copy()})
                d['gt_boxes'] = np.concatenate([d['gt_boxes'], g[:, -1:]], 1)
                dp.forward(d)
        times = []
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            call()
            if i >= warmup:
                times.append(time.perf_counter() - t0)
        out.update(_stats(times), threads=1)
        return out
    import torch
    from pcdet.datasets.augmentor import DeviceDataAugmentor
    from pcdet.datasets.processor.data_processor import DeviceDataProcessor
    dev = torch.device('cuda', 0)
    dp = DeviceDataProcessor(cfgs, PCR, True, frames[0].shape[1], device=dev)
    aug = DeviceDataAugmentor(queue) if route == 'fused' else None
    call = lambda: dp.process_batch(frames, gts, augmentor=aug)
    times = []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(time.perf_counter() - t0)
    out.update(_stats(times))
    try:                                                                   # launches of ONE call, as the device saw them
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        copies = [n for n in names if 'memcpy' in n.lower() or 'copybuffer' in n.lower()]
        out.update(kernels=len(names) - len(copies), copies=len(copies),
                   augment_kernels=len([n for n in names if n.startswith('(anonymous namespace)::aug_') or 'aug_' in n]))
    except Exception as e:                                                 # the timing above stands without the counts
        out.update(kernels=None, copies=None, profiler_error=repr(e)[:200])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='fused,plain,host')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_route(a.child, a.batch, a.points, a.steps, a.warmup)), flush=True)
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
