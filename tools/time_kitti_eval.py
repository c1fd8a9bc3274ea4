#!/usr/bin/env python
"""Time of get_official_eval_result at KITTI val scale on the device route, next to the host route, with a breakdown by launch.

Synthetic annos (tests/kitti_eval_cases.py's generator without the margin rule, which timing does not need): 3,769 frames, 3 classes,
ground-truth counts 0..12 per frame like the val split's (mean about 6 with DontCare), detections the jittered copies plus false
positives (mean about 8). Reported: wall time of the whole call (packing on the host, upload, launches, the one read-back) as
median / p10 / p90 over --repeat calls after --warmup calls, the host route once (or --host-repeat times), and per launch the device
time between events around each C-ABI call of one run (torch.sort included as its own row).
Needs a GPU; there is no fallback.
Usage: python tools/time_kitti_eval.py [--frames 3769] [--repeat 20] [--warmup 3] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'crb-active-3ddet_amd')):
    sys.path.insert(0, p)

CLASSES = ['Car', 'Pedestrian', 'Cyclist']


def stats(v):
    v = np.sort(np.asarray(v))
    return {'median_ms': float(np.median(v)) * 1e3, 'p10_ms': float(np.percentile(v, 10)) * 1e3, 'p90_ms': float(np.percentile(v, 90)) * 1e3}


def launch_breakdown(gt, dt):
    """device time of every crb_kitti_* call and of torch.sort in one evaluation (events around each, one synchronise at the end)"""
    import torch
    from crbhip import kitti_eval as dev
    from pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_eval
    marks = []

    class Timed(object):
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith('crb_kitti') or name == 'crb_kitti_stage_limit':
                return fn

            def call(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*a)
                e1.record()
                marks.append((name, e0, e1))
                return rc
            return call
    real, sort = dev.lib, torch.sort

    def timed_sort(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = sort(*a, **k)
        e1.record()
        marks.append(('torch.sort', e0, e1))
        return r
    dev.lib, torch.sort = Timed(), timed_sort
    try:
        kitti_eval.get_official_eval_result(gt, dt, CLASSES, route='device')
        torch.cuda.synchronize()
    finally:
        dev.lib, torch.sort = real, sort
    return {name: e0.elapsed_time(e1) for name, e0, e1 in marks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3769)
    ap.add_argument('--repeat', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-repeat', type=int, default=1)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs an MI355X: a time taken elsewhere says nothing'
    import kitti_eval_cases as kc
    from pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_eval
    gt, dt, _ = kc.make_annos(9, args.frames, kc.SMALL, lambda g, d: [])
    out = {'frames': args.frames, 'gt_boxes': int(sum(len(a['name']) for a in gt)), 'detections': int(sum(len(a['name']) for a in dt)),
           'combinations': 54}
    t0 = time.perf_counter()
    p = kitti_eval.pack_annos(gt, dt)
    out['pack_ms'] = (time.perf_counter() - t0) * 1e3
    out['pairs'] = int(p['pair_off'][-1])
    times = []
    for i in range(args.warmup + args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        text_dev, _ = kitti_eval.get_official_eval_result(gt, dt, CLASSES, route='device')      # ends in its read-back
        times.append(time.perf_counter() - t0)
    out['device_route'] = stats(times[args.warmup:])
    out['launches_ms'] = launch_breakdown(gt, dt)
    times = []
    for i in range(args.host_repeat):
        t0 = time.perf_counter()
        text_host, _ = kitti_eval.get_official_eval_result(gt, dt, CLASSES, route='host')
        times.append(time.perf_counter() - t0)
    out['host_route'] = stats(times)
    out['same_text'] = text_dev == text_host
    print(json.dumps(out, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(out, open(args.json, 'w'), indent=1)


if __name__ == '__main__':
    main()
