#!/usr/bin/env python
"""gt_sampling timings on one MI355X: a batch of --batch synthetic frames of --points points, the KITTI sample groups
(Car:20, Pedestrian:15, Cyclist:15, LIMIT_WHOLE_SCENE) and the object database of --db-frames synthetic frames, through
  world    : DeviceDataProcessor.process_batch(..., augmentor = flip + rotation + scaling)       the baseline, no sampling
  sampling : the same call with gt_sampling in front of the queue                                 select + paste + the baseline's kernels
  launches : crb_gt_sample_select and crb_gt_sample_paste alone on one drawn batch, device time between two events
  host     : the host mirror (DataAugmentor with gt_sampling + DataProcessor range masks) frame after frame on one core; its BEV
             IoU is the package default, the HIP kernel
Per route: median, p10 and p90 of the wall time of a whole call (draws, upload and the one size read-back included; `launches`:
device time) over --steps calls after --warmup calls, every call on fresh draws. `sampling` also reports the resident size of the
database. Each route runs in a child process of its own under a time limit; a route that fails or runs out of time ends the run.
Usage: python tools/time_gt_sampling.py [--batch 16] [--points 20000] [--db-frames 200] [--steps 30] [--warmup 5]
                                        [--routes world,sampling,launches,host]
Prints one JSON line per route."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
CHILD_TIME_LIMIT_S = 420
PCR = [0, -40, -3, 70.4, 40, 1]


def _setup(batch, points, db_frames, sampling):
    import numpy as np
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_frame
    from pcdet.model_cfgs import kitti_augmentor_cfg
    frames, gts = zip(*[kitti_frame(500 + f, points) for f in range(batch)])
    cfgs = [EasyDict({'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}),
            EasyDict({'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': EasyDict({'train': False, 'test': False})})]
    queue = kitti_augmentor_cfg()
    ds, infos = None, None
    if sampling:
        ds = SyntheticDataset(num_frames=db_frames, n_points=points)
        infos = ds.create_groundtruth_database(None)
    else:
        queue = queue[1:]
    np.random.seed(0)
    return list(frames), list(gts), cfgs, queue, ds, infos


def _stats(times):
    times = sorted(times)
    q = lambda f: 1e3 * times[min(len(times) - 1, int(f * len(times)))]
    return {'median_ms': q(0.5), 'p10_ms': q(0.1), 'p90_ms': q(0.9), 'calls': len(times)}


def run_route(route, batch, points, db_frames, steps, warmup):
    import numpy as np
    names = ['Car', 'Pedestrian', 'Cyclist']
    frames, gts, cfgs, queue, ds, infos = _setup(batch, points, db_frames, route != 'world')
    out = {'route': route, 'batch': batch, 'points_per_frame': points}
    if route == 'host':
        import torch
        from pcdet.datasets.augmentor import DataAugmentor
        from pcdet.datasets.processor.data_processor import DataProcessor
        torch.set_num_threads(1)
        aug = DataAugmentor(None, queue, names, db_infos=infos)
        dp = DataProcessor(cfgs[:1], PCR, training=True, num_point_features=frames[0].shape[1])
        cls = np.array(names)

        def call():
            for p, g in zip(frames, gts):
                d = aug.forward({'points': p.copy(), 'gt_boxes': g[:, :-1].copy(), 'gt_names': cls[g[:, -1].astype(np.int64) - 1],
                                 'sample_id_list': None})
                c = np.array([names.index(n) + 1 for n in d['gt_names']], dtype=np.float32).reshape(-1, 1)
                d['gt_boxes'] = np.concatenate([d['gt_boxes'], c], 1)
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
    aug = DeviceDataAugmentor(queue, names, db_infos=infos)
    if route in ('world', 'sampling'):
        times, pasted = [], []
        for i in range(warmup + steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = dp.process_batch(frames, gts, augmentor=aug)
            torch.cuda.synchronize()
            if i >= warmup:
                times.append(time.perf_counter() - t0)
                if route == 'sampling':
                    pasted.append(int(b['gt_sampling_valid'].sum()))
        out.update(_stats(times))
        if route == 'sampling':
            db = aug.database
            out.update(database_objects=db.num_objects, database_points=int(db.points.shape[0]), database_bytes=int(db.nbytes),
                       pasted_objects_per_batch=float(np.mean(pasted)))
        return out
    # launches: the two entry points alone, device time between events
    from crbhip import gt_sampling
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    db = aug.database.device_tensors(dev)
    cls = np.array(names)
    G = max(len(g) for g in gts)
    pad = np.zeros((batch, G, 8), np.float32)
    for k, g in enumerate(gts):
        pad[k, :len(g)] = g
    boxes, counts = t(pad), t(np.array([len(g) for g in gts], np.int32))
    pts = t(np.concatenate(frames, 0))
    off = t(np.concatenate([[0], np.cumsum([len(p) for p in frames])]).astype(np.int32))
    sel, pas = [], []
    for i in range(warmup + steps):
        _, _, draw = aug.draw_batch(batch, gt_names=[cls[g[:, -1].astype(np.int64) - 1] for g in gts])
        cand, cand_obj, goff = t(draw['cand']), t(draw['cand_obj']), t(draw['group_offsets'])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        valid, _, _, rows, pc = gt_sampling.select(boxes, counts, cand, cand_obj, goff, db)
        ev[1].record()
        gt_sampling.paste(pts, off, cand, cand_obj, valid, rows, pc, db, capacity=len(pts) + draw['n_cand_points'], lazy=True)
        ev[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            sel.append(1e-3 * ev[0].elapsed_time(ev[1]))
            pas.append(1e-3 * ev[1].elapsed_time(ev[2]))
    out.update(select={k: v for k, v in _stats(sel).items()}, paste={k: v for k, v in _stats(pas).items()},
               candidates_per_frame=int(draw['cand'].shape[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--db-frames', type=int, default=200)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='world,sampling,launches,host')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(run_route(a.child, a.batch, a.points, a.db_frames, a.steps, a.warmup)), flush=True)
        return
    for route in a.routes.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--child', route, '--batch', str(a.batch), '--points', str(a.points),
               '--db-frames', str(a.db_frames), '--steps', str(a.steps), '--warmup', str(a.warmup)]
        try:
            rc = subprocess.run(cmd, timeout=CHILD_TIME_LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:                                                        # nothing more is started after a failed route
            print(json.dumps({'route': route, 'rc': rc}), flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
