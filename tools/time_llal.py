#!/usr/bin/env python
"""LLAL timings on one MI355X: the PV-RCNN training step (fwd + bwd + AdamW) at --batch frames without a loss net,
with the loss net frozen (OPTIMIZATION.LOSS_NET_SKIP) and in the loss-net phase; and the query pass of `llal` against
`confidence` over a --pool frame synthetic pool at 16 frames per batch. Each variant runs in a fresh child process so that the
CRB_*_FUSED switches (read at import) take effect: --fused 0 times the torch restatements of the reduce=False losses.
Usage: python tools/time_llal.py [--batch 16] [--steps 6] [--warmup 2] [--pool 3000] [--fused 1] [--what step,query]
Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))


def time_step(variant, batch, steps, warmup, points=20000):
    import numpy as np
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import pv_rcnn_llal_cfg
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    cfg = pv_rcnn_llal_cfg()
    if variant == 'plain':
        cfg.MODEL.ROI_HEAD.pop('LOSS_NET')
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2)).to(dev).train()
    if variant == 'frozen':
        for p in model.roi_head.loss_net.parameters():
            p.requires_grad_(False)
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.01)
    batches = []
    for k in range(2):
        pts, off, gt = kitti_batch(100 + k * batch, batch, points)
        bidx = np.repeat(np.arange(batch, dtype=np.float32), np.diff(off))
        batches.append({'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev),
                        'point_frame_offsets': torch.from_numpy(off).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev),
                        'batch_size': batch, 'point_frame_counts_host': np.diff(off).tolist()})

    def step(i):
        opt.zero_grad(set_to_none=True)
        ret, tb, _ = model(dict(batches[i % 2]))
        ret['loss'].backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        return ret['loss']
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    times = []
    for i in range(steps):
        t0 = time.perf_counter()
        step(i)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    return {'what': 'step', 'variant': variant, 'batch': batch, 'median_ms': 1e3 * times[len(times) // 2],
            'min_ms': 1e3 * times[0], 'steps': steps}


def time_query(method, pool_frames, batch):
    import torch
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.model_cfgs import pv_rcnn_llal_cfg
    from pcdet.models import build_network
    from pcdet.query_strategies import build_strategy
    cfg = pv_rcnn_llal_cfg()
    cfg.ACTIVE_TRAIN.SELECT_NUMS = 100
    if method != 'llal':
        cfg.MODEL.ROI_HEAD.pop('LOSS_NET')
    pool = SyntheticDataset(num_frames=pool_frames, first_frame=10000)
    lab = SyntheticDataset(num_frames=4, first_frame=0)
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, pool).to(torch.device('cuda', 0))
    strat = build_strategy(method, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, batch, workers=8),
                           0, '/tmp', cfg)
    warm = build_strategy(method, model, build_synthetic_dataloader(lab, 2),
                          build_synthetic_dataloader(SyntheticDataset(num_frames=2 * batch, first_frame=9000), batch), 0, '/tmp', cfg)
    warm.query(cur_epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    picked = strat.query(cur_epoch=0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {'what': 'query', 'method': method, 'pool': pool_frames, 'batch': batch, 'seconds': dt, 'frames_per_s': pool_frames / dt,
            'picked': len(picked)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=6)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--pool', type=int, default=3000)
    ap.add_argument('--fused', default='1')
    ap.add_argument('--what', default='step,query')
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        kind, name = a.child.split(':')
        r = time_step(name, a.batch, a.steps, a.warmup) if kind == 'step' else time_query(name, a.pool, a.batch)
        r['fused'] = os.environ.get('CRB_RCNN_LOSS_FUSED', '1')
        print(json.dumps(r), flush=True)
        return
    jobs = []
    if 'step' in a.what:
        jobs += ['step:plain', 'step:frozen', 'step:lal']
    if 'query' in a.what:
        jobs += ['query:confidence', 'query:llal']
    env = dict(os.environ, CRB_RCNN_LOSS_FUSED=a.fused, CRB_POINT_HEAD_FUSED=a.fused)
    for j in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), '--child', j, '--batch', str(a.batch), '--steps', str(a.steps),
               '--warmup', str(a.warmup), '--pool', str(a.pool)]
        rc = subprocess.call(cmd, env=env)
        if rc != 0:
            print(json.dumps({'job': j, 'rc': rc}), flush=True)
            sys.exit(rc)


if __name__ == '__main__':
    main()
