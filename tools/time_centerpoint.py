#!/usr/bin/env python
"""CenterPoint timings on one MI355X, one process:
  kernels : the three kernel groups of csrc/center_head.hip - target assignment, loss forward + backward, decoding - against the torch
            route (CRB_CENTER_FUSED=0, the reference's formulation) on the same device, at the KITTI map: --batch x 3 x 200 x 176,
            three classes in one head, --boxes boxes per frame, NUM_MAX_OBJS 500, K = 500; the maps in channels_last memory, as the
            head's convolutions leave them.
  convs   : the head's convolutions on a (--batch, 512, 200, 176) channels_last map, training mode: shared_conv (+ BN + ReLU), the
            fused first layers of the five branches (one 64 -> 320 convolution + five BN + ReLU), the five final convolutions;
            forward and forward + backward.
  step    : CenterPoint forward + backward + grad-clip + fused AdamW at --batch frames of --points raw points, next to SECOND's step
            from the same run.
Device time between two events, one call per sample; per figure median, p10 and p90 over --steps samples after --warmup. No pass /
fail time is set. Run it under a time limit.
Usage: python tools/time_centerpoint.py [--batch 16] [--points 20000] [--boxes 30] [--steps 20] [--warmup 5] [--routes kernels,convs,step]
Prints one JSON line per route."""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))


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


def _head(dev, channels=512):
    import torch
    from pcdet.model_cfgs import centerpoint_cfg
    from pcdet.models.dense_heads import CenterHead
    cfg = centerpoint_cfg('kitti')
    torch.manual_seed(0)
    head = CenterHead(cfg.MODEL.DENSE_HEAD, channels, 3, cfg.CLASS_NAMES, None, [0, -40, -3, 70.4, 40, 1], [0.05, 0.05, 0.1],
                      predict_boxes_when_training=False)
    return cfg, head.to(dev).to(memory_format=torch.channels_last)


def run_kernels(args):
    import numpy as np
    import torch
    from crbhip import center_head as ch
    dev = torch.device('cuda', 0)
    cfg, head = _head(dev)
    B, H, W = args.batch, 200, 176
    rng = np.random.default_rng(0)
    gt = np.zeros((B, args.boxes + 4, 8), np.float32)
    sizes = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}
    for b in range(B):
        for i in range(args.boxes):
            c = int(rng.integers(1, 4))
            gt[b, i] = [rng.uniform(1, 69), rng.uniform(-39, 39), -1.0, *(np.array(sizes[c]) * rng.uniform(0.9, 1.1, 3)), rng.uniform(-3.1, 3.1), c]
    gt = torch.from_numpy(gt).to(dev)
    cl = lambda *s: torch.randn(s, device=dev).contiguous(memory_format=torch.channels_last)
    hm = (cl(B, 3, H, W) * 2 - 2.19).requires_grad_(True)
    reg = {n: cl(B, c, H, W).requires_grad_(True) for n, c in (('center', 2), ('center_z', 1), ('dim', 3), ('rot', 2))}
    order = list(reg)
    w = cfg.MODEL.DENSE_HEAD.LOSS_CONFIG.LOSS_WEIGHTS
    post = cfg.MODEL.DENSE_HEAD.POST_PROCESSING

    def assign():
        return head.assign_targets(gt, feature_map_size=(H, W))

    t = assign()

    def loss():
        for p in [hm] + list(reg.values()):
            p.grad = None
        parts = ch.center_loss(hm, t['heatmaps'][0], [reg[n] for n in order], t['target_boxes'][0], t['inds'][0], t['masks'][0],
                               w['code_weights'], w['cls_weight'], w['loc_weight'])
        (parts[0] + parts[1]).backward()

    def decode():
        return ch.decode(hm.detach(), [reg[n].detach() for n in order], post.MAX_OBJ_PER_SAMPLE, head.point_cloud_range, head.voxel_size, 8,
                         post.POST_CENTER_LIMIT_RANGE, post.SCORE_THRESH)

    def topk():
        return ch.top_cells(hm.detach(), post.MAX_OBJ_PER_SAMPLE)
    out = {'route': 'kernels', 'batch': B, 'map': [3, H, W], 'boxes_per_frame': args.boxes, 'objects': int(t['masks'][0].sum())}
    for fused in (True, False):
        ch.FUSED = fused
        tag = 'fused' if fused else 'torch_route'
        try:
            out[tag] = {'assign_targets': _timed(assign, args.steps, args.warmup), 'loss_forward_backward': _timed(loss, args.steps, args.warmup),
                        'decode_with_topk': _timed(decode, args.steps, args.warmup)}
        finally:
            ch.FUSED = True
    out['topk_alone'] = _timed(topk, args.steps, args.warmup)
    return out


def run_convs(args):
    import torch
    from pcdet.models.dense_heads import center_head as mod
    dev = torch.device('cuda', 0)
    _, head = _head(dev)
    head.train()
    x = torch.randn((args.batch, 512, 200, 176), device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sep = head.heads_list[0]
    with torch.no_grad():
        y = mod._run(head.shared_conv, x).detach()
    y.requires_grad_(True)

    def bwd(fn, inp):
        def go():
            inp.grad = None
            head.zero_grad(set_to_none=True)
            out = fn()
            out = sum(o.sum() for o in out.values()) if isinstance(out, dict) else out.sum()
            out.backward()
        return go

    def fwd(fn):
        def go():
            with torch.no_grad():
                fn()
        return go
    shared = lambda: mod._run(head.shared_conv, x)
    branches = lambda: sep(y)
    out = {'route': 'convs', 'batch': args.batch, 'map': [512, 200, 176]}
    out['shared_conv_forward'] = _timed(fwd(shared), args.steps, args.warmup)
    out['shared_conv_forward_backward'] = _timed(bwd(shared, x), args.steps, args.warmup)
    for fused in (True, False):
        mod.FUSED_HEAD_CONVS = fused
        tag = 'branches_fused_first_layers' if fused else 'branches_separate_first_layers'
        try:
            out[tag + '_forward'] = _timed(fwd(branches), args.steps, args.warmup)
            out[tag + '_forward_backward'] = _timed(bwd(branches, y), args.steps, args.warmup)
        finally:
            mod.FUSED_HEAD_CONVS = True
    return out


def run_step(args):
    import numpy as np
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import centerpoint_cfg, second_cfg
    from pcdet.models import build_network
    dev = torch.device('cuda', 0)
    batches = []
    for k in range(2):
        pts, off, gt = kitti_batch(k * args.batch, args.batch, args.points)
        bidx = np.repeat(np.arange(args.batch, dtype=np.float32), np.diff(off))[:, None]
        batches.append({'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                        'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': args.batch})
    out = {'route': 'step', 'batch': args.batch, 'points_per_frame': args.points}
    for name, cfg in (('centerpoint', centerpoint_cfg('kitti')), ('second', second_cfg('kitti'))):
        torch.manual_seed(0)
        model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=args.batch, n_points=args.points)).to(dev).train()
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
        out[name] = _timed(step, args.steps, args.warmup)
        out[name]['frames_per_s'] = args.batch / (out[name]['median_ms'] * 1e-3)
        del model, opt
        torch.cuda.empty_cache()
    out['peak_allocated_MB'] = torch.cuda.max_memory_allocated(dev) / 2 ** 20
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--boxes', type=int, default=30)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='kernels,convs,step')
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'needs an MI355X: a timing on the host says nothing'
    runs = {'kernels': run_kernels, 'convs': run_convs, 'step': run_step}
    with warnings.catch_warnings():
        warnings.filterwarnings('ignore', message='.*torch route.*')
        for route in a.routes.split(','):
            print(json.dumps(runs[route](a)), flush=True)


if __name__ == '__main__':
    main()
