#!/usr/bin/env python
"""VectorPool aggregation of PV-RCNN++: the fused route (csrc/vector_pool.hip + batched GEMMs) against the torch route of the same
commit (CRB_VECTOR_POOL_FUSED=0: the reference's expressions on the same three-NN / voxel-query results), and against
aggregation='sa' (StackSAModuleMSG layers), on the same frames:
  * each of the four VectorPool layers (raw_points, x_conv3, x_conv4, RoI grid pool) alone, forward + backward, on the inputs it
    receives in a training step
  * the training step (forward, backward, clip, AdamW)
The routes alternate inside every round; each figure is a host clock around calls that end in a device synchronise; median, p10 and
p90 over the rounds are reported.
Usage: python tools/time_vector_pool.py [--batch 16] [--points 20000] [--rounds 9] [--steps 7]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def stats(v):
    return {'median': round(float(np.median(v)), 3), 'p10': round(float(np.percentile(v, 10)), 3), 'p90': round(float(np.percentile(v, 90)), 3),
            'n': len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--steps', type=int, default=7)
    a = ap.parse_args()
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import pv_rcnn_plusplus_cfg
    from pcdet.models import build_network
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    assert torch.cuda.is_available(), 'needs an MI355X'
    dev = torch.device('cuda', 0)
    pts, off, gt = kitti_batch(100, a.batch, a.points)
    bidx = np.repeat(np.arange(a.batch, dtype=np.float32), np.diff(off))
    base = {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
            'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': a.batch, 'point_frame_counts_host': np.diff(off).tolist()}
    models = {}
    for agg in ('vector_pool', 'sa'):
        torch.manual_seed(0)
        m = build_network(pv_rcnn_plusplus_cfg('kitti', aggregation=agg).MODEL, 3, SyntheticDataset(num_frames=2)).to(dev)
        m.train()
        models[agg] = (m, torch.optim.AdamW(m.parameters(), lr=1e-4, weight_decay=0.01))

    def step(agg):
        m, opt = models[agg]
        opt.zero_grad(set_to_none=True)
        ret, _, _ = m(dict(base))
        ret['loss'].backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 10.0)
        opt.step()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def set_fused(on):
        pm.VECTOR_POOL_FUSED = on

    # the inputs each VectorPool layer receives in a training step
    vp = models['vector_pool'][0]
    layers = {'raw_points': vp.pfe.SA_rawpoints, 'x_conv3': vp.pfe.SA_layers[0], 'x_conv4': vp.pfe.SA_layers[1],
              'roi_grid_pool': vp.roi_head.roi_grid_pool_layer}
    captured, hooks = {}, []
    for name, layer in layers.items():
        def hook(mod, args, kwargs, name=name):
            captured[name] = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in kwargs.items()}
        hooks.append(layer.register_forward_pre_hook(hook, with_kwargs=True))
    set_fused(True)
    step('vector_pool')
    for h in hooks:
        h.remove()
    out = {'batch': a.batch, 'points': a.points, 'layers': {}, 'shapes': {}}

    def layer_pass(name):
        kw = dict(captured[name])
        kw['features'] = kw['features'].clone().requires_grad_(True)
        _, y = layers[name](**kw)
        y.sum().backward()

    for name in layers:
        kw = captured[name]
        out['shapes'][name] = {'support_rows': int(kw['xyz'].shape[0]), 'new_rows': int(kw['new_xyz'].shape[0]), 'channels': int(kw['features'].shape[1])}
        res = {'fused': [], 'torch': []}
        for on in (True, False):                               # warm-up
            set_fused(on)
            layer_pass(name)
        for _ in range(a.rounds):
            for key, on in (('fused', True), ('torch', False)):
                set_fused(on)
                res[key].append(timed(lambda: layer_pass(name)))
        out['layers'][name] = {k: stats(v) for k, v in res.items()}
    for p in vp.parameters():
        p.grad = None
    routes = (('vector_pool_fused', 'vector_pool', True), ('vector_pool_torch', 'vector_pool', False), ('sa', 'sa', True))
    times = {r[0]: [] for r in routes}
    for key, agg, on in routes:                                # warm-up
        set_fused(on)
        step(agg)
    for _ in range(a.steps):
        for key, agg, on in routes:
            set_fused(on)
            times[key].append(timed(lambda: step(agg)))
    set_fused(True)
    out['train_step_ms'] = {k: stats(v) for k, v in times.items()}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
