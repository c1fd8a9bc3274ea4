#!/usr/bin/env python
"""SECOND multi-head timings on one MI355X, one process, at --batch frames of the KITTI configuration
(second_multihead_cfg(): 176 x 200 map, 70,400 anchors per head, 211,200 per frame):
  assign : AxisAlignedTargetAssigner with USE_MULTIHEAD through crb_assign_targets, --boxes boxes per frame
  loss   : the three losses of all heads forward + backward with respect to the head outputs, on the kernel (csrc/multihead_loss.hip)
           and on the torch restatement (AnchorHeadMulti.loss_torch), same tensors
  post   : per-class post-processing (threshold, NMS_PRE_MAXSIZE 4096, NMS 0.1, NMS_POST_MAXSIZE 500, per frame x head x class) on the
           device route (csrc/multiclass_nms.hip: one launch sequence, one read-back) and on the loop route (CRB_MULTICLASS_NMS=0: the
           full decode + multi_classes_nms per frame and head), same head outputs; two score distributions: `sparse` (about 100
           anchors of a segment above SCORE_THRESH, a trained detector's regime) and `dense` (about 3,900, near NMS_PRE_MAXSIZE)
  step   : SECONDNet from second_multihead_cfg() forward + backward + grad-clip + AdamW at --batch frames of --points raw points, next
           to the single-head SECOND step from the same run
Device time between two events, one call per sample (the loop route's host synchronisations fall between the events and count); per
figure median, p10 and p90 over --steps samples after --warmup. No pass / fail time is set. Run it under a time limit.
Usage: python tools/time_multihead.py [--batch 16] [--points 20000] [--boxes 30] [--steps 20] [--warmup 5] [--routes assign,loss,post,step]
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
    return {'median_ms': round(q(0.5), 4), 'p10_ms': round(q(0.1), 4), 'p90_ms': round(q(0.9), 4), 'samples': len(ms)}


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


def _head(dev):
    import numpy as np
    import torch
    from pcdet.model_cfgs import second_multihead_cfg
    from pcdet.models.dense_heads import AnchorHeadMulti
    cfg = second_multihead_cfg()
    torch.manual_seed(0)
    head = AnchorHeadMulti(cfg.MODEL.DENSE_HEAD, 512, 3, cfg.CLASS_NAMES, np.array([1408, 1600, 40]), np.array([0, -40, -3, 70.4, 40, 1], np.float32),
                           predict_boxes_when_training=False)
    return cfg, head.to(dev)


def _outputs(dev, B, mean=-4.6, std=1.5, grad=False):
    import torch
    g = torch.Generator(device='cpu').manual_seed(1)
    mk = lambda c, m, s: [(torch.randn((B, 70400, c), generator=g) * s + m).to(dev).requires_grad_(grad) for _ in range(3)]
    return mk(1, mean, std), mk(7, 0.0, 0.3), mk(2, 0.0, 1.5)


def _gt(dev, B, boxes):
    import numpy as np
    import torch
    from pcdet.datasets.synthetic import kitti_batch
    _, _, gt = kitti_batch(0, B, 2000)
    gt = gt[:, :boxes] if gt.shape[1] >= boxes else np.concatenate([gt, np.zeros((B, boxes - gt.shape[1], 8), np.float32)], 1)
    return torch.from_numpy(np.ascontiguousarray(gt)).to(dev)


def run_assign(args, dev):
    _, head = _head(dev)
    gt = _gt(dev, args.batch, args.boxes)
    return {'route': 'assign', 'batch': args.batch, 'boxes_per_frame': int((gt[:, :, 7] > 0).sum(1).float().mean()),
            'assign_targets': _timed(lambda: head.assign_targets(gt_boxes=gt), args.steps, args.warmup)}


def run_loss(args, dev):
    from pcdet.models.dense_heads import anchor_head_multi as ahm
    _, head = _head(dev)
    head.train()
    cls, box, dirs = _outputs(dev, args.batch, grad=True)
    head.forward_ret_dict.update(head.assign_targets(gt_boxes=_gt(dev, args.batch, args.boxes)))
    head.forward_ret_dict.update({'cls_preds': cls, 'box_preds': box, 'dir_cls_preds': dirs})

    def once():
        loss, _ = head.get_loss()
        loss.backward()
        for t in cls + box + dirs:
            t.grad = None
    out = {'route': 'loss', 'batch': args.batch}
    for name, fused in (('kernel', True), ('torch', False)):
        ahm.FUSED_LOSS = fused
        try:
            out['fwd_bwd_' + name] = _timed(once, args.steps, args.warmup)
        finally:
            ahm.FUSED_LOSS = True
    return out


def run_post(args, dev):
    import torch
    from pcdet.models.dense_heads import anchor_head_multi as ahm
    from pcdet.models.detectors.post_processing import multiclass_post_processing
    cfg, head = _head(dev)
    head.eval()
    model = type('M', (), {'model_cfg': cfg.MODEL})()
    out = {'route': 'post', 'batch': args.batch}
    for regime, std in (('sparse', 0.8), ('dense', 1.5)):
        cls, box, dirs = _outputs(dev, args.batch, std=std)
        passing = float(sum((torch.sigmoid(c) >= cfg.MODEL.POST_PROCESSING.SCORE_THRESH).sum() for c in cls)) / (3 * args.batch)
        out['%s_candidates_per_segment' % regime] = round(passing, 1)
        for name, device_route in (('device', True), ('loop', False)):
            def once():
                bd = {'batch_size': args.batch, 'batch_cls_preds': cls, 'cls_preds_normalized': False,
                      'multihead_label_mapping': [h.head_label_indices for h in head.rpn_heads],
                      'multihead_box_decoder': head._head_decoder(args.batch, box, dirs)}
                if not device_route:
                    bd['batch_box_preds'] = head.generate_predicted_boxes(args.batch, cls, box, dirs)[1]
                with torch.no_grad():
                    return multiclass_post_processing(model, bd)
            ahm.MULTICLASS_NMS = device_route
            try:
                out['%s_%s' % (regime, name)] = _timed(once, args.steps, args.warmup)
                out['%s_%s_boxes_per_frame' % (regime, name)] = sum(len(p['pred_scores']) for p in once()[0]) / args.batch
            finally:
                ahm.MULTICLASS_NMS = True
    return out


def run_step(args, dev):
    import numpy as np
    import torch
    from pcdet.datasets import SyntheticDataset
    from pcdet.datasets.synthetic import kitti_batch
    from pcdet.model_cfgs import second_cfg, second_multihead_cfg
    from pcdet.models import build_network
    B = args.batch
    pts, off, gt = kitti_batch(0, B, args.points)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))[:, None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    points, offsets, gtb = t(np.concatenate([bidx, pts], 1)), t(off), t(gt)
    out = {'route': 'step', 'batch': B, 'points': args.points}
    for name, cfg in (('multihead', second_multihead_cfg()), ('single_head', second_cfg('kitti'))):
        torch.manual_seed(0)
        model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=B, n_points=args.points)).to(dev).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True)

        def once():
            ret, _, _ = model({'points': points, 'point_frame_offsets': offsets, 'gt_boxes': gtb, 'batch_size': B})
            opt.zero_grad(set_to_none=True)
            ret['loss'].backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
            opt.step()
        out['train_step_' + name] = _timed(once, args.steps, args.warmup)
        del model, opt
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--boxes', type=int, default=30)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--routes', default='assign,loss,post,step')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    warnings.filterwarnings('ignore', message='.*torch route.*')
    runs = {'assign': run_assign, 'loss': run_loss, 'post': run_post, 'step': run_step}
    for r in args.routes.split(','):
        print(json.dumps(runs[r](args, dev)), flush=True)
