#!/usr/bin/env python
"""Part-A2 timings on one MI355X, one process:
  targets : crb_part_targets (one launch for all frames) against the reference's route written out here - a loop over the frames, each
            with a boolean-mask gather, two points_in_boxes_gpu queries, the label arithmetic and the part-label expressions
            (pcdet/models/dense_heads/point_head_template.py:74-122);
  losses  : crb_part_loss_forward + crb_part_loss_backward (forward and backward) against the reference's get_cls_layer_loss +
            get_part_layer_loss and autograd (:131-173, with its max(1, pos.item()) host read; F.binary_cross_entropy spelled out in
            its own arithmetic, see reference_losses).
The torch route is the reference's expressions, not the code under test (crbhip.part_head.*_torch is the batched restatement the
tests use). --batch frames of --rows voxel centres each (ragged: frame b has rows - 37 b), --boxes ground truths per frame in --slots
rows; half of the points inside enlarged boxes. Both routes are checked against each other at the timed size before anything is timed.
Host time around a device synchronise (the reference's route stalls on the host, which device events between launches would not
show), samples of the two routes alternating; per figure median, p10 and p90 over --steps samples after --warmup. No pass / fail time
is set. Run it under a time limit.
  pooling : the RoI-aware pooling of PartA2FCHead forward + backward with its peak memory, sparse route (csrc/roiaware_sparse.hip: one
            launch sequence for all frames, rows of the sparse tensor) against the dense route (two RoIAwarePool3d calls per frame,
            `sum(-1).nonzero()`, gather), on what PartA2Net hands its RoI head for --batch synthetic KITTI frames: UNetV2's voxel
            centres and 16 point features, the point head's part offsets and scores, 128 RoIs per frame sampled from proposals drawn
            around the ground truths, POOL_SIZE 12, 128 points per cell;
  step    : PartA2Net (parta2_net_cfg, DP_RATIO as in the yaml) forward + backward on those frames in frames/s, both routes.
Usage: python tools/time_parta2.py [--batch 16] [--rows 16000] [--boxes 30] [--slots 40] [--steps 30] [--warmup 5]
                                   [--legs head,pooling,step] [--points 16384]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

EXTRA = [0.2, 0.2, 0.2]
ALPHA, GAMMA, W_CLS, W_PART = 0.25, 2.0, 1.0, 1.0


def _stats(ms):
    ms = sorted(ms)
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    return {'median_ms': q(0.5), 'p10_ms': q(0.1), 'p90_ms': q(0.9), 'samples': len(ms)}


def _timed_pair(fns, steps, warmup):
    """the routes of `fns` alternating, host clock around a synchronise -> {name: stats}"""
    import torch
    out = {k: [] for k in fns}
    for i in range(warmup + steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                out[k].append((time.perf_counter() - t0) * 1e3)
    return {k: _stats(v) for k, v in out.items()}


def make_inputs(args, dev):
    import numpy as np
    import torch
    import part_cases as cases
    rng = np.random.default_rng(3)
    gt = np.stack([cases._boxes(rng, args.boxes, args.slots, (4.0, 66.0)) for _ in range(args.batch)])
    rows = []
    for b in range(args.batch):
        n = args.rows - 37 * b
        idx = rng.integers(0, args.boxes, n // 2)
        loc = rng.uniform(-0.5, 0.5, (n // 2, 3)) * (gt[b, idx, 3:6] + np.asarray(EXTRA, np.float32))
        c, s = np.cos(gt[b, idx, 6].astype(np.float64)), np.sin(gt[b, idx, 6].astype(np.float64))
        near = np.stack([loc[:, 0] * c - loc[:, 1] * s + gt[b, idx, 0], loc[:, 0] * s + loc[:, 1] * c + gt[b, idx, 1], loc[:, 2] + gt[b, idx, 2]], 1)
        far = np.stack([rng.uniform(cases.PCR[k], cases.PCR[k + 3], n - n // 2) for k in range(3)], 1)
        pts = np.concatenate([near, far])[rng.permutation(n)]
        rows.append(np.concatenate([np.full((n, 1), b), pts], 1))
    points = torch.from_numpy(np.concatenate(rows).astype(np.float32)).to(dev)
    N = points.shape[0]
    cls = torch.from_numpy(rng.uniform(-8, 8, (N, 3)).astype(np.float32)).to(dev)
    prt = torch.from_numpy(rng.uniform(-8, 8, (N, 3)).astype(np.float32)).to(dev)
    return points, torch.from_numpy(gt).to(dev), cls, prt


def reference_targets(points, gt_boxes, num_class):
    """point_head_template.py:74-122 as the reference runs it: frame by frame"""
    import torch
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    from pcdet.utils import box_utils, common_utils
    B = gt_boxes.shape[0]
    extend = box_utils.enlarge_box3d(gt_boxes.view(-1, gt_boxes.shape[-1]), extra_width=EXTRA).view(B, -1, gt_boxes.shape[-1])
    bs_idx = points[:, 0]
    labels = points.new_zeros(points.shape[0]).long()
    part = gt_boxes.new_zeros((points.shape[0], 3))
    for k in range(B):
        mask = bs_idx == k
        single = points[mask][:, 1:4]
        lab = labels.new_zeros(mask.sum())
        idx = roiaware_pool3d_utils.points_in_boxes_gpu(single.unsqueeze(0), gt_boxes[k:k + 1, :, 0:7].contiguous()).long().squeeze(0)
        fg = idx >= 0
        ext = roiaware_pool3d_utils.points_in_boxes_gpu(single.unsqueeze(0), extend[k:k + 1, :, 0:7].contiguous()).long().squeeze(0)
        lab[fg ^ (ext >= 0)] = -1
        box = gt_boxes[k][idx[fg]]
        lab[fg] = 1 if num_class == 1 else box[:, -1].long()
        labels[mask] = lab
        p = part.new_zeros((mask.sum(), 3))
        t = common_utils.rotate_points_along_z((single[fg] - box[:, 0:3]).view(-1, 1, 3), -box[:, 6]).view(-1, 3)
        p[fg] = t / box[:, 3:6] + torch.tensor([0.5, 0.5, 0.5]).view(1, 3).type_as(t)
        part[mask] = p
    return labels, part


def reference_losses(cls_preds, part_preds, labels, part_labels, loss_fn):
    """point_head_template.py:131-173"""
    import torch
    num_class = cls_preds.shape[1]
    positives = labels > 0
    cls_weights = ((labels == 0) * 1.0 + 1.0 * positives).float()
    pos_normalizer = positives.sum(dim=0).float()
    cls_weights /= torch.clamp(pos_normalizer, min=1.0)
    one_hot = cls_preds.new_zeros(*list(labels.shape), num_class + 1)
    one_hot.scatter_(-1, (labels * (labels >= 0).long()).unsqueeze(dim=-1).long(), 1.0)
    loss_cls = loss_fn(cls_preds, one_hot[..., 1:], weights=cls_weights).sum() * W_CLS
    pos_mask = labels > 0
    norm = max(1, (pos_mask > 0).sum().item())
    # F.binary_cross_entropy's own arithmetic as torch expressions: part labels leave [0, 1] by the 1e-5 margin of the containment test
    # (4 rows of the default inputs) and the device kernel behind F.binary_cross_entropy asserts 0 <= target <= 1
    p = torch.sigmoid(part_preds)
    src = (part_labels - 1) * torch.log(1 - p).clamp(min=-100) - part_labels * torch.log(p).clamp(min=-100)
    loss_part = (src.sum(dim=-1) * pos_mask.float()).sum() / (3 * norm) * W_PART
    return loss_cls, loss_part


def detector_batch(B, n_points, dev, seed=9):
    """B synthetic KITTI frames with 128 proposals per frame drawn around the ground truths"""
    import numpy as np
    import torch
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(500, B, n_points)
    rng = np.random.default_rng(seed)
    rois = np.zeros((B, 128, 7), np.float32)
    labels = np.ones((B, 128), np.int64)
    for b in range(B):
        real = gt[b][gt[b][:, 7] > 0]
        for r in range(128):
            g = real[r % len(real)]
            rois[b, r] = g[:7] + np.concatenate([rng.normal(0, 0.3, 3), g[3:6] * rng.uniform(-0.1, 0.2, 3), rng.normal(0, 0.15, 1)])
            labels[b, r] = int(g[7])
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))[:, None]

    def batch():
        return {'points': torch.from_numpy(np.concatenate([bidx, pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
                'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': B, 'rois': torch.from_numpy(rois).to(dev),
                'roi_scores': torch.ones((B, 128), device=dev), 'roi_labels': torch.from_numpy(labels).to(dev)}
    return batch


def _peak_of(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def detector_legs(args, dev, legs):
    import torch
    from crbhip import roiaware_sparse
    from crbhip.part_head import frame_offsets
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import parta2_net_cfg
    from pcdet.models import build_network
    from pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils import roiaware_pool_sparse
    torch.manual_seed(0)
    cfg = parta2_net_cfg('kitti')
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=args.points)).to(dev)
    model.train()
    batch = detector_batch(args.batch, args.points, dev)
    out = {}

    def step():
        model.zero_grad(set_to_none=True)
        ret, _, _ = model(batch())
        ret['loss'].backward()
        return ret['loss']
    if 'pooling' in legs:
        bd = batch()
        with torch.no_grad():
            model(bd)
        head = model.roi_head
        rois = bd['rois'][..., :7].contiguous()
        frame = bd['point_coords'][:, 0].contiguous()
        xyz = bd['point_coords'][:, 1:4].contiguous()
        off = frame_offsets(frame.view(-1, 1), args.batch)
        part0, feat0 = head.part_features(bd).detach(), bd['point_features'].detach()
        pool = head.roiaware_pool3d_layer

        def sparse():
            part, feat = part0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
            c, p, f, _ = roiaware_pool_sparse(rois, xyz, off, part, feat, pool.out_size, pool.max_pts_each_voxel)
            torch.autograd.backward([p, f], [torch.ones_like(p), torch.ones_like(f)])
            return c, p, f, part.grad, feat.grad

        def dense():
            part, feat = part0.clone().requires_grad_(True), feat0.clone().requires_grad_(True)
            pp, pr = [], []
            for b in range(args.batch):
                m = frame == b
                cur_xyz, cur_roi = xyz[m].contiguous(), rois[b].contiguous()
                pp.append(pool(cur_roi, cur_xyz, part[m].contiguous(), pool_method='avg'))
                pr.append(pool(cur_roi, cur_xyz, feat[m].contiguous(), pool_method='max'))
            pp, pr = torch.cat(pp), torch.cat(pr)
            idx = pp.sum(dim=-1).nonzero()
            r, x, y, z = idx.unbind(1)
            p, f = pp[r, x, y, z], pr[r, x, y, z]
            torch.autograd.backward([p, f], [torch.ones_like(p), torch.ones_like(f)])
            return idx.int(), p, f, part.grad, feat.grad
        a, b = sparse(), dense()
        agree = {'rows': int(a[0].shape[0]), 'points': int(xyz.shape[0]), 'coords_equal': bool(torch.equal(a[0], b[0])),
                 'part_equal': bool(torch.equal(a[1], b[1])), 'feat_equal': bool(torch.equal(a[2], b[2])),
                 'grad_part_max_diff': float((a[3] - b[3]).abs().max()), 'grad_feat_max_diff': float((a[4] - b[4]).abs().max())}
        assert agree['coords_equal'] and agree['part_equal'] and agree['feat_equal'], agree
        del a, b
        t = _timed_pair({'sparse': sparse, 'dense': dense}, args.steps, args.warmup)
        t['sparse']['peak_mb'], t['dense']['peak_mb'] = _peak_of(sparse), _peak_of(dense)
        t['speedup_median'] = t['dense']['median_ms'] / t['sparse']['median_ms']
        t['agreement'] = agree
        out['pooling_forward_backward'] = t
    if 'step' in legs:
        res = {}
        for name, on in (('sparse', True), ('dense', False)):
            roiaware_sparse.ENABLED = on
            st = _timed_pair({name: step}, args.steps, args.warmup)[name]
            st['frames_per_s'] = args.batch / (st['median_ms'] * 1e-3)
            res[name] = st
        roiaware_sparse.ENABLED = True
        out['training_step'] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--rows', type=int, default=16000)
    ap.add_argument('--boxes', type=int, default=30)
    ap.add_argument('--slots', type=int, default=40)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--legs', default='head,pooling,step')
    ap.add_argument('--points', type=int, default=16384)
    args = ap.parse_args()
    legs = args.legs.split(',')
    import torch
    assert torch.cuda.is_available(), 'needs an MI355X'
    if 'head' not in legs:
        print(json.dumps(detector_legs(args, torch.device('cuda', 0), legs)))
        return
    from crbhip import part_head
    from pcdet.utils import loss_utils
    assert part_head.FUSED
    dev = torch.device('cuda', 0)
    points, gt, cls, prt = make_inputs(args, dev)
    focal = loss_utils.SigmoidFocalClassificationLoss(alpha=ALPHA, gamma=GAMMA)

    # the two routes on the timed inputs: same labels; part labels, losses and gradients to f32 rounding
    lab, part, _ = part_head.part_targets(points, gt, EXTRA, 3)
    lab_r, part_r = reference_targets(points, gt, 3)
    same_labels = bool(torch.equal(lab, lab_r))
    part_diff = float((part - part_r).abs().max())

    def fused_losses():
        c, p = cls.clone().requires_grad_(True), prt.clone().requires_grad_(True)
        lc, lp, _ = part_head.part_loss(c, p, lab, part, ALPHA, GAMMA, W_CLS, W_PART)
        (lc + lp).backward()
        return lc, lp, c.grad, p.grad

    def torch_losses():
        c, p = cls.clone().requires_grad_(True), prt.clone().requires_grad_(True)
        lc, lp = reference_losses(c, p, lab, part, focal)
        (lc + lp).backward()
        return lc, lp, c.grad, p.grad
    a, b = fused_losses(), torch_losses()
    check = {'labels_equal': same_labels, 'part_labels_max_diff': part_diff,
             'loss_cls_rel_diff': abs(float(a[0].detach()) - float(b[0].detach())) / abs(float(b[0].detach())), 'loss_part_rel_diff': abs(float(a[1].detach()) - float(b[1].detach())) / abs(float(b[1].detach())),
             'grad_cls_max_diff': float((a[2] - b[2]).abs().max()), 'grad_part_max_diff': float((a[3] - b[3]).abs().max())}
    assert same_labels and part_diff < 1e-5 and check['loss_cls_rel_diff'] < 1e-5 and check['loss_part_rel_diff'] < 1e-5, check

    out = {'rows': int(points.shape[0]), 'batch': args.batch, 'boxes': args.boxes, 'slots': args.slots,
           'positives': int((lab > 0).sum()), 'agreement': check}
    t = _timed_pair({'fused': lambda: part_head.part_targets(points, gt, EXTRA, 3), 'reference_route': lambda: reference_targets(points, gt, 3)},
                    args.steps, args.warmup)
    out['targets'] = t
    t = _timed_pair({'fused': fused_losses, 'reference_route': torch_losses}, args.steps, args.warmup)
    out['losses_forward_backward'] = t
    for k in ('targets', 'losses_forward_backward'):
        out[k]['speedup_median'] = out[k]['reference_route']['median_ms'] / out[k]['fused']['median_ms']
    out.update(detector_legs(args, dev, legs))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
