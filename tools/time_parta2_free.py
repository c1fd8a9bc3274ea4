"""Times the anchor-free Part-A2 pieces on the GPU: the point head's box targets, its three losses (forward + backward), decode +
proposals, and the detector's training step - each against the torch route of the same commit (what CRB_PART_HEAD_FUSED=0 /
CRB_POINT_HEAD_FUSED=0 select; for the proposals the reference's per-frame loop over the stacked rows), the step also against PartA2Net's.

  python tools/time_parta2_free.py [--frames 16] [--points 20000] [--iters 50] [--step-iters 10]

Each leg: warm-up, then `iters` rounds in which the two sides alternate; every call is timed with device events; median / p10 / p90
in milliseconds, one JSON line per leg. The head legs run on 16 x 20,000 voxel centres of synthetic KITTI frames (points of the frames
themselves, so that ground truths own points); the step runs the synthetic frames through the whole detector."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'crb-active-3ddet_amd'))

MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]
EXTRA = [0.2, 0.2, 0.2]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def ab(name, sides, iters, warmup=5):
    """sides: {label: callable}; alternates them -> prints one JSON line"""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(iters):
        for k, fn in sides.items():
            t[k].append(timed(fn))
    out = {'leg': name, 'iters': iters}
    for k, v in t.items():
        out[k] = {'median_ms': round(float(np.median(v)), 4), 'p10_ms': round(float(np.percentile(v, 10)), 4),
                  'p90_ms': round(float(np.percentile(v, 90)), 4)}
    print(json.dumps(out), flush=True)
    return out


def head_inputs(frames, points, dev):
    from pcdet.datasets.synthetic import kitti_frame
    rows, gts = [], []
    for f in range(frames):
        p, g = kitti_frame(100 + f, points)
        rows.append(np.concatenate([np.full((len(p), 1), f, np.float32), p[:, :3]], 1))
        gts.append(g)
    G = max(len(g) for g in gts)
    gt = np.zeros((frames, G, 8), np.float32)
    for f, g in enumerate(gts):
        gt[f, :len(g)] = g
    pts = torch.from_numpy(np.concatenate(rows)).to(dev)
    gen = torch.Generator(device='cpu').manual_seed(3)
    N = pts.shape[0]
    cls = (torch.rand((N, 3), generator=gen) * 16 - 8).to(dev)
    part = (torch.rand((N, 3), generator=gen) * 16 - 8).to(dev)
    box = torch.cat([torch.randn((N, 6), generator=gen) * 0.3, torch.randn((N, 2), generator=gen) + 0.5], 1).to(dev)
    return pts, torch.from_numpy(gt).to(dev), cls, part, box


def per_frame_proposals(cls_preds, box_preds, batch_index, batch_size, nms):
    """the reference's loop (roi_head_template.py:70-104) on the stacked rows"""
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    post = nms.NMS_POST_MAXSIZE
    rois = box_preds.new_zeros((batch_size, post, box_preds.shape[-1]))
    scores = box_preds.new_zeros((batch_size, post))
    labels = box_preds.new_zeros((batch_size, post), dtype=torch.long)
    for b in range(batch_size):
        m = batch_index == b
        bp, cp = box_preds[m], cls_preds[m]
        s, lab = torch.max(cp, dim=1)
        top, idx = torch.topk(s, k=min(nms.NMS_PRE_MAXSIZE, s.shape[0]))
        keep, _ = iou3d_nms_utils.nms_gpu(bp[idx][:, 0:7], top, nms.NMS_THRESH)
        sel = idx[keep[:post]]
        rois[b, :len(sel)], scores[b, :len(sel)], labels[b, :len(sel)] = bp[sel], s[sel], lab[sel]
    return rois, scores, labels + 1


def step_batch(frames, points, dev, first=300):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(first, frames, points)
    bidx = np.repeat(np.arange(frames, dtype=np.float32), np.diff(off))
    return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
            'gt_boxes': torch.from_numpy(gt).to(dev), 'batch_size': frames, 'point_frame_counts_host': np.diff(off).tolist(),
            'frame_id': np.array(['%06d' % (first + i) for i in range(frames)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--points', type=int, default=20000)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--step-iters', type=int, default=10)
    ap.add_argument('--legs', default='targets,losses,proposals,step')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    dev = torch.device('cuda', 0)
    from crbhip import part_head, point_box
    from pcdet.config import EasyDict
    from pcdet.models.dense_heads import point_head_template
    from pcdet.utils.box_coder_utils import PointResidualCoder
    assert part_head.FUSED and point_head_template.FUSED
    coder = PointResidualCoder(use_mean_size=True, mean_size=MEAN_SIZE)
    legs = args.legs.split(',')
    B = args.frames
    if set(legs) & {'targets', 'losses', 'proposals'}:
        pts, gt, cls, part, box = head_inputs(B, args.points, dev)
        labels, _, box_labels, part_labels = point_box.point_box_targets(pts, gt, EXTRA, 3, coder)
        print(json.dumps({'rows': int(pts.shape[0]), 'positives': int((labels > 0).sum()), 'gt_rows_per_frame': int(gt.shape[1])}), flush=True)
    if 'targets' in legs:
        ab('targets', {'fused': lambda: point_box.point_box_targets(pts, gt, EXTRA, 3, coder),
                       'torch': lambda: point_box.point_box_targets_torch(pts, gt, EXTRA, 3, coder)}, args.iters)
    if 'losses' in legs:
        w = (0.25, 2.0, (1.0,) * 8, 1.0 / 9.0, 1.0, 1.0, 1.0)

        def run(route):
            c, p, x = (t.detach().requires_grad_(True) for t in (cls, part, box))
            lc, lp, lb, _ = route(c, p, x, labels, part_labels, box_labels, *w)
            (lc + lp + lb).backward()
        ab('losses forward + backward', {'fused': lambda: run(point_box.point_box_loss), 'torch': lambda: run(point_box.point_box_loss_torch)},
           args.iters)
    if 'proposals' in legs:
        from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
        nms = EasyDict({'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000, 'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8})
        head = RoIHeadTemplate(num_class=1, model_cfg=EasyDict({'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5},
                                                                 'LOSS_CONFIG': {'LOSS_WEIGHTS': {'code_weights': [1.0] * 7}}}))

        def fused():
            c, b, n = point_box.point_box_decode(pts, cls, box, coder, B)
            head.proposal_layer({'batch_size': B, 'batch_cls_preds': c, 'batch_box_preds': b, 'batch_counts': n}, nms)

        def loop():
            c, b = point_box.point_box_decode_torch(pts, cls, box, coder)
            per_frame_proposals(c, b, pts[:, 0], B, nms)
        ab('decode + proposals', {'fused': fused, 'torch': loop}, max(5, args.iters // 5))
    if 'step' in legs:
        from pcdet.datasets import SyntheticDataset
        from pcdet.model_cfgs import parta2_free_cfg, parta2_net_cfg
        from pcdet.models import build_network
        ds = SyntheticDataset(num_frames=B, n_points=args.points)
        models = {}
        for name, cfg in (('free', parta2_free_cfg()), ('parta2', parta2_net_cfg('kitti'))):
            torch.manual_seed(0)
            models[name] = build_network(cfg.MODEL, 3, ds).to(dev).train()

        base = step_batch(B, args.points, dev)               # uploaded once: the timed window holds the detector alone

        def step(name, fused):
            part_head.FUSED = point_head_template.FUSED = fused
            try:
                m = models[name]
                ret, _, _ = m(dict(base))
                m.zero_grad(set_to_none=True)
                ret['loss'].backward()
            finally:
                part_head.FUSED = point_head_template.FUSED = True
        ab('training step', {'PointRCNN fused': lambda: step('free', True), 'PointRCNN torch routes': lambda: step('free', False),
                             'PartA2Net': lambda: step('parta2', True)}, args.step_iters, warmup=3)


if __name__ == '__main__':
    main()
