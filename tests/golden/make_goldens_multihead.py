"""Golden vectors of the SECOND multi-head family (tests/golden/ref_multihead.npz) from the reference's own AnchorHeadMulti,
AxisAlignedTargetAssigner, loss_utils and model_nms_utils.multi_classes_nms.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_multihead.py [targets] [loss] [select] [head] [forward] [cfg] [rpn <dump.npz>]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, feeds the seeded
inputs of tests/multihead_cases.py and stores outputs, per (frame, head) where the reference produces them per (frame, head). Float
quantities are recorded from an f32 run and an f64 run of the same reference code; e_ref_* = max|f32 - f64| is the reference's own f32
error, the unit of the tests' bars. A part that is not named keeps what the existing file holds.
`rpn` is no reference output: it merges the dump of csrc/rpn_loss.hip's single-head outputs made with the PARENT commit's build
(multihead_cases.rpn_single_outputs on an MI355X, saved as an .npz whose path is given after the word rpn)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import multihead_cases as cases                # noqa: E402
from _constants import EasyDict                # noqa: E402

_np = mg._np


def _ref_head(layout, grid, **kw):
    from pcdet.models.dense_heads.anchor_head_multi import AnchorHeadMulti
    torch.manual_seed(0)
    return AnchorHeadMulti(EasyDict(cases.head_cfg(layout, **kw)), **cases.head_kwargs(grid))


def _assign(head, gt, dtype):
    head.anchors = [a.to(dtype) for a in head.anchors]
    t = head.assign_targets(gt_boxes=torch.from_numpy(gt.copy()).to(dtype))
    return _np(t['box_cls_labels']), _np(t['box_reg_targets'])


def gen_targets(out):
    """the reference's assigner with USE_MULTIHEAD on every ground-truth set, f32 and f64 (labels must agree)"""
    for name, (grid, _, _) in cases.GT_CASES.items():
        gt = cases.make_gt(name)
        l32, t32 = _assign(_ref_head('three', grid), gt, torch.float32)
        l64, t64 = _assign(_ref_head('three', grid), gt, torch.float64)
        assert np.array_equal(l32, l64), name
        # the head layout does not enter: the multi-head order is the classes one after another
        for lay in ('two', 'one'):
            l2, t2 = _assign(_ref_head(lay, grid), gt, torch.float32)
            assert np.array_equal(l2, l32) and np.array_equal(t2, t32, equal_nan=True), (name, lay)
        tag = 'targets_' + name
        out[tag + '_labels'], out[tag + '_reg'] = l32.astype(np.int8), t32.astype(np.float32)
        out[tag + '_e_ref'] = np.abs(t32.astype(np.float64) - t64).reshape(-1, 7).max(0)
        print('  %-18s positives per frame %s, ignored %s, e_ref per column %s' % (
            tag, (l32 > 0).sum(1).tolist(), (l32 < 0).sum(1).tolist(), np.array2string(out[tag + '_e_ref'], precision=2)))


def _ref_loss(case, labels, targets, dtype):
    layout, separate, use_dir, grid = cases.LOSS_CASES[case]
    head = _ref_head(layout, grid, separate=separate, use_dir=use_dir)
    head.anchors = [a.to(dtype) for a in head.anchors]
    cls, box, dirs = cases.make_preds(case)
    leaf = lambda arrs: None if arrs is None else [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrs]
    cls, box, dirs = leaf(cls), leaf(box), leaf(dirs)
    pack = (lambda ts: ts) if separate else (lambda ts: torch.cat(ts, dim=1))
    head.forward_ret_dict = {'cls_preds': pack(cls), 'box_preds': pack(box), 'box_cls_labels': torch.from_numpy(labels.copy()),
                             'box_reg_targets': torch.from_numpy(targets.copy()).to(dtype)}
    if dirs is not None:
        head.forward_ret_dict['dir_cls_preds'] = pack(dirs)
    cls_loss, _ = head.get_cls_layer_loss()
    box_loss, tb = head.get_box_reg_layer_loss()
    (cls_loss + box_loss).backward()
    dir_loss = tb.get('rpn_loss_dir', 0.0)
    res = {'loss': np.array([float(cls_loss), float(box_loss) - dir_loss, dir_loss], np.float64)}
    for key, ts in (('cls', cls), ('box', box), ('dir', dirs)):
        if ts is not None:
            res['g_' + key] = [_np(t.grad) for t in ts]
    return res


def gen_loss(out):
    """the reference's get_cls_layer_loss + get_box_reg_layer_loss per case, f32 and f64, on the planted labels / targets"""
    for case, (layout, separate, use_dir, grid) in cases.LOSS_CASES.items():
        src = 'targets_tiny' if grid == cases.TINY else 'targets_mixed'
        labels, targets = cases.plant_targets(out[src + '_labels'], out[src + '_reg'], grid)
        r32, r64 = _ref_loss(case, labels, targets, torch.float32), _ref_loss(case, labels, targets, torch.float64)
        tag = 'loss_' + case
        # (the loc / dir split of the f32 run goes through .item() sums: the parts carry the total's rounding)
        out[tag + '_f32'], out[tag + '_f64'] = r32['loss'], r64['loss']
        out[tag + '_e_ref'] = np.abs(r32['loss'] - r64['loss'])
        msg = []
        for key in ('g_cls', 'g_box', 'g_dir'):
            if key not in r64:
                continue
            e = max(np.abs(a.astype(np.float64) - b).max() for a, b in zip(r32[key], r64[key]))
            out['%s_e_ref_%s' % (tag, key)] = np.array([e])
            for h, g in enumerate(r64[key]):
                out['%s_%s_%d_rows_f64' % (tag, key, h)] = g[:, ::cases.GRAD_ROWS].copy()
            msg.append('%s %.3g (max %.3g)' % (key, e, max(np.abs(g).max() for g in r64[key])))
        print('  %-28s loss %s e_ref %s; gradient e_ref %s' % (tag, np.array2string(r64['loss'], precision=6),
                                                                np.array2string(out[tag + '_e_ref'], precision=2), ', '.join(msg)))
    # The three loss values are single numbers: one run's |f32 - f64| can land far below half an f32 step of the value by accident
    # (two_sep_dir: 2.4e-7 on 505.8, whose f32 neighbours are 3.1e-5 apart), a bar no f32 result can be held to. The unit of the
    # loss values' bars is therefore the reference's f32 error RELATIVE to the value, the largest over all cases, per component.
    rel = np.zeros(3)
    for case in cases.LOSS_CASES:
        f64 = out['loss_%s_f64' % case]
        rel = np.maximum(rel, np.where(f64 != 0, out['loss_%s_e_ref' % case] / np.where(f64 != 0, np.abs(f64), 1.0), 0.0))
    out['loss_e_ref_rel'] = rel
    print('  loss values: e_ref relative to the value, largest over the cases: %s' % np.array2string(rel, precision=3))


def _install_normal_nms(oracle):
    mod = sys.modules['pcdet.ops.iou3d_nms.iou3d_nms_cuda']

    def nms_normal_gpu(boxes, keep, thresh):
        k = oracle.nms(boxes.numpy(), float(thresh), rotated=False)
        keep[:len(k)] = torch.from_numpy(k.astype(np.int64))
        return len(k)
    mod.nms_normal_gpu = nms_normal_gpu


def gen_select(out):
    """AnchorHeadMulti.generate_predicted_boxes + model_nms_utils.multi_classes_nms per (frame, head) as the reference's
    post_processing loops them (NMS answered by the oracle's C restatement), after the margins of the case have been checked"""
    from pcdet.models.model_utils import model_nms_utils
    oracle = mg._install_cpu_ops()
    _install_normal_nms(oracle)
    for name, c in cases.SEL_CASES.items():
        d = cases.make_selection(name)
        head = _ref_head(c['layout'], c['grid']).eval()
        t = lambda arrs: [torch.from_numpy(a) for a in arrs]
        cls, boxes = head.generate_predicted_boxes(batch_size=cases.B, cls_preds=t(d['cls']), box_preds=t(d['box']), dir_cls_preds=t(d['dir']))
        sizes = cases.head_sizes(c['layout'], True, c['grid'])
        per_head, start = [], 0
        for n, _, _ in sizes:
            per_head.append(_np(boxes[:, start:start + n]))
            start += n
        cand = cases.check_selection_margins(name, per_head)
        nms = EasyDict(cases.nms_cfg(name))
        counts = np.zeros((cases.B, len(sizes)), np.int64)
        tag = 'sel_' + name
        for b in range(cases.B):
            rows, start = {'scores': [], 'labels': [], 'boxes': []}, 0
            for h, (n, _, _) in enumerate(sizes):
                s, l, bx = model_nms_utils.multi_classes_nms(cls_scores=torch.sigmoid(cls[h][b]), box_preds=boxes[b, start:start + n],
                                                             nms_config=nms, score_thresh=c['thresh'])
                rows['scores'].append(_np(s))
                rows['labels'].append(_np(head.rpn_heads[h].head_label_indices[l]))
                rows['boxes'].append(_np(bx).reshape(-1, 7))
                counts[b, h] = len(s)
                start += n
            for k, v in rows.items():
                out['%s_%s_%d' % (tag, k, b)] = np.concatenate(v, 0)
        out[tag + '_counts'] = counts
        out[tag + '_candidates'] = np.array([[sum(len(cand[(b, h, k)]) for k in range(C)) for h, (_, C, _) in enumerate(sizes)] for b in range(cases.B)])
        print('  %-16s candidates per (frame, head) %s, kept %s' % (tag, out[tag + '_candidates'].tolist(), counts.tolist()))


def gen_head(out):
    """state-dict keys and shapes of the reference's AnchorHeadMulti in the configurations the round-trip test builds"""
    for tag, kw in (('three', dict(layout='three')), ('two_all', dict(layout='two', separate=False)),
                    ('sep_reg', dict(layout='two', sep_reg=True)), ('layers', dict(layout='three', head_layers=True, use_dir=False)),
                    ('no_shared', dict(layout='one', shared=None))):
        sd = _ref_head(grid=cases.GRID, **kw).state_dict()
        out['head_%s_keys' % tag] = np.array(list(sd.keys()))
        out['head_%s_shapes' % tag] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
        print('  head_%s: %d entries' % (tag, len(sd)))
        if tag == 'sep_reg':
            # the bias initialisation of the classification tower's last convolution and of the regression towers
            out['head_sep_reg_biases'] = np.array([float(v.float().mean()) for k, v in sd.items() if k.endswith('bias') and 'conv_' in k
                                                   and v.dim() == 1 and k.rsplit('.', 2)[-2] == '3'])


def gen_forward(out):
    """the reference head's forward outputs (multi-head layout) in train mode with seeded weights, f32 and f64"""
    from _constants import seeded_state
    for tag, kw in cases.FORWARD_CASES.items():
        res = {}
        for dtype in (torch.float32, torch.float64):
            head = _ref_head(grid=cases.GRID, **kw)
            head.load_state_dict(seeded_state(head, cases.FORWARD_SEED))
            head = head.to(dtype).train()
            head.anchors = [a.to(dtype) for a in head.anchors]
            head({'spatial_features_2d': torch.from_numpy(cases.forward_input()).to(dtype), 'batch_size': cases.B,
                  'gt_boxes': torch.from_numpy(cases.make_gt('mixed').copy()).to(dtype)})
            fr = head.forward_ret_dict
            res[dtype] = {k: [_np(t) for t in (fr[k] if isinstance(fr[k], list) else [fr[k]])] for k in ('cls_preds', 'box_preds', 'dir_cls_preds') if k in fr}
        for k in res[torch.float32]:
            for h, (a, b) in enumerate(zip(res[torch.float32][k], res[torch.float64][k])):
                out['fwd_%s_%s_%d_f64' % (tag, k, h)] = b[:, ::cases.FORWARD_ROWS].copy()
                out['fwd_%s_%s_%d_shape' % (tag, k, h)] = np.array(b.shape)
                out['fwd_%s_%s_%d_e_ref' % (tag, k, h)] = np.array([np.abs(a.astype(np.float64) - b).max()])
        print('  fwd_%s: %s' % (tag, {k: [list(t.shape) for t in v] for k, v in res[torch.float64].items()}))


def gen_cfg(out):
    """the values of kitti_models/second_multihead.yaml, as data (JSON)"""
    import yaml
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/kitti_models/second_multihead.yaml')))
    out['cfg_json'] = np.array(json.dumps({'CLASS_NAMES': y['CLASS_NAMES'], 'MODEL': y['MODEL'], 'OPTIMIZATION': y['OPTIMIZATION']}, sort_keys=True))


def gen_rpn(out, path):
    d = np.load(path)
    for k in d.files:
        out['rpn_parent_' + k] = d[k]
    print('  %d arrays of the parent build\'s single-head outputs' % len(d.files))


if __name__ == '__main__':
    mg.import_reference()
    argv = sys.argv[1:]
    rpn_path = None
    if 'rpn' in argv:
        rpn_path = argv.pop(argv.index('rpn') + 1)
    parts = {'targets': gen_targets, 'loss': gen_loss, 'select': gen_select, 'head': gen_head, 'forward': gen_forward, 'cfg': gen_cfg,
             'rpn': lambda o: gen_rpn(o, rpn_path)}
    only = argv or [p for p in parts if p != 'rpn']
    prefix = {'targets': 'targets_', 'loss': 'loss_', 'select': 'sel_', 'head': 'head_', 'forward': 'fwd_', 'cfg': 'cfg_', 'rpn': 'rpn_parent_'}
    d = {}
    if os.path.exists(cases.GOLDEN):
        old = np.load(cases.GOLDEN)
        d = {k: old[k] for k in old.files if not any(k.startswith(prefix[n]) for n in only)}
    for name in only:
        print(name)
        parts[name](d)
    np.savez_compressed(cases.GOLDEN, **d)
    print(os.path.basename(cases.GOLDEN), '%.1f KB' % (os.path.getsize(cases.GOLDEN) / 1024))
