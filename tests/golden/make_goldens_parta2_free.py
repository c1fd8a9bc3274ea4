"""Golden vectors of the anchor-free Part-A2 (PartA2_free.yaml): tests/golden/ref_part_box.npz from the reference's own
PointIntraPartOffsetHead with its box branch, PointHeadBox and RoIHeadTemplate.proposal_layer on stacked per-point boxes, and
tests/golden/ref_parta2_free.npz from one training step and one eval pass of the reference's own PointRCNN detector.

Runs ONLY in the authoring container (needs the reference tree); the .npz files it writes are committed and are the only things that
travel. Usage:  python tests/golden/make_goldens_parta2_free.py [box] [net]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py (points-in-boxes, the
rotated overlap and the NMS are answered by the oracle, _install_cpu_ops; the spconv oracle and the pooling stub are those of
make_goldens_parta2.py / make_goldens_parta2_net.py), feeds the seeded cases of tests/part_box_cases.py and stores outputs.

box, per case: the reference's assign_targets (f32; its rotate_points_along_z casts to f32, so the f64 side of the labels is the numpy
definition of tests/part_box_cases.py), get_loss with its autograd in f32 and in f64 on the SAME f32 labels (the f64 run keeps f32 row
weights: it is checked against the definition at 2e-7 and the definition is stored), generate_predicted_boxes in f32 against the
definition. e_ref_* = max|f32 - f64| is the reference's own f32 error, the unit of the tests' bars.
proposals: a stacked input (420 / 150 / 0 rows) through generate_predicted_boxes and proposal_layer with NMS_PRE_MAXSIZE 300,
NMS_POST_MAXSIZE 64; the seed is the first at which no pair of candidates has a BEV IoU within 1e-4 of NMS_THRESH (asserted)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import part_box_cases as pb                    # noqa: E402
import part_cases                              # noqa: E402
from _constants import EasyDict                # noqa: E402

_np = mg._np
LOSS_KEYS = ('loss_cls', 'loss_part', 'loss_box', 'pos', 'd_cls', 'd_part', 'd_box')


def head_cfg(num_class, part=True, fc=(16,)):
    cfg = {'CLS_FC': list(fc), 'REG_FC': list(fc), 'CLASS_AGNOSTIC': False,
           'TARGET_CONFIG': {'GT_EXTRA_WIDTH': part_cases.EXTRA, 'BOX_CODER': 'PointResidualCoder',
                             'BOX_CODER_CONFIG': {'use_mean_size': True, 'mean_size': pb.MEAN_SIZE[:1] if num_class == 1 else pb.MEAN_SIZE}},
           'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss', 'LOSS_WEIGHTS': dict(pb.LOSS_WEIGHTS, code_weights=pb.CODE_WEIGHTS)}}
    if part:
        cfg['PART_FC'] = list(fc)
    return EasyDict(cfg)


def _ref_head(num_class, part=True):
    from pcdet.models.dense_heads.point_head_box import PointHeadBox
    from pcdet.models.dense_heads.point_intra_part_head import PointIntraPartOffsetHead
    torch.manual_seed(0)
    return (PointIntraPartOffsetHead if part else PointHeadBox)(num_class=num_class, input_channels=16, model_cfg=head_cfg(num_class, part))


def _loss_runs(head, case, labels, part32, box32):
    runs = {}
    for dtype in (torch.float32, torch.float64):
        cls = torch.from_numpy(case['cls_preds']).to(dtype).requires_grad_(True)
        prt = torch.from_numpy(case['part_preds']).to(dtype).requires_grad_(True)
        box = torch.from_numpy(case['box_preds']).to(dtype).requires_grad_(True)
        head.forward_ret_dict = {'point_cls_preds': cls, 'point_part_preds': prt, 'point_box_preds': box, 'point_cls_labels': labels,
                                 'point_part_labels': part32.to(dtype), 'point_box_labels': box32.to(dtype)}
        tb = {}
        loss_cls, tb = head.get_cls_layer_loss(tb)
        loss_part, tb = head.get_part_layer_loss(tb)
        loss_box, tb = head.get_box_layer_loss(tb)
        total, tb2 = head.get_loss()
        assert abs(float(total.detach()) - float((loss_cls + loss_part + loss_box).detach())) < 1e-6 * max(1.0, abs(float(total.detach())))
        assert sorted(tb2) == ['point_loss_box', 'point_loss_cls', 'point_loss_part', 'point_pos_num']
        g_cls, = torch.autograd.grad(loss_cls, cls)
        g_prt, = torch.autograd.grad(loss_part, prt, allow_unused=True)
        g_box, = torch.autograd.grad(loss_box, box, allow_unused=True)
        runs[dtype] = {'loss_cls': _np(loss_cls).reshape(1), 'loss_part': _np(loss_part).reshape(1), 'loss_box': _np(loss_box).reshape(1),
                       'pos': np.array([tb['point_pos_num']]), 'd_cls': _np(g_cls),
                       'd_part': _np(g_prt) if g_prt is not None else np.zeros(prt.shape),
                       'd_box': _np(g_box) if g_box is not None else np.zeros(box.shape)}
    return runs


def _store_losses(out, tag, runs, d, keys=LOSS_KEYS):
    """the f64 side of every key, the f32 side of the scalars (the f32 gradients would double the file; e_ref carries what the tests
    need of them)"""
    for k in keys:
        v32, v64 = runs[torch.float32][k], runs[torch.float64][k]
        # the reference's f64 run keeps f32 row weights (`.float()`: 1 / pos rounded to f32), so it is the definition only to 1e-7; the
        # definition is stored as the f64 side and e_ref includes that rounding
        assert np.abs(v64 - d[k]).max() <= 2e-7 * max(1.0, np.abs(d[k]).max()), (tag, k, np.abs(v64 - d[k]).max())
        v64 = np.asarray(d[k], np.float64).reshape(v64.shape)
        out['%s_f64_%s' % (tag, k)] = v64
        if v32.size == 1:
            out['%s_f32_%s' % (tag, k)] = v32
        out['%s_e_ref_%s' % (tag, k)] = np.array([np.abs(v32.astype(np.float64) - v64).max()])


def gen_box(out):
    for name in pb.CASES:
        case = pb.make_case(name)
        head = _ref_head(case['num_class'])
        tgt = head.assign_targets({'point_coords': torch.from_numpy(case['points']), 'gt_boxes': torch.from_numpy(case['gt_boxes'].copy())})
        labels, part32, box32 = tgt['point_cls_labels'], tgt['point_part_labels'], tgt['point_box_labels']
        assert np.array_equal(_np(labels), case['labels']), name
        assert (_np(box32)[case['owner'] < 0] == 0).all()
        out[name + '_labels'], out[name + '_owner'] = _np(labels), case['owner']
        out[name + '_part_f32'], out[name + '_box_f32'] = _np(part32), _np(box32)   # (the f64 side is the definition: part_box_cases)
        out[name + '_e_ref_part'] = np.array([np.abs(_np(part32).astype(np.float64) - case['part_labels_f64']).max()])
        out[name + '_e_ref_box'] = np.array([np.abs(_np(box32).astype(np.float64) - case['box_labels_f64']).max()])
        # PointHeadBox: the same labels and box labels, no part labels
        tgt_b = _ref_head(case['num_class'], part=False).assign_targets(
            {'point_coords': torch.from_numpy(case['points']), 'gt_boxes': torch.from_numpy(case['gt_boxes'].copy())})
        assert torch.equal(tgt_b['point_cls_labels'], labels) and torch.equal(tgt_b['point_box_labels'], box32) and \
            tgt_b['point_part_labels'] is None
        runs = _loss_runs(head, case, labels, part32, box32)
        d = pb.box_loss_f64(case['cls_preds'], case['part_preds'], case['box_preds'], _np(labels), _np(part32), _np(box32))
        _store_losses(out, name, runs, d)
        if name == 'tiles':                                  # a NaN box label on one positive row: the prediction takes its place
            box_nan = box32.clone()
            box_nan[pb.nan_row(case), pb.NAN_CODE] = float('nan')
            runs_nan = _loss_runs(head, case, labels, part32, box_nan)
            d_nan = pb.box_loss_f64(case['cls_preds'], case['part_preds'], case['box_preds'], _np(labels), _np(part32), _np(box_nan))
            assert d_nan['d_box'][pb.nan_row(case), pb.NAN_CODE] == 0 and d['d_box'][pb.nan_row(case), pb.NAN_CODE] != 0
            _store_losses(out, name + '_nan', runs_nan, d_nan, keys=('loss_box', 'd_box'))
        # generate_predicted_boxes
        pts = torch.from_numpy(case['points'])
        cls32, dec32 = head.generate_predicted_boxes(pts[:, 1:4], torch.from_numpy(case['cls_preds']), torch.from_numpy(case['box_preds']))
        dec64, _ = pb.decode_f64(case['points'], case['cls_preds'], case['box_preds'], case['mean_size'])
        assert np.array_equal(_np(cls32), case['cls_preds'])
        out[name + '_decode_f32'] = _np(dec32)                                       # (the f64 side is the definition)
        out[name + '_e_ref_decode'] = np.array([np.abs(_np(dec32).astype(np.float64) - dec64).max()])
        print('  %-7s N %5d pos %5d  losses %.6f %.6f %.6f  e_ref: %s' % (
            name, len(case['points']), int((case['labels'] > 0).sum()), float(d['loss_cls']), float(d['loss_part']), float(d['loss_box']),
            ' '.join('%s %.1e' % (k, out['%s_e_ref_%s' % (name, k)][0]) for k in ('box', 'decode', 'loss_box', 'd_box', 'loss_cls', 'd_cls'))))
    out['tb_keys'] = np.array(['point_loss_box', 'point_loss_cls', 'point_loss_part', 'point_pos_num'])
    for tag, part in (('head', True), ('box_head', False)):
        sd = _ref_head(3, part).state_dict()
        out[tag + '_keys'] = np.array(sorted(sd.keys()))
        out[tag + '_shapes'] = np.array([str(tuple(v.shape)) for _, v in sorted(sd.items())])
    gen_proposals(out)


def gen_proposals(out):
    from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
    from pcdet.config import cfg as ref_cfg
    import oracle
    ref_cfg.CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']                 # (proposal_layer sizes full_cls_scores by it)
    head = _ref_head(3)
    nms = EasyDict(pb.PROPOSAL_NMS)
    roi_cfg = EasyDict({'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5},
                        'LOSS_CONFIG': {'LOSS_WEIGHTS': {'code_weights': [1.0] * 7}}})
    roi_head = RoIHeadTemplate(num_class=1, model_cfg=roi_cfg)
    for seed in range(400, 500):
        case = pb.proposal_case(seed)
        pts = torch.from_numpy(case['points'])
        cls, boxes = head.generate_predicted_boxes(pts[:, 1:4], torch.from_numpy(case['cls_preds']), torch.from_numpy(case['box_preds']))
        margin, o = np.inf, 0
        for n in case['counts']:
            if n:
                s = _np(cls)[o:o + n].max(1)
                cand = _np(boxes)[o:o + n][np.argsort(-s)[:nms.NMS_PRE_MAXSIZE]]
                iou = oracle.boxes_pairwise(cand, cand, 1).astype(np.float64)
                margin = min(margin, float(np.abs(iou - nms.NMS_THRESH).min()))
            o += n
        if margin > pb.PROPOSAL_IOU_MARGIN:
            break
    else:
        raise AssertionError('no seed keeps the candidates away from NMS_THRESH')
    bd = roi_head.proposal_layer({'batch_size': case['batch_size'], 'batch_cls_preds': cls, 'batch_box_preds': boxes, 'batch_index': pts[:, 0]},
                                 nms_config=nms)
    dec64, _ = pb.decode_f64(case['points'], case['cls_preds'], case['box_preds'], pb.mean_size(3))
    out['prop_seed'], out['prop_iou_margin'] = np.array([seed]), np.array([margin])
    out['prop_e_ref_decode'] = np.array([np.abs(_np(boxes).astype(np.float64) - dec64).max()])
    for k in ('rois', 'roi_scores', 'roi_labels', 'full_cls_scores'):
        out['prop_' + k] = _np(bd[k])
    kept = (_np(bd['rois'])[..., 3] > 0).sum(1)
    print('  proposals: seed %d, IoU margin %.2e, kept %s of %s rows, e_ref decode %.1e' % (
        seed, margin, kept.tolist(), case['counts'], out['prop_e_ref_decode'][0]))
    assert 0 < kept[0] < nms.NMS_POST_MAXSIZE or kept[0] == nms.NMS_POST_MAXSIZE
    assert 0 < kept[1] and kept[2] == 0 and (_np(bd['roi_labels'])[2] == 1).all()


# ---- the detector ---------------------------------------------------------------------------------------------------------------
KINK, TIE_MARGIN, PLANE_MARGIN = 1e-4, 1e-5, 2e-6
# the eval pass's final NMS: second-stage boxes of about 1 m agree to about 1e-6 m between f32 implementations, which moves a BEV IoU by
# some 1e-5; scores (sigmoid) agree far better than 1e-3. The ORDER of two predictions may differ (score gaps are not kept): the
# test matches predictions by position
SCORE_MARGIN, IOU_MARGIN = 1e-3, 5e-5
SEEDS = range(5, 25)


def _pool_case(inter, rois, cfg):
    """what the RoI head pools with DISABLE_PART (xyz in place of the part offsets), as a case of tests/roiaware_cases.py"""
    pc = _np(inter['point_coords'])
    score = _np(inter['point_cls_scores']).reshape(-1, 1)
    B = rois.shape[0]
    return {'rois': rois[..., :7].astype(np.float32), 'pts': np.ascontiguousarray(pc[:, 1:4]),
            'off': np.searchsorted(pc[:, 0], np.arange(B + 1)).astype(np.int32),
            'part': np.concatenate([pc[:, 1:4], score], 1).astype(np.float32), 'feat': _np(inter['point_features']),
            'o': int(cfg.ROI_AWARE_POOL.POOL_SIZE), 'max_pts': int(cfg.ROI_AWARE_POOL.MAX_POINTS_PER_VOXEL)}


def _tie_margin(d, case):
    tie = np.inf
    for kept in d['kept']:
        if len(kept) > 1:
            f = np.sort(case['feat'][kept].astype(np.float64), axis=0)
            gap, live = f[-1] - f[-2], ~((f[-1] == 0) & (f[-2] == 0))
            if live.any():
                tie = min(tie, float(gap[live].min()))
    return tie


def gen_net(out, oracle):
    """ref_parta2_free.npz: one training step and one eval pass of the reference's PointRCNN (PartA2_free.yaml with the reductions of
    part_box_cases.net_overrides) on the reduced U-Net grid. Discrete decisions are kept away from their thresholds as in
    make_goldens_parta2_net.py (ReLU kinks, max ties, cell planes; SEG_MASK_SCORE_THRESH is 0, so there is no score mask) and the
    margins are asserted; ground truth is an input placed on some proposals of the first stage."""
    import yaml
    import make_goldens_parta2 as mp
    import make_goldens_parta2_net as mn
    import roiaware_cases as rc
    from _constants import seeded_state
    from pcdet.config import cfg as ref_cfg
    mp._install_spconv_torch(oracle)
    mn.install_pool_stub(oracle)
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/kitti_models/PartA2_free.yaml')))
    model_cfg, class_names = pb.net_overrides(EasyDict(y['MODEL'])), y['CLASS_NAMES']
    ref_cfg.CLASS_NAMES, ref_cfg.MODEL = class_names, model_cfg
    from pcdet.models import build_network
    from pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer
    pcr = np.array(part_cases.UNET_PCR, np.float32)

    class Dataset:
        pass
    ds = Dataset()
    ds.class_names, ds.grid_size, ds.point_cloud_range, ds.voxel_size = class_names, np.array(part_cases.UNET_GRID), pcr, part_cases.UNET_VOXEL
    ds.depth_downsample_factor = None
    ds.point_feature_encoder = EasyDict(num_point_features=4)
    torch.manual_seed(0)
    model = build_network(model_cfg=model_cfg, num_class=3, dataset=ds)
    assert type(model).__name__ == 'PointRCNN'
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'UNetV2', 'PointIntraPartOffsetHead', 'PartA2FCHead']
    out['keys'] = np.array(sorted(model.state_dict().keys()))
    out['shapes'] = np.array([str(tuple(v.shape)) for _, v in sorted(model.state_dict().items())])
    overrides = {}

    def reload():
        sd = seeded_state(model, pb.NET_SEED)
        for k in pb.NET_SMALL:
            sd[k] = sd[k] * 0.1
        sd.update({k: torch.from_numpy(v) for k, v in overrides.items()})
        model.load_state_dict(sd)
    reload()
    model.train()
    nb = pb.net_batch()
    B = nb['batch_size']

    def make_batch(gt):
        return {'points': torch.from_numpy(nb['points'].copy()), 'voxels': torch.from_numpy(nb['voxels'].copy()), 'voxel_num_points': torch.from_numpy(nb['voxel_num_points'].copy()),
                'voxel_coords': torch.from_numpy(nb['voxel_coords'].copy()), 'gt_boxes': torch.from_numpy(gt.copy()), 'batch_size': B,
                'frame_id': np.array(['%06d' % i for i in range(B)])}
    head = model.roi_head
    gt0 = np.zeros((B, pb.NET_GT, 8), np.float32)

    # ReLU kinks of the first stage (train-mode BatchNorm; the predictions do not read the ground truth)
    with torch.no_grad():
        bd0 = model.vfe(make_batch(gt0))
    kink = {'backbone_3d': mn.settle_kinks(model.backbone_3d, lambda: model.backbone_3d(dict(bd0)), 'backbone_3d.', overrides)}
    with torch.no_grad():
        bd1 = model.backbone_3d(dict(bd0))
    kink['point_head'] = mn.settle_kinks(model.point_head, lambda: model.point_head(dict(bd1)), 'point_head.', overrides)

    # pass 1: the proposals of the first stage; ground truth is an INPUT placed on some of them
    with torch.no_grad():
        bd = head.proposal_layer(model.point_head(dict(bd1)), nms_config=head.model_cfg.NMS_CONFIG['TRAIN'])
    prop = {k: bd[k].detach().clone() for k in ('rois', 'roi_scores', 'roi_labels')}
    rng = np.random.default_rng(77)
    gt = np.zeros((B, pb.NET_GT, 8), np.float32)
    for b in range(B):
        k = 0
        for r, lab in zip(prop['rois'][b].numpy(), prop['roi_labels'][b].numpy()):
            ok = (r[3:6] > 0.3).all() and (r[3:6] < 5).all() and pcr[0] < r[0] < pcr[3] and pcr[1] < r[1] < pcr[4] and pcr[2] < r[2] < pcr[5]
            if ok and all(np.hypot(*(r[:2] - g[:2])) > 0.8 for g in gt[b, :k]):
                gt[b, k, :7] = r + np.concatenate([rng.uniform(-0.05, 0.05, 3), r[3:6] * rng.uniform(-0.04, 0.04, 3), rng.uniform(-0.04, 0.04, 1)])
                gt[b, k, 7] = lab
                k += 1
            if k == pb.NET_GT - 1:
                break
        assert k >= 3, k
    out['gt'] = gt
    centres, o = _np(bd['point_coords'])[:, 1:4], int(model_cfg.ROI_HEAD.ROI_AWARE_POOL.POOL_SIZE)
    voff = np.searchsorted(_np(bd['point_coords'])[:, 0], np.arange(B + 1))
    # the voxel centres keep 1e-4 off the faces of the ground truths and their enlarged twins (f32 and f64 containment agree)
    for b in range(B):
        assert not part_cases._near_a_face(centres[voff[b]:voff[b + 1]], gt[b], part_cases.EXTRA).any()

    # cell planes: the sampler seed whose RoIs keep the voxel centres farthest from faces and cell planes
    best = (-1.0, None)
    for seed in SEEDS:
        np.random.seed(seed); torch.manual_seed(seed)
        t = head.assign_targets({'batch_size': B, 'gt_boxes': torch.from_numpy(gt.copy()), **{k: v.clone() for k, v in prop.items()}})
        m = mn.plane_margin(centres, voff, _np(t['rois']), o)
        if m > best[0]:
            best = (m, seed)
    plane, sampler_seed = best
    print('  sampler seed %d, plane margin %.3g' % (sampler_seed, plane))
    assert plane > PLANE_MARGIN
    out['sampler_seed'] = np.array([sampler_seed])

    sampled, captured, inter, state = [], {}, {}, {}
    orig = ProposalTargetLayer.subsample_rois
    orig_pl, orig_pool, orig_forward = head.proposal_layer, head.roiaware_pool, head.forward

    def recording(self, max_overlaps):
        idx = orig(self, max_overlaps)
        sampled.append(idx.clone())
        return idx

    def capture(bdict, nms_config):
        first = bdict.get('rois', None) is None
        if first:
            for k in ('batch_cls_preds', 'batch_box_preds', 'batch_index'):
                captured['stacked_' + k] = bdict[k].detach().clone()
        bdict = orig_pl(bdict, nms_config=nms_config)
        if first:
            captured.update({k: bdict[k].detach().clone() for k in ('rois', 'roi_scores', 'roi_labels')})
        return bdict

    def pool_capture(bdict):
        for k in ('point_coords', 'point_features', 'point_cls_scores', 'rois'):
            inter[k] = bdict[k].detach().clone()
        p = orig_pool(bdict)
        inter['coords'] = p[0].detach().sum(dim=-1).nonzero().int()
        return p

    def head_capture(bdict):
        state['bd'] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in bdict.items()}
        return orig_forward(bdict)
    head.roiaware_pool, head.proposal_layer = pool_capture, capture

    def step(gt_now, grad):
        del sampled[:]
        ProposalTargetLayer.subsample_rois = recording
        np.random.seed(sampler_seed); torch.manual_seed(sampler_seed)
        try:
            with torch.enable_grad() if grad else torch.no_grad():
                return model(make_batch(gt_now))
        finally:
            ProposalTargetLayer.subsample_rois = orig

    # ReLU kinks of the RoI head on the step's own pooled rows
    assert float(model_cfg.ROI_HEAD.SEG_MASK_SCORE_THRESH) == 0.0
    reload()
    head.forward = head_capture
    step(gt, False)
    head.forward = orig_forward

    def run_head():
        np.random.seed(sampler_seed); torch.manual_seed(sampler_seed)
        ProposalTargetLayer.subsample_rois = recording
        try:
            head(dict(state['bd']))
        finally:
            ProposalTargetLayer.subsample_rois = orig
    kink['roi_head'] = mn.settle_kinks(head, run_head, 'roi_head.', overrides)
    for k, v in overrides.items():
        out['bias/' + k] = v

    # the step
    reload()
    ret, tb, _ = step(gt, True)
    loss = ret['loss']
    model.zero_grad()
    loss.backward()
    assert len(sampled) == B
    for k in prop:
        assert torch.equal(captured[k], prop[k]), k
    fr, pr = head.forward_ret_dict, model.point_head.forward_ret_dict
    out['proposals'], out['proposal_scores'], out['proposal_labels'] = (_np(captured[k]) for k in ('rois', 'roi_scores', 'roi_labels'))
    out['stacked_cls_preds'], out['stacked_box_preds'] = _np(captured['stacked_batch_cls_preds']), _np(captured['stacked_batch_box_preds'])
    out['sampled'] = np.stack([_np(s) for s in sampled]).astype(np.int64)
    out['rois'] = _np(fr['rois'])
    assert np.array_equal(out['rois'], np.take_along_axis(out['proposals'], out['sampled'][:, :, None], axis=1))
    out['point_coords'], out['point_cls_scores'] = _np(inter['point_coords']), _np(inter['point_cls_scores'])
    out['point_cls_labels'], out['point_box_labels'] = _np(pr['point_cls_labels']), _np(pr['point_box_labels'])
    out['coords'] = _np(inter['coords'])
    out['rcnn_cls'], out['rcnn_reg'] = _np(fr['rcnn_cls']), _np(fr['rcnn_reg'])
    out['loss'] = np.array([float(loss.detach())])
    out['tb_keys'] = np.array(sorted(tb.keys()))
    out['tb_vals'] = np.array([float(tb[k]) for k in sorted(tb.keys())], np.float64)
    params = dict(model.named_parameters())
    for n, sl in pb.NET_GRADS.items():
        out['grad/' + n] = _np(params[n].grad)[sl].copy()
        out['gradmax/' + n] = np.array([float(params[n].grad.abs().max())])
        assert np.abs(out['grad/' + n]).max() > 0, n

    # margins of the final step
    case = _pool_case(inter, out['rois'], model_cfg.ROI_HEAD)
    d = rc.pool_definition(case)
    assert np.array_equal(d['coords'], out['coords'])                 # the numpy definition gives the reference's rows
    tie, plane = _tie_margin(d, case), mn.plane_margin(case['pts'], case['off'], out['rois'], o)
    out['margins'] = np.array([min(kink.values()), tie, plane])
    print('  margins: kinks %s, max ties %.3g, cell planes %.3g' % (kink, tie, plane))
    assert min(kink.values()) > KINK and tie > TIE_MARGIN and plane > PLANE_MARGIN
    print('  loss %.5f' % float(loss), {k: round(float(v), 5) for k, v in tb.items()})
    print('  voxels %d, rows %d, positives %d, fg rois %d' % (len(centres), len(out['coords']), int((out['point_cls_labels'] > 0).sum()),
                                                              int((_np(fr['rcnn_cls_labels']) > 0.5).sum())))
    assert np.isfinite(out['loss']).all() and (out['point_cls_labels'] > 0).sum() > 0

    # the eval pass (running statistics of the seeded state): proposals of the first stage, then the pred_dicts on them
    # (the reference's post_processing reads the class names from DENSE_HEAD.ANCHOR_GENERATOR_CONFIG and records the dense head's
    # rpn_preds, neither of which this yaml has: its eval pass runs only with the list supplied and an empty rpn_preds entry)
    model.model_cfg.DENSE_HEAD = EasyDict({'ANCHOR_GENERATOR_CONFIG': [{'class_name': c} for c in class_names]})
    reload()                                                  # (the training passes above moved the running statistics)
    orig_pp = model.post_processing
    model.post_processing = lambda bdict: orig_pp(dict(bdict, rpn_preds=None))
    model.eval()
    captured.clear()
    with torch.no_grad():
        pred_dicts, _ = model(make_batch(gt))
    head.roiaware_pool, head.proposal_layer = orig_pool, orig_pl
    out['eval_proposals'], out['eval_proposal_scores'], out['eval_proposal_labels'] = (_np(captured[k]) for k in ('rois', 'roi_scores', 'roi_labels'))
    case = _pool_case(inter, out['eval_proposals'], model_cfg.ROI_HEAD)
    plane_eval = mn.plane_margin(case['pts'], case['off'], out['eval_proposals'], o)
    post = model_cfg.POST_PROCESSING
    for b, p in enumerate(pred_dicts):
        out['pred_boxes_%d' % b], out['pred_scores_%d' % b], out['pred_labels_%d' % b] = (_np(p[k]) for k in ('pred_boxes', 'pred_scores', 'pred_labels'))
    # margins of the final NMS: every second-stage score off SCORE_THRESH, every pair of boxes above it off NMS_THRESH (what decides
    # WHICH boxes are predicted), and the smallest gap between two scores (what decides their order)
    with torch.no_grad():
        bd = model.roi_head(model.point_head(model.backbone_3d(model.vfe(make_batch(gt)))))
    thr_margin = iou_margin = gap = np.inf
    for b in range(B):
        s = _np(torch.sigmoid(bd['batch_cls_preds'][b])).reshape(-1)
        live = _np(bd['batch_box_preds'][b])[s > post.SCORE_THRESH]
        iou = oracle.boxes_pairwise(live, live, 1).astype(np.float64)
        thr_margin, iou_margin = min(thr_margin, float(np.abs(s - post.SCORE_THRESH).min())), min(iou_margin, float(np.abs(iou - post.NMS_CONFIG.NMS_THRESH).min()))
        gap = min(gap, float(np.diff(np.sort(s[s > post.SCORE_THRESH])).min()))
    nms_margin = min(thr_margin, iou_margin)
    print('  eval margins: score threshold %.3g, IoU %.3g, score gap %.3g' % (thr_margin, iou_margin, gap))
    out['eval_margins'] = np.array([plane_eval, thr_margin, iou_margin, gap])
    print('  eval: predictions %s, cell planes %.3g, final NMS margin %.3g' % ([len(p['pred_scores']) for p in pred_dicts], plane_eval, nms_margin))
    assert plane_eval > PLANE_MARGIN and thr_margin > SCORE_MARGIN and iou_margin > IOU_MARGIN and sum(len(p['pred_scores']) for p in pred_dicts) > 0


if __name__ == '__main__':
    which = sys.argv[1:] or ['box', 'net']
    mg.import_reference()
    oracle_mod = mg._install_cpu_ops()
    if 'box' in which:
        d = {}
        gen_box(d)
        mg.save('ref_part_box.npz', d)
    if 'net' in which:
        d = {}
        gen_net(d, oracle_mod)
        mg.save('ref_parta2_free.npz', d)
