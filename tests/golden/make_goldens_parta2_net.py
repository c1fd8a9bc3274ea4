"""Golden of the Part-A2 detector (tests/golden/ref_parta2_net.npz): one training step of the reference's own PartA2Net on the CPU.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_parta2_net.py
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, as gen_pvrcnn_detector
does - the spconv oracle with the torch gather-GEMM and the transposed inverse convolution of make_goldens_parta2.py, _install_cpu_ops,
the pooling stub of gen_partA2 (here with its backward) - feeds two synthetic frames on the grid and point count of the PV-RCNN golden,
DP_RATIO 0, seeded weights, and stores outputs.

Discrete decisions are kept away from their thresholds and the margins are asserted here:
  ReLU kinks   BatchNorm biases of the 3-D backbone, the 2-D backbone and the RoI head are shifted, ReLU by ReLU in execution order, until
               every ReLU input of the step lies farther than KINK from zero (as for UNetV2; the shifted biases travel in the golden);
  score mask   the point head's class bias is shifted until no point inside a sampled RoI scores within MASK_MARGIN of 0.3;
  max ties     the two largest values of a pooled cell and channel are either both exactly zero (post-ReLU features: the first point
               wins on both sides and no gradient flows) or farther apart than TIE_MARGIN;
  cell planes  the sampler seed is the one, of SEEDS, whose sampled RoIs keep the voxel centres farthest from their faces and cell
               planes; that distance must exceed PLANE_MARGIN (RoIs are outputs of the first stage and voxel centres a lattice: neither
               can be moved, so the margin is what f32 rotation leaves, not the 1e-4 of the seeded cases)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import make_goldens_parta2 as mp               # noqa: E402
import part_cases                              # noqa: E402
import roiaware_cases as rc                    # noqa: E402
from _constants import EasyDict, PV_KINDS, PV_FIRST_FRAME, pv_seeded_state  # noqa: E402

PA2_GRADS = rc.PA2_GRADS

_np = mg._np
KINK, MASK_MARGIN, TIE_MARGIN, PLANE_MARGIN = 1e-4, 1e-5, 1e-5, 2e-6
SEEDS = range(5, 25)


def install_pool_stub(oracle):
    """roiaware_pool3d_cuda.forward as in gen_partA2 and its backward: max -> the argmax point, avg -> grad / n to the kept points"""
    pool_mod = sys.modules['pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda']

    def forward(rois, pts, feat, argmax, pts_idx, pooled, method):
        o = tuple(int(v) for v in pooled.shape[1:4])
        p, a, i = oracle.roiaware_pool(rois.detach().numpy(), pts.detach().numpy(), feat.detach().numpy(), o, int(pts_idx.shape[-1]), int(method))
        pooled.copy_(torch.from_numpy(p)); argmax.copy_(torch.from_numpy(a)); pts_idx.copy_(torch.from_numpy(i))

    def backward(pts_idx, argmax, grad_out, grad_in, method):
        C = grad_out.shape[-1]
        g = grad_out.numpy().reshape(-1, C).astype(np.float64)
        gi = np.zeros(tuple(grad_in.shape), np.float64)
        if method == 0:
            am = argmax.numpy().reshape(-1, C)
            cell, ch = np.nonzero(am >= 0)
            np.add.at(gi, (am[cell, ch], ch), g[cell, ch])
        else:
            idx = pts_idx.numpy().reshape(-1, pts_idx.shape[-1])
            for c in np.nonzero(idx[:, 0] > 0)[0]:
                n = idx[c, 0]
                gi[idx[c, 1:1 + n]] += g[c] / n
        grad_in.copy_(torch.from_numpy(gi.astype(np.float32)))
    pool_mod.forward, pool_mod.backward = forward, backward


def settle_kinks(module, run, prefix, overrides):
    """shift BatchNorm biases of `module`, ReLU by ReLU in execution order, until every ReLU input of run() is farther than KINK from 0"""
    for _ in range(400):
        last, seen, hooks = [None], [], []
        for name, m in module.named_modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: last.__setitem__(0, name)))
            elif isinstance(m, torch.nn.ReLU):
                hooks.append(m.register_forward_pre_hook(
                    lambda mod, i: seen.append((last[0], _np(i[0]).swapaxes(0, 1).reshape(i[0].shape[1], -1).astype(np.float64)))))
        with torch.no_grad():
            run()
        for h in hooks:
            h.remove()
        first = next(((n, v) for n, v in seen if np.abs(v).min() <= KINK), None)
        if first is None:
            smallest = min(float(np.abs(v).min()) for _, v in seen)
            print('  kinks %-12s %d ReLU calls, smallest |input| %.3g' % (prefix, len(seen), smallest))
            return smallest
        name, v = first
        bn = module.get_submodule(name)
        shift = np.array([part_cases.nudge(v[c], 2 * KINK) for c in range(v.shape[0])])
        bn.bias.data += torch.from_numpy(shift.astype(np.float32))
        overrides[prefix + name + '.bias'] = _np(bn.bias).copy()
    raise AssertionError('kink margins not met in ' + prefix)


def pool_case(inter, rois, cfg):
    """what the RoI head pools, as a case of tests/roiaware_cases.py"""
    pc = _np(inter['point_coords'])
    score = _np(inter['point_cls_scores']).reshape(-1, 1)
    lead = np.where(score < cfg.SEG_MASK_SCORE_THRESH, np.float32(0), _np(inter['point_part_offset']))
    B = rois.shape[0]
    return {'rois': rois[..., :7].astype(np.float32), 'pts': np.ascontiguousarray(pc[:, 1:4]),
            'off': np.searchsorted(pc[:, 0], np.arange(B + 1)).astype(np.int32), 'part': np.concatenate([lead, score], 1).astype(np.float32),
            'feat': _np(inter['point_features']), 'o': int(cfg.ROI_AWARE_POOL.POOL_SIZE), 'max_pts': int(cfg.ROI_AWARE_POOL.MAX_POINTS_PER_VOXEL)}


def plane_margin(pts, off, rois, o):
    m = np.inf
    for b in range(len(off) - 1):
        for roi in rois[b]:
            if roi[3:6].min() > 0 and off[b + 1] > off[b]:
                m = min(m, float(rc.locate(pts[off[b]:off[b + 1]], roi[:7], o)[2].min()))
    return m


def gen(out):
    oracle = mg._install_cpu_ops()
    mp._install_spconv_torch(oracle)
    install_pool_stub(oracle)
    import yaml
    from pcdet.config import cfg as ref_cfg
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/kitti_models/PartA2.yaml')))
    model_cfg, class_names = EasyDict(y['MODEL']), y['CLASS_NAMES']
    model_cfg.ROI_HEAD.DP_RATIO = 0.0
    _, pcr_l, vs_l, n_feat, _, max_vox = PV_KINDS['kitti']
    ref_cfg.CLASS_NAMES, ref_cfg.MODEL = class_names, model_cfg
    from pcdet.models import build_network
    from pcdet.models.roi_heads.target_assigner.proposal_target_layer import ProposalTargetLayer
    pcr, vs = np.array(pcr_l, np.float32), np.array(vs_l, np.float32)
    grid = np.round((pcr[3:6] - pcr[0:3]) / vs).astype(np.int64)

    class Dataset:
        pass
    ds = Dataset()
    ds.class_names, ds.grid_size, ds.point_cloud_range, ds.voxel_size = class_names, grid, pcr, list(vs)
    ds.depth_downsample_factor = None
    ds.point_feature_encoder = EasyDict(num_point_features=n_feat)
    torch.manual_seed(0)
    model = build_network(model_cfg=model_cfg, num_class=3, dataset=ds)
    assert type(model).__name__ == 'PartA2Net'
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'UNetV2', 'HeightCompression', 'BaseBEVBackbone', 'AnchorHeadSingle',
                                                             'PointIntraPartOffsetHead', 'PartA2FCHead']
    out['keys'] = np.array(sorted(model.state_dict().keys()))
    out['shapes'] = np.array([str(tuple(v.shape)) for _, v in sorted(model.state_dict().items())])
    overrides = {}

    def reload():
        sd = pv_seeded_state(model)
        sd.update({k: torch.from_numpy(v) for k, v in overrides.items()})
        model.load_state_dict(sd)
    reload()
    model.train()
    pts, off, gt0 = mg.pvrcnn_detector_inputs('kitti')
    B = len(off) - 1
    voxels, coords, npts, _ = oracle.voxelize_batch(pts, off, pcr[:3], vs, grid, max_vox, 5)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))

    def make_batch(gt):
        return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)), 'voxels': torch.from_numpy(voxels.copy()),
                'voxel_coords': torch.from_numpy(coords.astype(np.float32)), 'voxel_num_points': torch.from_numpy(npts.astype(np.float32)),
                'gt_boxes': torch.from_numpy(gt.copy()), 'batch_size': B,
                'frame_id': np.array(['%06d' % (PV_FIRST_FRAME + i) for i in range(B)])}
    head, nms_cfg = model.roi_head, model.roi_head.model_cfg.NMS_CONFIG['TRAIN']

    # ReLU kinks of the first stage (train-mode BatchNorm: the forward pass does not read the ground truth)
    with torch.no_grad():
        bd0 = model.vfe(make_batch(gt0))
    kink = {'backbone_3d': settle_kinks(model.backbone_3d, lambda: model.backbone_3d(dict(bd0)), 'backbone_3d.', overrides)}
    with torch.no_grad():
        bd1 = model.map_to_bev_module(model.backbone_3d(dict(bd0)))
    kink['backbone_2d'] = settle_kinks(model.backbone_2d, lambda: model.backbone_2d(dict(bd1)), 'backbone_2d.', overrides)

    # pass 1: the proposals of the first stage; ground truth is an INPUT placed on some of them (as gen_pvrcnn_detector)
    with torch.no_grad():
        bd = model.dense_head(model.backbone_2d(dict(bd1)))
        bd = head.proposal_layer(bd, nms_config=nms_cfg)
    prop = {k: bd[k].detach().clone() for k in ('rois', 'roi_scores', 'roi_labels')}
    rng = np.random.default_rng(77)
    gt = np.zeros((B, 10, 8), np.float32)
    for b in range(B):
        k = 0
        for r, lab in zip(prop['rois'][b].numpy(), prop['roi_labels'][b].numpy()):
            ok = (r[3:6] > 0.3).all() and (r[3:6] < 8).all() and pcr[0] + 1 < r[0] < pcr[3] - 1 and pcr[1] + 1 < r[1] < pcr[4] - 1 and \
                pcr[2] + 0.5 < r[2] < pcr[5] - 0.5
            if ok and all(np.hypot(*(r[:2] - g[:2])) > 3.0 for g in gt[b, :k]):
                gt[b, k, :7] = r + np.concatenate([rng.uniform(-0.06, 0.06, 3), r[3:6] * rng.uniform(-0.04, 0.04, 3), rng.uniform(-0.04, 0.04, 1)])
                gt[b, k, 7] = lab
                k += 1
            if k == 8:
                break
        assert k >= 4, k
    out['gt'] = gt
    centres, o = _np(bd['point_coords'])[:, 1:4], int(model_cfg.ROI_HEAD.ROI_AWARE_POOL.POOL_SIZE)
    voff = np.searchsorted(_np(bd['point_coords'])[:, 0], np.arange(B + 1))

    # cell planes: the sampler seed whose RoIs keep the voxel centres farthest from faces and cell planes
    best = (-1.0, None)
    for seed in SEEDS:
        np.random.seed(seed); torch.manual_seed(seed)
        t = head.assign_targets({'batch_size': B, 'gt_boxes': torch.from_numpy(gt.copy()), **{k: v.clone() for k, v in prop.items()}})
        m = plane_margin(centres, voff, _np(t['rois']), o)
        if m > best[0]:
            best = (m, seed)
    plane, sampler_seed = best
    print('  sampler seed %d, plane margin %.3g' % (sampler_seed, plane))
    assert plane > PLANE_MARGIN
    out['sampler_seed'] = np.array([sampler_seed])

    sampled, captured, inter = [], {}, {}
    orig = ProposalTargetLayer.subsample_rois
    orig_pl, orig_pool = head.proposal_layer, head.roiaware_pool

    def recording(self, max_overlaps):
        idx = orig(self, max_overlaps)
        sampled.append(idx.clone())
        return idx

    def capture(bdict, nms_config):
        first = bdict.get('rois', None) is None
        bdict = orig_pl(bdict, nms_config=nms_config)
        if first:
            captured.update({k: bdict[k].detach().clone() for k in ('rois', 'roi_scores', 'roi_labels')})
        return bdict

    def pool_capture(bdict):
        for k in ('point_coords', 'point_features', 'point_cls_scores', 'point_part_offset', 'rois'):
            inter[k] = bdict[k].detach().clone()
        p = orig_pool(bdict)
        inter['coords'] = p[0].detach().sum(dim=-1).nonzero().int()
        return p
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

    # score mask: shift the class bias of the point head until no point inside a sampled RoI scores near the threshold
    thr = float(model_cfg.ROI_HEAD.SEG_MASK_SCORE_THRESH)
    for _ in range(200):
        reload()
        step(gt, False)
        case = pool_case(inter, _np(inter['rois']), model_cfg.ROI_HEAD)
        d = rc.pool_definition(case)
        used = np.unique(np.concatenate(d['kept']))
        mask_margin = float(np.abs(case['part'][used, 3] - thr).min())
        if mask_margin > MASK_MARGIN:
            break
        key = 'point_head.cls_layers.0.bias'
        overrides[key] = (overrides.get(key, _np(model.state_dict()[key])) + np.float32(1e-3)).astype(np.float32)
    else:
        raise AssertionError('score mask margin not met')

    # ReLU kinks of the RoI head on the step's own pooled rows (its input does not depend on its own BatchNorm biases)
    reload()
    state = {}
    orig_forward = head.forward

    def head_capture(bdict):
        state['bd'] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in bdict.items()}
        return orig_forward(bdict)
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
    kink['roi_head'] = settle_kinks(head, run_head, 'roi_head.', overrides)
    for k, v in overrides.items():
        out['bias/' + k] = v

    # the step
    reload()
    ret, tb, _ = step(gt, True)
    head.roiaware_pool, head.proposal_layer = orig_pool, orig_pl
    loss = ret['loss']
    model.zero_grad()
    loss.backward()
    assert len(sampled) == B
    for k in prop:
        assert torch.equal(captured[k], prop[k]), k
    fr = head.forward_ret_dict
    out['proposals'], out['proposal_scores'], out['proposal_labels'] = (_np(captured[k]) for k in ('rois', 'roi_scores', 'roi_labels'))
    out['sampled'] = np.stack([_np(s) for s in sampled]).astype(np.int64)
    out['rois'] = _np(fr['rois'])
    assert np.array_equal(out['rois'], np.take_along_axis(out['proposals'], out['sampled'][:, :, None], axis=1))
    out['point_coords'] = _np(inter['point_coords'])
    out['point_cls_scores'], out['point_part_offset'] = _np(inter['point_cls_scores']), _np(inter['point_part_offset'])
    out['coords'] = _np(inter['coords'])
    out['rcnn_cls'], out['rcnn_reg'] = _np(fr['rcnn_cls']), _np(fr['rcnn_reg'])
    out['loss'] = np.array([float(loss.detach())])
    out['tb_keys'] = np.array(sorted(tb.keys()))
    out['tb_vals'] = np.array([float(tb[k]) for k in sorted(tb.keys())], np.float64)
    params = dict(model.named_parameters())
    for n, sl in PA2_GRADS.items():
        out['grad/' + n] = _np(params[n].grad)[sl].copy()
        out['gradmax/' + n] = np.array([float(params[n].grad.abs().max())])
        assert np.abs(out['grad/' + n]).max() > 0, n

    # margins of the final step
    case = pool_case(inter, out['rois'], model_cfg.ROI_HEAD)
    d = rc.pool_definition(case)
    assert np.array_equal(d['coords'], out['coords'])                 # the numpy definition gives the reference's rows
    used = np.unique(np.concatenate(d['kept']))
    mask_margin = float(np.abs(case['part'][used, 3] - thr).min())
    tie = np.inf
    for kept in d['kept']:
        if len(kept) > 1:
            f = np.sort(case['feat'][kept].astype(np.float64), axis=0)
            gap, top = f[-1] - f[-2], f[-1]
            live = ~((top == 0) & (f[-2] == 0))
            if live.any():
                tie = min(tie, float(gap[live].min()))
    plane = plane_margin(case['pts'], case['off'], out['rois'], o)
    out['margins'] = np.array([min(kink.values()), mask_margin, tie, plane])
    print('  margins: kinks %s, score mask %.3g, max ties %.3g, cell planes %.3g' % (kink, mask_margin, tie, plane))
    assert min(kink.values()) > KINK and mask_margin > MASK_MARGIN and tie > TIE_MARGIN and plane > PLANE_MARGIN
    print('  loss %.5f' % float(loss), {k: round(float(v), 5) for k, v in tb.items()})
    print('  voxels %d, rows %d, fg rois %d' % (len(coords), len(out['coords']), int((_np(fr['rcnn_cls_labels']) > 0.5).sum())))
    assert np.isfinite(out['loss']).all()
    # the parameter / buffer names and shapes of the yaml as it stands (DP_RATIO 0.3: the dropout layers move the indices of the FC stacks)
    model_cfg.ROI_HEAD.DP_RATIO = float(y['MODEL']['ROI_HEAD']['DP_RATIO'])
    full = build_network(model_cfg=model_cfg, num_class=3, dataset=ds)
    out['keys_yaml'] = np.array(sorted(full.state_dict().keys()))
    out['shapes_yaml'] = np.array([str(tuple(v.shape)) for _, v in sorted(full.state_dict().items())])
    assert len(out['keys_yaml']) == len(out['keys']) and list(out['keys_yaml']) != list(out['keys'])


if __name__ == '__main__':
    mg.import_reference()
    d = {}
    gen(d)
    mg.save('ref_parta2_net.npz', d)
