"""Golden vectors of SECOND-IoU (tests/golden/ref_second_iou.npz) from the reference's own SECONDHead and SECONDNetIoU.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_second_iou.py [pool] [head] [detector]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, feeds the seeded
inputs of tests/second_iou_cases.py, and stores inputs + outputs. A part that is not named keeps what the existing file holds."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import second_iou_cases as cases               # noqa: E402
from _constants import EasyDict, seeded_state, pv_seeded_state, PV_KINDS   # noqa: E402

_np = mg._np


def _ref_head(dp_ratio, iou_loss='BinaryCrossEntropy'):
    from pcdet.models.roi_heads.second_head import SECONDHead
    torch.manual_seed(3)
    head = SECONDHead(input_channels=cases.POOL_C, model_cfg=EasyDict(cases.head_cfg(dp_ratio, iou_loss)), num_class=1)
    head.load_state_dict(seeded_state(head, cases.HEAD_SEED))
    return head


def _pool_batch(bev, rois):
    return {'batch_size': bev.shape[0], 'rois': torch.from_numpy(rois),
            'spatial_features_2d': torch.from_numpy(bev).permute(0, 3, 1, 2).contiguous(),
            'dataset_cfg': EasyDict(cases.dataset_cfg_dict())}


def gen_pool(out):
    """the reference's roi_grid_pool on the constructed RoIs, G = 7 and G = 4, next to the f64 definition and the reference's own
    f32 error against it (e_ref: the yardstick of the kernel's bound)"""
    bev, rois, extra = cases.pool_case_inputs()
    out['pool_bev'], out['pool_rois'], out['pool_rois_extra'] = bev, rois, extra
    geo = cases.pool_geometry()
    for G in cases.POOL_GRIDS:
        head = _ref_head(0.0)
        head.model_cfg.ROI_GRID_POOL.GRID_SIZE = G
        ref = _np(head.roi_grid_pool(_pool_batch(bev, rois)))
        ref9 = _np(head.roi_grid_pool(_pool_batch(bev, np.concatenate([rois, extra], -1))))
        assert np.array_equal(ref, ref9)                     # the extra RoI columns are not read
        f64 = cases.pool_f64(bev, rois, G, *geo)
        e_ref = float(np.abs(ref.astype(np.float64) - f64).max())
        out['pool_ref_g%d' % G], out['pool_f64_g%d' % G], out['pool_e_ref_g%d' % G] = ref, f64, np.array([e_ref])
        R = cases.POOL_R
        for b in range(cases.POOL_B):
            assert np.all(ref[b * R + cases.ROW_OUTSIDE] == 0) and np.abs(ref[b * R + cases.ROW_PADDING]).max() > 1e-2
            assert all(np.all(ref[b * R + r] != 0) for r in range(5))          # fully inside: no zero-padded sample
        print('  pool G=%d: e_ref %.3g on outputs up to %.3g' % (G, e_ref, np.abs(ref).max()))


def gen_head(out):
    """SECONDHead at IN_CHANNEL 8: state_dict keys and shapes, the eval logits for DP_RATIO 0 and 0.3, one training step with the
    sampler's picks injected: logits, the loss of each kind, gradients under BinaryCrossEntropy"""
    bev, rois, _ = cases.pool_case_inputs()
    for dp, tag in ((0.0, 'dp0'), (0.3, 'dp3')):
        head = _ref_head(dp)
        sd = head.state_dict()
        out['head_keys_' + tag] = np.array(list(sd.keys()))
        out['head_shapes_' + tag] = np.array([','.join(str(v) for v in t.shape) for t in sd.values()])
        head.eval()
        with torch.no_grad():
            bd = head(_pool_batch(bev, rois))
        out['head_eval_' + tag] = _np(bd['batch_cls_preds'])
        assert bd['cls_preds_normalized'] is False and bd['batch_box_preds'] is bd['rois']
    s_rois, s_gt, s_iou, s_scores, s_labels = cases.head_sample()
    for kind in cases.LOSS_KINDS:
        head = _ref_head(0.0, kind)
        head.train()
        head.proposal_target_layer.sample_rois_for_rcnn = lambda batch_dict: tuple(
            torch.from_numpy(a.copy()) for a in (s_rois, s_gt, s_iou, s_scores, s_labels))
        bd = _pool_batch(bev, rois)
        bd['gt_boxes'] = torch.from_numpy(s_gt)
        head(bd)
        loss, tb = head.get_loss()
        out['head_loss_' + kind] = np.array([float(loss.detach()), tb['rcnn_loss_iou'], tb['rcnn_loss']])
        if kind == 'BinaryCrossEntropy':
            head.zero_grad()
            loss.backward()
            out['head_rcnn_iou'] = _np(head.forward_ret_dict['rcnn_iou'])
            out['head_labels'] = _np(head.forward_ret_dict['rcnn_cls_labels'])
            for n, p in head.named_parameters():
                if n == 'shared_fc_layer.0.weight' or n.startswith('iou_layers.'):
                    out['head_grad/' + n] = _np(p.grad)
        print('  head %s: loss %.6f' % (kind, float(loss)))


def gen_detector(out):
    """the reference's SECONDNetIoU built from kitti_models/second_iou.yaml (DP_RATIO 0: train-mode dropout draws are not
    reproducible across implementations), run the way make_goldens.gen_pvrcnn_detector runs PVRCNN: spconv answered by the oracle,
    weights seeded by parameter name, two synthetic frames, ground truth placed on first-stage proposals, the sampler's picks
    recorded. One training step (loss, tb_dict, gradient slices) and one eval pass (frame 0's pred dict for two score types)."""
    import yaml
    oracle = mg._install_cpu_ops()
    mg._install_spconv_oracle(oracle)
    from pcdet.config import cfg as ref_cfg
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/kitti_models/second_iou.yaml')))
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
    ds.dataset_cfg = EasyDict({'POINT_CLOUD_RANGE': list(pcr_l), 'DATA_PROCESSOR': [{'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': list(vs_l)}]})
    torch.manual_seed(0)
    model = build_network(model_cfg=model_cfg, num_class=3, dataset=ds)
    model.load_state_dict(pv_seeded_state(model))
    model.train()
    sd = model.state_dict()
    out['det_keys'] = np.array(sorted(sd.keys()))
    out['det_shapes'] = np.array([','.join(str(v) for v in sd[k].shape) for k in sorted(sd.keys())])

    import importlib.util                       # by path: the name `pcdet` is the reference's package in this process
    spec = importlib.util.spec_from_file_location(
        'crb_synthetic', os.path.join(os.path.dirname(os.path.dirname(HERE)), 'crb-active-3ddet_amd', 'pcdet', 'datasets', 'synthetic.py'))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    pts, off, gt0 = syn.kitti_batch(cases.DET_FIRST_FRAME, 2, cases.DET_POINTS)
    B = len(off) - 1
    voxels, coords, npts, _ = oracle.voxelize_batch(pts, off, pcr[:3], vs, grid, max_vox, 5)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))

    def make_batch(gt):
        return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)), 'voxels': torch.from_numpy(voxels.copy()),
                'voxel_coords': torch.from_numpy(coords.astype(np.float32)), 'voxel_num_points': torch.from_numpy(npts.astype(np.float32)),
                'gt_boxes': torch.from_numpy(gt.copy()), 'batch_size': B,
                'frame_id': np.array(['%06d' % (cases.DET_FIRST_FRAME + i) for i in range(B)])}
    captured = {}
    orig_pl = model.roi_head.proposal_layer

    def capture(bd, nms_config):
        bd = orig_pl(bd, nms_config=nms_config)
        captured['rois'], captured['labels'] = bd['rois'].detach().clone(), bd['roi_labels'].detach().clone()
        captured['scores'] = bd['roi_scores'].detach().clone()
        return bd
    model.roi_head.proposal_layer = capture
    np.random.seed(5); torch.manual_seed(5)
    with torch.no_grad():
        model(make_batch(gt0))
    rng = np.random.default_rng(77)
    gt = np.zeros((B, 10, 8), np.float32)
    for b in range(B):
        k = 0
        for r, lab in zip(captured['rois'][b].numpy(), captured['labels'][b].numpy()):
            ok = (r[3:6] > 0.3).all() and (r[3:6] < 8).all() and pcr[0] + 1 < r[0] < pcr[3] - 1 and pcr[1] + 1 < r[1] < pcr[4] - 1 and \
                pcr[2] + 0.5 < r[2] < pcr[5] - 0.5
            if ok and all(np.hypot(*(r[:2] - g[:2])) > 3.0 for g in gt[b, :k]):
                gt[b, k, :7] = r + np.concatenate([rng.uniform(-0.06, 0.06, 3), r[3:6] * rng.uniform(-0.04, 0.04, 3), rng.uniform(-0.04, 0.04, 1)])
                gt[b, k, 7] = lab
                k += 1
            if k == 8:
                break
        assert k >= 4, k
    out['det_gt'] = gt
    model.load_state_dict(pv_seeded_state(model))        # (pass 1 advanced the running statistics)
    sampled = []
    orig = ProposalTargetLayer.subsample_rois

    def recording(self, max_overlaps):
        idx = orig(self, max_overlaps)
        sampled.append(idx.clone())
        return idx
    ProposalTargetLayer.subsample_rois = recording
    inter = {}
    orig_pool = model.roi_head.roi_grid_pool

    def pool_capture(bd):
        p = orig_pool(bd)
        inter['pooled'] = p.detach().clone()
        return p
    model.roi_head.roi_grid_pool = pool_capture
    np.random.seed(5); torch.manual_seed(5)
    try:
        ret, tb, _ = model(make_batch(gt))
    finally:
        ProposalTargetLayer.subsample_rois = orig
        model.roi_head.roi_grid_pool = orig_pool
    out['det_proposals'], out['det_proposal_labels'] = _np(captured['rois']), _np(captured['labels'])
    out['det_pooled'] = _np(inter['pooled'])[cases.DET_POOLED].copy()           # (64 of 256 RoIs, 8 of 512 channels, 7, 7)
    loss = ret['loss']
    model.zero_grad()
    loss.backward()
    out['det_loss'] = np.array([float(loss.detach())])
    out['det_tb_keys'] = np.array(sorted(tb.keys()))
    out['det_tb_vals'] = np.array([float(tb[k]) for k in sorted(tb.keys())], np.float64)
    out['det_sampled'] = np.stack([_np(s) for s in sampled]).astype(np.int64)
    frd = model.roi_head.forward_ret_dict
    out['det_rcnn_iou'], out['det_rcnn_labels'], out['det_rois'] = _np(frd['rcnn_iou']), _np(frd['rcnn_cls_labels']), _np(frd['rois'])
    params = dict(model.named_parameters())
    for n, sl in cases.DET_GRADS.items():
        out['det_grad/' + n] = _np(params[n].grad)[sl].copy()
        out['det_gradmax/' + n] = np.array([float(params[n].grad.abs().max())])
    print('  loss %.5f' % float(loss), {k: round(float(v), 5) for k, v in tb.items()})
    print('  voxels', len(coords), 'sampled', out['det_sampled'].shape, 'soft labels > 0.5:', int((out['det_rcnn_labels'] > 0.5).sum()))
    assert np.isfinite(out['det_loss']).all() and all(np.abs(out['det_grad/' + n]).max() > 0 for n in cases.DET_GRADS)
    # ---- eval pass on the seeded state
    model.load_state_dict(pv_seeded_state(model))
    model.eval()
    held = {}
    orig_pp = model.post_processing

    def pp(bd):
        held['bd'] = bd
        return orig_pp(bd)
    model.post_processing = pp
    with torch.no_grad():
        pred, recall = model(make_batch(gt))
        bd = held['bd']
        out['ev_rois'], out['ev_iou_logits'] = _np(bd['batch_box_preds']), _np(bd['batch_cls_preds'])
        out['ev_roi_scores'], out['ev_roi_labels'] = _np(bd['roi_scores']), _np(bd['roi_labels'])
        out['ev_recall_keys'] = np.array(sorted(recall.keys()))
        out['ev_recall_vals'] = np.array([recall[k] for k in sorted(recall.keys())], np.int64)
        model_cfg.POST_PROCESSING.NMS_CONFIG.SCORE_TYPE = 'weighted_iou_cls'
        model_cfg.POST_PROCESSING.NMS_CONFIG.SCORE_WEIGHTS = EasyDict(cases.DET_SCORE_WEIGHTS)
        pred_w, _ = orig_pp(bd)
    for tag, p in (('iou', pred), ('weighted', pred_w)):
        for key in ('pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores'):
            out['ev_%s_%s' % (tag, key)] = _np(p[0][key])
        out['ev_%s_counts' % tag] = np.array([len(d['pred_scores']) for d in p], np.int64)
        print('  eval %s: boxes per frame' % tag, out['ev_%s_counts' % tag])
        assert out['ev_%s_counts' % tag][0] >= 3


if __name__ == '__main__':
    mg.import_reference()
    parts = {'pool': gen_pool, 'head': gen_head, 'detector': gen_detector}
    only = sys.argv[1:] or list(parts)
    prefix = {'pool': ('pool_',), 'head': ('head_',), 'detector': ('det_', 'ev_')}
    d = {}
    if os.path.exists(cases.GOLDEN):
        old = np.load(cases.GOLDEN)
        d = {k: old[k] for k in old.files if not any(k.startswith(p) for n in only for p in prefix[n])}
    for name in only:
        print(name)
        parts[name](d)
    np.savez_compressed(cases.GOLDEN, **d)
    print(os.path.basename(cases.GOLDEN), '%.1f KB' % (os.path.getsize(cases.GOLDEN) / 1024))
