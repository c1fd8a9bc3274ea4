"""Generate ref_spc.npz and ref_pvrcnn_plusplus.npz from the reference's own SPC sampling and PVRCNNPlusPlus (companion of
make_goldens.py, whose import recipe and detector helpers it reuses).

Runs ONLY where the reference tree is mounted; the .npz files it writes are committed and are the only thing that travels.
Usage:  python tests/golden/make_goldens_spc.py [ref_spc.npz] [ref_pvrcnn_plusplus.npz]

The reference's compiled stack_farthest_point_sampling_wrapper is answered by stack_fps_kernel below: its kernel thread by thread in
numpy (tests/spc_cases.py:fps_tree: 1024 strided threads, the LDS tree, global indices), checked here against the total-order
restatement the tests use (fps_order).

ref_spc.npz, for the frame cases of tests/spc_cases.py (seeds 0, 1) and (K, S) in (64, 6), (7, 6), (64, 1), (7, 1):
  * the inputs (points, counts, rois) as generated, so that the tests notice a generator that drifted
  * per frame sample_points_with_roi's mask; per frame sector_fps's segment lengths and quotas as its FPS call received them;
    VoxelSetAbstraction.get_sampled_points' keypoints (sum M_b, 4) through the reference's own class
  * the quota case's quotas, and the picks of every FPS case
ref_pvrcnn_plusplus.npz: one training step of the reference's PVRCNNPlusPlus on the reduced KITTI configuration of
ref_pvrcnn_detector.npz (same two frames, seeded weights, 256 keypoints, no dropout) with the PFE section of pv_rcnn_plusplus.yaml
(SPC, 6 sectors, 1.6 m; bev / x_conv3 / x_conv4 / raw_points; RoI-filtered neighbours 2.4 / 4.0 / 6.4 m) on StackSAModuleMSG layers:
first-stage proposals with scores and labels, the recorded RoI sampler indices, the sampled rois, point_coords, loss, every tb_dict
entry, the second-stage outputs and the gradients of pv_grads('waymo') (the two-voxel-source naming). The sampler seed is the first
one whose sampled rois keep every real point of the two frames outside the margins of tests/spc_cases.py."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_goldens as mg                                                    # noqa: E402
from make_goldens import import_reference, save, _np, EasyDict              # noqa: E402
from _constants import PV_FIRST_FRAME, PV_KEYPOINTS, PV_KINDS, pv_grads, pv_seeded_state   # noqa: E402
import spc_cases as cases                                                    # noqa: E402

KS = ((64, 6), (7, 6), (64, 1), (7, 1))
SEEDS = (0, 1)
fps_calls = []


def stack_fps_kernel(xyz, temp, xyz_batch_cnt, output, npoint):
    """pointnet2_stack_cuda.stack_farthest_point_sampling_wrapper"""
    cnt, m = [int(v) for v in xyz_batch_cnt], [int(v) for v in npoint]
    assert all(a <= b for a, b in zip(m, cnt)), 'the reference kernel reads out of range when m > n'
    assert float(temp.min()) == 1e10
    idx = cases.fps_tree(xyz.numpy(), cnt, m)
    assert np.array_equal(idx, cases.fps_order(xyz.numpy(), cnt, m))
    fps_calls.append((cnt, m))
    output.copy_(torch.from_numpy(idx.astype(np.int32)))


def install_stack_fps():
    sys.modules['pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda'].stack_farthest_point_sampling_wrapper = stack_fps_kernel
    torch.cuda.IntTensor = torch.IntTensor
    torch.cuda.FloatTensor = torch.FloatTensor


def spc_pfe_cfg(K, S):
    return EasyDict({'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': K, 'NUM_OUTPUT_FEATURES': 8,
                     'SAMPLE_METHOD': 'SPC', 'SPC_SAMPLING': {'NUM_SECTORS': S, 'SAMPLE_RADIUS_WITH_ROI': cases.RADIUS},
                     'FEATURES_SOURCE': ['raw_points'],
                     'SA_LAYER': {'raw_points': {'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]}}})


def gen_spc(out):
    install_stack_fps()
    from pcdet.models.backbones_3d.pfe import voxel_set_abstraction as ref
    for seed in SEEDS:
        c = cases.frame_case(seed)
        pre = 'case%d/' % seed
        out[pre + 'points'], out[pre + 'counts'], out[pre + 'rois'] = c['points'], np.array(c['counts']), c['rois']
        out[pre + 'special'] = c['special']
        bidx = np.repeat(np.arange(len(c['counts']), dtype=np.float32), c['counts'])
        points = torch.from_numpy(np.concatenate([bidx[:, None], c['points'], np.zeros((len(bidx), 1), np.float32)], 1))
        rois = torch.from_numpy(c['rois'])
        masks, s = [], 0
        for b, n in enumerate(c['counts']):
            # (a part size below the frame length: the reference's chunked branch, which changes no value)
            kept, mask = ref.sample_points_with_roi(rois[b], points[s:s + n, 1:4], c['radius'], 700)
            assert len(kept) == max(int(mask.sum()), 1)
            masks.append(_np(mask))
            s += n
        out[pre + 'mask'] = np.concatenate(masks)
        for K, S in KS:
            pfe = ref.VoxelSetAbstraction(spc_pfe_cfg(K, S), [0.05, 0.05, 0.1], [-70.4, -70.4, -3, 70.4, 70.4, 1], num_rawpoint_features=4)
            del fps_calls[:]
            kp = pfe.get_sampled_points({'batch_size': len(c['counts']), 'points': points, 'rois': rois})
            assert len(fps_calls) == len(c['counts'])
            key = pre + 'K%d_S%d/' % (K, S)
            out[key + 'keypoints'] = _np(kp)
            out[key + 'seg_frame'] = np.concatenate([[b] * len(cnt) for b, (cnt, _) in enumerate(fps_calls)])
            out[key + 'seg_n'] = np.concatenate([cnt for cnt, _ in fps_calls])
            out[key + 'seg_m'] = np.concatenate([m for _, m in fps_calls])
            print('  case %d K %d S %d: %d keypoints in %d segments' % (seed, K, S, len(kp), len(out[key + 'seg_n'])))
    q = cases.quota_case()
    del fps_calls[:]
    ref.sector_fps(torch.from_numpy(q['points']), q['K'], q['S'])
    out['quota/points'], out['quota/seg_m'] = q['points'], np.array(fps_calls[0][1])
    assert out['quota/seg_m'].tolist() == q['quotas']
    for name, (xyz, cnt, m) in cases.fps_cases().items():
        out['fps/' + name] = cases.fps_tree(xyz, cnt, m)


def plusplus_model_cfg():
    """the reduced KITTI configuration of ref_pvrcnn_detector.npz with the PFE section of pv_rcnn_plusplus.yaml on StackSAModuleMSG
    layers (what pcdet.model_cfgs.pv_rcnn_plusplus_cfg('kitti') builds in the port)"""
    m, names = mg.pvrcnn_model_cfg('kitti')
    m.NAME = 'PVRCNNPlusPlus'
    m.PFE.SAMPLE_METHOD = 'SPC'
    m.PFE.SPC_SAMPLING = EasyDict({'NUM_SECTORS': 6, 'SAMPLE_RADIUS_WITH_ROI': 1.6})
    m.PFE.NUM_OUTPUT_FEATURES = 90
    m.PFE.FEATURES_SOURCE = ['bev', 'x_conv3', 'x_conv4', 'raw_points']
    for src, radius in (('raw_points', 2.4), ('x_conv3', 4.0), ('x_conv4', 6.4)):
        m.PFE.SA_LAYER[src].update({'FILTER_NEIGHBOR_WITH_ROI': True, 'RADIUS_OF_NEIGHBOR_WITH_ROI': radius})
    m.ROI_HEAD.NMS_CONFIG.TEST.update({'NMS_POST_MAXSIZE': 100, 'SCORE_THRESH': 0.1})
    return m, names


def margins_hold(points, off, rois):
    for b in range(len(off) - 1):
        p = points[off[b]:off[b + 1], :3]
        _, _, slack, gap = cases.mask_f64(p, rois[b], 1.6)
        if not ((slack > 1e-4).all() and (gap > 1e-4).all() and (cases.sector_f64(p, 6)[1] > 1e-5).all()):
            return False
    return True


def gen_pvrcnn_plusplus(out):
    oracle = mg._install_cpu_ops()
    mg._install_pointnet2_ops(oracle)
    install_stack_fps()
    mg._install_spconv_oracle(oracle)
    from pcdet.config import cfg as ref_cfg
    model_cfg, class_names = plusplus_model_cfg()
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
    assert type(model).__name__ == 'PVRCNNPlusPlus'
    model.load_state_dict(pv_seeded_state(model))
    model.train()
    out['pv_keys'] = np.array(sorted(model.state_dict().keys()))
    pts, off, gt0 = mg.pvrcnn_detector_inputs('kitti')
    B = len(off) - 1
    voxels, coords, npts, _ = oracle.voxelize_batch(pts, off, pcr[:3], vs, grid, max_vox, 5)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))

    def make_batch(gt):
        return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)), 'voxels': torch.from_numpy(voxels.copy()),
                'voxel_coords': torch.from_numpy(coords.astype(np.float32)), 'voxel_num_points': torch.from_numpy(npts.astype(np.float32)),
                'gt_boxes': torch.from_numpy(gt.copy()), 'batch_size': B,
                'frame_id': np.array(['%06d' % (PV_FIRST_FRAME + i) for i in range(B)])}
    # pass 1 (no gradients, eval-free: train mode as the step itself): the proposals of the randomly initialised first stage.
    # Ground truth is an INPUT placed on some of those proposals, as in make_goldens.gen_pvrcnn_detector.
    head = model.roi_head
    nms_cfg = head.model_cfg.NMS_CONFIG['TRAIN']
    with torch.no_grad():
        bd = make_batch(gt0)
        for mod in (model.vfe, model.backbone_3d, model.map_to_bev_module, model.backbone_2d, model.dense_head):
            bd = mod(bd)
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
    out['pv_gt'] = gt
    # the sampler seed: the first whose sampled rois keep every real point of the frames outside the margins
    for sampler_seed in range(5, 40):
        np.random.seed(sampler_seed)
        torch.manual_seed(sampler_seed)
        t = head.assign_targets({'batch_size': B, 'gt_boxes': torch.from_numpy(gt.copy()), **{k: v.clone() for k, v in prop.items()}})
        if margins_hold(pts, off, _np(t['rois'])):
            break
    else:
        raise AssertionError('no sampler seed keeps the points outside the margins')
    print('  sampler seed', sampler_seed)
    out['pv_sampler_seed'] = np.array([sampler_seed])
    model.load_state_dict(pv_seeded_state(model))        # (pass 1 advanced the running statistics)
    batch = make_batch(gt)
    sampled, captured, inter = [], {}, {}
    orig = ProposalTargetLayer.subsample_rois
    orig_pl, orig_pool = head.proposal_layer, head.roi_grid_pool

    def recording(self, max_overlaps):
        idx = orig(self, max_overlaps)
        sampled.append(idx.clone())
        return idx

    def capture(bd, nms_config):
        first = bd.get('rois', None) is None                # (the RoI head calls it again and returns early: rois exist)
        bd = orig_pl(bd, nms_config=nms_config)
        if first:
            captured.update({k: bd[k].detach().clone() for k in ('rois', 'roi_scores', 'roi_labels')})
        return bd

    def pool_capture(bd):
        inter['point_coords'] = bd['point_coords'].detach().clone()
        inter['point_features'] = bd['point_features'].detach().clone()
        inter['point_cls_scores'] = bd['point_cls_scores'].detach().clone()
        return orig_pool(bd)
    ProposalTargetLayer.subsample_rois = recording
    head.roi_grid_pool, head.proposal_layer = pool_capture, capture
    np.random.seed(sampler_seed)
    torch.manual_seed(sampler_seed)
    del fps_calls[:]
    try:
        ret, tb, _ = model(batch)
    finally:
        ProposalTargetLayer.subsample_rois = orig
        head.roi_grid_pool, head.proposal_layer = orig_pool, orig_pl
    assert len(sampled) == B and len(fps_calls) == B
    for k in prop:
        assert torch.equal(captured[k], prop[k]), k          # (the step's first stage = pass 1's: train-mode BatchNorm reads the batch)
    out['pv_proposals'], out['pv_proposal_scores'], out['pv_proposal_labels'] = (_np(captured[k]) for k in ('rois', 'roi_scores', 'roi_labels'))
    out['pv_sampled'] = np.stack([_np(s) for s in sampled]).astype(np.int64)
    out['pv_rois'] = _np(head.forward_ret_dict['rois'])
    assert margins_hold(pts, off, out['pv_rois'])
    assert np.array_equal(out['pv_rois'], np.take_along_axis(out['pv_proposals'], out['pv_sampled'][:, :, None], axis=1))
    out['pv_point_coords'] = _np(inter['point_coords'])
    out['pv_point_features'] = _np(inter['point_features'])[:, :32].copy()
    out['pv_point_cls_scores'] = _np(inter['point_cls_scores'])
    out['pv_seg_n'] = np.concatenate([cnt for cnt, _ in fps_calls])
    out['pv_seg_m'] = np.concatenate([m for _, m in fps_calls])
    loss = ret['loss']
    model.zero_grad()
    loss.backward()
    out['pv_loss'] = np.array([float(loss.detach())])
    out['pv_tb_keys'] = np.array(sorted(tb.keys()))
    out['pv_tb_vals'] = np.array([float(tb[k]) for k in sorted(tb.keys())], np.float64)
    fr = head.forward_ret_dict
    out['pv_rcnn_cls'], out['pv_rcnn_reg'] = _np(fr['rcnn_cls']), _np(fr['rcnn_reg'])
    out['pv_rcnn_cls_gt'], out['pv_rcnn_reg_gt'] = _np(fr['rcnn_cls_labels']), _np(fr['rcnn_reg_gt'])     # (what PVRCNN's step returns)
    params = dict(model.named_parameters())
    for n, sl in pv_grads('waymo').items():
        out['pv_grad/' + n] = _np(params[n].grad)[sl].copy()
        out['pv_gradmax/' + n] = np.array([float(params[n].grad.abs().max())])
    print('  loss %.5f' % float(loss), {k: round(float(v), 5) for k, v in tb.items()})
    print('  keypoints', out['pv_point_coords'].shape, 'per frame', np.bincount(out['pv_point_coords'][:, 0].astype(int)).tolist(),
          'segments', out['pv_seg_n'].tolist(), out['pv_seg_m'].tolist(), 'fg rois', int((out['pv_rcnn_cls_gt'] > 0.5).sum()))
    assert np.isfinite(out['pv_loss']).all() and all(np.abs(out['pv_grad/' + n]).max() > 0 for n in pv_grads('waymo'))


if __name__ == '__main__':
    import_reference()
    only = sys.argv[1:]
    for name, fn in (('ref_spc.npz', gen_spc), ('ref_pvrcnn_plusplus.npz', gen_pvrcnn_plusplus)):
        if only and name not in only:
            continue
        d = {}
        fn(d)
        save(name, d)
