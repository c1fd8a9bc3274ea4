"""Golden vectors of Voxel R-CNN (tests/golden/ref_voxel_rcnn.npz) from the reference's own NeighborVoxelSAModuleMSG and VoxelRCNNHead.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_voxel_rcnn.py [module] [head]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, answers
pointnet2_stack_cuda.voxel_query_wrapper / group_points_wrapper / group_points_grad_wrapper and the spconv tensor (indices,
features, spatial_shape, batch_size) with the restatement of tests/voxel_rcnn_cases.py, feeds the seeded inputs and stores
outputs. A part that is not named keeps what the existing file holds."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import voxel_rcnn_cases as cases               # noqa: E402
from _constants import EasyDict, seeded_state  # noqa: E402

_np = mg._np
# margins of the recorded pre-activation values (f64): a maximum closer than this to the runner-up of another row, or to the ReLU's
# kink, could be decided differently by two correct f32 evaluations, and the gradient would then move by a whole entry
GAP_MAX, GAP_RELU_MAX, GAP_RELU_AVG = 1e-5, 1e-5, 1e-6


class SparseLevel:
    def __init__(self, coords, feats, shape, batch_size):
        self.indices, self.features, self.spatial_shape, self.batch_size = coords, feats, list(shape), batch_size


def install_ops():
    m = sys.modules['pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda']

    def voxel_query_wrapper(M, Z, Y, X, nsample, radius, rz, ry, rx, new_xyz, xyz, new_coords, point_indices, idx):
        got, empty = cases.voxel_query_np([rz, ry, rx], radius, nsample, xyz.detach().float().numpy(), new_xyz.detach().float().numpy(),
                                          new_coords.numpy(), point_indices.numpy())
        got[empty, 0] = -1                                   # what the kernel leaves for an empty ball
        idx.copy_(torch.from_numpy(got))

    def _rows(idx, feat_cnt, idx_cnt):
        off = torch.repeat_interleave(torch.cumsum(feat_cnt.long(), 0) - feat_cnt.long(), idx_cnt.long())
        return idx.long() + off[:, None]

    def group_points_wrapper(B, M, C, nsample, feat, feat_cnt, idx, idx_cnt, out):
        out.copy_(feat.detach()[_rows(idx, feat_cnt, idx_cnt)].permute(0, 2, 1))

    def group_points_grad_wrapper(B, M, C, N, nsample, grad_out, idx, idx_cnt, feat_cnt, grad_feat):
        rows = _rows(idx, feat_cnt, idx_cnt).reshape(-1)
        grad_feat.index_add_(0, rows, grad_out.permute(0, 2, 1).reshape(-1, C))
    m.voxel_query_wrapper, m.group_points_wrapper, m.group_points_grad_wrapper = voxel_query_wrapper, group_points_wrapper, group_points_grad_wrapper
    torch.cuda.IntTensor = torch.IntTensor
    torch.cuda.FloatTensor = torch.FloatTensor
    from pcdet.utils import common_utils
    # the reference's dense index (its scatter indexes with a list of tensors, which torch 2 rejects) answered by the restatement
    common_utils.generate_voxel2pinds = lambda sp: torch.from_numpy(cases.dense_index(sp.indices.numpy(), sp.spatial_shape, sp.batch_size))


class as_f64:
    """the reference allocates its grouped tensors as torch.cuda.FloatTensor: the f64 run answers that with DoubleTensor"""
    def __enter__(self):
        torch.cuda.FloatTensor = torch.DoubleTensor

    def __exit__(self, *a):
        torch.cuda.FloatTensor = torch.FloatTensor


def _ref_module(p, pool):
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    mod = NeighborVoxelSAModuleMSG(query_ranges=[p['ranges']], radii=[p['radius']], nsamples=[p['nsample']],
                                   mlps=[[p['c_in'], p['c'], p['c_out']]], pool_method=pool)
    mod.load_state_dict(seeded_state(mod, cases.MODULE_SEED))
    return mod


def _run_module(mod, p, q, dtype, training):
    xyz, new_xyz, new_coords = q
    mod = mod.to(dtype).train(training)
    G = p['grid']
    cap = {}
    h1 = mod.mlps_in[0].register_forward_hook(lambda m, i, o: cap.__setitem__('features_in', o.detach()[0].t().clone()))
    h2 = mod.mlps_out[0].register_forward_pre_hook(lambda m, i: cap.__setitem__('pooled', i[0].detach()[0].t().clone()))
    feats = torch.from_numpy(p['feats']).to(dtype).requires_grad_(True)
    cnt = torch.from_numpy(np.bincount(p['coords'][:, 0], minlength=cases.B).astype(np.int32))
    new_cnt = torch.full((cases.B,), cases.R * G ** 3, dtype=torch.int32)
    bxyz = torch.from_numpy(new_coords[:, [0, 3, 2, 1]].copy())                       # the module's input order [b, x, y, z]
    out = mod(xyz=torch.from_numpy(xyz).to(dtype), xyz_batch_cnt=cnt, new_xyz=torch.from_numpy(new_xyz).to(dtype),
              new_xyz_batch_cnt=new_cnt, new_coords=bxyz, features=feats,
              voxel2point_indices=torch.from_numpy(cases.dense_index(p['coords'])))
    h1.remove(); h2.remove()
    res = {'out': out.detach(), 'features_in': cap['features_in'], 'pooled': cap['pooled']}
    wout = torch.from_numpy(np.random.default_rng(p['seed'] + 9).normal(0, 1, tuple(out.shape))).to(dtype)
    mod.zero_grad()
    ((out * wout).sum() / out.shape[0]).backward()       # eval mode too: the frozen-BatchNorm fine-tuning path
    res['grad/features'] = feats.grad.detach()
    for n, t in mod.named_parameters():
        res['grad/' + n] = t.grad.detach()
    if training:
        for n, t in mod.named_buffers():
            res['buf/' + n] = t.detach().clone()
    return res


def gen_module(out):
    """per level case, pool method and mode: the reference module in f32 and in f64 on the restated query, e_ref = the reference's f32
    error against the f64 pooling definition (on the f32 run's own features_in) and against its own f64 run (outputs, gradients;
    large arrays are stored as every fourth row, cases.ROWS)"""
    for name in cases.LEVEL_CASES:
        p = cases.level_case(name)
        q = cases.case_query_inputs(p)
        xyz, new_xyz, new_coords = q
        worst = cases.assert_radius_margin(p['ranges'], p['radius'], xyz, new_xyz, new_coords, p['coords'], p['radius_margin'])
        idx, empty = cases.voxel_query_np(p['ranges'], p['radius'], p['nsample'], xyz, new_xyz, new_coords, cases.dense_index(p['coords']))
        out['q_%s_idx' % name], out['q_%s_empty' % name] = idx, empty
        G3 = p['grid'] ** 3
        per_roi = (~empty).reshape(-1, G3).sum(1)
        assert per_roi[cases.ROI_EMPTY] == 0 and per_roi[cases.ROI_CLUSTER] == G3 and 0 < per_roi[cases.ROI_BIG] < G3
        print('  case %s: N %d, M %d, radius margin %.3g, non-empty balls per RoI %s' % (name, len(xyz), len(new_xyz), worst, per_roi.tolist()))
        for pool in cases.POOLS:
            for training in (True, False):
                tag = 'm_%s_%s_%s' % (name, pool, 'train' if training else 'eval')
                r32 = _run_module(_ref_module(p, pool), p, q, torch.float32, training)
                with as_f64():
                    r64 = _run_module(_ref_module(p, pool), p, q, torch.float64, training)
                mod = _ref_module(p, pool)
                conv, bn = mod.mlps_pos[0][0], mod.mlps_pos[0][1]
                stats = {} if training else {'mean': _np(bn.running_mean), 'var': _np(bn.running_var)}
                f64, pre, bm, bv = cases.pool_f64(_np(r32['features_in']), xyz, new_xyz, idx, empty, _np(conv.weight), _np(bn.weight),
                                                 _np(bn.bias), bn.eps, pool, **stats)
                # the f64 definition is what the reference computes: its own f64 run on its own f64 features_in agrees
                chk = cases.pool_f64(_np(r64['features_in']), xyz, new_xyz, idx, empty, _np(conv.weight), _np(bn.weight), _np(bn.bias),
                                     bn.eps, pool, **stats)[0]
                assert np.abs(chk - _np(r64['pooled'])).max() < 1e-11, np.abs(chk - _np(r64['pooled'])).max()
                if pool == 'max_pool':
                    act = np.maximum(pre, 0)
                    top = act.max(1)
                    for m_ in range(len(idx)):                     # runner-up among the OTHER rows of the ball
                        if empty[m_]:
                            continue
                        rows = idx[m_]
                        best_row = rows[act[m_].argmax(0)]          # (C)
                        other = np.where(rows[:, None] != best_row[None, :], act[m_], -np.inf).max(0)
                        live = top[m_] > 0
                        assert np.all(top[m_][live] - other[live] > GAP_MAX), 'a near-tie of the maximum: change MODULE_SEED'
                    assert np.abs(pre.max(1))[~empty].min() > GAP_RELU_MAX, 'a maximum on the ReLU kink: change MODULE_SEED'
                else:
                    assert np.abs(pre).min() > GAP_RELU_AVG, 'a value on the ReLU kink (%.3g): change MODULE_SEED' % np.abs(pre).min()
                out[tag + '_pooled_e_ref'] = np.array([np.abs(_np(r32['pooled']).astype(np.float64) - f64).max()])
                out[tag + '_out'] = _np(r32['out'])[cases.ROWS]
                out[tag + '_e_ref_out'] = np.array([np.abs(_np(r32['out']).astype(np.float64) - _np(r64['out'])).max()])
                if training:
                    out[tag + '_bn_mean'], out[tag + '_bn_var'] = bm, bv
                for key in r32:
                    if key.startswith('grad/') or key.startswith('buf/'):
                        out[tag + '_' + key] = _np(r32[key])[cases.ROWS] if key == 'grad/features' else _np(r32[key])
                        if r32[key].dtype.is_floating_point:
                            out[tag + '_e_ref_' + key] = np.array([np.abs(_np(r32[key]).astype(np.float64) - _np(r64[key])).max()])
                            out[tag + '_max_' + key] = np.array([np.abs(_np(r64[key])).max()])
                print('    %s: pooled e_ref %.3g on values up to %.3g' % (tag, out[tag + '_pooled_e_ref'][0], np.abs(f64).max()))


def _ref_head(dp_ratio):
    from pcdet.models.roi_heads.voxelrcnn_head import VoxelRCNNHead
    torch.manual_seed(3)
    head = VoxelRCNNHead(backbone_channels=dict(cases.HEAD_CHANNELS), model_cfg=EasyDict(cases.head_cfg(dp_ratio)),
                         point_cloud_range=np.array(cases.HEAD_PCR, np.float32), voxel_size=list(cases.VOXEL), num_class=1)
    head.load_state_dict(seeded_state(head, cases.HEAD_SEED))
    return head


def _head_batch(rois, levels):
    feats = {n: SparseLevel(torch.from_numpy(c), torch.from_numpy(f), cases.head_level_shape(cases.HEAD_STRIDES[n]), cases.B)
             for n, (c, f) in levels.items()}
    return {'batch_size': cases.B, 'rois': torch.from_numpy(rois.copy()), 'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long),
            'roi_scores': torch.zeros(rois.shape[:2]), 'multi_scale_3d_features': feats, 'multi_scale_3d_strides': dict(cases.HEAD_STRIDES)}


def gen_head(out):
    """VoxelRCNNHead on two levels: state_dict keys and shapes, eval predictions for DP_RATIO 0 and 0.3, one training step with the
    sampler's picks injected: loss, every tb_dict entry, every parameter's gradient"""
    rois, levels = cases.head_inputs()
    for dp, tag in ((0.0, 'dp0'), (0.3, 'dp3')):
        head = _ref_head(dp)
        sd = head.state_dict()
        out['head_keys_' + tag] = np.array(list(sd.keys()))
        out['head_shapes_' + tag] = np.array([','.join(str(v) for v in t.shape) for t in sd.values()])
        head.eval()
        with torch.no_grad():
            bd = head(_head_batch(rois, levels))
        out['head_eval_cls_' + tag], out['head_eval_box_' + tag] = _np(bd['batch_cls_preds']), _np(bd['batch_box_preds'])
        assert bd['cls_preds_normalized'] is False
    s_rois, s_gt, s_iou, s_scores, s_labels = cases.head_sample()
    head = _ref_head(0.0)
    head.train()
    head.proposal_target_layer.sample_rois_for_rcnn = lambda batch_dict: tuple(
        torch.from_numpy(a.copy()) for a in (s_rois, s_gt, s_iou, s_scores, s_labels))
    bd = _head_batch(rois, levels)
    bd['gt_boxes'] = torch.from_numpy(s_gt)
    head(bd)
    loss, tb = head.get_loss()
    head.zero_grad()
    loss.backward()
    out['head_loss'] = np.array([float(loss.detach())])
    out['head_tb_keys'] = np.array(sorted(tb.keys()))
    out['head_tb_vals'] = np.array([float(tb[k]) for k in sorted(tb.keys())], np.float64)
    frd = head.forward_ret_dict
    out['head_rcnn_cls'], out['head_rcnn_reg'] = _np(frd['rcnn_cls']), _np(frd['rcnn_reg'])
    out['head_cls_labels'], out['head_reg_valid'] = _np(frd['rcnn_cls_labels']), _np(frd['reg_valid_mask'])
    for n, t in head.named_parameters():
        out['head_grad/' + n] = _np(t.grad)[:8] if n == 'shared_fc_layer.0.weight' else _np(t.grad)
    for n, t in head.named_buffers():
        if 'roi_grid_pool_layers' in n:
            out['head_buf/' + n] = _np(t)
    print('  head: loss %.6f' % float(loss), {k: round(float(v), 5) for k, v in tb.items()}, 'fg', int(out['head_reg_valid'].sum()))
    assert np.isfinite(out['head_loss']).all() and out['head_reg_valid'].sum() >= 2


if __name__ == '__main__':
    mg.import_reference()
    install_ops()
    parts = {'module': gen_module, 'head': gen_head}
    only = sys.argv[1:] or list(parts)
    prefix = {'module': ('q_', 'm_'), 'head': ('head_',)}
    d = {}
    if os.path.exists(cases.GOLDEN):
        old = np.load(cases.GOLDEN)
        d = {k: old[k] for k in old.files if not any(k.startswith(p) for n in only for p in prefix[n])}
    for name in only:
        print(name)
        parts[name](d)
    np.savez_compressed(cases.GOLDEN, **d)
    print(os.path.basename(cases.GOLDEN), '%.1f KB' % (os.path.getsize(cases.GOLDEN) / 1024))
