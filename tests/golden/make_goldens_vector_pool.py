"""Generate ref_vector_pool.npz and ref_pvrcnn_plusplus_vp.npz from the reference's own VectorPoolAggregationModuleMSG and
PVRCNNPlusPlus (companion of make_goldens.py / make_goldens_spc.py, whose import recipe and detector step it reuses).

Runs ONLY where the reference tree is mounted; the .npz files it writes are committed and are the only thing that travels.
Usage:  python tests/golden/make_goldens_vector_pool.py [ref_vector_pool.npz] [ref_pvrcnn_plusplus_vp.npz]

The reference's compiled wrappers (query_stacked_local_neighbor_idxs, query_three_nn_by_stacked_local_idxs, vector_pool and its
gradient, three_interpolate and its gradient) are answered by the numpy restatements of tests/vector_pool_cases.py; its autograd
Functions with their grow-and-retry loops, its modules and its detector run unmodified on the CPU.

ref_vector_pool.npz
  * nn/<case>/idx, dist          ThreeNNForVectorPoolByTwoStep on every case of three_nn_cases()
  * voxel/<case>/features, local_xyz, cnt, grad      VectorPoolWithVoxelQuery (pooling_type 1) forward and backward on voxel_cases()
  * module/<name>/keys, out_train, out_eval, grad/<parameter>, grad_features     VectorPoolAggregationModuleMSG with seeded weights on
    module_case(): a training step (loss = sum(out * probe)) and an eval pass from the same state
ref_pvrcnn_plusplus_vp.npz: make_goldens_spc.gen_pvrcnn_plusplus with the four VectorPool sections of
  tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml (raw_points reduced to 1 channel: KITTI clouds carry one feature) and the gradients of
  vector_pool_cases.VP_GRADS."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import make_goldens as mg                                                    # noqa: E402
import make_goldens_spc as mgs                                               # noqa: E402
from make_goldens import import_reference, save, _np, EasyDict              # noqa: E402
from _constants import seeded_state                                          # noqa: E402
import vector_pool_cases as vc                                               # noqa: E402

MODULE_SEED = 91
calls = {'lists': 0, 'retries': 0, 'voxel': 0}


def install_vector_pool_ops():
    m = sys.modules['pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda']

    def query_lists(support_xyz, xyz_cnt, new_xyz, new_cnt, stack, start_len, cumsum, avg_length, max_dist, nsample, neighbor_type):
        lists = vc.query_neighbors(_np(support_xyz), _np(xyz_cnt), _np(new_xyz), _np(new_cnt), max_dist, int(nsample), int(neighbor_type))
        cap, cur = int(avg_length) * len(lists), 0
        calls['lists'] += 1
        for i, rows in enumerate(lists):                      # (the cursor hands out the offsets in arrival order: here row order)
            start_len[i, 0], start_len[i, 1] = cur, len(rows)
            if cur < cap:
                k = min(len(rows), cap - cur)
                stack[cur:cur + k] = torch.from_numpy(rows[:k].astype(np.int32))
            cur += len(rows)
        cumsum[0] = cur
        calls['retries'] += cur > cap

    def three_nn_lists(support_xyz, new_xyz, centers, out_idx, out_dist2, stack, start_len, M, G):
        s, sl = _np(stack).astype(np.int64), _np(start_len)
        lists = [s[a:a + n] for a, n in sl]
        idx, d2 = vc.three_nn_over_lists(_np(support_xyz), _np(centers), lists)
        out_idx.copy_(torch.from_numpy(idx))
        out_dist2.copy_(torch.from_numpy(d2))

    def three_interpolate(features, idx, weight, out):
        f, i, w = _np(features), _np(idx).astype(np.int64), _np(weight)
        out.copy_(torch.from_numpy(w[:, 0:1] * f[i[:, 0]] + w[:, 1:2] * f[i[:, 1]] + w[:, 2:3] * f[i[:, 2]]))

    def three_interpolate_grad(grad_out, idx, weight, grad_features):
        g, i, w = _np(grad_out), _np(idx).astype(np.int64), _np(weight)
        acc = np.zeros(tuple(grad_features.shape), np.float32)
        for j in range(3):
            np.add.at(acc, i[:, j], g * w[:, j:j + 1])
        grad_features.copy_(torch.from_numpy(acc))

    def vector_pool(support_xyz, xyz_cnt, feats, new_xyz, new_cnt, new_features, new_local_xyz, cnt, grouped, gx, gy, gz, R, use_xyz,
                    num_max_sum_points, nsample, neighbor_type, pooling_type):
        assert pooling_type == 1 and use_xyz == 1
        f, l, c, pick = vc.voxel_pool(_np(support_xyz), _np(xyz_cnt), _np(feats), _np(new_xyz), _np(new_cnt), (gx, gy, gz), R, int(nsample),
                                      int(neighbor_type))
        new_features.copy_(torch.from_numpy(f))
        new_local_xyz.copy_(torch.from_numpy(l))
        cnt.copy_(torch.from_numpy(c))
        mm, gg = np.nonzero(pick >= 0)
        rows = np.stack([pick[mm, gg], mm, gg], 1).astype(np.int32)
        k = min(len(rows), int(num_max_sum_points))
        grouped[:k] = torch.from_numpy(rows[:k])
        calls['voxel'] += 1
        return len(rows)

    def vector_pool_grad(grad_new_features, cnt, grouped, grad_support):
        g, c, rows = _np(grad_new_features), _np(cnt), _np(grouped)
        G = c.shape[1]
        g = g.reshape(g.shape[0], G, -1)
        acc = np.zeros(tuple(grad_support.shape), np.float32)
        for s, m_, g_ in rows:
            acc[s] += g[m_, g_] * np.float32(1.0 / max(float(c[m_, g_]), 1.0))
        grad_support.copy_(torch.from_numpy(acc))
    m.query_stacked_local_neighbor_idxs_wrapper_stack = query_lists
    m.query_three_nn_by_stacked_local_idxs_wrapper_stack = three_nn_lists
    m.three_interpolate_wrapper, m.three_interpolate_grad_wrapper = three_interpolate, three_interpolate_grad
    m.vector_pool_wrapper, m.vector_pool_grad_wrapper = vector_pool, vector_pool_grad
    torch.cuda.IntTensor = torch.IntTensor
    torch.cuda.FloatTensor = torch.FloatTensor


def gen_vector_pool(out):
    install_vector_pool_ops()
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_utils as ref_utils
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as ref_modules
    t = torch.from_numpy
    for name, c in vc.three_nn_cases().items():
        # (a first capacity of 2 per new point where the lists are longer: the reference's grow-and-retry loop runs)
        first = 2 if name.startswith('frames') else 1000
        dist, idx, avg = ref_utils.three_nn_for_vector_pool_by_two_step(
            t(c['support']), t(c['xyz_cnt']), t(c['new_xyz']), t(c['centers']), t(c['new_cnt']), c['R'], c['nsample'], c['ntype'], first,
            c['centers'].shape[1], c['mult'])
        out['nn/%s/idx' % name], out['nn/%s/dist' % name] = _np(idx), _np(dist)
        want_idx, want_dist, _ = vc.three_nn(c['support'], c['xyz_cnt'], c['new_xyz'], c['new_cnt'], c['centers'], c['R'] * c['mult'], c['nsample'],
                                             c['ntype'])
        assert np.array_equal(want_idx, _np(idx))
        print('  nn', name, 'empty cells', int((want_idx[:, :, 0] < 0).sum()), 'avg length', int(avg))
    assert calls['retries'] > 0
    for name, c in vc.voxel_cases().items():
        feats = t(c['feats']).requires_grad_(True)
        G = int(np.prod(c['grid']))
        f, l, mean, cnt = ref_utils.vector_pool_with_voxel_query_op(
            t(c['support']), t(c['xyz_cnt']), feats, t(c['new_xyz']), t(c['new_cnt']), *c['grid'], c['R'], c['feats'].shape[1], 1, 1, c['nsample'],
            c['ntype'], 1)
        probe = np.random.default_rng(3).normal(0, 1, tuple(f.shape)).astype(np.float32)
        (f * t(probe)).sum().backward()
        pre = 'voxel/%s/' % name
        out[pre + 'features'], out[pre + 'local_xyz'], out[pre + 'cnt'] = _np(f), _np(l), _np(cnt).astype(np.int32)
        out[pre + 'probe'], out[pre + 'grad'] = probe, _np(feats.grad)
        assert cnt.shape == (len(c['new_xyz']), G)
        print('  voxel', name, 'filled', int(cnt.sum()), 'mean points', int(mean))
    mc = vc.module_case()
    for name, (c_in, cfg) in vc.module_cfgs().items():
        torch.manual_seed(0)
        mod = ref_modules.VectorPoolAggregationModuleMSG(input_channels=c_in, config=EasyDict(cfg))
        state = seeded_state(mod, MODULE_SEED)
        pre = 'module/%s/' % name
        out[pre + 'keys'] = np.array(sorted(mod.state_dict().keys()))
        kw = lambda f: dict(xyz=t(mc['xyz']), xyz_batch_cnt=t(mc['xyz_cnt']), new_xyz=t(mc['new_xyz']), new_xyz_batch_cnt=t(mc['new_cnt']), features=f)
        mod.load_state_dict(state)
        mod.train()
        feats = t(mc['features']).requires_grad_(True)
        _, y = mod(**kw(feats))
        probe = np.random.default_rng(4).normal(0, 1, tuple(y.shape)).astype(np.float32)
        (y * t(probe)).sum().backward()
        out[pre + 'out_train'], out[pre + 'probe'], out[pre + 'grad_features'] = _np(y), probe, _np(feats.grad)
        for k, p in mod.named_parameters():
            out[pre + 'grad/' + k] = _np(p.grad)
        out[pre + 'running_mean'] = _np(mod.msg_post_mlps[1].running_mean).copy()         # (a copy: the state is loaded again below)
        mod.load_state_dict(state)
        mod.eval()
        with torch.no_grad():
            _, y = mod(**kw(t(mc['features'])))
        out[pre + 'out_eval'] = _np(y)
        print('  module', name, tuple(y.shape), len(out[pre + 'keys']), 'keys')


def vp_model_cfg():
    """make_goldens_spc.plusplus_model_cfg() with the yaml's VectorPool sections (what pv_rcnn_plusplus_cfg('kitti', 'vector_pool') builds)"""
    import yaml
    m, names = plusplus_sa_cfg()
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml')))['MODEL']
    m.PFE.SA_LAYER = EasyDict(y['PFE']['SA_LAYER'])
    m.PFE.SA_LAYER.raw_points.NUM_REDUCED_CHANNELS = 1
    m.ROI_HEAD.ROI_GRID_POOL = EasyDict(y['ROI_HEAD']['ROI_GRID_POOL'])
    return m, names


plusplus_sa_cfg = mgs.plusplus_model_cfg


def gen_pvrcnn_plusplus_vp(out):
    install_vector_pool_ops()
    mgs.plusplus_model_cfg = vp_model_cfg
    mgs.pv_grads = lambda kind: vc.VP_GRADS
    try:
        mgs.gen_pvrcnn_plusplus(out)
    finally:
        mgs.plusplus_model_cfg = plusplus_sa_cfg
    assert calls['voxel'] >= 2 and calls['lists'] >= 6
    assert any('separate_local_aggregation_layer' in k for k in out['pv_keys']) and any('msg_post_mlps' in k for k in out['pv_keys'])


if __name__ == '__main__':
    import_reference()
    only = sys.argv[1:]
    for name, fn in (('ref_vector_pool.npz', gen_vector_pool), ('ref_pvrcnn_plusplus_vp.npz', gen_pvrcnn_plusplus_vp)):
        if only and name not in only:
            continue
        d = {}
        fn(d)
        save(name, d)
