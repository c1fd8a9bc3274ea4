"""Golden vectors of CenterPoint's centre head (tests/golden/ref_centerpoint.npz) from the reference's own CenterHead, centernet_utils
and loss_utils.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_centerpoint.py [targets] [loss] [decode] [head] [cfg] [detector]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, feeds the seeded
inputs of tests/center_cases.py and stores outputs. Float quantities are recorded from an f32 run and an f64 run of the same reference
code (or, for the targets, against the f64 numpy definition of tests/center_cases.py); e_ref_* = max|f32 - f64| is the reference's own
f32 error, the unit of the tests' bars. A part that is not named keeps what the existing file holds."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import center_cases as cases                   # noqa: E402
from _constants import EasyDict, seeded_state  # noqa: E402

_np = mg._np
HM_ROWS = 8                                    # rows of the hm gradient that are stored in f64 (plus the planted cells)


def _head_cfg(heads, nmax, order, code_weights):
    return EasyDict({
        'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': heads, 'SHARED_CONV_CHANNEL': 64, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
        'SEPARATE_HEAD_CFG': {'HEAD_ORDER': order, 'HEAD_DICT': {n: {'out_channels': cases.REG_CHANNELS[n], 'num_conv': 2} for n in order}},
        'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': cases.STRIDE, 'NUM_MAX_OBJS': nmax, 'GAUSSIAN_OVERLAP': cases.OVERLAP,
                                   'MIN_RADIUS': cases.MIN_RADIUS},
        'LOSS_CONFIG': {'LOSS_WEIGHTS': dict(cases.LOSS_WEIGHTS, code_weights=code_weights)},
        'POST_PROCESSING': {'SCORE_THRESH': cases.SCORE_THRESH, 'POST_CENTER_LIMIT_RANGE': cases.DECODE_LIMIT, 'MAX_OBJ_PER_SAMPLE': cases.DECODE_K,
                            'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}}})


def _ref_head(heads, nmax=20, order=None, channels=32):
    from pcdet.models.dense_heads.center_head import CenterHead
    order = order or cases.HEAD_ORDER
    D = sum(cases.REG_CHANNELS[n] for n in order)
    torch.manual_seed(0)
    return CenterHead(model_cfg=_head_cfg(heads, nmax, order, cases.LOSS_WEIGHTS['code_weights'][:D]), input_channels=channels,
                      num_class=len(cases.CLASSES), class_names=cases.CLASSES, grid_size=np.array([cases.W * cases.STRIDE, cases.H * cases.STRIDE, 40]),
                      point_cloud_range=np.array(cases.PCR, np.float32), voxel_size=cases.VOXEL, predict_boxes_when_training=False)


def gen_targets(out):
    """the reference's assign_targets per case (it writes into the boxes it is handed: a copy), checked against the f64 definition"""
    from pcdet.models.model_utils import centernet_utils
    for name in cases.TARGET_CASES:
        case = cases.make_targets_case(name)
        head = _ref_head(case['heads'], case['nmax'])
        ret = head.assign_targets(torch.from_numpy(case['gt_boxes'].copy()), feature_map_size=(cases.H, cases.W))
        d = cases.targets_f64(case['gt_boxes'], case['heads'], case['nmax'])
        class_head, _, _ = cases.class_tables(case['heads'])
        for h in range(len(case['heads'])):
            tag = 'targets_%s_%d' % (name, h)
            heat, tb, inds, masks = (_np(ret[k][h]) for k in ('heatmaps', 'target_boxes', 'inds', 'masks'))
            assert np.array_equal(inds, d[h]['inds']) and np.array_equal(masks, d[h]['masks']), tag
            # the reference's f32 integer radii against the definition's
            for b in range(cases.B):
                rows = [box for box in case['gt_boxes'][b] if 1 <= box[-1] <= 3 and class_head[int(box[-1]) - 1] == h][:case['nmax']]
                for k, box in enumerate(rows):
                    if box[3] <= 0 or box[4] <= 0:
                        continue
                    t = torch.from_numpy(np.asarray(box))
                    r = centernet_utils.gaussian_radius(t[3:4] / cases.VOXEL[0] / cases.STRIDE, t[4:5] / cases.VOXEL[1] / cases.STRIDE, cases.OVERLAP)
                    assert max(int(r), cases.MIN_RADIUS) == d[h]['radius'][b, k], (tag, b, k)
            assert np.array_equal(heat == 1, d[h]['heatmap'] == 1) and np.array_equal(heat != 0, d[h]['heatmap'] != 0), tag
            ulps = np.abs(heat.astype(np.float64) - d[h]['heatmap']) / cases.ulp_f32(d[h]['heatmap'])
            assert ulps.max() <= 1, (tag, ulps.max())
            if name in ('one_head', 'two_heads', 'edges'):
                assert masks.sum(1).min() >= 1, tag
            out[tag + '_heatmap'], out[tag + '_target_boxes'], out[tag + '_inds'], out[tag + '_masks'] = heat, tb, inds, masks
            out[tag + '_e_ref'] = np.abs(tb.astype(np.float64) - d[h]['target_boxes']).reshape(-1, tb.shape[-1]).max(0)
            print('  %-22s masks %s, unit peaks %d, heatmap within %.2f ulp, e_ref per column %s' % (
                tag, masks.sum(1).tolist(), int((heat == 1).sum()), ulps.max(), np.array2string(out[tag + '_e_ref'], precision=2)))


def _ref_loss(case, dtype):
    head = _ref_head(case['heads'], order=case['order'])          # (get_loss walks the pred dicts it is given: one head)
    t = lambda a: torch.from_numpy(a).to(dtype).requires_grad_(True)
    pred = {'hm': t(case['hm'])}
    pred.update({n: t(case['reg'][n]) for n in case['order']})
    leaves = dict(pred)
    head.forward_ret_dict = {'pred_dicts': [pred], 'target_dicts': {
        'heatmaps': [torch.from_numpy(case['heatmap']).to(dtype)], 'target_boxes': [torch.from_numpy(case['target_boxes']).to(dtype)],
        'inds': [torch.from_numpy(case['inds'])], 'masks': [torch.from_numpy(case['masks'])]}}
    loss, tb = head.get_loss()
    loss.backward()
    res = {'loss': np.array([tb['hm_loss_head_0'], tb['loc_loss_head_0']], np.float64), 'g_hm': _np(leaves['hm'].grad)}
    res['g_reg'] = np.concatenate([_np(leaves[n].grad) for n in case['order']], 1)
    return res


def gen_loss(out):
    """the reference's get_loss (FocalLossCenterNet + RegLossCenterNet + the head's weights) on one head per case, f32 and f64"""
    for name in cases.LOSS_CASES:
        for h in range(len(cases.TARGET_CASES[name][0])):
            case = cases.make_loss_case(name, h)
            tag = 'loss_%s_%d' % (name, h)
            r32, r64 = _ref_loss(case, torch.float32), _ref_loss(case, torch.float64)
            assert np.abs(r64['loss'] - cases.loss_f64(case)).max() < 1e-9 * max(1.0, np.abs(r64['loss']).max()), tag
            p = case['planted']
            assert (r64['g_hm'][p] == 0).all() and (r32['g_hm'][p] == 0).all(), tag     # the clamp passes no gradient
            out[tag + '_f32'], out[tag + '_f64'] = r32['loss'], r64['loss']
            out[tag + '_e_ref'] = np.abs(r32['loss'] - r64['loss'])
            for k in ('g_hm', 'g_reg'):
                out['%s_e_ref_%s' % (tag, k)] = np.array([np.abs(r32[k].astype(np.float64) - r64[k]).max()])
            out[tag + '_g_hm_rows_f64'] = r64['g_hm'][:, :, :HM_ROWS].copy()
            flat = r64['g_reg'].reshape(cases.B, r64['g_reg'].shape[1], -1)
            out[tag + '_g_reg_at_inds_f64'] = np.stack([flat[b][:, case['inds'][b]].T for b in range(cases.B)])
            out[tag + '_g_reg_nonzero'] = np.array([int((r64['g_reg'] != 0).sum())])
            print('  %-20s loss %s e_ref %s; gradient e_ref hm %.3g (max %.3g) reg %.3g (max %.3g)' % (
                tag, r64['loss'], out[tag + '_e_ref'], out[tag + '_e_ref_g_hm'][0], np.abs(r64['g_hm']).max(), out[tag + '_e_ref_g_reg'][0],
                np.abs(r64['g_reg']).max()))


def _ref_decode(case, dtype):
    from pcdet.models.model_utils import centernet_utils
    t = lambda a: torch.from_numpy(a).to(dtype)
    reg = {n: t(case['reg'][n]) for n in case['order']}

    def run(thresh, limit):
        return centernet_utils.decode_bbox_from_heatmap(
            heatmap=t(case['hm']).sigmoid(), rot_cos=reg['rot'][:, 0:1], rot_sin=reg['rot'][:, 1:2], center=reg['center'],
            center_z=reg['center_z'], dim=reg['dim'].exp(), vel=reg.get('vel', None), point_cloud_range=cases.PCR, voxel_size=cases.VOXEL,
            feature_map_stride=cases.STRIDE, K=cases.DECODE_K, circle_nms=False, score_thresh=thresh,
            post_center_limit_range=torch.tensor(limit).to(dtype))
    full = run(None, [-1e6] * 3 + [1e6] * 3)
    cut = run(cases.SCORE_THRESH, cases.DECODE_LIMIT)
    res = {k: np.stack([_np(f[k]) for f in full]) for k in ('pred_boxes', 'pred_scores', 'pred_labels')}
    assert res['pred_scores'].shape == (cases.B, cases.DECODE_K)
    res['keep'] = np.stack([np.isin(_np(f['pred_scores']), _np(c['pred_scores'])) for f, c in zip(full, cut)])
    assert all(int(k.sum()) == len(c['pred_scores']) for k, c in zip(res['keep'], cut))
    return res


def gen_decode(out):
    """centernet_utils.decode_bbox_from_heatmap in f32 and f64: all K rows of every frame (a first call without limits) and the keep
    mask (the rows a second call with POST_CENTER_LIMIT_RANGE and SCORE_THRESH returns)"""
    for name in cases.DECODE_CASES:
        case = cases.make_decode_case(name)
        tag = 'decode_' + name
        r32, r64 = _ref_decode(case, torch.float32), _ref_decode(case, torch.float64)
        d = cases.decode_f64(case)
        assert np.abs(r64['pred_boxes'] - d['boxes']).max() < 1e-10 and np.abs(r64['pred_scores'] - d['scores']).max() < 1e-12, tag
        for r in (r32, r64):
            assert np.array_equal(r['pred_labels'], d['labels']) and np.array_equal(r['keep'], d['keep']), tag
        out[tag + '_boxes'], out[tag + '_scores'] = r32['pred_boxes'], r32['pred_scores']
        out[tag + '_boxes_f64'], out[tag + '_scores_f64'] = r64['pred_boxes'], r64['pred_scores']
        out[tag + '_labels'], out[tag + '_keep'] = r64['pred_labels'].astype(np.int64), r64['keep']
        out[tag + '_e_ref_boxes'] = np.abs(r32['pred_boxes'].astype(np.float64) - r64['pred_boxes']).reshape(-1, r64['pred_boxes'].shape[-1]).max(0)
        out[tag + '_e_ref_scores'] = np.array([np.abs(r32['pred_scores'].astype(np.float64) - r64['pred_scores']).max()])
        print('  %-14s kept %s of %d, e_ref boxes %s scores %.3g' % (tag, r64['keep'].sum(1).tolist(), cases.DECODE_K,
                                                                   np.array2string(out[tag + '_e_ref_boxes'], precision=2), out[tag + '_e_ref_scores'][0]))


def gen_head(out):
    """state-dict keys and shapes of the reference's CenterHead at 32 input channels, one-head and two-head configurations"""
    for tag, heads in (('one', cases.ONE_HEAD), ('two', cases.TWO_HEADS)):
        sd = _ref_head(heads).state_dict()
        out['head_%s_keys' % tag] = np.array(list(sd.keys()))
        out['head_%s_shapes' % tag] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
        print('  head_%s: %d entries' % (tag, len(sd)))


def gen_cfg(out):
    """the values of waymo_models/centerpoint_without_resnet.yaml, as data (JSON)"""
    import yaml
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/waymo_models/centerpoint_without_resnet.yaml')))
    out['cfg_json'] = np.array(json.dumps({'CLASS_NAMES': y['CLASS_NAMES'], 'MODEL': y['MODEL'], 'OPTIMIZATION': y['OPTIMIZATION']}, sort_keys=True))


def _f64_sparse_convs():
    """make_goldens._install_spconv_oracle answers the sparse convolutions with the oracle's f32 C code. For the f64 run of the
    detector the same rulebooks drive a gather + matmul in torch ops (any dtype, autograd), and dense() keeps the features' dtype."""
    from oracle.second_cpu import _OracleConv
    import oracle
    spp = sys.modules['spconv.pytorch']
    Conv, Tensor = spp.conv.SparseConvolution, spp.SparseConvTensor

    def gather_conv(x, w, nbr):
        idx = torch.from_numpy(np.where(nbr < 0, len(x), nbr).astype(np.int64))
        xp = torch.cat([x, x.new_zeros((1, x.shape[1]))], 0)
        y = x.new_zeros((len(nbr), w.shape[2]))
        for k in range(w.shape[0]):
            y = y + xp[idx[:, k]] @ w[k]
        return y

    def forward(self, x):
        coords = x.indices.numpy()
        K = int(np.prod(self.kernel_size))
        if self.subm:
            if self.indice_key not in x.rulebooks:
                x.rulebooks[self.indice_key] = oracle.subm_nbr(coords, x.spatial_shape, self.kernel_size)
            nbr, out = x.rulebooks[self.indice_key], x
        else:
            oc, oshape = oracle.spconv_out(coords, x.spatial_shape, self.kernel_size, self.stride, self.padding)
            nbr = oracle.spconv_nbr(coords, x.spatial_shape, oc, self.kernel_size, self.stride, self.padding)
            out = Tensor(None, torch.from_numpy(oc), oshape, x.batch_size)
        w = self.weight.reshape(self.weight.shape[0], K, -1).permute(1, 2, 0).contiguous()           # (K, Cin, Cout)
        f = x.features
        return out.replace_feature(gather_conv(f, w, nbr) if f.dtype == torch.float64 else _OracleConv.apply(f, w, nbr, len(coords)))

    def dense(self):
        c = self.indices.long()
        d, h, w = self.spatial_shape
        out = torch.zeros(self.batch_size, d, h, w, self.features.shape[1], dtype=self.features.dtype)
        out = out.index_put((c[:, 0], c[:, 1], c[:, 2], c[:, 3]), self.features)
        return out.permute(0, 4, 1, 2, 3).contiguous()
    Conv.forward, Tensor.dense = forward, dense


def gen_detector(out):
    """one training step and one eval pass of the reference's CenterPoint built from waymo_models/centerpoint_without_resnet.yaml on
    the KITTI geometry (KITTI class names, POST_CENTER_LIMIT_RANGE = the KITTI range), spconv answered by the oracle, weights seeded by
    parameter name, two synthetic frames. Every quantity from three runs: f32 in NCHW memory, f32 in channels_last memory (the layout
    the device route runs the 2-D part in) and f64; e_ref = the larger f32 error. Targets are assigned from the f32 boxes in all runs."""
    import yaml
    oracle = mg._install_cpu_ops()
    mg._install_spconv_oracle(oracle)
    _f64_sparse_convs()
    from pcdet.config import cfg as ref_cfg
    from pcdet.models import build_network
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/waymo_models/centerpoint_without_resnet.yaml')))
    names = cases.CLASSES
    pcr, vs = np.array(cases.DET_PCR, np.float32), np.array(cases.DET_VOXEL, np.float32)
    grid = np.round((pcr[3:6] - pcr[0:3]) / vs).astype(np.int64)

    chosen = {'thresh': 0.0}

    def model_cfg():
        m = EasyDict(y['MODEL'])
        m.DENSE_HEAD.POST_PROCESSING.SCORE_THRESH = chosen['thresh']
        m.DENSE_HEAD.CLASS_NAMES_EACH_HEAD = [list(names)]
        m.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE = [0, -40, -3, 70.4, 40, 1]
        return m

    class Dataset:
        pass
    ds = Dataset()
    ds.class_names, ds.grid_size, ds.point_cloud_range, ds.voxel_size = names, grid, pcr, list(vs)
    ds.depth_downsample_factor = None
    ds.point_feature_encoder = EasyDict(num_point_features=4)

    def build(dtype, channels_last):
        m = model_cfg()
        ref_cfg.CLASS_NAMES, ref_cfg.MODEL = names, m
        torch.manual_seed(0)
        model = build_network(model_cfg=m, num_class=3, dataset=ds)
        model.load_state_dict(cases.det_state(seeded_state(model, cases.DET_SEED)))
        model = model.to(dtype)
        if channels_last:                                             # (the 2-D part; the sparse weights are 5-D)
            model.backbone_2d.to(memory_format=torch.channels_last)
            model.dense_head.to(memory_format=torch.channels_last)
        return model

    import importlib.util                       # by path: the name `pcdet` is the reference's package in this process
    spec = importlib.util.spec_from_file_location(
        'crb_synthetic', os.path.join(os.path.dirname(os.path.dirname(HERE)), 'crb-active-3ddet_amd', 'pcdet', 'datasets', 'synthetic.py'))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    pts, off, gt = syn.kitti_batch(cases.DET_FIRST_FRAME, 2, cases.DET_POINTS)
    B = len(off) - 1
    voxels, coords, npts, _ = oracle.voxelize_batch(pts, off, pcr[:3], vs, grid, cases.DET_MAX_VOXELS, 5)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))
    print('  voxels %d, boxes per frame %s' % (len(coords), (gt[:, :, 7] > 0).sum(1).tolist()))

    def batch(dtype):
        return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)), 'voxels': torch.from_numpy(voxels.copy()).to(dtype),
                'voxel_coords': torch.from_numpy(coords.astype(np.float32)), 'voxel_num_points': torch.from_numpy(npts.astype(np.float32)).to(dtype),
                'gt_boxes': torch.from_numpy(gt.copy()), 'batch_size': B}
    # SCORE_THRESH of the eval pass: seeded weights leave most of the map at one background value (ties), so the threshold is set
    # between two picks of the f64 run that are far apart, above a run of picks that are pairwise far apart (cases.DET_SCORE_GAP)
    with torch.no_grad():
        m0 = build(torch.float64, False).eval()
        m0(batch(torch.float64))
        hm = m0.dense_head.forward_ret_dict['pred_dicts'][0]['hm'].sigmoid().flatten(1)
    n_keep = []
    for b in range(B):
        u = np.sort(_np(hm[b]))[::-1][:cases.DET_MAX_KEEP + 1]
        ok = -np.diff(u) >= cases.DET_SCORE_GAP
        n_keep.append(int(np.argmin(ok)) if not ok.all() else cases.DET_MAX_KEEP)
    u = np.sort(_np(hm[0]))[::-1]
    n = min(n_keep)
    assert n >= 4, n_keep
    chosen['thresh'] = float(max((np.sort(_np(hm[b]))[::-1][n - 1] + np.sort(_np(hm[b]))[::-1][n]) / 2 for b in range(B)))
    for b in range(B):
        ub = np.sort(_np(hm[b]))[::-1]
        assert np.abs(ub[:cases.DET_MAX_KEEP + 1] - chosen['thresh']).min() >= cases.DET_SCORE_GAP / 4, b
    out['det_ev_score_thresh'] = np.array([chosen['thresh']])
    print('  SCORE_THRESH %.8f: picks above it per frame %s' % (chosen['thresh'], [int((_np(hm[b]) > chosen['thresh']).sum()) for b in range(B)]))
    res, ev = {}, {}
    for tag, dtype, cl in (('f32', torch.float32, False), ('f32_cl', torch.float32, True), ('f64', torch.float64, False)):
        model = build(dtype, cl).train()
        ret, tb, _ = model(batch(dtype))
        model.zero_grad()
        ret['loss'].backward()
        params = dict(model.named_parameters())
        r = {'loss': np.array([float(ret['loss'].detach())], np.float64), 'tb_vals': np.array([float(tb[k]) for k in sorted(tb)], np.float64)}
        for n, sl in cases.DET_GRADS.items():
            r['grad/' + n] = _np(params[n].grad)[sl].copy()
        res[tag] = r
        out['det_tb_keys'] = np.array(sorted(tb))
        out['det_keys'] = np.array(list(model.state_dict().keys()))
        out['det_objects'] = np.array([int(model.dense_head.forward_ret_dict['target_dicts']['masks'][0].sum())])
        model = build(dtype, cl).eval()                               # (the step advanced the running statistics)
        with torch.no_grad():
            pred, recall = model(batch(dtype))
        ev[tag] = {k: _np(pred[0][k]) for k in ('pred_boxes', 'pred_scores', 'pred_labels')}
        ev[tag]['counts'] = np.array([len(p['pred_scores']) for p in pred], np.int64)
        print('  %-6s loss %.6f, eval boxes per frame %s' % (tag, r['loss'][0], ev[tag]['counts'].tolist()))
    for key, a32 in res['f32'].items():
        a64 = res['f64'][key]
        out['det_' + key], out['det_f64_' + key] = a32, a64
        e = [np.abs(res[t][key].astype(np.float64) - a64).max() for t in ('f32', 'f32_cl')]
        out['det_e_ref_' + key] = np.array([max(e)])
        print('    %-48s e_ref %.3g (NCHW %.3g, channels_last %.3g) on values up to %.3g' % (key, max(e), e[0], e[1], np.abs(a64).max()))
    # the eval pass: the three runs must pick the same boxes (else the case does not pin the post-processing); e_ref as above
    for t in ('f32', 'f32_cl'):
        assert np.array_equal(ev[t]['counts'], ev['f64']['counts']) and np.array_equal(ev[t]['pred_labels'], ev['f64']['pred_labels']), t
    assert ev["f64"]["counts"].min() >= 3
    out['det_ev_counts'], out['det_ev_pred_labels'] = ev['f64']['counts'], ev['f64']['pred_labels'].astype(np.int64)
    for key in ('pred_boxes', 'pred_scores'):
        out['det_ev_f64_' + key] = ev['f64'][key]
        e = max(np.abs(ev[t][key].astype(np.float64) - ev['f64'][key]).max() for t in ('f32', 'f32_cl'))
        out['det_ev_e_ref_' + key] = np.array([e])
        print('    eval %-12s e_ref %.3g' % (key, e))
    assert np.isfinite(res['f32']['loss']).all() and out['det_objects'][0] > 0


if __name__ == '__main__':
    mg.import_reference()
    parts = {'targets': gen_targets, 'loss': gen_loss, 'decode': gen_decode, 'head': gen_head, 'cfg': gen_cfg, 'detector': gen_detector}
    only = sys.argv[1:] or list(parts)
    prefix = {'targets': ('targets_',), 'loss': ('loss_',), 'decode': ('decode_',), 'head': ('head_',), 'cfg': ('cfg_',), 'detector': ('det_',)}
    d = {}
    if os.path.exists(cases.GOLDEN):
        old = np.load(cases.GOLDEN)
        d = {k: old[k] for k in old.files if not any(k.startswith(p) for n in only for p in prefix[n])}
    for name in only:
        print(name)
        parts[name](d)
    np.savez_compressed(cases.GOLDEN, **d)
    print(os.path.basename(cases.GOLDEN), '%.1f KB' % (os.path.getsize(cases.GOLDEN) / 1024))
