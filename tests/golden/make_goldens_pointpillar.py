"""Golden vectors of PointPillars (tests/golden/ref_pointpillar.npz) from the reference's own PillarVFE, PointPillarScatter and
PointPillar.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_pointpillar.py [vfe] [scatter] [detector] [cfg]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, feeds the seeded
inputs of tests/pillar_cases.py and stores outputs. Every float quantity is recorded from an f32 run and an f64 run of the same
reference module; e_ref_* = max|f32 - f64| is the reference's own f32 error, the unit of the tests' bars. A part that is not named
keeps what the existing file holds."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import pillar_cases as cases                   # noqa: E402
from _constants import EasyDict                # noqa: E402

_np = mg._np


def _ref_vfe(C, dtype):
    from pcdet.models.backbones_3d.vfe.pillar_vfe import PillarVFE
    vfe = PillarVFE(model_cfg=EasyDict(cases.vfe_cfg()), num_point_features=C, voxel_size=cases.VOXEL, point_cloud_range=cases.PCR)
    vfe.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.weights(C).items()})
    return vfe.to(dtype)


def _run_vfe(case, name, dtype, training):
    vfe = _ref_vfe(case['voxels'].shape[2], dtype).train(training)
    bd = {'voxels': torch.from_numpy(case['voxels']).to(dtype), 'voxel_num_points': torch.from_numpy(case['num_points']).to(dtype),
          'voxel_coords': torch.from_numpy(case['coords']).to(dtype)}
    out = vfe(bd)['pillar_features'].reshape(len(case['num_points']), -1)
    res = {'out': out.detach()}
    if training:
        (out * torch.from_numpy(cases.grad_out(name)).to(dtype)).sum().backward()
        p = vfe.pfn_layers[0]
        res.update({'dW': p.linear.weight.grad, 'dgamma': p.norm.weight.grad, 'dbeta': p.norm.bias.grad,
                    'running_mean': p.norm.running_mean.detach().clone(), 'running_var': p.norm.running_var.detach().clone()})
    return res


def gen_vfe(out):
    """per case: the reference's PillarVFE in train mode (output, dW, dgamma, dbeta, updated running statistics) and in eval mode
    (output), f32 values + e_ref against its own f64 run; the f64 run equals the numpy definition of tests/pillar_cases.py"""
    for name in cases.CASES:
        case = cases.make_case(name)
        w = cases.weights(case['voxels'].shape[2])
        print('  case %s: M %d, %d pillar redraws in %d rounds, margin / required >= %.2f' % (
            name, len(case['num_points']), case['redraws'], case['rounds'], case['margin_ratio']))
        for training in (True, False):
            tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
            r32, r64 = _run_vfe(case, name, torch.float32, training), _run_vfe(case, name, torch.float64, training)
            d = cases.vfe_f64(case, w, training)
            assert np.abs(d['out'] - _np(r64['out'])).max() < 1e-10, np.abs(d['out'] - _np(r64['out'])).max()
            if training:
                assert np.abs(d['running_mean'] - _np(r64['running_mean'])).max() < 1e-10
                assert np.abs(d['running_var'] - _np(r64['running_var'])).max() < 1e-10
            for key in r32:
                a32, a64 = _np(r32[key]), _np(r64[key])
                out['%s_%s' % (tag, key)] = a32
                out['%s_f64_%s' % (tag, key)] = a64
                out['%s_e_ref_%s' % (tag, key)] = np.array([np.abs(a32.astype(np.float64) - a64).max()])
                print('    %s %-13s e_ref %.3g on values up to %.3g' % (tag, key, out['%s_e_ref_%s' % (tag, key)][0], np.abs(a64).max()))
    from pcdet.models.backbones_3d.vfe.pillar_vfe import PillarVFE
    vfe = PillarVFE(model_cfg=EasyDict(cases.vfe_cfg()), num_point_features=4, voxel_size=cases.VOXEL, point_cloud_range=cases.PCR)
    out['vfe_keys'] = np.array(list(vfe.state_dict().keys()))


def gen_scatter(out):
    """the reference's PointPillarScatter on case a: the rows are the reference's own train-mode f32 output"""
    from pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter import PointPillarScatter
    case = cases.make_case('a')
    feats = _run_vfe(case, 'a', torch.float32, True)['out']
    sc = PointPillarScatter(model_cfg=EasyDict({'NUM_BEV_FEATURES': cases.COUT}), grid_size=np.array(cases.GRID))
    bd = sc({'pillar_features': feats, 'voxel_coords': torch.from_numpy(case['coords']).float()})
    out['scatter_map'] = _np(bd['spatial_features'])
    assert out['scatter_map'].shape == (case['B'], cases.COUT, cases.GRID[1], cases.GRID[0])


def _ref_yaml():
    import yaml
    return yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/kitti_models/pointpillar.yaml')))


def gen_cfg(out):
    """the values of kitti_models/pointpillar.yaml, as data (JSON)"""
    y = _ref_yaml()
    d = y['DATA_CONFIG']
    vox = [p for p in d['DATA_PROCESSOR'] if p['NAME'] == 'transform_points_to_voxels'][0]
    out['cfg_json'] = np.array(json.dumps({
        'CLASS_NAMES': y['CLASS_NAMES'], 'MODEL': y['MODEL'], 'POINT_CLOUD_RANGE': d['POINT_CLOUD_RANGE'], 'VOXEL_SIZE': vox['VOXEL_SIZE'],
        'MAX_POINTS_PER_VOXEL': vox['MAX_POINTS_PER_VOXEL'], 'MAX_NUMBER_OF_VOXELS': vox['MAX_NUMBER_OF_VOXELS'],
        'AUG_NAMES': [a['NAME'] for a in d['DATA_AUGMENTOR']['AUG_CONFIG_LIST']]}, sort_keys=True))


def _kitti_batch():
    import importlib.util                       # by path: the name `pcdet` is the reference's package in this process
    spec = importlib.util.spec_from_file_location(
        'crb_synthetic', os.path.join(os.path.dirname(os.path.dirname(HERE)), 'crb-active-3ddet_amd', 'pcdet', 'datasets', 'synthetic.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kitti_batch


def _ref_detector(dtype, overrides=None):
    from pcdet.config import cfg as ref_cfg
    from pcdet.models import build_network
    y = _ref_yaml()
    ref_cfg.CLASS_NAMES = y['CLASS_NAMES']
    ref_cfg.MODEL = EasyDict(y['MODEL'])

    class Dataset:
        pass
    ds = Dataset()
    ds.class_names, ds.grid_size = y['CLASS_NAMES'], np.array(cases.GRID, np.int64)
    ds.point_cloud_range, ds.voxel_size = np.array(cases.PCR, np.float32), list(cases.VOXEL)
    ds.depth_downsample_factor = None
    ds.point_feature_encoder = EasyDict(num_point_features=4)
    model = build_network(model_cfg=EasyDict(y['MODEL']), num_class=3, dataset=ds)
    sd = model.state_dict()
    seeded = cases.detector_state([(k, tuple(v.shape), v.dtype.is_floating_point) for k, v in sd.items()], overrides=overrides)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(sd[k].shape) for k, v in seeded.items()})
    return model.to(dtype).train()


def _batch(inp, dtype):
    return {'voxels': torch.from_numpy(inp['voxels']).to(dtype), 'voxel_coords': torch.from_numpy(inp['voxel_coords']).to(dtype),
            'voxel_num_points': torch.from_numpy(inp['voxel_num_points']).to(dtype),
            'gt_boxes': torch.from_numpy(inp['gt_boxes']), 'batch_size': inp['batch_size']}


def _kink_margins(inp):
    """shift the BatchNorm biases of the seeded detector, layer by layer in execution order, until every BatchNorm output of the
    reference's f64 forward pass is farther than cases.DET_KINK from the ReLU kink (for the pillar net: its maximum over the slots)
    -> {state-dict key of the bias: f32 array}"""
    overrides = {}
    for _ in range(64):
        model = _ref_detector(torch.float64, overrides)
        seen, hooks = [], []
        for name, m in model.named_modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                def hook(mod, i, o, name=name):
                    o = o.detach()
                    per_channel = o.max(2)[0].t() if o.dim() == 3 else o.permute(1, 0, 2, 3).reshape(o.shape[1], -1)   # (C, n)
                    seen.append((name, per_channel.numpy()))
                hooks.append(m.register_forward_hook(hook))
        with torch.no_grad():
            for cur in model.module_list[:-1]:                      # up to the dense head
                inp_b = cur(inp_b) if cur is not model.module_list[0] else cur(_batch(inp, torch.float64))
        for h in hooks:
            h.remove()
        worst = min(float(np.abs(v).min()) for _, v in seen)
        first = next(((n, v) for n, v in seen if np.abs(v).min() <= cases.DET_KINK), None)
        if first is None:
            print('  kink margins: %d BatchNorm layers, %d with shifted biases, smallest |pre-activation| %.3g' % (len(seen), len(overrides), worst))
            return overrides
        name, v = first
        key = name + '.bias'
        bias = _np(dict(model.named_parameters())[key]).astype(np.float64)
        shift = np.array([cases.nudge_bias(v[c]) for c in range(v.shape[0])])
        overrides[key] = (bias + shift).astype(np.float32)
        print('    %-32s %3d channels shifted, largest shift %.3g' % (key, int((shift != 0).sum()), np.abs(shift).max()))
    raise AssertionError('kink margins not met')


def gen_detector(out):
    """one training step of the reference's PointPillar on the reduced grid, f32 and f64 (the targets are assigned from the f32
    anchors and boxes in both): loss, every tb_dict entry, three gradients, each with e_ref = the larger error of two f32 runs of the
    reference (NCHW and channels_last memory) against its f64 run; the state-dict key list; the BatchNorm
    biases shifted off the ReLU kinks (cases.DET_KINK), which the tests load on top of the seeded state"""
    inp = cases.detector_inputs(_kitti_batch())
    print('  pillars %d, boxes per frame %s' % (len(inp['voxels']), (inp['gt_boxes'][:, :, 7] > 0).sum(1).tolist()))
    assert (inp['gt_boxes'][:, :, 7] > 0).sum(1).min() >= 1
    overrides = _kink_margins(inp)
    for k, v in overrides.items():
        out['det_bias/' + k] = v
    res = {}
    # two f32 evaluations of the reference: its own NCHW memory, and channels_last memory (the layout the device route runs the
    # 2-D part in; the same torch modules take other kernels and other summation orders there)
    for tag, dtype in (('f32', torch.float32), ('f32_cl', torch.float32), ('f64', torch.float64)):
        model = _ref_detector(dtype, overrides)
        if tag == 'f32_cl':
            model = model.to(memory_format=torch.channels_last)
        ret, tb, _ = model(_batch(inp, dtype))
        model.zero_grad()
        ret['loss'].backward()
        params = dict(model.named_parameters())
        r = {'loss': np.array([float(ret['loss'].detach())], np.float64)}
        r['tb_vals'] = np.array([float(tb[k]) for k in sorted(tb)], np.float64)
        for n, sl in cases.DET_GRADS.items():
            r['grad/' + n] = _np(params[n].grad)[sl].copy()
        res[tag] = r
        out['det_tb_keys'] = np.array(sorted(tb))
        out['det_keys'] = np.array(list(model.state_dict().keys()))
        out['det_pos'] = np.array([int((model.dense_head.forward_ret_dict['box_cls_labels'] > 0).sum())])
    for key, a32 in res['f32'].items():
        a64 = res['f64'][key]
        out['det_' + key] = a32
        out['det_f64_' + key] = a64
        e = [np.abs(res[t][key].astype(np.float64) - a64).max() for t in ('f32', 'f32_cl')]
        out['det_e_ref_nchw_' + key], out['det_e_ref_cl_' + key] = np.array([e[0]]), np.array([e[1]])
        out['det_e_ref_' + key] = np.array([max(e)])                # the reference's f32 error: the larger of its two f32 runs
        print('    %-48s e_ref %.3g (NCHW %.3g, channels_last %.3g) on values up to %.3g' % (key, max(e), e[0], e[1], np.abs(a64).max()))
    print('  loss %.6f, positives %d' % (res['f64']['loss'][0], out['det_pos'][0]), dict(zip(out['det_tb_keys'], res['f64']['tb_vals'].round(5))))
    assert out['det_pos'][0] > 0 and np.isfinite(res['f32']['loss']).all()


if __name__ == '__main__':
    mg.import_reference()
    parts = {'vfe': gen_vfe, 'scatter': gen_scatter, 'cfg': gen_cfg, 'detector': gen_detector}
    only = sys.argv[1:] or list(parts)
    prefix = {'vfe': ('vfe_',), 'scatter': ('scatter_',), 'cfg': ('cfg_',), 'detector': ('det_',)}
    d = {}
    if os.path.exists(cases.GOLDEN):
        old = np.load(cases.GOLDEN)
        d = {k: old[k] for k in old.files if not any(k.startswith(p) for n in only for p in prefix[n])}
    for name in only:
        print(name)
        parts[name](d)
    np.savez_compressed(cases.GOLDEN, **d)
    print(os.path.basename(cases.GOLDEN), '%.1f KB' % (os.path.getsize(cases.GOLDEN) / 1024))
