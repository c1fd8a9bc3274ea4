"""Golden vectors of the two-layer dynamic pillar net (tests/golden/ref_dyn_pillar.npz) from the reference's own DynamicPillarVFE.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_dyn_pillar.py
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py (torch_scatter by the
stand-in of make_goldens_dyn_voxel.py), feeds the seeded points and weights of tests/dyn_pillar_cases.py and stores outputs.
Per case, train and eval, from an f32 and an f64 run of the reference's module: output, voxel_coords, the six parameter gradients
under a seeded grad_out (train), the updated running statistics (train), and e_ref_* = max|f32 - f64| of each, the reference's own
f32 error and the unit of the tests' bars. The f64 run is asserted to equal the numpy definition of the cases file. The NaN rows are
taken out before the reference sees them (its floor(NaN).int() is undefined). Also: the state-dict key list."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import make_goldens_dyn_voxel as mv            # noqa: E402
import dyn_pillar_cases as cases               # noqa: E402
from _constants import EasyDict                # noqa: E402

_np = mg._np


def _ref_vfe(C, dtype):
    from pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import DynamicPillarVFE
    vfe = DynamicPillarVFE(model_cfg=EasyDict(cases.vfe_cfg()), num_point_features=C, voxel_size=cases.VOXEL, grid_size=cases.GRID,
                           point_cloud_range=cases.PCR)
    vfe.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in cases.weights(C).items()})
    return vfe.to(dtype)


def _run(case, dtype, training):
    pts = case['points'][~np.isnan(case['points']).any(1)]
    vfe = _ref_vfe(case['C'], dtype).train(training)
    bd = vfe({'points': torch.from_numpy(pts).to(dtype), 'batch_size': case['B']})
    out = bd['pillar_features']
    res = {'out': out.detach(), 'coords': bd['voxel_coords']}
    if training:
        (out * torch.from_numpy(cases.grad_out(case['name'], out.shape[0])).to(dtype)).sum().backward()
        for i, p in enumerate(vfe.pfn_layers):
            res.update({'dW%d' % (i + 1): p.linear.weight.grad, 'dgamma%d' % (i + 1): p.norm.weight.grad, 'dbeta%d' % (i + 1): p.norm.bias.grad,
                        'running_mean%d' % (i + 1): p.norm.running_mean.detach().clone(),
                        'running_var%d' % (i + 1): p.norm.running_var.detach().clone()})
    return res


def gen_detector(out):
    """one training step of the reference's CenterPoint built from waymo_models/centerpoint_dyn_pillar_1x.yaml on the 64 x 64 grid of
    the cases file, weights seeded by parameter name (pillar_cases.detector_state), two synthetic frames: loss, every tb_dict entry and
    three gradients from three runs - f32 in NCHW memory, f32 in channels_last memory (the layout the device route runs the 2-D part
    in) and f64; e_ref = the larger f32 error; the BatchNorm biases shifted off the ReLU kinks. Also the yaml's values as JSON."""
    import json
    import importlib.util
    import yaml
    import pillar_cases
    from pcdet.config import cfg as ref_cfg
    from pcdet.models import build_network
    y = yaml.safe_load(open(os.path.join(mg.REF, 'tools/cfgs/waymo_models/centerpoint_dyn_pillar_1x.yaml')))
    d = y['DATA_CONFIG']
    out['cfg_json'] = np.array(json.dumps({'CLASS_NAMES': y['CLASS_NAMES'], 'MODEL': y['MODEL'], 'POINT_CLOUD_RANGE': d['POINT_CLOUD_RANGE'],
                                           'VOXEL_SIZE': d['DATA_PROCESSOR'][2]['VOXEL_SIZE']}, sort_keys=True))

    class Dataset:
        pass
    ds = Dataset()
    ds.class_names, ds.grid_size = cases.DET_CLASSES, np.array(cases.DET_GRID, np.int64)
    ds.point_cloud_range, ds.voxel_size = np.array(cases.DET_PCR, np.float32), list(cases.DET_VOXEL)
    ds.depth_downsample_factor = None
    ds.point_feature_encoder = EasyDict(num_point_features=5)

    def build(dtype, channels_last, overrides=None):
        m = EasyDict(y['MODEL'])
        ref_cfg.CLASS_NAMES, ref_cfg.MODEL = cases.DET_CLASSES, m
        model = build_network(model_cfg=m, num_class=3, dataset=ds)
        sd = model.state_dict()
        seeded = pillar_cases.detector_state([(k, tuple(v.shape), v.dtype.is_floating_point) for k, v in sd.items()], seed=cases.DET_SEED,
                                             overrides=overrides)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)).reshape(sd[k].shape) for k, v in seeded.items()})
        model = model.to(dtype)
        if channels_last:
            model.backbone_2d.to(memory_format=torch.channels_last)
            model.dense_head.to(memory_format=torch.channels_last)
        return model.train()

    spec = importlib.util.spec_from_file_location(
        'crb_synthetic', os.path.join(os.path.dirname(os.path.dirname(HERE)), 'crb-active-3ddet_amd', 'pcdet', 'datasets', 'synthetic.py'))
    syn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(syn)
    inp = cases.detector_inputs(syn.kitti_batch)
    print('  points %d, boxes per frame %s' % (len(inp['points']), (inp['gt_boxes'][:, :, 7] > 0).sum(1).tolist()))
    def batch(dtype):
        return {'points': torch.from_numpy(inp['points']).to(dtype), 'gt_boxes': torch.from_numpy(inp['gt_boxes'].copy()),
                'batch_size': inp['batch_size']}

    # shift the BatchNorm biases, layer by layer in execution order, until every BatchNorm output of the reference's f64 forward pass is
    # farther than pillar_cases.DET_KINK from the ReLU kink (see there for why); the tests load the shifted biases on top of the seeds
    overrides = {}
    for _ in range(96):
        model = build(torch.float64, False, overrides)
        seen, hooks = [], []
        for name, mod in model.named_modules():
            if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                def hook(mod, i, o, name=name):
                    o = o.detach()
                    seen.append((name, (o.t() if o.dim() == 2 else o.permute(1, 0, 2, 3).reshape(o.shape[1], -1)).numpy()))
                hooks.append(mod.register_forward_hook(hook))
        with torch.no_grad():
            model(batch(torch.float64))
        for h in hooks:
            h.remove()
        first = next(((n, v) for n, v in seen if np.abs(v).min() <= pillar_cases.DET_KINK), None)
        if first is None:
            print('  kink margins: %d BatchNorm layers, %d with shifted biases, smallest |pre-activation| %.3g' % (
                len(seen), len(overrides), min(float(np.abs(v).min()) for _, v in seen)))
            break
        name, v = first
        bias = _np(dict(model.named_parameters())[name + '.bias']).astype(np.float64)
        shift = np.array([pillar_cases.nudge_bias(v[c]) for c in range(v.shape[0])])
        overrides[name + '.bias'] = (bias + shift).astype(np.float32)
        print('    %-40s %3d channels shifted, largest shift %.3g' % (name + '.bias', int((shift != 0).sum()), np.abs(shift).max()))
    else:
        raise AssertionError('kink margins not met')
    for k, v in overrides.items():
        out['det_bias/' + k] = v
    res = {}
    for tag, dtype, cl in (('f32', torch.float32, False), ('f32_cl', torch.float32, True), ('f64', torch.float64, False)):
        model = build(dtype, cl, overrides)
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
        print('  %-6s loss %.6f, objects %d' % (tag, r['loss'][0], out['det_objects'][0]))
    for key, a32 in res['f32'].items():
        a64 = res['f64'][key]
        out['det_' + key], out['det_f64_' + key] = a32, a64
        e = [np.abs(res[t][key].astype(np.float64) - a64).max() for t in ('f32', 'f32_cl')]
        out['det_e_ref_' + key] = np.array([max(e)])
        print('    %-48s e_ref %.3g (NCHW %.3g, channels_last %.3g) on values up to %.3g' % (key, max(e), e[0], e[1], np.abs(a64).max()))
    assert np.isfinite(res['f32']['loss']).all() and out['det_objects'][0] > 0


def main():
    mg.import_reference()
    mv.install_torch_scatter()
    out = {}
    for name in cases.CASES:
        case = cases.make_case(name)
        print('  case %s: N %d, %d point redraws in %d rounds' % (name, len(case['points']), case['redraws'], case['rounds']))
        w = cases.weights(case['C'])
        for training in (True, False):
            tag = 'vfe_%s_%s' % (name, 'train' if training else 'eval')
            r32, r64 = _run(case, torch.float32, training), _run(case, torch.float64, training)
            d = cases.net_f64(case['points'], case['B'], w, training)
            assert (_np(r32['coords']) == d['coords']).all() and (_np(r64['coords']) == d['coords']).all()
            assert np.abs(d['out'] - _np(r64['out'])).max() < 1e-10, np.abs(d['out'] - _np(r64['out'])).max()
            if training:
                for k in cases.STATS:
                    assert np.abs(d[k] - _np(r64[k])).max() < 1e-10, k
            for key in r32:
                if key == 'coords':
                    out['%s_coords' % tag] = _np(r32[key]).astype(np.int32)
                    continue
                a32, a64 = _np(r32[key]), _np(r64[key])
                out['%s_%s' % (tag, key)] = a32
                out['%s_f64_%s' % (tag, key)] = a64
                out['%s_e_ref_%s' % (tag, key)] = np.array([np.abs(a32.astype(np.float64) - a64).max()])
                print('    %s %-14s e_ref %.3g on values up to %.3g' % (tag, key, out['%s_e_ref_%s' % (tag, key)][0], np.abs(a64).max()))
    print('detector')
    gen_detector(out)
    out['vfe_keys'] = np.array(list(_ref_vfe(4, torch.float32).state_dict().keys()))
    path = os.path.join(HERE, 'ref_dyn_pillar.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
