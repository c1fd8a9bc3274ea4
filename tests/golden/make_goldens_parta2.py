"""Golden vectors of the Part-A2 point head (tests/golden/ref_part_head.npz) from the reference's own PointIntraPartOffsetHead, and of
its sparse U-Net (tests/golden/ref_unetv2.npz) from the reference's own UNetV2.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_parta2.py [head] [unet]
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py (points-in-boxes is
answered by the oracle, _install_cpu_ops), feeds the seeded cases of tests/part_cases.py and stores outputs.

Per case: the reference's assign_targets (f32; its rotate_points_along_z casts the rotation to f32, so it has no f64 run: the f64 side
of the part labels is the numpy definition of tests/part_cases.py, as the CenterPoint targets golden does it) and get_loss with its
autograd in f32 and in f64 on the SAME labels and part labels (the f32 ones). The reference's f64 run keeps f32 class weights, so it is
checked against the numpy definition (2e-7) and the definition is what is stored as the f64 side. e_ref_* = max|f32 - f64| is the
reference's own f32 error, the unit of the tests' bars."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import part_cases as cases                     # noqa: E402
from _constants import EasyDict, seeded_state  # noqa: E402

_np = mg._np


def _ref_head(num_class):
    from pcdet.models.dense_heads.point_intra_part_head import PointIntraPartOffsetHead
    cfg = EasyDict({'CLS_FC': [16], 'PART_FC': [16], 'CLASS_AGNOSTIC': False,
                    'TARGET_CONFIG': {'GT_EXTRA_WIDTH': cases.EXTRA},
                    'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': dict(cases.LOSS_WEIGHTS)}})
    torch.manual_seed(0)
    return PointIntraPartOffsetHead(num_class=num_class, input_channels=16, model_cfg=cfg)


def gen_head(out):
    for name in cases.CASES:
        case = cases.make_case(name)
        head = _ref_head(case['num_class'])
        tgt = head.assign_targets({'point_coords': torch.from_numpy(case['points']), 'gt_boxes': torch.from_numpy(case['gt_boxes'])})
        labels, part32 = tgt['point_cls_labels'], tgt['point_part_labels']
        d_lab, d_part, d_owner = cases.targets_f64(case['points'], case['gt_boxes'], case['num_class'])
        assert np.array_equal(_np(labels), d_lab), name
        out[name + '_labels'], out[name + '_owner'] = _np(labels), d_owner
        out[name + '_part_f32'], out[name + '_part_f64'] = _np(part32), d_part
        out[name + '_e_ref_part'] = np.array([np.abs(_np(part32).astype(np.float64) - d_part).max()])
        runs = {}
        for dtype in (torch.float32, torch.float64):
            cls = torch.from_numpy(case['cls_preds']).to(dtype).requires_grad_(True)
            prt = torch.from_numpy(case['part_preds']).to(dtype).requires_grad_(True)
            head.forward_ret_dict = {'point_cls_preds': cls, 'point_part_preds': prt, 'point_cls_labels': labels,
                                     'point_part_labels': part32.to(dtype)}
            tb = {}
            loss_cls, tb = head.get_cls_layer_loss(tb)
            loss_part, tb = head.get_part_layer_loss(tb)
            total, tb2 = head.get_loss()
            assert abs(float(total.detach()) - float((loss_cls + loss_part).detach())) < 1e-6 * max(1.0, abs(float(total.detach())))
            g_cls, = torch.autograd.grad(loss_cls, cls)
            g_prt, = torch.autograd.grad(loss_part, prt, allow_unused=True)
            runs[dtype] = {'loss_cls': _np(loss_cls).reshape(1), 'loss_part': _np(loss_part).reshape(1),
                           'pos': np.array([tb['point_pos_num']]), 'd_cls': _np(g_cls),
                           'd_part': _np(g_prt) if g_prt is not None else np.zeros(prt.shape)}
            assert sorted(tb2) == ['point_loss_cls', 'point_loss_part', 'point_pos_num']
        d = cases.losses_f64(case['cls_preds'], case['part_preds'], _np(labels), _np(part32))
        for k, v64 in runs[torch.float64].items():
            v32 = runs[torch.float32][k]
            # the reference's f64 run keeps f32 class weights (`.float()`, point_head_template.py:137-139: 1 / pos rounded to f32), so it
            # is the definition only to 1e-7; the definition is stored as the f64 side and e_ref includes that rounding
            assert np.abs(v64 - d[k]).max() <= 2e-7 * max(1.0, np.abs(d[k]).max()), (name, k)
            v64 = np.asarray(d[k], np.float64).reshape(v64.shape)
            out['%s_f32_%s' % (name, k)], out['%s_f64_%s' % (name, k)] = v32, v64
            out['%s_e_ref_%s' % (name, k)] = np.array([np.abs(v32.astype(np.float64) - v64).max()])
        print('  %-7s N %5d pos %5d ignored %4d  loss_cls %.6f loss_part %.6f  e_ref: %s' % (
            name, len(case['points']), int((d_lab > 0).sum()), int((d_lab < 0).sum()), float(runs[torch.float64]['loss_cls'][0]),
            float(runs[torch.float64]['loss_part'][0]),
            ' '.join('%s %.1e' % (k, out['%s_e_ref_%s' % (name, k)][0]) for k in ('part', 'loss_cls', 'loss_part', 'd_cls', 'd_part'))))
    out['tb_keys'] = np.array(['point_loss_cls', 'point_loss_part', 'point_pos_num'])
    out['head_keys'] = np.array(sorted(_ref_head(3).state_dict().keys()))
    out['head_shapes'] = np.array([str(tuple(v.shape)) for _, v in sorted(_ref_head(3).state_dict().items())])


# ---- UNetV2 -------------------------------------------------------------------------------------------------------------------
def _install_spconv_torch(oracle):
    """mg._install_spconv_oracle (rulebooks by the oracle's restated semantics) with two changes for this golden: the gather-GEMM is
    plain torch (y = sum_o x[nbr[:, o]] @ w[o], autograd, any dtype: the oracle's C convolution is f32 only and the golden wants an
    f64 run), and an inverse convolution over the TRANSPOSED pair table of the strided layer that carries the same indice_key: output
    on that layer's input set, y[i] = sum_o x[j] @ w[o] over the pairs (i, j, o) of the forward table."""
    mg._install_spconv_oracle(oracle)
    spp = sys.modules['spconv.pytorch']
    Base, Tensor = spp.conv.SparseConvolution, spp.SparseConvTensor

    def gather_conv(x, w, nbr, n_out):
        y = x.new_zeros((n_out, w.shape[2]))
        for o in range(w.shape[0]):
            rows = np.nonzero(nbr[:, o] >= 0)[0]
            if len(rows):
                y = y.index_add(0, torch.from_numpy(rows), x[torch.from_numpy(nbr[rows, o].astype(np.int64))] @ w[o])
        return y

    def forward(self, x):
        coords = x.indices.numpy()
        K = int(np.prod(self.kernel_size))
        if getattr(self, 'inverse', False):
            nbr, in_coords, in_shape = x.rulebooks[self.indice_key]
            assert len(nbr) == len(coords)
            nbr_t = np.full((len(in_coords), K), -1, np.int32)
            j, o = np.nonzero(nbr >= 0)
            nbr_t[nbr[j, o], o] = j
            nbr, out = nbr_t, Tensor(None, torch.from_numpy(in_coords), in_shape, x.batch_size)
        elif self.subm:
            if self.indice_key not in x.rulebooks:
                x.rulebooks[self.indice_key] = oracle.subm_nbr(coords, x.spatial_shape, self.kernel_size)
            nbr, out = x.rulebooks[self.indice_key], x
            assert len(nbr) == len(coords)
        else:
            oc, oshape = oracle.spconv_out(coords, x.spatial_shape, self.kernel_size, self.stride, self.padding)
            nbr = oracle.spconv_nbr(coords, x.spatial_shape, oc, self.kernel_size, self.stride, self.padding)
            x.rulebooks[self.indice_key] = (nbr, coords, list(x.spatial_shape))
            out = Tensor(None, torch.from_numpy(oc), oshape, x.batch_size)
        out.rulebooks = x.rulebooks                      # one table dictionary for the whole network, as spconv's indice_dict
        w = self.weight.reshape(self.weight.shape[0], K, -1).permute(1, 2, 0)
        return out.replace_feature(gather_conv(x.features, w, nbr, len(nbr)))
    Base.forward = forward

    class SubMConv3d(Base):                              # (the U-Net's lateral block names kernel_size by keyword)
        def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None, **kw):
            super().__init__(in_channels, out_channels, kernel_size, 1, padding, bias, indice_key, subm=True)

    class SparseInverseConv3d(Base):
        def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=True, **kw):
            super().__init__(in_channels, out_channels, kernel_size, 1, 0, bias, indice_key, subm=False)
            self.inverse = True
    spp.SubMConv3d, spp.SparseInverseConv3d = SubMConv3d, SparseInverseConv3d


def _ref_unet(dtype, overrides):
    from pcdet.models.backbones_3d.spconv_unet import UNetV2
    torch.manual_seed(0)
    m = UNetV2(EasyDict({'NAME': 'UNetV2', 'RETURN_ENCODED_TENSOR': True}), 4, np.array(cases.UNET_GRID), cases.UNET_VOXEL, cases.UNET_PCR)
    sd = seeded_state(m, cases.UNET_SEED)
    sd.update({k: torch.from_numpy(v) for k, v in overrides.items()})
    m.load_state_dict(sd)
    return m.to(dtype).train()


def _unet_batch(dtype):
    feats, coords, B = cases.unet_inputs()
    return {'voxel_features': torch.from_numpy(feats).to(dtype), 'voxel_coords': torch.from_numpy(coords.astype(np.float32)), 'batch_size': B}


def _unet_kink_margins():
    """shift BatchNorm biases, ReLU by ReLU in execution order, until every ReLU input of the reference's f64 forward pass is farther
    than cases.UNET_KINK from zero -> {state-dict key of the bias: f32 array}. (A ReLU's input is the output of the BatchNorm that ran
    last before it, plus the identity in the lateral blocks: shifting that bias shifts the input by the same amount.)"""
    overrides = {}
    for _ in range(200):
        model = _ref_unet(torch.float64, overrides)
        last, seen, hooks = [None], [], []
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                hooks.append(m.register_forward_hook(lambda mod, i, o, name=name: last.__setitem__(0, name)))
            elif isinstance(m, torch.nn.ReLU):
                hooks.append(m.register_forward_pre_hook(lambda mod, i: seen.append((last[0], _np(i[0]).T.copy()))))
        with torch.no_grad():
            model(_unet_batch(torch.float64))
        for h in hooks:
            h.remove()
        first = next(((n, v) for n, v in seen if np.abs(v).min() <= cases.UNET_KINK), None)
        if first is None:
            print('  kink margins: %d ReLU calls, %d shifted biases, smallest |input| %.3g' % (
                len(seen), len(overrides), min(float(np.abs(v).min()) for _, v in seen)))
            return overrides
        name, v = first
        key = name + '.bias'
        bias = _np(model.state_dict()[key]).astype(np.float64)
        # (the f32 bias is what both runs load: the shift is taken so that the margin holds for the rounded value, checked next round)
        overrides[key] = (bias + np.array([cases.nudge(v[c], 2 * cases.UNET_KINK) for c in range(v.shape[0])])).astype(np.float32)
    raise AssertionError('kink margins not met')


def gen_unet(out):
    """ref_unetv2.npz: the reference's UNetV2 in train mode on the reduced grid, f32 and f64"""
    overrides = _unet_kink_margins()
    for k, v in overrides.items():
        out['bias/' + k] = v
    res = {}
    for tag, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        model = _ref_unet(dtype, overrides)
        bd = model(_unet_batch(dtype))
        enc = bd['encoded_spconv_tensor']
        order = cases.linear_order(_np(enc.indices), enc.spatial_shape)
        r1, r2 = cases.unet_probe(bd['point_features'].shape[0], len(order))
        loss = (bd['point_features'] * torch.from_numpy(r1).to(dtype)).sum() + \
            (enc.features[torch.from_numpy(order)] * torch.from_numpy(r2).to(dtype)).sum()
        loss.backward()
        params = dict(model.named_parameters())
        res[tag] = {'point_features': _np(bd['point_features']), 'encoded_features': _np(enc.features)[order],
                    'loss': _np(loss).reshape(1)}
        res[tag].update({'grad/' + n: _np(params[n].grad)[sl] for n, sl in cases.UNET_GRADS.items()})
        if tag == 'f32':
            out['point_coords'], out['encoded_indices'] = _np(bd['point_coords']), _np(enc.indices)[order].astype(np.int32)
            out['encoded_shape'] = np.array(enc.spatial_shape)
            out['keys'] = np.array(sorted(model.state_dict().keys()))
            out['shapes'] = np.array([str(tuple(v.shape)) for _, v in sorted(model.state_dict().items())])
            assert bd['encoded_spconv_tensor_stride'] == 8 and model.num_point_features == 16
    for k, v64 in res['f64'].items():
        out['f64_' + k] = v64
        out['e_ref_' + k] = np.array([np.abs(res['f32'][k].astype(np.float64) - v64).max()])
        print('  %-36s max|f64| %.3e  e_ref %.3e' % (k, np.abs(v64).max(), out['e_ref_' + k][0]))
    print('  voxels %d, encoded rows %d, shape %s' % (len(out['point_coords']), len(out['encoded_indices']), out['encoded_shape'].tolist()))


if __name__ == '__main__':
    which = sys.argv[1:] or ['head', 'unet']
    mg.import_reference()
    oracle = mg._install_cpu_ops()
    if 'head' in which:
        out = {}
        gen_head(out)
        mg.save('ref_part_head.npz', out)
    if 'unet' in which:
        _install_spconv_torch(oracle)
        out = {}
        gen_unet(out)
        mg.save('ref_unetv2.npz', out)
