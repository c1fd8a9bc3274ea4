"""GPU: UNetV2 (pcdet/models/backbones_3d/spconv_unet.py) against the reference's own UNetV2 on a reduced grid
(tests/golden/ref_unetv2.npz, written by tests/golden/make_goldens_parta2.py; the case and its ReLU margins: tests/part_cases.py).

Bars. point_coords and the encoded tensor's indices: equal. point_features, the encoded rows, the probe loss and four gradients (encoder,
bottom, decoder, last lateral block): max|device - reference f64| <= 4 * e_ref, e_ref = max|reference f32 - reference f64| of the same
quantity. Every figure is printed as a multiple of e_ref before it is asserted.
Measured on the MI355X (multiples of e_ref, bar 4): point_features 1.52, encoded rows 1.44, loss 0.50, gradients
conv_input.0.weight 1.78, conv4.0.0.weight 2.26, inv_conv3.0.weight 2.76, conv_up_t1.conv1.weight 1.77."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import part_cases as cases  # noqa: E402
from _constants import EasyDict, seeded_state  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_unetv2.npz')
ENCODER_KEYS = {'subm1', 'subm2', 'subm3', 'subm4', 'spconv2', 'spconv3', 'spconv4', 'spconv_down2'}


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def make_unet(gold, dev, **cfg):
    """the golden's state: seeded over the key list of the full module (one stream in name order), its shifted biases on top"""
    from pcdet.models.backbones_3d import UNetV2
    torch.manual_seed(0)
    build = lambda c: UNetV2(EasyDict(dict({'NAME': 'UNetV2'}, **c)), 4, np.array(cases.UNET_GRID), cases.UNET_VOXEL, cases.UNET_PCR)
    m = build(cfg)
    sd = seeded_state(build({'RETURN_ENCODED_TENSOR': True}), cases.UNET_SEED)
    sd.update({k[len('bias/'):]: torch.from_numpy(v) for k, v in gold.items() if k.startswith('bias/')})
    m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()})
    return m.to(dev)


def batch(dev):
    feats, coords, B = cases.unet_inputs()
    return {'voxel_features': torch.from_numpy(feats).to(dev), 'voxel_coords': torch.from_numpy(coords).to(dev), 'batch_size': B}


def _check(tag, got, want, e_ref):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    print('%-36s err %.3e  e_ref %.3e  multiple %.2f' % (tag, err, e_ref, err / e_ref))
    return err <= 4 * e_ref


@pytest.fixture(scope='module')
def step(gold, dev):
    """one train-mode forward + backward along the golden's probe, shared by the tests that read it"""
    model = make_unet(gold, dev).train()
    bd = model(batch(dev))
    enc = bd['encoded_spconv_tensor']
    order = cases.linear_order(enc.indices.cpu().numpy(), enc.spatial_shape)
    r1, r2 = cases.unet_probe(bd['point_features'].shape[0], len(order))
    ot = torch.from_numpy(order).to(dev)
    loss = (bd['point_features'].double() * torch.from_numpy(r1).to(dev)).sum() + \
        (enc.features[ot].double() * torch.from_numpy(r2).to(dev)).sum()
    loss.backward()
    torch.cuda.synchronize()
    return model, bd, order, loss


def test_state_dict_keys_are_the_reference_s(gold, dev):
    sd = make_unet(gold, 'cpu').state_dict()
    assert sorted(sd) == list(gold['keys'])
    assert [str(tuple(v.shape)) for _, v in sorted(sd.items())] == list(gold['shapes'])


def test_outputs_against_the_reference(gold, step):
    model, bd, order, loss = step
    enc = bd['encoded_spconv_tensor']
    assert model.num_point_features == 16 and bd['encoded_spconv_tensor_stride'] == 8
    assert np.array_equal(bd['point_coords'].cpu().numpy(), gold['point_coords'])
    assert np.array_equal(enc.indices.cpu().numpy()[order], gold['encoded_indices']) and list(enc.spatial_shape) == list(gold['encoded_shape'])
    ok = [_check('point_features', bd['point_features'].detach().cpu().numpy(), gold['f64_point_features'], gold['e_ref_point_features'][0]),
          _check('encoded_features', enc.features.detach().cpu().numpy()[order], gold['f64_encoded_features'], gold['e_ref_encoded_features'][0]),
          _check('loss', loss.detach().cpu().numpy().reshape(1), gold['f64_loss'], gold['e_ref_loss'][0])]
    assert all(ok)


def test_gradients_against_the_reference(gold, step):
    model = step[0]
    params = dict(model.named_parameters())
    ok = [_check('grad/' + n, params[n].grad.cpu().numpy()[sl], gold['f64_grad/' + n], gold['e_ref_grad/' + n][0])
          for n, sl in cases.UNET_GRADS.items()]
    assert all(ok)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_the_decoder_builds_no_table_of_its_own(step):
    """every decoder layer found its rulebook through its indice_key: the dictionary holds the encoder's keys and nothing else"""
    enc = step[1]['encoded_spconv_tensor']
    assert set(enc.indice_dict.keys()) == ENCODER_KEYS


def test_eval_mode_runs(gold, dev):
    model = make_unet(gold, dev).eval()
    with torch.no_grad():
        bd = model(batch(dev))
    torch.cuda.synchronize()
    assert np.array_equal(bd['point_coords'].cpu().numpy(), gold['point_coords'])
    assert bd['point_features'].shape == (len(gold['point_coords']), 16) and bool(torch.isfinite(bd['point_features']).all())
    assert bd['encoded_spconv_tensor'].features.shape == (len(gold['encoded_indices']), 128)
    assert set(bd['encoded_spconv_tensor'].indice_dict.keys()) == ENCODER_KEYS


def test_without_the_encoded_tensor(gold, dev):
    model = make_unet(gold, dev, RETURN_ENCODED_TENSOR=False).train()
    assert model.conv_out is None
    bd = model(batch(dev))
    torch.cuda.synchronize()
    assert 'encoded_spconv_tensor' not in bd
    assert _check('point_features (no conv_out)', bd['point_features'].detach().cpu().numpy(), gold['f64_point_features'],
                  gold['e_ref_point_features'][0])


def test_a_lazily_voxelized_batch_gives_the_rows_of_an_eager_one(gold, dev):
    """raw points through MeanVFE: with the voxel count left on the device (the backbone's table plan reads it back with its level sizes)
    and with cut tensors - the same rows, bit for bit"""
    from pcdet.models.backbones_3d.vfe import MeanVFE
    rng = np.random.default_rng(7)
    lo, hi = np.array(cases.UNET_PCR[:3]), np.array(cases.UNET_PCR[3:])
    pts = [np.concatenate([np.full((n, 1), b), rng.uniform(lo + 0.01, hi - 0.01, (n, 3)), rng.uniform(0, 1, (n, 1))], 1)
           for b, n in enumerate((1500, 1100))]
    pts = torch.from_numpy(np.concatenate(pts).astype(np.float32)).to(dev)
    vfe = MeanVFE(EasyDict({'NAME': 'MeanVFE'}), 4, voxel_size=cases.UNET_VOXEL, point_cloud_range=cases.UNET_PCR,
                  grid_size=list(cases.UNET_GRID)).train()
    model = make_unet(gold, dev).train()
    outs = []
    for lazy in (False, True):
        bd = {'points': pts, 'batch_size': 2}
        if lazy:
            bd['_lazy_voxel_count'] = True
        with torch.no_grad():
            bd = model(vfe(bd))
        torch.cuda.synchronize()
        if lazy:
            from pcdet.models.backbones_3d.vfe import mean_vfe
            assert not mean_vfe.LAZY_VOXEL_COUNT or 'voxel_count_dev' not in bd      # the plan consumed the device count
        outs.append((bd['point_coords'], bd['point_features'], bd['encoded_spconv_tensor'].indices, bd['encoded_spconv_tensor'].features))
    assert outs[0][0].shape[0] > 1000
    for a, b in zip(*outs):
        assert torch.equal(a, b)
