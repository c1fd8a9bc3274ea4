"""CPU: the torch route of the Part-A2 point head's targets and losses (crbhip/part_head.py) against the reference's own head
(tests/golden/ref_part_head.npz), the head's surface and state-dict keys, and what the head refuses.

Bars: labels and owners equal (the cases keep every point 1e-4 m off every face); part labels, losses and gradients of the f32 torch
route within 4 * e_ref of the f64 values, of the f64 torch route within 1e-12 relative: it is the same expressions."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import part_cases as cases  # noqa: E402
from _constants import EasyDict  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_part_head.npz')
W = cases.LOSS_WEIGHTS
LOSS_ARGS = (cases.ALPHA, cases.GAMMA, W['point_cls_weight'], W['point_part_weight'])


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def head_cfg(**target):
    return EasyDict({'NAME': 'PointIntraPartOffsetHead', 'CLS_FC': [16], 'PART_FC': [16], 'CLASS_AGNOSTIC': False,
                     'TARGET_CONFIG': dict({'GT_EXTRA_WIDTH': cases.EXTRA}, **target),
                     'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': dict(cases.LOSS_WEIGHTS)}})


@pytest.mark.parametrize('name', list(cases.CASES))
def test_torch_route_of_the_targets_against_the_reference(gold, name):
    from crbhip import part_head
    case = cases.make_case(name)
    for dtype, bar in ((torch.float32, 4 * gold[name + '_e_ref_part'][0]), (torch.float64, 1e-12)):
        lab, part, owner = part_head.part_targets(torch.from_numpy(case['points']).to(dtype), torch.from_numpy(case['gt_boxes']).to(dtype),
                                                  cases.EXTRA, case['num_class'])
        assert lab.dtype == torch.int64 and part.dtype == dtype and owner.dtype == torch.int32
        assert np.array_equal(lab.numpy(), gold[name + '_labels']) and np.array_equal(owner.numpy(), gold[name + '_owner'])
        err = np.abs(part.double().numpy() - gold[name + '_part_f64']).max() if len(lab) else 0.0
        print(name, dtype, 'part labels err %.3e bar %.3e' % (err, bar))
        assert err <= bar


@pytest.mark.parametrize('name', list(cases.CASES))
def test_torch_route_of_the_losses_against_the_reference(gold, name):
    from crbhip import part_head
    case = cases.make_case(name)
    labels = torch.from_numpy(gold[name + '_labels'])
    for dtype in (torch.float32, torch.float64):
        cls = torch.from_numpy(case['cls_preds']).to(dtype).requires_grad_(True)
        prt = torch.from_numpy(case['part_preds']).to(dtype).requires_grad_(True)
        lc, lp, pos = part_head.part_loss(cls, prt, labels, torch.from_numpy(gold[name + '_part_f32']).to(dtype), *LOSS_ARGS)
        (lc + lp).backward()
        got = {'loss_cls': lc.detach().numpy(), 'loss_part': lp.detach().numpy(), 'd_cls': cls.grad.numpy(), 'd_part': prt.grad.numpy()}
        assert float(pos) == gold[name + '_f64_pos'][0]
        for k, v in got.items():
            want = gold['%s_f64_%s' % (name, k)]
            err = np.abs(v.astype(np.float64).reshape(want.shape) - want).max()
            bar = 4 * gold['%s_e_ref_%s' % (name, k)][0] if dtype == torch.float32 else 1e-12 * max(1.0, np.abs(want).max())
            print(name, dtype, k, 'err %.3e bar %.3e' % (err, bar))
            assert err <= bar, (name, k)


def test_definition_of_the_cases_matches_the_golden(gold):
    for name in cases.CASES:
        case = cases.make_case(name)
        lab, part, owner = cases.targets_f64(case['points'], case['gt_boxes'], case['num_class'])
        assert np.array_equal(lab, gold[name + '_labels']) and np.array_equal(owner, gold[name + '_owner'])
        assert np.array_equal(part, gold[name + '_part_f64'])
    assert cases.make_case('ragged')['counts'] == [1337, 1, 0] and cases.make_case('tiles')['points'].shape[0] == 3 * cases.LOSS_TILE + 77
    assert cases.make_case('no_pos')['points'].shape[0] < cases.LOSS_TILE and cases.CASES['ragged'][3] > cases.BOX_CHUNK


def test_head_surface_and_state_dict_keys(gold):
    from pcdet.models import dense_heads
    from pcdet.models.dense_heads import PointIntraPartOffsetHead
    assert dense_heads.__all__['PointIntraPartOffsetHead'] is PointIntraPartOffsetHead
    head = PointIntraPartOffsetHead(num_class=3, input_channels=16, model_cfg=head_cfg())
    sd = head.state_dict()
    assert sorted(sd) == list(gold['head_keys'])
    assert [str(tuple(v.shape)) for _, v in sorted(sd.items())] == list(gold['head_shapes'])
    assert head.box_layers is None


def test_head_forward_and_loss_on_host_tensors(gold):
    """the host route end to end: scores and part offsets written, targets assigned in training, the reference's tb_dict keys as
    detached 0-dim tensors, gradients down to the layers"""
    from pcdet.models.dense_heads import PointIntraPartOffsetHead
    case = cases.make_case('ragged')
    torch.manual_seed(0)
    head = PointIntraPartOffsetHead(num_class=3, input_channels=16, model_cfg=head_cfg())
    head.train()
    N = len(case['points'])
    batch = {'point_features': torch.randn(N, 16), 'point_coords': torch.from_numpy(case['points']),
             'gt_boxes': torch.from_numpy(case['gt_boxes']), 'batch_size': 3}
    out = head(batch)
    assert out['point_cls_scores'].shape == (N,) and out['point_part_offset'].shape == (N, 3)
    ret = head.forward_ret_dict
    assert torch.equal(out['point_part_offset'], torch.sigmoid(ret['point_part_preds']))
    assert torch.equal(out['point_cls_scores'], torch.sigmoid(ret['point_cls_preds']).max(-1)[0])
    assert np.array_equal(ret['point_cls_labels'].numpy(), gold['ragged_labels'])
    loss, tb = head.get_loss()
    assert sorted(tb) == sorted(gold['tb_keys']) and all(v.dim() == 0 and not v.requires_grad for v in tb.values())
    assert float(tb['point_pos_num']) == gold['ragged_f64_pos'][0]
    assert abs(float(loss.detach()) - float(tb['point_loss_cls'] + tb['point_loss_part'])) <= 1e-6 * abs(float(loss.detach()))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    head.eval()
    head(batch)
    assert 'point_cls_labels' not in head.forward_ret_dict


def test_a_box_coder_in_the_config_raises():
    from pcdet.models.dense_heads import PointIntraPartOffsetHead
    with pytest.raises(NotImplementedError):
        PointIntraPartOffsetHead(num_class=3, input_channels=16,
                                 model_cfg=head_cfg(BOX_CODER='PointResidualCoder', BOX_CODER_CONFIG={'use_mean_size': False}))


def test_the_other_target_modes_of_the_template_are_as_before():
    """ret_part_labels opens the new mode; ret_box_labels and the ball constraint still raise, as they did"""
    from pcdet.models.dense_heads import PointIntraPartOffsetHead
    head = PointIntraPartOffsetHead(num_class=3, input_channels=16, model_cfg=head_cfg())
    pts, gt = torch.zeros((4, 4)), torch.zeros((1, 2, 8))
    for kw in ({'ret_box_labels': True}, {'use_ball_constraint': True, 'set_ignore_flag': False},
               {'ret_part_labels': True, 'ret_box_labels': True}):
        with pytest.raises(AssertionError):
            head.assign_stack_targets(pts, gt, extend_gt_boxes=gt, **kw)


# ---- UNetV2 ---------------------------------------------------------------------------------------------------------------------
def test_unetv2_state_dict_keys_are_the_reference_s():
    from pcdet.models import backbones_3d
    g = dict(np.load(os.path.join(os.path.dirname(GOLD), 'ref_unetv2.npz')))
    m = backbones_3d.__all__['UNetV2'](EasyDict({'NAME': 'UNetV2'}), 4, np.array(cases.UNET_GRID), cases.UNET_VOXEL, cases.UNET_PCR)
    sd = m.state_dict()
    assert sorted(sd) == list(g['keys']) and [str(tuple(v.shape)) for _, v in sorted(sd.items())] == list(g['shapes'])
    assert m.num_point_features == 16 and m.sparse_shape == [25, 32, 32]
    assert not any(k.endswith('conv1.bias') or k.endswith('conv2.bias') for k in sd)          # the lateral blocks are bias-free
    m = backbones_3d.__all__['UNetV2'](EasyDict({'NAME': 'UNetV2', 'RETURN_ENCODED_TENSOR': False}), 4, np.array(cases.UNET_GRID),
                                       cases.UNET_VOXEL, cases.UNET_PCR)
    assert m.conv_out is None and not any(k.startswith('conv_out') for k in m.state_dict())


def test_channel_reduction_adds_adjacent_channels():
    """of a concatenation [bottom, lateral] of 2 x 3 channels reduced to 3: (b0 + b1, b2 + l0, l1 + l2), not bottom + lateral"""
    from pcdet.models.backbones_3d import UNetV2
    from spconv.pytorch import SparseConvTensor
    feats = torch.tensor([[1.0, 2.0, 4.0, 8.0, 16.0, 32.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]])
    x = SparseConvTensor(feats, torch.zeros((2, 4), dtype=torch.int32), [1, 1, 2], 1)
    out = UNetV2.channel_reduction(x, 3)
    assert out.features.tolist() == [[3.0, 12.0, 48.0], [2.0, 2.0, 2.0]]
    assert out.indices is x.indices or torch.equal(out.indices, x.indices)
