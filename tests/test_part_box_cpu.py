"""CPU: the torch routes of the point heads' box branch (crbhip/point_box.py) against the reference's own heads
(tests/golden/ref_part_box.npz), PointResidualCoder, the heads' surfaces and state-dict keys, the config factory and what is refused.

Bars: labels and owners equal (the cases keep every point 1e-4 m off every face); box labels, decoded boxes, losses and gradients of the
f32 torch route within 4 * e_ref of the f64 values (the numpy definitions of tests/part_box_cases.py, which the golden's maker checked
against the reference's f64 run), of the f64 torch route within 1e-12 * max(1, |want|): it is the same expressions."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import part_box_cases as pb  # noqa: E402
import part_cases as cases  # noqa: E402
from _constants import EasyDict  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_part_box.npz')
W = pb.LOSS_WEIGHTS
LOSS_ARGS = (cases.ALPHA, cases.GAMMA, pb.CODE_WEIGHTS, pb.BETA, W['point_cls_weight'], W['point_part_weight'], W['point_box_weight'])


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def coder(num_class=3):
    from pcdet.utils.box_coder_utils import PointResidualCoder
    return PointResidualCoder(use_mean_size=True, mean_size=pb.MEAN_SIZE[:1] if num_class == 1 else pb.MEAN_SIZE)


def head_cfg(name='PointIntraPartOffsetHead', use_mean_size=True, **extra):
    cfg = {'NAME': name, 'CLS_FC': [16], 'REG_FC': [16], 'CLASS_AGNOSTIC': False,
           'TARGET_CONFIG': {'GT_EXTRA_WIDTH': cases.EXTRA, 'BOX_CODER': 'PointResidualCoder',
                             'BOX_CODER_CONFIG': {'use_mean_size': use_mean_size, 'mean_size': pb.MEAN_SIZE}},
           'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss', 'LOSS_WEIGHTS': dict(pb.LOSS_WEIGHTS, code_weights=pb.CODE_WEIGHTS)}}
    if name == 'PointIntraPartOffsetHead':
        cfg['PART_FC'] = [16]
    cfg.update(extra)
    return EasyDict(cfg)


def bar_of(gold, key, dtype, want):
    return 4 * gold[key][0] if dtype == torch.float32 else 1e-12 * max(1.0, float(np.abs(want).max()) if want.size else 1.0)


@pytest.mark.parametrize('name', pb.CASES)
def test_torch_route_of_the_targets_against_the_reference(gold, name):
    from crbhip import point_box
    c = pb.case(name)
    for dtype in (torch.float32, torch.float64):
        lab, owner, box, part = point_box.point_box_targets(torch.from_numpy(c['points']).to(dtype), torch.from_numpy(c['gt_boxes']).to(dtype),
                                                            cases.EXTRA, c['num_class'], coder(c['num_class']))
        assert lab.dtype == torch.int64 and box.dtype == dtype and part.dtype == dtype and owner.dtype == torch.int32
        assert np.array_equal(lab.numpy(), gold[name + '_labels']) and np.array_equal(owner.numpy(), gold[name + '_owner'])
        assert (box.numpy()[c['owner'] < 0] == 0).all()
        for got, want, key in ((box, c['box_labels_f64'], 'box'), (part, c['part_labels_f64'], 'part')):
            err = np.abs(got.double().numpy() - want).max()
            bar = bar_of(gold, '%s_e_ref_%s' % (name, key), dtype, want)
            print(name, dtype, key, 'labels err %.3e bar %.3e' % (err, bar))
            assert err <= bar
    _, _, box, part = point_box.point_box_targets(torch.from_numpy(c['points']), torch.from_numpy(c['gt_boxes']), cases.EXTRA,
                                                  c['num_class'], coder(c['num_class']), with_part=False)
    assert part is None and box.shape == (len(c['points']), 8)


@pytest.mark.parametrize('name', pb.CASES + ('tiles_nan',))
@pytest.mark.parametrize('with_part', [True, False])
def test_torch_route_of_the_losses_against_the_reference(gold, name, with_part):
    from crbhip import point_box
    tag, name = name, name.split('_nan')[0]
    c = pb.case(name)
    labels = torch.from_numpy(gold[name + '_labels'])
    box_labels = gold[name + '_box_f32'].copy()
    if tag != name:
        box_labels[pb.nan_row(c), pb.NAN_CODE] = np.nan
    for dtype in (torch.float32, torch.float64):
        cls = torch.from_numpy(c['cls_preds']).to(dtype).requires_grad_(True)
        prt = torch.from_numpy(c['part_preds']).to(dtype).requires_grad_(True) if with_part else None
        box = torch.from_numpy(c['box_preds']).to(dtype).requires_grad_(True)
        lc, lp, lb, pos = point_box.point_box_loss(cls, prt, box, labels, torch.from_numpy(gold[name + '_part_f32']).to(dtype) if with_part else None,
                                                   torch.from_numpy(box_labels).to(dtype), *LOSS_ARGS)
        (lc + lp + lb).backward()
        got = {'loss_cls': lc, 'loss_box': lb, 'd_cls': cls.grad, 'd_box': box.grad}
        if with_part:
            got.update(loss_part=lp, d_part=prt.grad)
        else:
            assert float(lp) == 0.0
        assert float(pos) == gold[name + '_f64_pos'][0]
        for k, v in got.items():
            src = tag if k in ('loss_box', 'd_box') else name
            want = gold['%s_f64_%s' % (src, k)]
            err = np.abs(v.detach().numpy().astype(np.float64).reshape(want.shape) - want).max()
            bar = bar_of(gold, '%s_e_ref_%s' % (src, k), dtype, want)
            print(tag, dtype, k, 'err %.3e bar %.3e' % (err, bar))
            assert err <= bar, (tag, k)
    if name == 'no_pos':
        assert float(lb.detach()) == 0.0


@pytest.mark.parametrize('name', pb.CASES)
def test_torch_route_of_the_decode_against_the_reference(gold, name):
    from crbhip import point_box
    c = pb.case(name)
    want, _ = pb.decode_f64(c['points'], c['cls_preds'], c['box_preds'], c['mean_size'])
    for dtype in (torch.float32, torch.float64):
        cls, boxes, counts = point_box.point_box_decode(torch.from_numpy(c['points']).to(dtype), torch.from_numpy(c['cls_preds']).to(dtype),
                                                        torch.from_numpy(c['box_preds']).to(dtype), coder(c['num_class']), len(c['counts']))
        assert counts is None and np.array_equal(cls.numpy(), c['cls_preds'].astype(cls.numpy().dtype)) and boxes.shape == want.shape
        err = np.abs(boxes.double().numpy() - want).max()
        bar = bar_of(gold, name + '_e_ref_decode', dtype, want)
        print(name, dtype, 'decode err %.3e bar %.3e' % (err, bar))
        assert err <= bar
    assert np.abs(gold[name + '_decode_f32'].astype(np.float64) - want).max() == gold[name + '_e_ref_decode'][0]


def test_definitions_of_the_cases_match_the_golden(gold):
    for name in pb.CASES:
        c = pb.case(name)
        assert np.array_equal(c['labels'], gold[name + '_labels']) and np.array_equal(c['owner'], gold[name + '_owner'])
        for key, want in (('box', c['box_labels_f64']), ('part', c['part_labels_f64'])):
            assert np.abs(gold['%s_%s_f32' % (name, key)].astype(np.float64) - want).max() == gold['%s_e_ref_%s' % (name, key)][0]
        d = pb.box_loss_f64(c['cls_preds'], c['part_preds'], c['box_preds'], gold[name + '_labels'], gold[name + '_part_f32'],
                            gold[name + '_box_f32'])
        for k in ('loss_cls', 'loss_part', 'loss_box', 'pos', 'd_cls', 'd_part', 'd_box'):
            assert np.array_equal(np.asarray(d[k]).reshape(gold['%s_f64_%s' % (name, k)].shape), gold['%s_f64_%s' % (name, k)]), (name, k)
    assert pb.case('ragged')['counts'] == [1337, 1, 0] and pb.case('tiles')['points'].shape[0] == 3 * cases.LOSS_TILE + 77
    assert float(gold['no_pos_f64_loss_box'][0]) == 0.0 and gold['no_pos_f64_pos'][0] == 0.0
    assert pb.case('one')['num_class'] == 1 and set(np.unique(pb.case('one')['gt_boxes'][..., 7])) == {0.0, 1.0}
    # both smooth-L1 branches are met on the positive rows
    c = pb.case('tiles')
    n = np.abs((c['box_preds'] - gold['tiles_box_f32'])[c['labels'] > 0] * np.asarray(pb.CODE_WEIGHTS))
    assert (n < pb.BETA).mean() > 0.05 and (n > pb.BETA).mean() > 0.5 and np.abs(n - pb.BETA).min() > 0.9 * pb.BETA_MARGIN


def test_the_coder_round_trip_in_both_modes():
    from pcdet.utils.box_coder_utils import PointResidualCoder
    rng = np.random.default_rng(3)
    n = 200
    classes = torch.from_numpy(rng.integers(1, 4, n))
    gt = torch.from_numpy(np.concatenate([rng.uniform(-30, 30, (n, 3)), rng.uniform(0.4, 5, (n, 3)), rng.uniform(-3.1, 3.1, (n, 1)),
                                          rng.normal(0, 1, (n, 2))], 1))
    pts = gt[:, 0:3] + torch.from_numpy(rng.uniform(-2, 2, (n, 3)))
    for kw in ({'use_mean_size': True, 'mean_size': pb.MEAN_SIZE}, {'use_mean_size': False}):
        c = PointResidualCoder(**kw)
        assert c.code_size == 8 and c.use_mean_size == kw['use_mean_size']
        before = gt.clone()
        codes = c.encode_torch(gt, pts, classes)
        assert torch.equal(gt, before) and codes.shape == (n, 10)
        back = c.decode_torch(codes, pts, classes)
        assert back.shape == (n, 9) and (back - gt).abs().max() < 1e-12
    c = PointResidualCoder(use_mean_size=True, mean_size=pb.MEAN_SIZE)
    assert not c.mean_size.is_cuda and c.mean_size.dtype == torch.float32
    with pytest.raises(AssertionError):
        c.encode_torch(gt, pts, classes + 1)                 # a class beyond the mean sizes, as the reference asserts
    flat = PointResidualCoder(use_mean_size=False)
    assert torch.equal(flat.encode_torch(gt, pts)[:, 0:3], gt[:, 0:3] - pts)


def test_head_surfaces_and_state_dict_keys(gold):
    from pcdet.models import dense_heads, detectors
    from pcdet.models.dense_heads import PointHeadBox, PointIntraPartOffsetHead
    assert dense_heads.__all__['PointHeadBox'] is PointHeadBox and detectors.__all__['PointRCNN'].__name__ == 'PointRCNN'
    for cls, tag in ((PointIntraPartOffsetHead, 'head'), (PointHeadBox, 'box_head')):
        head = cls(num_class=3, input_channels=16, model_cfg=head_cfg(cls.__name__))
        sd = head.state_dict()
        assert sorted(sd) == list(gold[tag + '_keys'])
        assert [str(tuple(v.shape)) for _, v in sorted(sd.items())] == list(gold[tag + '_shapes'])
        assert head.box_layers is not None and head.box_coder.code_size == 8
        for name in ('get_box_layer_loss', 'generate_predicted_boxes', 'assign_targets', 'get_loss'):
            assert callable(getattr(head, name))


@pytest.mark.parametrize('name', ['PointIntraPartOffsetHead', 'PointHeadBox'])
def test_use_mean_size_false_still_raises(name):
    from pcdet.models import dense_heads
    with pytest.raises(NotImplementedError, match='use_mean_size'):
        dense_heads.__all__[name](num_class=3, input_channels=16, model_cfg=head_cfg(name, use_mean_size=False))


def test_box_labels_need_a_box_coder():
    """pins behaviour that must survive (it passes without the feature too): a head without a box coder refuses ret_box_labels"""
    from pcdet.models.dense_heads import PointIntraPartOffsetHead
    cfg = head_cfg()
    cfg.TARGET_CONFIG.pop('BOX_CODER')
    cfg.TARGET_CONFIG.pop('BOX_CODER_CONFIG')
    head = PointIntraPartOffsetHead(num_class=3, input_channels=16, model_cfg=cfg)
    assert head.box_layers is None
    pts, gt = torch.zeros((4, 4)), torch.zeros((1, 2, 8))
    for kw in ({'ret_box_labels': True}, {'ret_part_labels': True, 'ret_box_labels': True}):
        with pytest.raises(AssertionError):
            head.assign_stack_targets(pts, gt, extend_gt_boxes=gt, **kw)


@pytest.mark.parametrize('name', ['PointIntraPartOffsetHead', 'PointHeadBox'])
def test_head_host_route_end_to_end(gold, name):
    """scores written, targets assigned in training, the reference's tb_dict keys as detached 0-dim tensors, the stacked proposals of
    the reference, gradients down to box_layers"""
    from pcdet.models import dense_heads
    c = pb.case('ragged')
    part = name == 'PointIntraPartOffsetHead'
    torch.manual_seed(0)
    head = dense_heads.__all__[name](num_class=3, input_channels=16, model_cfg=head_cfg(name), predict_boxes_when_training=True)
    head.train()
    N = len(c['points'])
    batch = {'point_features': torch.randn(N, 16), 'point_coords': torch.from_numpy(c['points']),
             'gt_boxes': torch.from_numpy(c['gt_boxes']), 'batch_size': 3}
    out = head(batch)
    ret = head.forward_ret_dict
    assert torch.equal(out['point_cls_scores'], torch.sigmoid(ret['point_cls_preds']).max(-1)[0])
    assert np.array_equal(ret['point_cls_labels'].numpy(), gold['ragged_labels'])
    assert np.abs(ret['point_box_labels'].double().numpy() - c['box_labels_f64']).max() <= 4 * gold['ragged_e_ref_box'][0]
    assert ret['point_box_preds'].shape == (N, 8) and ('point_part_labels' in ret) == part
    assert out['batch_cls_preds'].shape == (N, 3) and out['batch_box_preds'].shape == (N, 7) and out['cls_preds_normalized'] is False
    assert torch.equal(out['batch_index'], batch['point_coords'][:, 0]) and 'batch_counts' not in out
    # the host route IS the coder's expression on the argmax class: the same bits
    want = head.box_coder.decode_torch(ret['point_box_preds'], batch['point_coords'][:, 1:4], ret['point_cls_preds'].max(dim=-1)[1] + 1)
    assert torch.equal(out['batch_box_preds'], want) and torch.equal(out['batch_cls_preds'], ret['point_cls_preds'])
    loss, tb = head.get_loss()
    keys = [k for k in gold['tb_keys'] if part or k != 'point_loss_part']
    assert sorted(tb) == sorted(keys) and all(v.dim() == 0 and not v.requires_grad for v in tb.values())
    assert float(tb['point_pos_num']) == gold['ragged_f64_pos'][0]
    total = sum(float(tb[k]) for k in keys if k != 'point_pos_num')
    assert abs(float(loss.detach()) - total) <= 1e-6 * abs(total)
    box_alone, tb_box = head.get_box_layer_loss()
    assert abs(float(box_alone.detach()) - float(tb['point_loss_box'])) <= 1e-6 * float(tb['point_loss_box']) and list(tb_box) == ['point_loss_box']
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    assert float(head.box_layers[-1].weight.grad.abs().max()) > 0
    head.eval()
    out = head(dict(batch))
    assert 'point_cls_labels' not in head.forward_ret_dict and out['batch_box_preds'].shape == (N, 7)
    head.predict_boxes_when_training = False
    head.train()
    out = head({k: v for k, v in batch.items() if not k.startswith('batch_') or k == 'batch_size'})
    assert 'batch_box_preds' not in out


def test_pack_stacked_gives_the_dense_layout():
    from crbhip import point_box
    c = pb.case('ragged')
    boxes, _ = pb.decode_f64(c['points'], c['cls_preds'], c['box_preds'], c['mean_size'])
    cls_d, box_d, counts = point_box.pack_stacked(torch.from_numpy(c['points'][:, 0]), torch.from_numpy(c['cls_preds']),
                                                  torch.from_numpy(boxes), 3)
    assert counts.tolist() == c['counts'] and counts.dtype == torch.int32
    assert np.array_equal(cls_d.numpy(), pb.pack_dense(c['counts'], c['cls_preds'], -np.inf))
    assert np.array_equal(box_d.numpy(), pb.pack_dense(c['counts'], boxes, 0.0))


def test_the_config_factory_has_the_yaml_s_values():
    from pcdet.model_cfgs import parta2_free_cfg
    m = parta2_free_cfg().MODEL
    assert m.NAME == 'PointRCNN' and 'BACKBONE_2D' not in m and 'DENSE_HEAD' not in m and 'MAP_TO_BEV' not in m
    assert m.BACKBONE_3D == {'NAME': 'UNetV2', 'RETURN_ENCODED_TENSOR': False}
    p = m.POINT_HEAD
    assert p.NAME == 'PointIntraPartOffsetHead' and p.CLS_FC == p.PART_FC == p.REG_FC == [128, 128] and p.CLASS_AGNOSTIC is False
    assert p.TARGET_CONFIG.BOX_CODER == 'PointResidualCoder' and p.TARGET_CONFIG.BOX_CODER_CONFIG.use_mean_size is True
    assert p.TARGET_CONFIG.BOX_CODER_CONFIG.mean_size == pb.MEAN_SIZE and p.TARGET_CONFIG.GT_EXTRA_WIDTH == [0.2, 0.2, 0.2]
    assert p.LOSS_CONFIG.LOSS_REG == 'WeightedSmoothL1Loss'
    assert p.LOSS_CONFIG.LOSS_WEIGHTS == {'point_cls_weight': 1.0, 'point_box_weight': 1.0, 'point_part_weight': 1.0, 'code_weights': [1.0] * 8}
    r = m.ROI_HEAD
    assert r.NAME == 'PartA2FCHead' and r.DISABLE_PART is True and r.SEG_MASK_SCORE_THRESH == 0.0 and r.DP_RATIO == 0.3
    assert r.NMS_CONFIG.TRAIN.NMS_PRE_MAXSIZE == 9000 and r.NMS_CONFIG.TRAIN.NMS_POST_MAXSIZE == 512 and r.NMS_CONFIG.TRAIN.NMS_THRESH == 0.8
    assert r.NMS_CONFIG.TEST.NMS_PRE_MAXSIZE == 9000 and r.NMS_CONFIG.TEST.NMS_POST_MAXSIZE == 100 and r.NMS_CONFIG.TEST.NMS_THRESH == 0.85
    assert r.ROI_AWARE_POOL == {'POOL_SIZE': 12, 'NUM_FEATURES': 128, 'MAX_POINTS_PER_VOXEL': 128}
    assert m.POST_PROCESSING.NMS_CONFIG.NMS_THRESH == 0.1 and m.POST_PROCESSING.SCORE_THRESH == 0.1
    assert parta2_free_cfg().OPTIMIZATION.LR == 0.003
