"""CPU: the centre head of CenterPoint on the torch route (crbhip.center_head.*_torch, CenterHead, centerpoint_cfg) against the
golden written by the reference's own CenterHead / centernet_utils / loss_utils (tests/golden/ref_centerpoint.npz) and the f64
definition of tests/center_cases.py. Also home of the runners and checks that tests/test_centerpoint_gpu.py and
tools/center_head_host_check.py apply to the kernels.

Bars (FACTOR = 4, the factor of the project's detector tests; e_ref = the reference's own f32 error recorded in the golden):
  targets   inds, masks, the cells with heatmap == 1 and the zero / non-zero pattern equal; every heatmap value within 1 f32 ulp (both
            sides round an f64 exp that is good to 1 ulp of f64); target_boxes: copied columns (z, extras) bit-equal, every other column
            within FACTOR * its e_ref of the f64 definition, bit-equal to the reference where e_ref is 0. All slots are compared.
  loss      forward within FACTOR * e_ref of the reference's f64 values; gradients within FACTOR * e_ref of the torch route in f64 (which
            equals the reference's f64 gradients where the golden holds them); exactly zero at the planted out-of-clamp logits.
  decode    classes and masks equal, boxes and scores within FACTOR * e_ref of the reference's f64, all K rows of every frame."""
import functools
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import center_cases as cases

FACTOR = 4.0
CPU = torch.device('cpu')


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(cases.GOLDEN)


@functools.lru_cache(maxsize=None)
def targets_case(name):
    case = cases.make_targets_case(name)
    return case, cases.targets_f64(case['gt_boxes'], case['heads'], case['nmax'])


@functools.lru_cache(maxsize=None)
def loss_case(name, h):
    return cases.make_loss_case(name, h)


@functools.lru_cache(maxsize=None)
def decode_case(name):
    return cases.make_decode_case(name)


class quiet(warnings.catch_warnings):
    """host or f64 tensors say that they take the torch route"""
    def __enter__(self):
        r = super().__enter__()
        warnings.filterwarnings('ignore', message='.*torch route.*')
        return r


# ---- runners ----------------------------------------------------------------------------------------------------------------
def run_targets(case, dev=CPU, gt=None, dtype=torch.float32):
    from crbhip import center_head as ch
    gt = torch.from_numpy(case['gt_boxes'] if gt is None else gt).to(dev).to(dtype)
    before = gt.clone()
    res = ch.assign_targets(gt, *cases.class_tables(case['heads']), cases.H, cases.W, cases.PCR, cases.VOXEL, cases.STRIDE, case['nmax'],
                            cases.OVERLAP, cases.MIN_RADIUS)
    assert torch.equal(torch.nan_to_num(gt), torch.nan_to_num(before)), 'gt_boxes written'
    return [{k: v.cpu().numpy() for k, v in zip(('heatmap', 'target_boxes', 'inds', 'masks'), r)} for r in res]


def check_targets(res, name):
    case, d = targets_case(name)
    g, bad = gold(), []
    for h, r in enumerate(res):
        tag = 'targets_%s_%d' % (name, h)
        for k in ('inds', 'masks'):
            if r[k].dtype != np.int64 or not np.array_equal(r[k], g['%s_%s' % (tag, k)]):
                bad.append('%s %s' % (tag, k))
        ref = g[tag + '_heatmap']
        if r['heatmap'].shape != ref.shape or not np.array_equal(r['heatmap'] == 1, ref == 1) or not np.array_equal(r['heatmap'] != 0, ref != 0):
            bad.append(tag + ' heatmap pattern')
            continue
        ulps = (np.abs(r['heatmap'].astype(np.float64) - ref.astype(np.float64)) / cases.ulp_f32(ref)).max()
        tb, ref_tb, e_ref = r['target_boxes'], g[tag + '_target_boxes'], g[tag + '_e_ref']
        err = np.abs(tb.astype(np.float64) - d[h]['target_boxes']).reshape(-1, tb.shape[-1]).max(0)
        print('%-22s objects %s, peaks %d, heatmap within %.2f ulp; target_boxes err / e_ref per column %s' % (
            tag, r['masks'].sum(1).tolist(), int((ref == 1).sum()), ulps, np.array2string(err / np.maximum(e_ref, 1e-30), precision=2)))
        if not ulps <= 1:
            bad.append(tag + ' heatmap values')
        for c in range(tb.shape[-1]):
            if c == 2 or c >= 8 or e_ref[c] == 0:
                if not np.array_equal(tb[..., c], ref_tb[..., c]):
                    bad.append('%s column %d not bit-equal' % (tag, c))
            elif not err[c] <= FACTOR * e_ref[c]:
                bad.append('%s column %d' % (tag, c))
    return bad


def _maps(case, dev, dtype, channels_last):
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    t = lambda a: torch.from_numpy(a).to(dev).to(dtype).contiguous(memory_format=fmt).requires_grad_(True)
    return t(case['hm']), [t(case['reg'][n]) for n in case['order']]


def run_loss(case, dev=CPU, dtype=torch.float32, channels_last=False):
    """-> {'loss' (2) f64, 'g_hm' (B,C,H,W), 'g_reg' (B,D,H,W)} numpy"""
    from crbhip import center_head as ch
    hm, reg = _maps(case, dev, dtype, channels_last)
    t = lambda a: torch.from_numpy(a).to(dev)
    loss = ch.center_loss(hm, t(case['heatmap']).to(dtype), reg, t(case['target_boxes']).to(dtype), t(case['inds']), t(case['masks']),
                          **cases.LOSS_WEIGHTS)
    assert loss.shape == (2,)
    (loss[0] + loss[1]).backward()
    return {'loss': loss.detach().double().cpu().numpy(), 'g_hm': hm.grad.cpu().numpy(), 'g_reg': torch.cat([r.grad for r in reg], 1).cpu().numpy()}


def check_loss(res, ref64, name, h):
    """res: the route under test; ref64: the torch route in f64 on the same device"""
    g, tag, bad = gold(), 'loss_%s_%d' % (name, h), []
    case = loss_case(name, h)
    err, e_ref = np.abs(res['loss'] - g[tag + '_f64']), g[tag + '_e_ref']
    print('%-20s loss %s err %s e_ref %s' % (tag, res['loss'], err, e_ref))
    if not (err <= FACTOR * e_ref).all():
        bad.append(tag + ' forward')
    for k in ('g_hm', 'g_reg'):
        e, bar = np.abs(res[k].astype(np.float64) - ref64[k]).max(), g['%s_e_ref_%s' % (tag, k)][0]
        print('%-20s %-5s err %.3g e_ref %.3g on values up to %.3g' % (tag, k, e, bar, np.abs(ref64[k]).max()))
        if res[k].dtype != np.float32 or not e <= FACTOR * bar:
            bad.append('%s %s' % (tag, k))
    if not (res['g_hm'][case['planted']] == 0).all():
        bad.append(tag + ' gradient at the out-of-clamp logits')
    if int((res['g_reg'] != 0).sum()) != int(g[tag + '_g_reg_nonzero'][0]):
        bad.append(tag + ' cells with a regression gradient')
    return bad


def run_decode(case, dev=CPU, dtype=torch.float32, channels_last=False):
    from crbhip import center_head as ch
    hm, reg = _maps(case, dev, dtype, channels_last)
    boxes, scores, labels, keep = ch.decode(hm, reg, cases.DECODE_K, cases.PCR, cases.VOXEL, cases.STRIDE, cases.DECODE_LIMIT, cases.SCORE_THRESH)
    return {'boxes': boxes.cpu().numpy(), 'scores': scores.cpu().numpy(), 'labels': labels.cpu().numpy(), 'keep': keep.cpu().numpy()}


def check_decode(res, name):
    g, tag, bad = gold(), 'decode_' + name, []
    if res['boxes'].shape != g[tag + '_boxes_f64'].shape or res['scores'].shape != (cases.B, cases.DECODE_K):
        return [tag + ' shapes']
    if not np.array_equal(res['labels'], g[tag + '_labels']) or res['keep'].dtype != np.bool_ or not np.array_equal(res['keep'], g[tag + '_keep']):
        bad.append(tag + ' classes / masks')
    err = np.abs(res['boxes'].astype(np.float64) - g[tag + '_boxes_f64']).reshape(-1, res['boxes'].shape[-1]).max(0)
    e_s = np.abs(res['scores'].astype(np.float64) - g[tag + '_scores_f64']).max()
    print('%-14s kept %s of %d; boxes err / e_ref %s; scores err %.3g e_ref %.3g' % (
        tag, res['keep'].sum(1).tolist(), cases.DECODE_K, np.array2string(err / np.maximum(g[tag + '_e_ref_boxes'], 1e-30), precision=2), e_s,
        g[tag + '_e_ref_scores'][0]))
    if not (err <= FACTOR * g[tag + '_e_ref_boxes']).all():
        bad.append(tag + ' boxes')
    if not e_s <= FACTOR * g[tag + '_e_ref_scores'][0]:
        bad.append(tag + ' scores')
    return bad


LOSS_HEADS = [(n, h) for n in cases.LOSS_CASES for h in range(len(cases.TARGET_CASES[n][0]))]


# ---- tests ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.TARGET_CASES))
def test_targets_torch_route(name):
    case, _ = targets_case(name)
    with quiet():
        assert not check_targets(run_targets(case), name)


def test_case_margins_and_contents():
    """a guard on tests/center_cases.py itself (it passes without the feature)"""
    for name in cases.TARGET_CASES:
        case, d = targets_case(name)
        for box in case['gt_boxes'].reshape(-1, case['gt_boxes'].shape[-1]):
            assert box[-1] == 0 or box[3] <= 0 or cases.has_margin(box)
        assert not case['gt_boxes'][:, -2:].any(), 'trailing all-zero rows'
    _, d = targets_case('overflow')
    assert d[0]['masks'].sum(1).tolist() == [4, 3]
    _, d = targets_case('empty_head')
    assert d[0]['masks'].sum() == 0 and not d[0]['heatmap'].any()
    case, d = targets_case('edges')
    assert (case['gt_boxes'][1, 0, 3] == 0) and d[0]['masks'][1, 0] == 0 and d[0]['masks'][1, 1] == 1      # dx = 0 keeps its slot
    assert d[0]['inds'][0, 0] == cases.H * cases.W - 1 and d[1]['inds'][0, 0] == cases.H * cases.W - 1     # last cell; clamped
    assert d[1]['inds'][1, 0] == d[1]['inds'][1, 1] and d[1]['masks'][1, :2].all()                          # two boxes in one cell


@pytest.mark.parametrize('name,h', LOSS_HEADS)
def test_loss_torch_route(name, h):
    case = loss_case(name, h)
    with quiet():
        ref64 = run_loss(case, dtype=torch.float64)
        res = run_loss(case)
    g, tag = gold(), 'loss_%s_%d' % (name, h)
    # the f64 torch route is the reference's f64: loss, the stored rows of the hm gradient, the regression gradient at the objects' cells
    assert np.abs(ref64['loss'] - g[tag + '_f64']).max() <= 1e-10 * max(1.0, np.abs(g[tag + '_f64']).max())
    rows = g[tag + '_g_hm_rows_f64']
    assert np.abs(ref64['g_hm'][:, :, :rows.shape[2]] - rows).max() <= 1e-13
    flat = ref64['g_reg'].reshape(cases.B, ref64['g_reg'].shape[1], -1)
    at = np.stack([flat[b][:, case['inds'][b]].T for b in range(cases.B)])
    assert np.abs(at - g[tag + '_g_reg_at_inds_f64']).max() <= 1e-13
    assert not check_loss(res, ref64, name, h)


def test_empty_head_gives_the_undivided_negative_loss():
    case = loss_case('empty_head', 0)
    assert not (case['heatmap'] == 1).any() and not case['masks'].any()
    with quiet():
        res = run_loss(case, dtype=torch.float64)
    x = case['hm'].astype(np.float64)
    p = np.clip(1 / (1 + np.exp(-x)), 1e-4, 1 - 1e-4)
    neg = (np.log(1 - p) * p ** 2 * (1 - case['heatmap'].astype(np.float64)) ** 4).sum()
    assert abs(res['loss'][0] + neg) <= 1e-10 * abs(neg) and res['loss'][1] == 0


@pytest.mark.parametrize('name', list(cases.DECODE_CASES))
@pytest.mark.parametrize('channels_last', [False, True])
def test_decode_torch_route(name, channels_last):
    with quiet():
        assert not check_decode(run_decode(decode_case(name), channels_last=channels_last), name)


def make_head(heads, channels=32, order=None, dev=CPU, nmax=20, **post):
    from pcdet.config import EasyDict
    from pcdet.model_cfgs import centerpoint_cfg
    from pcdet.models.dense_heads import CenterHead
    cfg = centerpoint_cfg('kitti').MODEL.DENSE_HEAD
    cfg.CLASS_NAMES_EACH_HEAD = heads
    cfg.TARGET_ASSIGNER_CONFIG.NUM_MAX_OBJS = nmax
    if order is not None:
        cfg.SEPARATE_HEAD_CFG.HEAD_ORDER = order
        cfg.SEPARATE_HEAD_CFG.HEAD_DICT = EasyDict({n: {'out_channels': cases.REG_CHANNELS[n], 'num_conv': 2} for n in order})
    cfg.POST_PROCESSING.update(post)
    torch.manual_seed(3)
    return CenterHead(cfg, channels, 3, cases.CLASSES, np.array([cases.W * 8, cases.H * 8, 40]), cases.PCR, cases.VOXEL,
                      predict_boxes_when_training=False).to(dev)


@pytest.mark.parametrize('tag,heads', [('one', cases.ONE_HEAD), ('two', cases.TWO_HEADS)])
def test_state_dict_keys_and_shapes(tag, heads):
    g = gold()
    sd = make_head(heads).state_dict()
    assert list(sd.keys()) == g['head_%s_keys' % tag].tolist()
    assert [list(v.shape) for v in sd.values()] == [json.loads(s) for s in g['head_%s_shapes' % tag]]


def test_initialisation_is_the_reference_one():
    head = make_head(cases.TWO_HEADS)
    for sep in head.heads_list:
        assert (sep.hm[-1].bias == -2.19).all()
        for n in cases.HEAD_ORDER:
            for m in getattr(sep, n).modules():
                if isinstance(m, torch.nn.Conv2d):
                    assert not m.bias.any() and 0.5 < float(m.weight.detach().std()) / (2.0 / (m.in_channels * 9)) ** 0.5 < 1.5   # Kaiming, fan_in


def test_waymo_cfg_equals_the_yaml():
    from pcdet.model_cfgs import centerpoint_cfg
    y = json.loads(str(gold()['cfg_json']))
    c = json.loads(json.dumps(centerpoint_cfg('waymo')))
    assert c['CLASS_NAMES'] == y['CLASS_NAMES'] and c['MODEL'] == y['MODEL'] and c['OPTIMIZATION'] == y['OPTIMIZATION']
    k = centerpoint_cfg('kitti')
    assert k.CLASS_NAMES == cases.CLASSES and k.MODEL.DENSE_HEAD.CLASS_NAMES_EACH_HEAD == [cases.CLASSES]
    assert k.MODEL.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE == [0, -40, -3, 70.4, 40, 1]
    for key in ('VFE', 'BACKBONE_3D', 'MAP_TO_BEV', 'BACKBONE_2D'):
        assert k.MODEL[key] == centerpoint_cfg('waymo').MODEL[key]


def _head_batch(dev=CPU, channels=32):
    case, _ = targets_case('two_heads')
    x = torch.from_numpy(np.random.default_rng(8).normal(0, 1, (cases.B, channels, cases.H, cases.W)).astype(np.float32)).to(dev)
    return {'spatial_features_2d': x, 'gt_boxes': torch.from_numpy(case['gt_boxes']).to(dev), 'batch_size': cases.B}


def test_head_training_step_leaves_gt_boxes_and_logits_alone():
    head = make_head(cases.TWO_HEADS).train()
    bd = _head_batch()
    before = bd['gt_boxes'].clone()
    with quiet():
        head(bd)
        logits = [p['hm'].detach().clone() for p in head.forward_ret_dict['pred_dicts']]
        loss, tb = head.get_loss()
    loss.backward()
    assert torch.equal(bd['gt_boxes'], before)
    assert all(torch.equal(p['hm'], l) for p, l in zip(head.forward_ret_dict['pred_dicts'], logits))
    assert sorted(tb) == ['hm_loss_head_0', 'hm_loss_head_1', 'loc_loss_head_0', 'loc_loss_head_1', 'rpn_loss']
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values()) and torch.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    t = head.forward_ret_dict['target_dicts']
    assert [int(m.sum()) for m in t['masks']] == [5, 10]


def test_fused_first_layers_equal_the_separate_modules():
    from pcdet.models.dense_heads import center_head as mod
    head = make_head(cases.ONE_HEAD).eval()
    x = _head_batch()['spatial_features_2d']
    with torch.no_grad():
        fused = head.heads_list[0](head.shared_conv(x))
        mod.FUSED_HEAD_CONVS = False
        try:
            plain = head.heads_list[0](head.shared_conv(x))
        finally:
            mod.FUSED_HEAD_CONVS = True
    for k in plain:
        assert fused[k].shape == plain[k].shape and (fused[k] - plain[k]).abs().max() <= 1e-5 * plain[k].abs().max(), k


def test_unsupported_settings_raise():
    with pytest.raises(NotImplementedError):
        make_head(cases.ONE_HEAD, NMS_CONFIG={'NMS_TYPE': 'circle_nms', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500})
    from pcdet.model_cfgs import centerpoint_cfg
    from pcdet.models.dense_heads import CenterHead
    with pytest.raises(NotImplementedError):
        CenterHead(centerpoint_cfg('kitti').MODEL.DENSE_HEAD, 32, 3, cases.CLASSES, None, cases.PCR, cases.VOXEL, predict_boxes_when_training=True)


def test_checkpoint_round_trip(tmp_path):
    a, b = make_head(cases.TWO_HEADS), make_head(cases.TWO_HEADS)
    with torch.no_grad():
        for p in a.parameters():
            p.add_(0.25)
    path = os.path.join(str(tmp_path), 'head.pth')
    torch.save({'model_state': a.state_dict()}, path)
    b.load_state_dict(torch.load(path)['model_state'])
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    a.eval(), b.eval()
    bd = _head_batch()
    with torch.no_grad(), quiet():
        pa, pb = a(dict(bd))['center_preds'], b(dict(bd))['center_preds']
    assert all(torch.equal(x[k], y[k]) for x, y in zip(pa, pb) for k in x)


def test_detector_is_registered():
    from pcdet.models.detectors import __all__ as detectors
    from pcdet.models.dense_heads import __all__ as heads
    assert 'CenterPoint' in detectors and 'CenterHead' in heads


def test_class_names_of_with_and_without_anchors():
    """post_processing.class_names_of: the anchor list where the dense head has one (dict-style and attribute-style configs), the
    detector's own class list for an anchor-free head"""
    from types import SimpleNamespace as NS
    from pcdet.config import EasyDict
    from pcdet.model_cfgs import centerpoint_cfg, second_cfg
    from pcdet.models.detectors.post_processing import class_names_of
    assert class_names_of(NS(model_cfg=second_cfg('kitti').MODEL, class_names=['x'])) == cases.CLASSES
    anchors = [{'class_name': 'Car'}, {'class_name': 'Cyclist'}]
    assert class_names_of(NS(model_cfg=NS(DENSE_HEAD=NS(ANCHOR_GENERATOR_CONFIG=anchors)))) == ['Car', 'Cyclist']
    assert class_names_of(NS(model_cfg=EasyDict({'DENSE_HEAD': {'ANCHOR_GENERATOR_CONFIG': anchors}}))) == ['Car', 'Cyclist']
    assert class_names_of(NS(model_cfg=centerpoint_cfg('kitti').MODEL, class_names=cases.CLASSES)) == cases.CLASSES

