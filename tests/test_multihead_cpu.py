"""CPU: AnchorHeadMulti / SingleHead, the multi-head target assignment, the torch restatement of the multi-head losses and the cases
of the per-class selection against the reference's recorded run (tests/golden/ref_multihead.npz, written by
tests/golden/make_goldens_multihead.py from the inputs of tests/multihead_cases.py).

Bars (FACTOR = 4, the factor of tests/test_centerpoint_cpu.py; e_ref = the reference's own f32 error recorded in the golden):
  targets   labels equal; regression targets within FACTOR * e_ref per column of the reference's f32 values (bit-equal where e_ref is 0)
  forward   every head output within FACTOR * e_ref of the reference's f64 rows
  loss      the torch route in f64 reproduces the reference's f64 values and gradient rows (1e-9: the same formulas in the same
            precision); in f32 the three values are within FACTOR * e_rel * |value| (e_rel: the reference's relative f32 error, largest over
            the cases; make_goldens_multihead.gen_loss says why it is relative) and the gradients within FACTOR * e_ref of the f64 run
  select    the margins of every selection case hold, and the definition's candidates per (frame, head) are the golden's"""
import json
import warnings

import numpy as np
import pytest
import torch

import multihead_cases as cases

FACTOR = 4.0


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def t_(a, dev=None, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype)


# ---- head --------------------------------------------------------------------------------------------------------------------
HEAD_CONFIGS = {'three': dict(layout='three'), 'two_all': dict(layout='two', separate=False), 'sep_reg': dict(layout='two', sep_reg=True),
                'layers': dict(layout='three', head_layers=True, use_dir=False), 'no_shared': dict(layout='one', shared=None)}


@pytest.mark.parametrize('tag', list(HEAD_CONFIGS))
def test_reference_state_dict_round_trips(gold, tag):
    """the reference's parameter names and shapes are this head's: a state_dict with the reference's keys loads strictly"""
    from golden._constants import seeded_state
    head = cases.make_head(**HEAD_CONFIGS[tag])
    sd = head.state_dict()
    keys, shapes = gold['head_%s_keys' % tag].tolist(), [tuple(json.loads(s)) for s in gold['head_%s_shapes' % tag].tolist()]
    assert sorted(sd) == sorted(keys)
    assert all(tuple(sd[k].shape) == s for k, s in zip(keys, shapes))
    ref_like = {k: v for k, v in seeded_state(head, 5).items()}
    head.load_state_dict({k: ref_like[k] for k in keys}, strict=True)
    now = head.state_dict()
    assert all(torch.equal(now[k], ref_like[k].to(now[k].dtype)) for k in keys)


def test_initialisation_and_registration():
    from pcdet.models import dense_heads
    assert dense_heads.__all__['AnchorHeadMulti'] is dense_heads.AnchorHeadMulti
    head = cases.make_head('two', sep_reg=True)
    prior = -np.log(99.0)
    for h in head.rpn_heads:
        assert isinstance(h, dense_heads.SingleHead) and isinstance(h.conv_cls, torch.nn.Sequential)
        assert torch.allclose(h.conv_cls[-1].bias, torch.full_like(h.conv_cls[-1].bias, prior))
        for tower in h.conv_box.values():                                 # kaiming_normal_(fan_out, relu), zero bias
            w = tower[-1].weight
            assert float(tower[-1].bias.abs().max()) == 0 and abs(float(w.std()) / np.sqrt(2.0 / (w.shape[0] * 9)) - 1) < 0.25
        assert list(h.conv_box) == ['conv_reg', 'conv_height', 'conv_size', 'conv_angle']
    head = cases.make_head('two')
    assert [h.num_class for h in head.rpn_heads] == [1, 2] and [h.num_anchors_per_location for h in head.rpn_heads] == [2, 4]
    assert [h.head_label_indices.tolist() for h in head.rpn_heads] == [[1], [2, 3]]
    assert all(torch.allclose(h.conv_cls.bias, torch.full_like(h.conv_cls.bias, prior)) for h in head.rpn_heads)
    assert [h.num_class for h in cases.make_head('two', separate=False).rpn_heads] == [3, 3]
    assert head._class_starts() == [0, 1] and head.head_anchor_ranges() == [(0, 546), (546, 1092)]


@pytest.mark.parametrize('tag', list(cases.FORWARD_CASES))
def test_forward_against_the_reference(gold, tag):
    from golden._constants import seeded_state
    head = cases.make_head(**cases.FORWARD_CASES[tag])
    head.load_state_dict(seeded_state(head, cases.FORWARD_SEED))
    bd = head({'spatial_features_2d': t_(cases.forward_input()), 'batch_size': cases.B, 'gt_boxes': t_(cases.make_gt('mixed'))})
    assert 'batch_cls_preds' not in bd                                    # one stage: nothing is decoded while training
    fr = head.forward_ret_dict
    for k in ('cls_preds', 'box_preds', 'dir_cls_preds'):
        if 'fwd_%s_%s_0_f64' % (tag, k) not in gold.files:
            assert k not in fr
            continue
        outs = fr[k] if isinstance(fr[k], list) else [fr[k]]
        assert isinstance(fr[k], list) == cases.FORWARD_CASES[tag].get('separate', True)
        for h, o in enumerate(outs):
            ref, e_ref = gold['fwd_%s_%s_%d_f64' % (tag, k, h)], gold['fwd_%s_%s_%d_e_ref' % (tag, k, h)][0]
            assert list(o.shape) == gold['fwd_%s_%s_%d_shape' % (tag, k, h)].tolist()
            err = np.abs(o.detach().numpy()[:, ::cases.FORWARD_ROWS].astype(np.float64) - ref).max()
            print('%s %s head %d: error %.3g, e_ref %.3g' % (tag, k, h, err, e_ref))
            assert err <= FACTOR * e_ref


def test_eval_forward_decodes_in_the_multihead_order():
    head = cases.make_head('two').eval()
    with torch.no_grad():
        bd = head({'spatial_features_2d': t_(cases.forward_input()), 'batch_size': cases.B})
    assert [tuple(c.shape) for c in bd['batch_cls_preds']] == [(3, 546, 1), (3, 1092, 2)] and bd['cls_preds_normalized'] is False
    assert [m.tolist() for m in bd['multihead_label_mapping']] == [[1], [2, 3]] and bd['batch_box_preds'].shape == (3, 1638, 7)
    idx = torch.from_numpy(np.random.RandomState(0).randint(0, 1092, (3, 9)))
    picked = bd['multihead_box_decoder'](1, idx)
    assert torch.equal(picked, torch.gather(bd['batch_box_preds'][:, 546:], 1, idx[..., None].expand(-1, -1, 7)))


# ---- targets -----------------------------------------------------------------------------------------------------------------
def check_targets(gold, name, out):
    labels, reg = out['box_cls_labels'].cpu().numpy(), out['box_reg_targets'].cpu().numpy()
    assert labels.dtype == np.int32 and np.array_equal(labels, gold['targets_%s_labels' % name].astype(np.int32))
    err = np.abs(reg.astype(np.float64) - gold['targets_%s_reg' % name].astype(np.float64)).reshape(-1, 7).max(0)
    print('%s: regression target error per column %s, e_ref %s' % (name, err, gold['targets_%s_e_ref' % name]))
    assert (err <= FACTOR * gold['targets_%s_e_ref' % name]).all()
    assert np.array_equal(out['reg_weights'].cpu().numpy(), (labels > 0).astype(np.float32))


@pytest.mark.parametrize('name', list(cases.GT_CASES))
def test_targets_against_the_reference(gold, name):
    head = cases.make_head('two', grid=cases.GT_CASES[name][0])
    out = head.assign_targets(t_(cases.make_gt(name)))
    check_targets(gold, name, out)
    labels = out['box_cls_labels'].numpy()
    assert (labels[-1] == 0).all()                                        # the frame without ground truth
    if name == 'noclass2':
        assert (labels[:, 546:1092] == 0).all()                           # the class without ground truth
    if name == 'mixed':
        # the class ids behind the last non-zero row of frame 1 are no boxes: the same frame with those rows cleared
        gt = np.array(cases.make_gt(name))
        gt[1, -2:, 7] = 0
        again = head.assign_targets(t_(gt))
        assert all(torch.equal(out[k], again[k]) for k in out)


def test_multihead_order_is_a_permutation_of_the_single_head_order():
    import anchor_head_cases as ahc
    single, _, _ = ahc.make_head(3, grid=cases.GRID)
    multi = cases.make_head('three')
    gt = t_(cases.make_gt('mixed'))
    s, m = single.assign_targets(gt), multi.assign_targets(gt)
    ny, nx = cases.GRID
    for k, tail in (('box_cls_labels', ()), ('box_reg_targets', (7,)), ('reg_weights', ())):
        a = s[k].view(cases.B, ny, nx, 3, 2, *tail).permute(0, 3, 4, 1, 2, *range(5, 5 + len(tail)))       # (B, class, rot, y, x)
        assert torch.equal(a.reshape(m[k].shape), m[k]), k


def test_sampling_and_height_matching_keep_raising():
    from pcdet.config import EasyDict
    from pcdet.models.dense_heads import AnchorHeadMulti
    for key, val in (('POS_FRACTION', 0.3), ('MATCH_HEIGHT', True)):
        cfg = cases.head_cfg('three')
        cfg['TARGET_ASSIGNER_CONFIG'][key] = val
        with pytest.raises(NotImplementedError):
            AnchorHeadMulti(EasyDict(cfg), **cases.head_kwargs(cases.GRID))


# ---- losses ------------------------------------------------------------------------------------------------------------------
def loss_head(case, gold, dev=None, dtype=torch.float32):
    """the head of a loss case with forward_ret_dict as its forward would leave it -> head, leaves {key: [tensor per head]}"""
    layout, separate, use_dir, grid = cases.LOSS_CASES[case]
    head = cases.make_head(layout, grid=grid, separate=separate, use_dir=use_dir)
    if dev is not None:
        head = head.to(dev)
    src = 'targets_tiny' if grid == cases.TINY else 'targets_mixed'
    labels, targets = cases.plant_targets(gold[src + '_labels'], gold[src + '_reg'], grid)
    cls, box, dirs = cases.make_preds(case)
    leaf = lambda arrs: None if arrs is None else [t_(a, dev, dtype).requires_grad_(True) for a in arrs]
    leaves = {'cls': leaf(cls), 'box': leaf(box), 'dir': leaf(dirs)}
    pack = (lambda ts: ts) if separate else (lambda ts: torch.cat(ts, dim=1))
    head.forward_ret_dict = {'cls_preds': pack(leaves['cls']), 'box_preds': pack(leaves['box']), 'box_cls_labels': t_(labels, dev),
                             'box_reg_targets': t_(targets, dev)}
    if dirs is not None:
        head.forward_ret_dict['dir_cls_preds'] = pack(leaves['dir'])
    return head, leaves


def loss_values(tb):
    return np.array([float(tb['rpn_loss_cls']), float(tb['rpn_loss_loc']), float(tb.get('rpn_loss_dir', 0.0))], np.float64)


def check_loss_values(gold, case, vals, what):
    ref = gold['loss_%s_f64' % case]
    err, bar = np.abs(vals - ref), FACTOR * gold['loss_e_ref_rel'] * np.abs(ref)
    print('%s %s: %s, reference f64 %s, error %s, bar %s' % (case, what, vals, ref, err, bar))
    assert (err <= bar).all(), (case, what)


@pytest.mark.parametrize('case', list(cases.LOSS_CASES))
def test_torch_route_against_the_reference(gold, case):
    head, leaves = loss_head(case, gold, dtype=torch.float64)
    loss, tb = head.get_loss()
    loss.backward()
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values())
    ref = gold['loss_%s_f64' % case]
    assert np.abs(loss_values(tb) - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    assert abs(float(tb['rpn_loss']) - ref.sum()) <= 1e-9 * ref.sum()
    g64 = {}
    for key, ts in leaves.items():
        for h, t in enumerate(ts or ()):
            rows = gold['loss_%s_g_%s_%d_rows_f64' % (case, key, h)]
            assert np.abs(t.grad.numpy()[:, ::cases.GRAD_ROWS] - rows).max() <= 1e-10
            g64[(key, h)] = t.grad.numpy()
    # the same route in f32
    head, leaves = loss_head(case, gold)
    loss, tb = head.get_loss()
    loss.backward()
    check_loss_values(gold, case, loss_values(tb), 'torch route f32')
    for (key, h), g in g64.items():
        err, e_ref = np.abs(leaves[key][h].grad.numpy().astype(np.float64) - g).max(), gold['loss_%s_e_ref_g_%s' % (case, key)][0]
        print('  gradient %s head %d: error %.3g, e_ref %.3g' % (key, h, err, e_ref))
        assert err <= FACTOR * e_ref


def test_planted_rows_of_the_loss_cases(gold):
    """what the loss cases plant is there: a positive outside its head's columns, ignored anchors on both head boundaries, NaN targets,
    logits of exactly 0, a frame without positives"""
    labels, targets = cases.plant_targets(gold['targets_mixed_labels'], gold['targets_mixed_reg'], cases.GRID)
    assert labels[0, cases.OUTSIDE_ANCHOR] == 3 and cases.OUTSIDE_ANCHOR < 546
    assert (labels[:, 544:549] == -1).all() and (labels[:, 1091:1094] == -1).all()
    assert np.isnan(targets[labels > 0]).any() and (labels[2] > 0).sum() == 0
    assert all((x == 0).sum() >= 1 for x in cases.make_preds('three_sep_dir')[0])
    # the all-zero target row: with SEPARATE_MULTIHEAD the head of class 1 sees the planted class-3 positive as background
    head, leaves = loss_head('three_sep_dir', gold, dtype=torch.float64)
    head.get_loss()[0].backward()
    x = leaves['cls'][0].detach()[0, cases.OUTSIDE_ANCHOR, 0]
    p = torch.sigmoid(x)
    npos = float((labels[0] > 0).sum())
    d_bg = 0.75 * (2 * p * p * (1 - p) * torch.nn.functional.softplus(x) + p * p * p) / npos / cases.B
    # (1 / npos is an f32 number in the reference, and so in the restatement: half an f32 step, 6e-8, relative)
    assert abs(float(leaves['cls'][0].grad[0, cases.OUTSIDE_ANCHOR, 0]) - float(d_bg)) < 1e-7 * float(d_bg)
    assert float(leaves['box'][0].grad[0, cases.OUTSIDE_ANCHOR].abs().sum()) > 0           # it is a positive of the regression loss


def test_fallback_conditions():
    from pcdet.utils import loss_utils
    head = cases.make_head('two')
    assert head.fused_loss_unsupported() is None
    head.model_cfg.NUM_DIR_BINS = 9
    assert 'direction bins' in head.fused_loss_unsupported()
    head.model_cfg.NUM_DIR_BINS = 2
    head.rpn_heads[1].num_class = 9
    assert 'classes in a head' in head.fused_loss_unsupported()
    head.rpn_heads[1].num_class = 2
    head.box_coder.code_size = 9
    assert 'code size' in head.fused_loss_unsupported()
    head.box_coder.code_size = 7
    head.cls_loss_func = torch.nn.Identity()
    assert 'classification loss' in head.fused_loss_unsupported()
    head.cls_loss_func = loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0)
    head.reg_loss_func = torch.nn.Identity()
    assert 'regression loss' in head.fused_loss_unsupported()


# ---- selection ---------------------------------------------------------------------------------------------------------------
def decoded_boxes(name, dev=None):
    """-> head (eval), the case's tensors, the decoded boxes per head"""
    c, d = cases.SEL_CASES[name], cases.make_selection(name)
    head = cases.make_head(c['layout'], grid=c['grid']).eval()
    if dev is not None:
        head = head.to(dev)
    ts = {k: [t_(a, dev) for a in v] for k, v in d.items()}
    with torch.no_grad():
        _, boxes = head.generate_predicted_boxes(cases.B, ts['cls'], ts['box'], ts['dir'])
    per_head, start = [], 0
    for n, _, _ in cases.head_sizes(c['layout'], True, c['grid']):
        per_head.append(boxes[:, start:start + n])
        start += n
    return head, ts, per_head


@pytest.mark.parametrize('name', list(cases.SEL_CASES))
def test_selection_cases_are_margin_safe(gold, name):
    _, _, per_head = decoded_boxes(name)
    cand = cases.check_selection_margins(name, [b.numpy() for b in per_head])
    sizes = cases.head_sizes(cases.SEL_CASES[name]['layout'], True, cases.SEL_CASES[name]['grid'])
    got = [[sum(len(cand[(b, h, k)]) for k in range(C)) for h, (_, C, _) in enumerate(sizes)] for b in range(cases.B)]
    assert got == gold['sel_%s_candidates' % name].tolist()


def test_selection_cases_cover_the_list(gold):
    c = cases.SEL_CASES
    cand = {n: gold['sel_%s_candidates' % n] for n in c}
    kept = {n: gold['sel_%s_counts' % n] for n in c}
    assert cand['base'][0, 0] == 0 and cand['base'][0, 1] == 1 and (cand['base'][2] == 0).all()        # none, one, a frame with none
    assert c['base']['hot'][0][2] > c['base']['pre'] == 64 and c['two_pre100']['pre'] == 100 and max(c['two_pre100']['hot'][0]) > 100
    assert (kept['post_cut'] % 3 == 0).any() and kept['post_cut'].max() <= 9 and c['post_cut']['post'] == 3
    assert (cand['all_pass'] == np.array([64, 128])).all() and c['all_pass']['thresh'] < 0
    assert c['normal']['nms'] == 'nms_normal_gpu' and (cand['tiny'] <= 12).all()


# ---- configuration and detector ----------------------------------------------------------------------------------------------
def test_second_multihead_cfg_holds_the_yaml_values(gold):
    from pcdet.model_cfgs import second_multihead_cfg
    ref = json.loads(str(gold['cfg_json']))
    cfg = second_multihead_cfg()
    plain = lambda v: {k: plain(x) for k, x in v.items()} if isinstance(v, dict) else ([plain(x) for x in v] if isinstance(v, list) else v)
    assert cfg.CLASS_NAMES == ref['CLASS_NAMES']
    for key in ('NAME', 'VFE', 'BACKBONE_3D', 'MAP_TO_BEV', 'BACKBONE_2D', 'DENSE_HEAD', 'POST_PROCESSING'):
        assert plain(cfg.MODEL[key]) == ref['MODEL'][key], key
    assert plain(cfg.OPTIMIZATION) == ref['OPTIMIZATION']


def test_secondnet_builds_from_the_configuration():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_multihead_cfg
    from pcdet.models import build_network
    cfg = second_multihead_cfg()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2))
    assert type(model).__name__ == 'SECONDNet' and type(model.dense_head).__name__ == 'AnchorHeadMulti'
    assert len(model.dense_head.rpn_heads) == 3 and model.dense_head.head_anchor_ranges() == [(0, 70400), (70400, 70400), (140800, 70400)]
    assert model.backbone_2d.defer_concat is False                       # the concatenated map is written: this head reads it whole
