"""GPU: the Part-A2 point head's kernels (csrc/part_head.hip through crbhip/part_head.py) against the reference's own head
(tests/golden/ref_part_head.npz, written by tests/golden/make_goldens_parta2.py), the points_in_boxes_gpu + crb_point_labels route of
PointHeadSimple, and the torch route in f64 on the device; PointIntraPartOffsetHead as a module on device tensors.

Bars. Labels and owners: equal. Part labels, the two losses and the two gradients: max|fused - f64| <= 4 * e_ref, e_ref = max|reference
f32 - f64| of the same quantity of the same case (golden); where the reference itself is exact (e_ref = 0: the no-positive case's part
quantities) the fused value is too. Every figure is printed as a multiple of e_ref before it is asserted.
Measured on the MI355X (multiples of e_ref, bar 4): part labels 0.35 ... 0.41 (f64, rounded once: half an ulp of 1);
loss_cls 0.05 ... 0.21, loss_part 0.00 ... 0.02 (f64 sums and an f64 result); d_cls 0.91 ... 0.92, d_part 0.66 ... 0.81 (f32 terms, as
the reference's); against the torch route in f64 on the device with upstream gradients 2.5 and -0.5 the same figures."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import part_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_part_head.npz')
W = cases.LOSS_WEIGHTS
LOSS_ARGS = (cases.ALPHA, cases.GAMMA, W['point_cls_weight'], W['point_part_weight'])


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope='module')
def made():
    return {name: cases.make_case(name) for name in cases.CASES}


def _targets(case, dev, gt=None, offsets=True):
    from crbhip import part_head
    assert part_head.FUSED
    off = torch.from_numpy(case['offsets']).to(dev) if offsets else None
    lab, part, owner = part_head.part_targets(torch.from_numpy(case['points']).to(dev),
                                              torch.from_numpy(case['gt_boxes'] if gt is None else gt).to(dev), cases.EXTRA,
                                              case['num_class'], offsets=off)
    torch.cuda.synchronize()
    return lab.cpu().numpy(), part.cpu().numpy(), owner.cpu().numpy()


def _losses(case, labels, part_labels, dev, dtype=torch.float32, route=None, upstream=(1.0, 1.0)):
    """-> dict of numpy arrays: loss_cls, loss_part, pos, d_cls, d_part"""
    from crbhip import part_head
    cls = torch.from_numpy(case['cls_preds']).to(dev, dtype).requires_grad_(True)
    prt = torch.from_numpy(case['part_preds']).to(dev, dtype).requires_grad_(True)
    lc, lp, pos = (route or part_head.part_loss)(cls, prt, torch.from_numpy(labels).to(dev), torch.from_numpy(part_labels).to(dev, dtype),
                                                 *LOSS_ARGS)
    (lc * upstream[0] + lp * upstream[1]).backward()
    torch.cuda.synchronize()
    g_prt = prt.grad if prt.grad is not None else torch.zeros_like(prt)
    return {'loss_cls': lc.detach().cpu().numpy().reshape(1), 'loss_part': lp.detach().cpu().numpy().reshape(1),
            'pos': pos.detach().cpu().numpy().reshape(1), 'd_cls': cls.grad.cpu().numpy(), 'd_part': g_prt.cpu().numpy()}


def _check(tag, got, want, e_ref):
    """prints max|got - want| and its multiple of e_ref -> True when within 4 * e_ref"""
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(want) else 0.0
    print('%-28s err %.3e  e_ref %.3e  multiple %s' % (tag, err, e_ref, ('%.2f' % (err / e_ref)) if e_ref > 0 else ('exact' if err == 0 else 'inf')))
    return err <= 4 * e_ref


@pytest.mark.parametrize('name', list(cases.CASES))
def test_targets_against_the_reference(dev, gold, made, name):
    """ragged frames, an empty frame, a frame without ground truth, 70 rows (two LDS passes), overlapping boxes, num_class 1 and 3,
    no positive at all: labels and owners equal, part labels within 4 * e_ref of the f64 definition; frame offsets handed in or derived"""
    case = made[name]
    lab, part, owner = _targets(case, dev)
    assert lab.dtype == np.int64 and part.dtype == np.float32 and owner.dtype == np.int32 and part.shape == (len(lab), 3)
    assert np.array_equal(lab, gold[name + '_labels'])
    assert np.array_equal(owner, gold[name + '_owner'])
    assert not part[lab <= 0].any()
    assert _check(name + ' part labels', part, gold[name + '_part_f64'], gold[name + '_e_ref_part'][0])
    lab2, part2, owner2 = _targets(case, dev, offsets=False)
    assert lab2.tobytes() == lab.tobytes() and part2.tobytes() == part.tobytes() and owner2.tobytes() == owner.tobytes()
    if name == 'ragged':
        assert (owner[:1337] >= cases.BOX_CHUNK).any()                       # an owner found in the second pass
        shared = gold[name + '_owner'][:1337]
        assert (shared == 0).any() and (shared == 10).any()
    if name == 'one':
        assert set(np.unique(lab)) == {-1, 0, 1}
    if name == 'no_pos':
        assert not (lab > 0).any() and (lab < 0).any()


def _existing_route(points, gt, num_class, dev):
    """points_in_boxes_gpu of the ground truths and of the enlarged ground truths + crb_point_labels, as PointHeadSimple assigns today"""
    from crbhip import lib, check, ptr, cur_stream
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    from pcdet.utils import box_utils
    B = gt.shape[0]
    M = len(points) // B
    pts = torch.from_numpy(points[:, 1:4]).to(dev).reshape(B, M, 3).contiguous()
    g = torch.from_numpy(gt).to(dev)
    large = box_utils.enlarge_box3d(g.view(-1, 8), extra_width=cases.EXTRA).view(B, -1, 8)
    inner = roiaware_pool3d_utils.points_in_boxes_gpu(pts, g[:, :, 0:7].contiguous())
    outer = roiaware_pool3d_utils.points_in_boxes_gpu(pts, large[:, :, 0:7].contiguous())
    labels = torch.empty((B * M,), dtype=torch.int64, device=dev)
    check(lib.crb_point_labels(ptr(inner), ptr(outer), ptr(g), B, M, int(g.shape[1]), 8, num_class, ptr(labels), cur_stream(dev)),
          'crb_point_labels')
    torch.cuda.synchronize()
    return labels.cpu().numpy(), inner.view(-1).cpu().numpy()


@pytest.mark.parametrize('num_class', [1, 3])
def test_labels_equal_the_points_in_boxes_route_on_and_beside_the_faces(dev, num_class):
    """points on the faces of boxes and enlarged boxes and one f32 step to either side: the same labels and owners as the two
    points_in_boxes_gpu queries + crb_point_labels, bit for bit (one containment function, csrc/pt_in_box.h)"""
    points, gt = cases.face_case()
    case = {'points': points, 'gt_boxes': gt, 'num_class': num_class,
            'offsets': np.array([0, len(points) // 2, len(points)], np.int32)}
    lab, _, owner = _targets(case, dev)
    want_lab, want_owner = _existing_route(points, gt, num_class, dev)
    assert np.array_equal(lab, want_lab) and np.array_equal(owner, want_owner)
    assert (lab > 0).sum() > 50 and (lab < 0).sum() > 50 and (lab == 0).sum() > 50      # the faces do separate the three labels


def test_labels_equal_the_points_in_boxes_route_on_a_random_case(dev, made):
    case = made['one']                                                       # (700, 500): pad the shorter frame for the (B,M,3) route
    pad = np.tile(np.array([[1.0, 1e6, 1e6, 1e6]], np.float32), (200, 1))
    points = np.concatenate([case['points'], pad])
    lab, _, owner = _targets(case, dev)
    want_lab, want_owner = _existing_route(points, case['gt_boxes'], 1, dev)
    assert np.array_equal(lab, want_lab[:1200]) and np.array_equal(owner, want_owner[:1200])


@pytest.mark.parametrize('name', list(cases.CASES))
def test_losses_and_gradients_against_the_reference(dev, gold, made, name):
    """one partial tile (no_pos), full + partial (ragged, one), three full + 77 rows (tiles); pos equal, the rest within 4 * e_ref of f64"""
    case = made[name]
    got = _losses(case, gold[name + '_labels'], gold[name + '_part_f32'], dev)
    assert got['pos'][0] == gold[name + '_f64_pos'][0]
    ok = [_check('%s %s' % (name, k), got[k], gold['%s_f64_%s' % (name, k)], gold['%s_e_ref_%s' % (name, k)][0])
          for k in ('loss_cls', 'loss_part', 'd_cls', 'd_part')]
    assert all(ok)
    if name == 'no_pos':
        assert got['pos'][0] == 0 and got['loss_part'][0] == 0 and not got['d_part'].any()


@pytest.mark.parametrize('name', ['ragged', 'tiles'])
def test_gradients_against_the_torch_route_in_f64_on_the_device(dev, gold, made, name):
    """upstream gradients other than one (2.5 and -0.5) through crb_part_loss_backward, against autograd of the torch route in f64;
    the bar scales with the upstream value"""
    from crbhip import part_head
    case = made[name]
    up = (2.5, -0.5)
    got = _losses(case, gold[name + '_labels'], gold[name + '_part_f32'], dev, upstream=up)
    ref = _losses(case, gold[name + '_labels'], gold[name + '_part_f32'], dev, dtype=torch.float64, route=part_head.part_loss_torch, upstream=up)
    assert ref['d_cls'].dtype == np.float64
    ok = [_check('%s %s vs torch f64' % (name, k), got[k], ref[k], gold['%s_e_ref_%s' % (name, k)][0] * abs(u))
          for k, u in (('loss_cls', 1.0), ('loss_part', 1.0), ('d_cls', up[0]), ('d_part', up[1]))]
    assert all(ok)


def test_two_calls_are_bit_equal(dev, gold, made):
    case = made['tiles']
    a, b = _targets(case, dev), _targets(case, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    la = _losses(case, a[0], a[1], dev)
    lb = _losses(case, a[0], a[1], dev)
    assert all(la[k].tobytes() == lb[k].tobytes() for k in la)


def test_a_permutation_of_the_ground_truth_rows_that_keeps_their_order_changes_nothing(dev, made):
    """the zero rows moved in between the real ones (relative order of the real rows kept): same labels, part labels, losses, gradients;
    the owner is the same box at its new index"""
    case = made['ragged']
    gt = case['gt_boxes']
    B, G = gt.shape[:2]
    moved, new_index = np.zeros_like(gt), np.full((B, G), -1, np.int64)
    for b in range(B):
        real = [g for g in range(G) if gt[b, g, 7] > 0]
        slots = sorted(np.random.default_rng(5 + b).permutation(G)[:len(real)].tolist())
        for g, s in zip(real, slots):
            moved[b, s], new_index[b, g] = gt[b, g], s
    assert not np.array_equal(moved, gt)
    lab, part, owner = _targets(case, dev)
    lab2, part2, owner2 = _targets(case, dev, gt=moved)
    assert lab2.tobytes() == lab.tobytes() and part2.tobytes() == part.tobytes()
    frame = case['points'][:, 0].astype(np.int64)
    assert np.array_equal(owner2, np.where(owner >= 0, new_index[frame, np.maximum(owner, 0)], -1))
    la, lb = _losses(case, lab, part, dev), _losses(case, lab2, part2, dev)
    assert all(la[k].tobytes() == lb[k].tobytes() for k in la)


def test_an_empty_batch_and_a_batch_without_ground_truth_rows(dev):
    from crbhip import part_head
    pts = torch.zeros((0, 4), device=dev)
    gt = torch.zeros((2, 3, 8), device=dev)
    lab, part, owner = part_head.part_targets(pts, gt, cases.EXTRA, 3)
    assert lab.shape == (0,) and part.shape == (0, 3) and owner.shape == (0,)
    lc, lp, pos = part_head.part_loss(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev), lab, part, *LOSS_ARGS)
    assert float(lc) == 0 and float(lp) == 0 and float(pos) == 0
    pts = torch.tensor([[0, 5.0, 1.0, -1.0], [1, 6.0, 2.0, -1.0]], device=dev)
    lab, part, owner = part_head.part_targets(pts, torch.zeros((2, 0, 8), device=dev), cases.EXTRA, 3)
    torch.cuda.synchronize()
    assert lab.tolist() == [0, 0] and owner.tolist() == [-1, -1] and not bool(part.any())


def test_part_labels_just_outside_the_unit_interval(dev, gold, made):
    """the containment test lets a point lie 1e-5 outside its box in x / y, so a part label can be a little below 0 or above 1: both
    routes take such labels as they are (the device kernel behind F.binary_cross_entropy would assert on them; neither route calls it)"""
    from crbhip import part_head
    case, name = made['one'], 'one'
    labels, part = gold[name + '_labels'], gold[name + '_part_f32'].copy()
    rows = np.nonzero(labels > 0)[0][:2]
    part[rows[0], 0], part[rows[1], 1] = -1.0073e-05, 1.0000174
    got = _losses(case, labels, part, dev)
    ref = _losses(case, labels, part, dev, dtype=torch.float64, route=part_head.part_loss_torch)
    ok = [_check('outside [0,1] %s' % k, got[k], ref[k], gold['%s_e_ref_%s' % (name, k)][0]) for k in ('loss_cls', 'loss_part', 'd_cls', 'd_part')]
    assert all(ok) and np.isfinite(got['loss_part']).all()


def test_the_head_module_on_the_device(dev, gold, made):
    """PointIntraPartOffsetHead end to end on device tensors (ragged frames): labels equal to the golden, tb_dict against the torch route
    in f64 on the head's own logits, gradients down to every layer, and two steps from the same state bit-equal under
    torch.use_deterministic_algorithms(True). Bar on the two losses: 1e-6 relative - an f32 term carries at most about 8 ulp
    (exp, log1p, a division, five products), the sums are f64 and add nothing to that."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from _constants import EasyDict
    from crbhip import part_head
    from pcdet.models.dense_heads import PointIntraPartOffsetHead, point_head_template
    assert point_head_template.FUSED and part_head.FUSED
    case = made['ragged']
    cfg = EasyDict({'NAME': 'PointIntraPartOffsetHead', 'CLS_FC': [16], 'PART_FC': [16], 'CLASS_AGNOSTIC': False,
                    'TARGET_CONFIG': {'GT_EXTRA_WIDTH': cases.EXTRA},
                    'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': dict(cases.LOSS_WEIGHTS)}})
    torch.manual_seed(0)
    head = PointIntraPartOffsetHead(num_class=3, input_channels=16, model_cfg=cfg).to(dev).train()
    state = {k: v.clone() for k, v in head.state_dict().items()}
    feats = torch.randn(len(case['points']), 16, generator=torch.Generator().manual_seed(1)).to(dev)
    runs = []
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            head.load_state_dict(state)
            head.zero_grad(set_to_none=True)
            out = head({'point_features': feats, 'point_coords': torch.from_numpy(case['points']).to(dev),
                        'gt_boxes': torch.from_numpy(case['gt_boxes']).to(dev), 'batch_size': 3})
            loss, tb = head.get_loss()
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.detach().cpu().numpy(), [p.grad.cpu().numpy() for p in head.parameters()]))
    finally:
        torch.use_deterministic_algorithms(was)
    ret = head.forward_ret_dict
    assert np.array_equal(ret['point_cls_labels'].cpu().numpy(), gold['ragged_labels'])
    assert out['point_cls_scores'].shape == (len(feats),) and out['point_part_offset'].shape == (len(feats), 3)
    assert sorted(tb) == sorted(gold['tb_keys']) and all(v.dim() == 0 and not v.requires_grad for v in tb.values())
    lc, lp, pos = part_head.part_loss_torch(ret['point_cls_preds'].detach().double(), ret['point_part_preds'].detach().double(),
                                            ret['point_cls_labels'], ret['point_part_labels'].double(), *LOSS_ARGS)
    for k, want in (('point_loss_cls', lc), ('point_loss_part', lp), ('point_pos_num', pos)):
        rel = abs(float(tb[k]) - float(want)) / max(abs(float(want)), 1e-30)
        print('head %-16s %.9g  f64 %.9g  relative %.2e' % (k, float(tb[k]), float(want), rel))
        assert rel <= 1e-6
    assert float(tb['point_pos_num']) == gold['ragged_f64_pos'][0]
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in runs[0][1])
    assert runs[0][0].tobytes() == runs[1][0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][1], runs[1][1]))
