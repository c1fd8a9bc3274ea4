"""GPU: the kernels of the point heads' box branch (csrc/point_box.hip through crbhip/point_box.py) against the reference's own heads
(tests/golden/ref_part_box.npz, written by tests/golden/make_goldens_parta2_free.py) and the f64 definitions of
tests/part_box_cases.py; the stacked branch of RoIHeadTemplate.proposal_layer against the reference's.

Bars. Labels, owners and part labels: the bits of crb_part_targets, labels and owners those of the golden. Box labels, decoded boxes,
the three losses and the three gradients: max|fused - f64| <= 4 * e_ref, e_ref = max|reference f32 - f64| of the same quantity of the
same case (golden); where the reference itself is exact (e_ref = 0: the no-positive case's box quantities) the fused value is too.
Every figure is printed as a multiple of e_ref before it is asserted.
Measured on the MI355X (multiples of e_ref, bar 4): box labels 0.49 ... 0.79 and decoded boxes 0.99 ... 1.00 (f64, rounded
once); loss_box 0.05 ... 0.10 (1.38 with the NaN label), d_box 0.63 ... 0.69 (f64 terms); loss_cls 0.05 ... 0.21, d_cls 0.91 ... 0.92, d_part
0.66 ... 0.81 (f32 terms, as the reference's). Proposals: the picks are the golden's (the case keeps every pair
of candidates 1e-4 off NMS_THRESH), scores and logits its bits, boxes within the decode bar.
Detector: one training step and one eval pass of PointRCNN (PartA2_free.yaml on the reduced U-Net grid) against the reference's own
(tests/golden/ref_parta2_free.npz), with the bars of tests/test_parta2_net_gpu.py, and two identical steps bit for bit. The head's
training step raises no host synchronisation beyond the decode's one read-back; the sorted max-pool backward that the deterministic mode
takes against the atomic one."""
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

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_part_box.npz')
W = pb.LOSS_WEIGHTS
LOSS_ARGS = (cases.ALPHA, cases.GAMMA, pb.CODE_WEIGHTS, pb.BETA, W['point_cls_weight'], W['point_part_weight'], W['point_box_weight'])
UPSTREAM = (2.5, -0.5, 1.75)


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLD))


def coder(num_class=3):
    from pcdet.utils.box_coder_utils import PointResidualCoder
    return PointResidualCoder(use_mean_size=True, mean_size=pb.MEAN_SIZE[:1] if num_class == 1 else pb.MEAN_SIZE)


def _check(tag, got, want, e_ref):
    """prints max|got - want| and its multiple of e_ref -> True when within 4 * e_ref"""
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) if np.size(want) else 0.0
    print('%-30s err %.3e  e_ref %.3e  multiple %s' % (tag, err, e_ref, ('%.2f' % (err / e_ref)) if e_ref > 0 else ('exact' if err == 0 else 'inf')))
    return err <= 4 * e_ref


@pytest.mark.parametrize('name', pb.CASES)
@pytest.mark.parametrize('with_part', [True, False])
def test_targets_against_part_targets_and_the_reference(dev, gold, name, with_part):
    from crbhip import part_head, point_box
    assert part_head.FUSED
    c = pb.case(name)
    pts, gt = torch.from_numpy(c['points']).to(dev), torch.from_numpy(c['gt_boxes']).to(dev)
    off = torch.from_numpy(c['offsets']).to(dev)
    lab, owner, box, part = point_box.point_box_targets(pts, gt, cases.EXTRA, c['num_class'], coder(c['num_class']), with_part=with_part,
                                                        offsets=off if with_part else None)
    lab0, part0, owner0 = part_head.part_targets(pts, gt, cases.EXTRA, c['num_class'], offsets=off)
    torch.cuda.synchronize()
    assert torch.equal(lab, lab0) and torch.equal(owner, owner0) and lab.dtype == torch.int64 and owner.dtype == torch.int32
    assert (part is None) if not with_part else torch.equal(part, part0)
    assert np.array_equal(lab.cpu().numpy(), gold[name + '_labels']) and np.array_equal(owner.cpu().numpy(), gold[name + '_owner'])
    box = box.cpu().numpy()
    assert box.dtype == np.float32 and (box[c['owner'] < 0] == 0).all()
    assert _check(name + ' box labels', box, c['box_labels_f64'], gold[name + '_e_ref_box'][0])


def _losses(c, gold, name, dev, with_part=True, nan=False, upstream=(1.0, 1.0, 1.0)):
    from crbhip import point_box
    box_labels = gold[name + '_box_f32'].copy()
    if nan:
        box_labels[pb.nan_row(c), pb.NAN_CODE] = np.nan
    cls = torch.from_numpy(c['cls_preds']).to(dev).requires_grad_(True)
    prt = torch.from_numpy(c['part_preds']).to(dev).requires_grad_(True) if with_part else None
    box = torch.from_numpy(c['box_preds']).to(dev).requires_grad_(True)
    lc, lp, lb, pos = point_box.point_box_loss(cls, prt, box, torch.from_numpy(gold[name + '_labels']).to(dev),
                                               torch.from_numpy(gold[name + '_part_f32']).to(dev) if with_part else None,
                                               torch.from_numpy(box_labels).to(dev), *LOSS_ARGS)
    assert lc.dtype == torch.float64 and lb.dtype == torch.float64
    (lc * upstream[0] + lp * upstream[1] + lb * upstream[2]).backward()
    torch.cuda.synchronize()
    out = {'loss_cls': lc.detach().cpu().numpy().reshape(1), 'loss_part': lp.detach().cpu().numpy().reshape(1),
           'loss_box': lb.detach().cpu().numpy().reshape(1), 'pos': pos.detach().cpu().numpy().reshape(1),
           'd_cls': cls.grad.cpu().numpy(), 'd_box': box.grad.cpu().numpy()}
    if with_part:
        out['d_part'] = prt.grad.cpu().numpy()
    return out


@pytest.mark.parametrize('name', pb.CASES + ('tiles_nan',))
@pytest.mark.parametrize('with_part', [True, False])
def test_losses_and_gradients_against_the_reference(dev, gold, name, with_part):
    """upstream gradients 2.5 / -0.5 / 1.75 on the three losses (a swapped pair shows); part_preds absent = PointHeadBox"""
    tag, name = name, name.split('_nan')[0]
    c = pb.case(name)
    got = _losses(c, gold, name, dev, with_part, nan=tag != name, upstream=UPSTREAM)
    again = _losses(c, gold, name, dev, with_part, nan=tag != name, upstream=UPSTREAM)
    assert all(np.array_equal(got[k], again[k], equal_nan=True) for k in got), 'two calls differ'
    assert got['pos'][0] == gold[name + '_f64_pos'][0]
    scale = {'d_cls': UPSTREAM[0], 'd_part': UPSTREAM[1], 'd_box': UPSTREAM[2]}
    ok = True
    for k in [k for k in got if k != 'pos']:
        if k == 'loss_part' and not with_part:
            assert got[k][0] == 0.0
            continue
        src = tag if k in ('loss_box', 'd_box') else name
        s = scale.get(k, 1.0)
        ok &= _check('%s %s' % (tag, k), got[k] / s, gold['%s_f64_%s' % (src, k)], gold['%s_e_ref_%s' % (src, k)][0])
    assert ok
    if name == 'no_pos':
        assert got['loss_box'][0] == 0.0 and not got['d_box'].any()
    if tag != name:
        assert got['d_box'][pb.nan_row(c), pb.NAN_CODE] == 0.0 and np.isfinite(got['loss_box']).all()


@pytest.mark.parametrize('name', pb.CASES)
def test_decode_against_the_definition(dev, gold, name):
    from crbhip import point_box
    c = pb.case(name)
    want, _ = pb.decode_f64(c['points'], c['cls_preds'], c['box_preds'], c['mean_size'])
    B = len(c['counts'])
    args = (torch.from_numpy(c['points']).to(dev), torch.from_numpy(c['cls_preds']).to(dev), torch.from_numpy(c['box_preds']).to(dev),
            coder(c['num_class']), B)
    for counts in (None, c['counts']):                       # the offsets read back once / host counts from the batch
        cls_d, box_d, n = point_box.point_box_decode(*args, counts=counts)
        torch.cuda.synchronize()
        assert n.dtype == torch.int32 and n.tolist() == c['counts'] and cls_d.shape == (B, max(c['counts']), c['num_class'])
        assert np.array_equal(cls_d.cpu().numpy(), pb.pack_dense(c['counts'], c['cls_preds'], -np.inf))
        box_d = box_d.cpu().numpy()
        pad = pb.pack_dense(c['counts'], np.ones((len(want), 1)), 0.0)[..., 0] == 0
        assert (box_d[pad] == 0).all()
        assert _check(name + ' decode', box_d, pb.pack_dense(c['counts'], want, 0.0), gold[name + '_e_ref_decode'][0])


def _roi_head():
    from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
    cfg = EasyDict({'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5},
                    'LOSS_CONFIG': {'LOSS_WEIGHTS': {'code_weights': [1.0] * 7}}})
    return RoIHeadTemplate(num_class=1, model_cfg=cfg)


@pytest.mark.parametrize('route', ['fused', 'stacked', 'stacked_torch_finish'])
def test_stacked_proposals_against_the_reference(dev, gold, route, monkeypatch):
    """frames of 420 / 150 / 0 rows, NMS_PRE_MAXSIZE 300, NMS_POST_MAXSIZE 64. fused: crb_point_box_decode -> dense + batch_counts;
    stacked: the torch decode -> the reference's stacked rows + batch_index, packed by the proposal layer (and its finish in torch)"""
    from crbhip import point_box
    from pcdet.models.roi_heads import roi_head_template
    c = pb.proposal_case(int(gold['prop_seed'][0]))
    pts, cls, codes = (torch.from_numpy(c[k]).to(dev) for k in ('points', 'cls_preds', 'box_preds'))
    B = c['batch_size']
    if route == 'fused':
        cls_d, box_d, n = point_box.point_box_decode(pts, cls, codes, coder(), B)
        bd = {'batch_size': B, 'batch_cls_preds': cls_d, 'batch_box_preds': box_d, 'batch_counts': n}
    else:
        cls_s, box_s = point_box.point_box_decode_torch(pts, cls, codes, coder())
        bd = {'batch_size': B, 'batch_cls_preds': cls_s, 'batch_box_preds': box_s, 'batch_index': pts[:, 0]}
        if route == 'stacked_torch_finish':
            monkeypatch.setattr(roi_head_template, 'FUSED_PROPOSAL', False)
    out = _roi_head().proposal_layer(bd, EasyDict(pb.PROPOSAL_NMS))
    torch.cuda.synchronize()
    assert 'batch_index' not in out and out['has_class_labels'] is True
    rois, scores, labels, full = (out[k].cpu().numpy() for k in ('rois', 'roi_scores', 'roi_labels', 'full_cls_scores'))
    assert rois.shape == (3, 64, 7) and labels.dtype == np.int64
    assert np.array_equal(scores, gold['prop_roi_scores']) and np.array_equal(labels, gold['prop_roi_labels'])
    assert np.array_equal(full, gold['prop_full_cls_scores'])
    assert (rois[2] == 0).all() and (labels[2] == 1).all() and (scores[2] == 0).all()
    # the picks, by their (distinct) scores, against the f64 decode of the picked rows
    want64, _ = pb.decode_f64(c['points'], c['cls_preds'], c['box_preds'], pb.mean_size(3))
    row_of = {float(s): i for i, s in enumerate(c['cls_preds'].max(1))}
    valid = gold['prop_rois'][..., 3] > 0
    assert np.array_equal(rois[..., 3] > 0, valid) and valid[:2].all()
    picks = np.array([row_of[float(s)] for s in scores[valid]])
    assert _check('proposal boxes (%s)' % route, rois[valid], want64[picks], gold['prop_e_ref_decode'][0])
    assert np.abs(rois.astype(np.float64) - gold['prop_rois']).max() <= 5 * gold['prop_e_ref_decode'][0]


# ---- the detector -------------------------------------------------------------------------------------------------------------
NET_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_parta2_free.npz')


@pytest.fixture(scope='module')
def net_gold():
    return dict(np.load(NET_GOLD))


def _net(dev, G):
    """PartA2_free's PointRCNN on the reduced U-Net grid with the golden's seeded state and kink margins"""
    from types import SimpleNamespace
    from golden._constants import seeded_state
    from pcdet.model_cfgs import parta2_free_cfg
    from pcdet.models import build_network
    ds = SimpleNamespace(class_names=['Car', 'Pedestrian', 'Cyclist'], grid_size=np.array(cases.UNET_GRID),
                         point_cloud_range=np.array(cases.UNET_PCR, np.float32), voxel_size=cases.UNET_VOXEL,
                         depth_downsample_factor=None, point_feature_encoder=SimpleNamespace(num_point_features=4))
    torch.manual_seed(0)
    model = build_network(pb.net_overrides(parta2_free_cfg().MODEL), 3, ds)
    assert type(model).__name__ == 'PointRCNN' and sorted(model.state_dict().keys()) == list(G['keys'])
    assert [str(tuple(v.shape)) for _, v in sorted(model.state_dict().items())] == list(G['shapes'])
    sd = seeded_state(model, pb.NET_SEED)
    for k in pb.NET_SMALL:
        sd[k] = sd[k] * 0.1
    sd.update({k[len('bias/'):]: torch.from_numpy(G[k]) for k in G if k.startswith('bias/')})
    model.load_state_dict(sd)
    return model.to(dev)


def _net_batch(dev, G):
    nb = pb.net_batch()
    b = {k: torch.from_numpy(nb[k]).to(dev) for k in ('points', 'voxels', 'voxel_num_points', 'voxel_coords')}
    b.update(batch_size=nb['batch_size'], gt_boxes=torch.from_numpy(G['gt']).to(dev), frame_id=np.array(['%06d' % i for i in range(nb['batch_size'])]))
    return b


# The model's own proposals against the reference's: first-stage scores and boxes agree to some 1e-6, so the two greedy scans differ only
# where two scores or an IoU and NMS_THRESH lie that close, and one such flip changes a few picks of its frame. The goldens do not keep
# these margins (the injected proposals carry the exact comparisons), so this is a loose check that the detector's own TRAIN / TEST
# proposal path gives the reference's boxes: at least 90 % of the reference's rois have a partner within 1e-3 in every coordinate.
OWN_PROPOSALS = 0.9


def _share_found(mine, ref):
    """share of the non-empty rois of ref (B,R,7) that have a roi of mine (same frame) within 1e-3 in all 7 values"""
    hit = total = 0
    for m, r in zip(mine, ref):
        r = r[r[:, 3] > 0]
        d = np.abs(r[:, None, :] - m[None, :, :])
        d[..., 6] = np.abs((d[..., 6] + np.pi) % (2 * np.pi) - np.pi)
        hit, total = hit + int((d.max(-1).min(1) <= 1e-3).sum()), total + len(r)
    return hit / max(total, 1)


def test_train_step_matches_the_reference_detector(dev, net_gold):
    """one training step of PointRCNN against the reference's own (tests/golden/ref_parta2_free.npz): the golden's first-stage proposals
    and recorded RoI-sampler draws make the injected roi_targets_dict, the model's own proposal layer still runs (dense, from
    crb_point_box_decode). Bars: those of tests/test_parta2_net_gpu.py::test_train_step_matches_the_reference_detector for the same
    quantities (point scores and first-stage boxes 1e-5, loss and tb_dict 2e-4, rcnn outputs 2e-3, gradients 2e-2 of the largest entry)."""
    G = net_gold
    model = _net(dev, G).train()
    b = _net_batch(dev, G)
    layer = model.roi_head.proposal_target_layer
    layer.injected_indices = torch.from_numpy(G['sampled'])
    try:
        b['roi_targets_dict'] = model.roi_head.assign_targets({
            'batch_size': 2, 'gt_boxes': b['gt_boxes'], 'rois': torch.from_numpy(G['proposals']).to(dev),
            'roi_scores': torch.from_numpy(G['proposal_scores']).to(dev), 'roi_labels': torch.from_numpy(G['proposal_labels']).to(dev)})
    finally:
        layer.injected_indices = None
    np.testing.assert_array_equal(b['roi_targets_dict']['rois'].cpu().numpy(), G['rois'])                # sampled rois: exact
    seen = {}
    own_layer = model.roi_head.proposal_layer

    def watching(bd, nms_config):
        seen.update(cls=bd['batch_cls_preds'].detach().clone(), box=bd['batch_box_preds'].detach().clone(), counts=bd['batch_counts'].clone())
        bd = own_layer(bd, nms_config=nms_config)
        seen.update(rois=bd['rois'].clone(), labels=bd['roi_labels'].clone())
        return bd
    model.roi_head.proposal_layer = watching
    try:
        ret, tb, _ = model(b)
    finally:
        del model.roi_head.proposal_layer
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    pc = b['point_coords'].cpu().numpy()
    mine, ref = np.lexsort(pc.T[::-1]), np.lexsort(G['point_coords'].T[::-1])
    np.testing.assert_array_equal(pc[mine], G['point_coords'][ref])
    _rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    # the first stage: scores, targets, and the dense proposals input (frame-padded rows of the reference's stacked ones)
    counts = seen['counts'].tolist()
    assert counts == np.bincount(pc[:, 0].astype(np.int64), minlength=2).tolist() and seen['cls'].shape == (2, max(counts), 3)
    flat = np.concatenate([np.arange(n) + f * max(counts) for f, n in enumerate(counts)])
    cls_rows, box_rows = seen['cls'].cpu().numpy().reshape(-1, 3)[flat], seen['box'].cpu().numpy().reshape(-1, 7)[flat]
    e_s = _rel(b['point_cls_scores'].detach().cpu().numpy().reshape(-1)[mine], G['point_cls_scores'].reshape(-1)[ref])
    e_c, e_b = _rel(cls_rows[mine], G['stacked_cls_preds'][ref]), _rel(box_rows[mine], G['stacked_box_preds'][ref])
    pr = model.point_head.forward_ret_dict
    np.testing.assert_array_equal(pr['point_cls_labels'].cpu().numpy()[mine], G['point_cls_labels'][ref])
    # box labels against the f64 definition: formed in f64 and rounded once, so within one f32 ulp of the value
    _, _, def_box, _ = pb.box_targets_f64(pc, G['gt'], 3, pb.mean_size(3))
    e_l = float((np.abs(pr['point_box_labels'].cpu().numpy() - def_box) / np.maximum(1.0, np.abs(def_box))).max())
    print('point scores %.2e, first-stage logits %.2e, boxes %.2e, box labels %.2e (of max(1, |label|), against f64), rows %d reference %d, loss %.6f reference %.6f' % (
        e_s, e_c, e_b, e_l, b['roi_grid_coords'].shape[0], len(G['coords']), float(ret['loss'].detach()), float(G['loss'][0])))
    assert e_s <= 1e-5 and e_c <= 1e-5 and e_b <= 1e-5 and e_l <= 2.0 ** -23
    assert seen['rois'].shape == (2, 64, 7) and torch.isfinite(seen['rois']).all() and int(seen['labels'].min()) >= 1
    found = _share_found(seen['rois'].cpu().numpy(), G['proposals'])
    print('own proposals: %.3f of the reference\'s found' % found)
    assert found >= OWN_PROPOSALS
    np.testing.assert_array_equal(b['roi_grid_coords'].cpu().numpy(), G['coords'])                          # RoI-grid coords: exact
    for k, want in zip(G['tb_keys'], G['tb_vals']):
        print('%-20s %.6f reference %.6f' % (k, float(tb[k]), want))
    np.testing.assert_allclose(float(ret['loss'].detach()), float(G['loss'][0]), rtol=2e-4)
    assert sorted(tb.keys()) == list(G['tb_keys'])
    for k, want in zip(G['tb_keys'], G['tb_vals']):
        np.testing.assert_allclose(float(tb[k]), want, rtol=2e-4, atol=2e-5, err_msg=str(k))
    fr = model.roi_head.forward_ret_dict
    for k in ('rcnn_cls', 'rcnn_reg'):
        got, want = fr[k].detach().float().cpu().numpy().reshape(G[k].shape), G[k]
        print('%s error %.2e of its largest entry' % (k, np.abs(got - want).max() / np.abs(want).max()))
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max(), k
    params = dict(model.named_parameters())
    worst = {}
    for n, sl in pb.NET_GRADS.items():
        got, want = params[n].grad.cpu().numpy()[sl], G['grad/' + n]
        worst[n] = float(np.abs(got - want).max()) / float(G['gradmax/' + n][0])
        print('%-44s gradient error %.2e of its largest entry' % (n, worst[n]))
    assert all(e <= 2e-2 for e in worst.values()), worst


def test_eval_pred_dicts_match_the_reference_detector(dev, net_gold):
    """the eval pass on the golden's first-stage proposals (the frames' own would order near-equal scores by rounding): the same
    number of predictions per frame, each matched to the reference's by position - the golden keeps the final NMS 5e-5 (IoU) and
    0.3 (score threshold) off its thresholds, not the score gaps, so the order may differ. Bars: labels equal, scores and boxes within
    2e-3 of the largest entry, the bar of the second stage's outputs in tests/test_parta2_net_gpu.py."""
    G = net_gold
    model = _net(dev, G).eval()
    b = _net_batch(dev, G)
    b.update(rois=torch.from_numpy(G['eval_proposals']).to(dev), roi_scores=torch.from_numpy(G['eval_proposal_scores']).to(dev),
             roi_labels=torch.from_numpy(G['eval_proposal_labels']).to(dev), has_class_labels=True)
    with torch.no_grad():
        pred, _ = model(b)
    torch.cuda.synchronize()
    assert len(pred) == 2
    for f, p in enumerate(pred):
        boxes, scores, labels = (p[k].cpu().numpy() for k in ('pred_boxes', 'pred_scores', 'pred_labels'))
        want_b, want_s, want_l = G['pred_boxes_%d' % f], G['pred_scores_%d' % f], G['pred_labels_%d' % f]
        assert len(scores) == len(want_s) > 0, (f, len(scores), len(want_s))
        match = np.abs(boxes[None, :, :3] - want_b[:, None, :3]).sum(-1).argmin(1)
        assert len(set(match.tolist())) == len(match)
        e_b = np.abs(boxes[match] - want_b).max() / np.abs(want_b).max()
        e_s = np.abs(scores[match] - want_s).max() / np.abs(want_s).max()
        print('frame %d: %d predictions, boxes %.2e, scores %.2e of the largest entry' % (f, len(scores), e_b, e_s))
        assert np.array_equal(labels[match], want_l) and e_b <= 2e-3 and e_s <= 2e-3
    # the same pass on the model's own proposals (NMS_CONFIG.TEST through the detector): loosely the reference's, see OWN_PROPOSALS
    own = _net_batch(dev, G)
    with torch.no_grad():
        pred_own, _ = model(own)
    found = _share_found(own['rois'].cpu().numpy(), G['eval_proposals'])
    print('own eval proposals: %.3f of the reference\'s found; predictions %s reference %s' % (
        found, [len(p['pred_scores']) for p in pred_own], [len(G['pred_scores_%d' % f]) for f in range(2)]))
    assert own['rois'].shape == (2, 32, 7) and found >= OWN_PROPOSALS and len(pred_own) == 2


def test_training_step_is_bit_reproducible_under_deterministic_algorithms(dev, net_gold):
    """two identical steps with the model's own proposals and sampler: the same bits in the loss, the proposals and the gradients"""
    import random
    model = _net(dev, net_gold).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    res = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            model.load_state_dict(state)
            random.seed(5); np.random.seed(5); torch.manual_seed(5)
            b = _net_batch(dev, net_gold)
            ret, tb, _ = model(b)
            model.zero_grad(set_to_none=True)
            ret['loss'].backward()
            res.append((ret['loss'].detach().clone(), b['rois'].clone(), tb['point_loss_box'].clone(), model.point_head.box_layers[0].weight.grad.clone(),
                        model.point_head.cls_layers[0].weight.grad.clone(), model.backbone_3d.conv_input[0].weight.grad.clone()))
    finally:
        torch.use_deterministic_algorithms(False)
    assert float(res[0][3].abs().sum()) > 0 and float(res[0][5].abs().sum()) > 0
    for a, c in zip(*res):
        assert torch.equal(a, c)


def test_head_training_step_raises_no_synchronisation(dev):
    """forward + get_loss + backward of the point head with its box branch: the reference synchronises per frame (boolean masks) and per
    loss (.item()). With predict_boxes_when_training the decode's padded width costs at most one read-back (the frame offsets), and none
    when the batch carries the frames' counts on the host"""
    import warnings
    from pcdet.models import dense_heads
    c = pb.case('ragged')
    cfg = EasyDict({'NAME': 'PointIntraPartOffsetHead', 'CLS_FC': [16], 'PART_FC': [16], 'REG_FC': [16], 'CLASS_AGNOSTIC': False,
                    'TARGET_CONFIG': {'GT_EXTRA_WIDTH': cases.EXTRA, 'BOX_CODER': 'PointResidualCoder',
                                      'BOX_CODER_CONFIG': {'use_mean_size': True, 'mean_size': pb.MEAN_SIZE}},
                    'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss', 'LOSS_WEIGHTS': dict(pb.LOSS_WEIGHTS, code_weights=pb.CODE_WEIGHTS)}})
    torch.manual_seed(0)
    head = dense_heads.__all__['PointIntraPartOffsetHead'](num_class=3, input_channels=16, model_cfg=cfg).to(dev).train()
    assert head.reg_loss_func.code_weights.is_cuda                   # (the buffer the loss must not read back)
    batch = {'point_features': torch.randn(len(c['points']), 16, device=dev), 'point_coords': torch.from_numpy(c['points']).to(dev),
             'gt_boxes': torch.from_numpy(c['gt_boxes']).to(dev), 'batch_size': 3}

    def step(extra):
        head(dict(batch, **extra))
        loss, _ = head.get_loss()
        loss.backward()
        return loss
    step({})                                                        # (first launches load code objects)
    head.predict_boxes_when_training = True
    step({})
    torch.cuda.synchronize()
    for predict, extra, allowed in ((False, {}, 0), (True, {'point_coords_counts_host': c['counts']}, 0), (True, {}, 1)):
        head.predict_boxes_when_training = predict
        head.zero_grad(set_to_none=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                loss = step(extra)
            finally:
                torch.cuda.set_sync_debug_mode('default')
            # (the mode announces itself once as a prototype feature: that notice is no synchronisation)
            syncs = [str(w.message) for w in rec if 'synchroniz' in str(w.message).lower() and 'prototype feature' not in str(w.message)]
        print('predict_boxes_when_training %s, host counts %s: synchronisation warnings: %s' % (predict, bool(extra), syncs))
        assert len(syncs) <= allowed, syncs
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(p.grad is not None for p in head.parameters())


def test_deterministic_max_pool_backward_is_the_atomic_one_in_another_order(dev):
    """RoIAwarePool3dFunction's max backward under torch.use_deterministic_algorithms(True) (a sorted accumulate) against the launch
    with float atomics: the same terms summed in another order. Bound per entry: n terms added in f32 in any order differ by at most
    (n - 1) * 2^-24 * sum|terms| from the exact sum, twice that between two orders; n <= the cells that can name one point as their
    maximum, bounded here by the RoI count."""
    from pcdet.ops.roiaware_pool3d import roiaware_pool3d_utils
    rng = np.random.default_rng(9)
    R, P, C = 24, 500, 16
    rois = np.concatenate([rng.uniform(-1, 1, (R, 3)), rng.uniform(2, 4, (R, 3)), rng.uniform(-3, 3, (R, 1))], 1).astype(np.float32)
    pts = torch.from_numpy(rng.uniform(-2.5, 2.5, (P, 3)).astype(np.float32)).to(dev)
    feat0 = torch.from_numpy(rng.normal(0, 1, (P, C)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.normal(0, 1, (R, 4, 4, 4, C)).astype(np.float32)).to(dev)
    pool = roiaware_pool3d_utils.RoIAwarePool3d(out_size=4, max_pts_each_voxel=64)
    grads = []
    for flag in (False, True):
        feat = feat0.clone().requires_grad_(True)
        torch.use_deterministic_algorithms(flag)
        try:
            pool(torch.from_numpy(rois).to(dev), pts, feat, pool_method='max').backward(g)
        finally:
            torch.use_deterministic_algorithms(False)
        grads.append(feat.grad.clone())
    again = feat0.clone().requires_grad_(True)
    torch.use_deterministic_algorithms(True)
    try:
        pool(torch.from_numpy(rois).to(dev), pts, again, pool_method='max').backward(g)
    finally:
        torch.use_deterministic_algorithms(False)
    torch.cuda.synchronize()
    assert torch.equal(again.grad, grads[1]) and float(grads[0].abs().sum()) > 0
    err, bound = float((grads[0] - grads[1]).abs().max()), 2 * (R - 1) * 2.0 ** -24 * R * float(g.abs().max())
    print('atomic vs sorted accumulate: max difference %.3e, bound %.3e' % (err, bound))
    assert err <= bound
