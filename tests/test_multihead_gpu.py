"""MI355X: the multi-head family on the device — target assignment through crb_assign_targets in the multi-head order, the loss kernels
of csrc/multihead_loss.hip, the per-class selection of csrc/multiclass_nms.hip and SECONDNet from second_multihead_cfg().

Bars as in tests/test_multihead_cpu.py (FACTOR = 4 times the reference's own f32 error recorded in tests/golden/ref_multihead.npz):
  targets   labels equal, regression targets within FACTOR * e_ref per column
  loss      the kernel's three values within FACTOR * e_rel * |value| of the reference's f64 values, every gradient within FACTOR * e_ref of
            the torch restatement run in f64 on the device; two runs bit-equal
  select    top_idx / counts equal the definition; kept boxes, labels, scores and num equal, bit for bit, the loop route
            (CRB_MULTICLASS_NMS=0) and the golden's per-(frame, head) outputs concatenated in head order; two runs bit-equal;
            the candidates kernel alone at a cut inside a run of equal scores and with PRE = 4,096; its sigmoid against torch.sigmoid
            on consecutive f32 logits around four thresholds; one host synchronisation in the detector's post-processing
  single    csrc/rpn_loss.hip, whose device functions moved into a shared header, gives the parent commit's bits"""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import multihead_cases as cases
import test_multihead_cpu as cpu
from test_multihead_cpu import FACTOR, gold, t_  # noqa: F401

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def no_fallback():
    with warnings.catch_warnings():
        warnings.filterwarnings('error', message='.*torch route.*')
        yield


# ---- targets -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(cases.GT_CASES))
def test_targets_on_the_device(gold, dev, name):
    from pcdet.models.dense_heads.target_assigner import axis_aligned_target_assigner as ata
    head = cases.make_head('two', grid=cases.GT_CASES[name][0]).to(dev)
    gt = t_(cases.make_gt(name), dev)
    assert ata.FUSED
    out = head.assign_targets(gt)
    cpu.check_targets(gold, name, out)
    again = head.assign_targets(gt)
    assert all(torch.equal(out[k], again[k]) for k in out)
    ata.FUSED = False
    try:
        host_route = head.assign_targets(gt)                              # the batched torch ops on the same tensors
    finally:
        ata.FUSED = True
    assert torch.equal(out['box_cls_labels'], host_route['box_cls_labels'])


# ---- losses ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(cases.LOSS_CASES))
def test_loss_kernel(gold, dev, case):
    runs = []
    for _ in range(2):
        head, leaves = cpu.loss_head(case, gold, dev)
        with no_fallback():
            loss, tb = head.get_loss()
        loss.backward()
        runs.append((cpu.loss_values(tb), float(tb['rpn_loss']), leaves))
    vals, total, leaves = runs[0]
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad and v.is_cuda for v in tb.values())
    cpu.check_loss_values(gold, case, vals, 'kernel')
    assert abs(total - vals.sum()) <= 1e-6 * total
    head64, leaves64 = cpu.loss_head(case, gold, dev, torch.float64)
    with warnings.catch_warnings(record=True) as rec:                     # (f64 is the torch route by definition: no warning)
        warnings.simplefilter('always')
        loss64, tb64 = head64.get_loss()
    assert not [w for w in rec if 'torch route' in str(w.message)]
    loss64.backward()
    for key, ts in leaves.items():
        for h, t in enumerate(ts or ()):
            g, g64 = t.grad, leaves64[key][h].grad
            assert g is not None and g.shape == t.shape and g.dtype == torch.float32
            err, e_ref = float((g.double() - g64).abs().max()), gold['loss_%s_e_ref_g_%s' % (case, key)][0]
            print('  gradient %s head %d: error %.3g, e_ref %.3g' % (key, h, err, e_ref))
            assert err <= FACTOR * e_ref, (key, h)
            assert torch.equal(g, runs[1][2][key][h].grad), 'two runs differ'
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_loss_per_frame_sums_and_positives(gold, dev):
    """crbhip.multihead.multihead_loss itself: (B,3) per-frame values whose mean over the frames are the head's losses, npos = the
    frame's positives over all heads; the frame without positives divides by 1"""
    from crbhip import multihead, rpn_loss
    case = 'two_sep_dir'
    head, leaves = cpu.loss_head(case, gold, dev)
    d = head.forward_ret_dict
    cfg = rpn_loss.make_cfg(3, 2, [1.0] * 7, 1.0, 2.0, 0.2, head.model_cfg.DIR_OFFSET)
    per_frame, npos = multihead.multihead_loss(leaves['cls'], leaves['box'], leaves['dir'], d['box_cls_labels'], d['box_reg_targets'],
                                               head._flat_anchors().view(-1, 7), cfg, class_starts=[0, 1], return_npos=True)
    assert per_frame.shape == (cases.B, 3) and npos.tolist() == (d['box_cls_labels'] > 0).sum(1).float().tolist() and npos[-1] == 0
    cpu.check_loss_values(gold, case, (per_frame.detach().sum(0) / cases.B).double().cpu().numpy(), 'per-frame rows')
    per_frame = per_frame.detach()
    assert float(per_frame[-1, 1]) == 0 and float(per_frame[-1, 2]) == 0 and float(per_frame[-1, 0]) > 0
    # classification weights: the kernel's pos / neg weights against the restatement with the same LOSS_WEIGHTS
    lw = dict(cases.LOSS_WEIGHTS, pos_cls_weight=2.0, neg_cls_weight=0.5)
    res = []
    for dtype in (torch.float32, torch.float64):
        h2, _ = cpu.loss_head(case, gold, dev, dtype)
        h2.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS.update(lw)
        with no_fallback():
            res.append(float(h2.get_loss()[1]['rpn_loss_cls']))
    assert abs(res[0] - res[1]) <= FACTOR * gold['loss_e_ref_rel'][0] * abs(res[1]) and abs(res[1] / float(per_frame.sum(0)[0] / cases.B) - 1) > 0.1


def test_fallback_selects_the_torch_route_and_warns(gold, dev):
    from pcdet.utils import loss_utils

    class OtherFocal(loss_utils.SigmoidFocalClassificationLoss):
        pass
    head, _ = cpu.loss_head('two_sep_dir', gold, dev)
    head.cls_loss_func = OtherFocal(alpha=0.25, gamma=2.0)
    with pytest.warns(UserWarning, match='torch route'):
        loss, tb = head.get_loss()
    ref, tb_ref = head.loss_torch()
    assert torch.equal(loss, ref)
    cpu.check_loss_values(gold, 'two_sep_dir', cpu.loss_values(tb), 'torch route on the device')


def test_head_training_step_raises_no_synchronisation(dev):
    head = cases.make_head('two').to(dev).to(memory_format=torch.channels_last)
    bd = {'spatial_features_2d': t_(cases.forward_input(), dev).contiguous(memory_format=torch.channels_last), 'batch_size': cases.B,
          'gt_boxes': t_(cases.make_gt('mixed'), dev)}
    with no_fallback():
        head(dict(bd))
        head.get_loss()[0].backward()                                     # (first launches load code objects)
        torch.cuda.synchronize()
        head.zero_grad(set_to_none=True)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter('always')
            warnings.filterwarnings('error', message='.*torch route.*')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                head(dict(bd))
                loss, tb = head.get_loss()
                loss.backward()
            finally:
                torch.cuda.set_sync_debug_mode('default')
            syncs = [str(w.message) for w in rec if 'synchroniz' in str(w.message).lower() and 'prototype feature' not in str(w.message)]
    print('synchronisation warnings:', syncs)
    assert not syncs
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())


def test_single_head_kernel_gives_the_parent_builds_bits(gold):
    """csrc/rpn_loss.hip now takes its per-anchor terms from csrc/rpn_loss_terms.h: same outputs as the parent commit's build, recorded
    in the golden, on the single-head loss cases of tests/anchor_head_cases.py"""
    out = cases.rpn_single_outputs()
    assert len(out) >= 8 * 5 and all('rpn_parent_' + k in gold.files for k in out)
    bad = [k for k, v in out.items() if not np.array_equal(v, gold['rpn_parent_' + k])]
    assert not bad, bad


# ---- selection ---------------------------------------------------------------------------------------------------------------
def prepare_selection(name, dev):
    """the case's tensors on the device, the head's decoder and label mapping"""
    head, ts, per_head = cpu.decoded_boxes(name, dev)
    mapping = [h.head_label_indices for h in head.rpn_heads]
    return head, ts, per_head, mapping, head._head_decoder(cases.B, ts['box'], ts['dir'])


def run_selection(name, prep):
    from pcdet.config import EasyDict
    from pcdet.models.model_utils import model_nms_utils
    _, ts, _, mapping, decode = prep
    return model_nms_utils.multi_classes_nms_batched(ts['cls'], decode, mapping, EasyDict(cases.nms_cfg(name)), cases.SEL_CASES[name]['thresh'])


@pytest.mark.parametrize('name', list(cases.SEL_CASES))
def test_selection_against_the_loop_route_and_the_reference(gold, dev, name):
    from pcdet.config import EasyDict
    from pcdet.models.model_utils import model_nms_utils
    c = cases.SEL_CASES[name]
    prep = prepare_selection(name, dev)
    head, ts, per_head, mapping, _ = prep
    run_selection(name, prep)                                             # (first launches load code objects)
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            rec = run_selection(name, prep)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    msgs = [str(w.message) for w in seen if 'prototype feature' not in str(w.message)]
    print('warnings of the device route:', msgs)
    assert not [m for m in msgs if 'synchroniz' in m.lower() or 'torch route' in m]     # no synchronisation, no fallback
    num = rec['num'].cpu().tolist()                                       # the single read-back
    # candidates against the definition, segment by segment (head-major rows)
    sizes = cases.head_sizes(c['layout'], True, c['grid'])
    d = cases.make_selection(name)
    top_idx, top_logit, counts = rec['top_idx'].cpu().numpy(), rec['top_logit'].cpu().numpy(), rec['counts'].cpu().numpy()
    row0 = 0
    for h, (n, C, _) in enumerate(sizes):
        for b in range(cases.B):
            for k in range(C):
                want = cases.candidates_definition(d['cls'][h][b, :, k], c['thresh'], c['pre'])
                r = row0 + b * C + k
                assert counts[r] == len(want), (h, b, k)
                assert np.array_equal(top_idx[r, :len(want)], want) and (top_idx[r, len(want):] == 0).all(), (h, b, k)
                assert np.array_equal(top_logit[r, :len(want)], d['cls'][h][b, want, k]) and (top_logit[r, len(want):] == 0).all()
        row0 += cases.B * C
    # the loop route on the same tensors
    nms = EasyDict(cases.nms_cfg(name))
    P = rec['pred_boxes'].shape[1]
    assert P == sum(C for _, C, _ in sizes) * c['post']
    for b in range(cases.B):
        loop = {'scores': [], 'labels': [], 'boxes': []}
        per = []
        for h in range(len(sizes)):
            s, l, bx = model_nms_utils.multi_classes_nms(torch.sigmoid(ts['cls'][h][b]), per_head[h][b], nms, c['thresh'])
            loop['scores'].append(s)
            loop['labels'].append(mapping[h][l])
            loop['boxes'].append(bx)
            per.append(len(s))
        k = num[b]
        assert per == gold['sel_%s_counts' % name][b].tolist() and k == sum(per), (b, per, k)
        got = {'scores': rec['pred_scores'][b, :k], 'labels': rec['pred_labels'][b, :k], 'boxes': rec['pred_boxes'][b, :k]}
        for key in got:
            want, ref = torch.cat(loop[key], 0), gold['sel_%s_%s_%d' % (name, key, b)]
            g = got[key].cpu().numpy()
            assert torch.equal(got[key], want), (b, key, 'loop route')
            if key != 'scores':           # (the golden's scores: test_selection_scores_against_the_reference)
                assert g.shape == ref.shape and np.array_equal(g, ref.astype(g.dtype)), (b, key, 'golden')
        for key in ('pred_scores', 'pred_labels', 'pred_boxes', 'pred_anchor', 'seg_of'):
            assert not rec[key][b, k:].any(), (b, key)                    # rows past num[b] are zero
        # every kept box is the decode of its own anchor of its own head, its score the sigmoid of that logit
        seg_head = [h for h, (_, C, _) in enumerate(sizes) for _ in range(C)]
        seg_col = [j for _, C, _ in sizes for j in range(C)]
        for i in range(k):
            g_, a = int(rec['seg_of'][b, i]), int(rec['pred_anchor'][b, i])
            assert torch.equal(rec['pred_boxes'][b, i], per_head[seg_head[g_]][b, a])
            assert rec['pred_scores'][b, i] == torch.sigmoid(ts['cls'][seg_head[g_]][b, a, seg_col[g_]])
    # two runs
    again = run_selection(name, prep)
    assert all(torch.equal(rec[k], again[k]) for k in rec)


@pytest.mark.parametrize('name', list(cases.SEL_CASES))
def test_selection_scores_against_the_reference(gold, dev, name):
    """the kept scores equal the golden's, bit for bit. They are torch.sigmoid of the kept logits on the device; the golden's are
    torch.sigmoid of the same logits on the host that ran the reference. The two differ in their exp, which may miss the correctly
    rounded value by a step; the cases report only scores of logits at which the add and the divide of 1 / (1 + exp(-x)) round such a
    difference away (multihead_cases.sigmoid_stable, asserted for every candidate by check_selection_margins)."""
    rec = run_selection(name, prepare_selection(name, dev))
    num = rec['num'].cpu().tolist()
    worst = 0.0
    for b in range(cases.B):
        g, ref = rec['pred_scores'][b, :num[b]].cpu().numpy(), gold['sel_%s_scores_%d' % (name, b)]
        assert g.shape == ref.shape
        if len(g):
            worst = max(worst, float(np.abs(g.astype(np.float64) - ref).max()))
    print('%s: largest |device score - golden score| %.3g' % (name, worst))
    assert worst == 0


@pytest.mark.parametrize('name', list(cases.CUT_CASES))
def test_candidates_at_the_cut_and_with_the_full_sort(dev, name):
    """crb_multiclass_candidates alone against the definition: the cut inside a run of equal scores (the radix select goes on through
    the index digits: the smaller anchor indices of the run are taken), just behind and exactly in front of a run, a run that fits
    whole, and PRE = 4,096 with more, exactly as many and one more passing anchor (the whole 32 KB sort)"""
    from crbhip import multihead
    c, x = cases.CUT_CASES[name], cases.make_cut_case(name)
    runs = [multihead.candidates([t_(x, dev)], cases.CUT_THRESH, c['pre']) for _ in range(2)]
    top_idx, top_logit, counts = (t.cpu().numpy() for t in runs[0])
    assert top_idx.shape == (2 * c['C'], c['pre'])
    for b in range(2):
        for k in range(c['C']):
            want = cases.candidates_definition(x[b, :, k], cases.CUT_THRESH, c['pre'])
            r = b * c['C'] + k
            assert counts[r] == len(want), (b, k)
            assert np.array_equal(top_idx[r, :len(want)], want) and (top_idx[r, len(want):] == 0).all(), (b, k)
            assert np.array_equal(top_logit[r, :len(want)], x[b, want, k]), (b, k)
    assert all(torch.equal(a, b_) for a, b_ in zip(*runs))


@pytest.mark.parametrize('thresh', [0.01, 0.1, 0.3, 0.9])
def test_kernel_sigmoid_is_torch_sigmoid_on_the_device(dev, thresh):
    """the candidates kernel thresholds and orders by its own 1 / (1 + exp(-x)); the loop route thresholds and orders torch.sigmoid(x).
    Both are the same f32 number on the device: on the 65,536 CONSECUTIVE f32 logits around the threshold's logit the kernel passes
    exactly the anchors whose torch.sigmoid is >= the threshold, and on 65,536 logits spread over [-12, 12] it also orders them as
    (torch.sigmoid descending, index ascending) does, runs of equal scores included"""
    from crbhip import multihead
    x0 = np.float32(np.log(thresh / (1.0 - thresh)))
    near = (np.array([x0]).view(np.int32)[0] + np.arange(-32768, 32768, dtype=np.int32)).view(np.float32)
    wide = np.linspace(-12.0, 12.0, 65536).astype(np.float32)
    assert np.isfinite(near).all() and len(np.unique(near)) == 65536
    for logits in (near, wide):
        x = t_(np.random.RandomState(3).permutation(logits).reshape(16, 4096, 1), dev)
        s = torch.sigmoid(x)[..., 0]
        top_idx, _, counts = multihead.candidates([x], thresh, 4096)
        passing = s >= thresh
        assert 0 < int(passing.sum()) < 65536
        assert torch.equal(counts.long(), passing.sum(1))
        s_host, idx_host, n_host = s.cpu().numpy(), top_idx.cpu().numpy(), counts.cpu().numpy()
        for b in range(16):
            cand = np.nonzero(s_host[b] >= np.float32(thresh))[0]
            order = cand[np.lexsort((cand, -s_host[b][cand].astype(np.float64)))]
            assert np.array_equal(idx_host[b, :n_host[b]], order), b


def test_post_processing_reads_back_once(dev):
    """multiclass_post_processing on the device route: the launch sequence, the gather of the kept boxes' logit rows and the slicing
    into pred dicts make ONE host synchronisation, the read-back of the frame counts (no gt_boxes: no recall bookkeeping)"""
    from pcdet.config import EasyDict
    from pcdet.models.detectors.post_processing import multiclass_post_processing
    name = 'two_pre100'
    head, ts, _, mapping, decode = prepare_selection(name, dev)
    model = type('Model', (), {})()
    model.model_cfg = EasyDict({'POST_PROCESSING': {'SCORE_THRESH': cases.SEL_CASES[name]['thresh'], 'RECALL_THRESH_LIST': [0.3, 0.5, 0.7],
                                                    'OUTPUT_RAW_SCORE': False, 'NMS_CONFIG': cases.nms_cfg(name)}})
    bd = lambda: {'batch_size': cases.B, 'batch_cls_preds': ts['cls'], 'cls_preds_normalized': False, 'multihead_label_mapping': mapping,
                  'multihead_box_decoder': decode}
    with no_fallback():
        multiclass_post_processing(model, bd())                           # (first launches load code objects)
        torch.cuda.synchronize()
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            torch.cuda.set_sync_debug_mode('warn')
            try:
                pred, _ = multiclass_post_processing(model, bd())
            finally:
                torch.cuda.set_sync_debug_mode('default')
    syncs = [str(w.message) for w in seen if 'synchroniz' in str(w.message).lower() and 'prototype feature' not in str(w.message)]
    print('synchronisation warnings:', syncs)
    assert len(syncs) == 1
    assert [len(p['pred_scores']) for p in pred] == gold_counts(name)


def gold_counts(name):
    return np.load(cases.GOLDEN)['sel_%s_counts' % name].sum(1).tolist()


# ---- detector ----------------------------------------------------------------------------------------------------------------
POINTS = 8000


def _detector(dev, seeded=False):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_multihead_cfg
    from pcdet.models import build_network
    cfg = second_multihead_cfg()
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=POINTS))
    if seeded:
        from golden._constants import seeded_state
        # (every entry but the heads' class-id buffers, which are no weights)
        model.load_state_dict({k: v for k, v in seeded_state(model, 3).items() if not k.endswith('head_label_indices')}, strict=False)
    return cfg, model.to(dev)


def _batch(dev):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(40, 2, POINTS)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {'points': t(np.concatenate([bidx[:, None], pts], 1)), 'point_frame_offsets': t(off), 'batch_size': 2,
            'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': t(gt), 'frame_id': np.array(['000040', '000041'])}


def _step(dev, fused=True):
    from pcdet.models.dense_heads import anchor_head_multi as ahm
    cfg, model = _detector(dev)
    model.train()
    ahm.FUSED_LOSS = fused
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings('error' if fused else 'ignore', message='.*torch route.*')
            ret, tb, _ = model(_batch(dev))
        ret['loss'].backward()
    finally:
        ahm.FUSED_LOSS = True
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    return float(ret['loss'].detach()), {k: float(v) for k, v in tb.items()}, grads, model


def test_training_step_on_both_head_routes(gold, dev):
    """second_multihead.yaml's detector on two synthetic frames: 70,400 anchors per head, 211,200 per frame"""
    loss, tb, grads, model = _step(dev, True)
    assert type(model).__name__ == 'SECONDNet' and type(model.dense_head).__name__ == 'AnchorHeadMulti'
    assert set(tb) == {'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir', 'rpn_loss', 'loss_rpn'} and np.isfinite(loss)
    assert model.dense_head.forward_ret_dict['box_cls_labels'].shape == (2, 211200)
    missing = [n for n, g in grads.items() if g is None or not torch.isfinite(g).all()]
    assert not missing, missing
    loss_t, tb_t, _, _ = _step(dev, False)
    e_rel = gold['loss_e_ref_rel']
    bars = {'rpn_loss_cls': e_rel[0], 'rpn_loss_loc': e_rel[1], 'rpn_loss_dir': e_rel[2], 'rpn_loss': e_rel.max(), 'loss_rpn': e_rel.max()}
    for k, rel in bars.items():
        print('%-14s kernel %.8f torch route %.8f, difference %.3g, bar %.3g' % (k, tb[k], tb_t[k], abs(tb[k] - tb_t[k]), FACTOR * rel * abs(tb_t[k])))
        assert abs(tb[k] - tb_t[k]) <= FACTOR * rel * abs(tb_t[k]), k
    assert abs(loss - loss_t) <= FACTOR * e_rel.max() * abs(loss_t)


def test_training_step_is_bit_reproducible(dev):
    torch.use_deterministic_algorithms(True)
    try:
        a, b = _step(dev), _step(dev)
    finally:
        torch.use_deterministic_algorithms(False)
    assert a[0] == b[0] and a[1] == b[1]
    diff = [n for n in a[2] if not torch.equal(a[2][n], b[2][n])]
    assert not diff, diff


def _eval_pass(dev, device_route, thresh=None):
    from pcdet.models.dense_heads import anchor_head_multi as ahm
    cfg, model = _detector(dev, seeded=True)
    if thresh is not None:
        cfg.MODEL.POST_PROCESSING.SCORE_THRESH = thresh
    model.eval()
    ahm.MULTICLASS_NMS = device_route
    try:
        with torch.no_grad(), no_fallback():
            bd = _batch(dev)
            pred, recall = model(bd)
    finally:
        ahm.MULTICLASS_NMS = True
    return cfg, model, pred, recall, bd


def test_eval_pass_on_both_nms_routes(dev):
    """the same pred dicts from the device route and from the per-segment loop. Seeded weights leave most of the map at one background
    value per head (ties, which the loop's topk may order either way): SCORE_THRESH is put between two scores of the batch above the
    first tie, at most 600 anchors from the top"""
    _, model, _, _, bd = _eval_pass(dev, True)
    scores = torch.cat([torch.sigmoid(c.float()).reshape(-1) for c in bd['batch_cls_preds']]).sort(descending=True)[0]
    top = scores[:601].double().cpu().numpy()
    tied = np.nonzero(np.diff(top) == 0)[0]
    n = int(tied[0]) if len(tied) else 600                                # top[:n] are distinct and above every tie
    print('distinct scores above the first tie: %d' % n)
    assert n >= 20 and top[n - 1] > top[n]
    thresh = float((top[n - 1] + top[n]) / 2)
    res = {}
    for route in (True, False):
        _, _, pred, recall, bd = _eval_pass(dev, route, thresh)
        assert ('batch_box_preds' in bd) == (not route)                   # the device route decodes the picks only
        res[route] = (pred, recall)
    pred, recall = res[True]
    assert len(pred) == 2 and sum(len(p['pred_scores']) for p in pred) > 0 and 'gt' in recall and recall == res[False][1]
    for p, q in zip(pred, res[False][0]):
        assert set(p) == set(q) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_logits'}
        n = len(p['pred_scores'])
        assert p['pred_boxes'].shape == (n, 7) and p['pred_labels'].dtype == torch.int64 and p['pred_logits'].shape == (n, 1)
        for k in p:
            assert torch.equal(p[k], q[k]), k
        assert torch.equal(torch.sigmoid(p['pred_logits'][:, 0]), p['pred_scores']) and bool((p['pred_scores'] >= thresh).all())
        lab = p['pred_labels'].tolist()
        assert lab == sorted(lab) and set(lab) <= {1, 2, 3}              # head order; best first inside a class
        for c in set(lab):
            s = p['pred_scores'][p['pred_labels'] == c]
            assert bool((s[:-1] >= s[1:]).all())


def test_random_strategy_evaluation_and_eval_one_epoch(dev, tmp_path):
    import random
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.query_strategies import build_strategy
    from pcdet.utils.eval_utils import eval_one_epoch
    cfg, model = _detector(dev, seeded=True)
    cfg.MODEL.POST_PROCESSING.SCORE_THRESH = 0.9
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': 'random', 'AGGREGATION': 'mean', 'SELECT_NUMS': 2})
    pool = SyntheticDataset(num_frames=4, first_frame=300, n_points=POINTS)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS)
    strat = build_strategy('random', model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 2), 0, str(tmp_path), cfg)
    random.seed(5)
    with no_fallback():
        picked = strat.query(cur_epoch=0)
    assert len(picked) == 2 and len(set(picked)) == 2 and set(picked) <= set(pool.sample_id_list), picked
    ds = SyntheticDataset(num_frames=4, training=False, n_points=POINTS)
    seen = []
    keep = ds.generate_prediction_dicts
    ds.generate_prediction_dicts = lambda *a, **k: seen.append(keep(*a, **k)) or seen[-1]
    with no_fallback():
        ret = eval_one_epoch(cfg, model, build_synthetic_dataloader(ds, batch_size=2))
    assert all('recall/rcnn_%s' % t in ret for t in (0.3, 0.5, 0.7)) and 'Car_3d/moderate_R40' in ret
    annos = [a for batch in seen for a in batch]
    assert len(annos) == 4
    text, ap = ds.evaluation(annos, ds.class_names)
    assert isinstance(text, str) and 'AP' in text and 'Car' in text and 'Cyclist' in text and isinstance(ap, dict)
