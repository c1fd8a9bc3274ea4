"""GPU: the anchor head's target, loss and proposal kernels (csrc/target_assign.hip, csrc/rpn_loss.hip, csrc/proposal_layer.hip) away
from the shipped 3-class / 2-bin / gamma 2 configuration, on the cases of tests/anchor_head_cases.py (checked on the CPU by
tests/test_anchor_head_limits_cpu.py). The reference is oracle/anchor_head_oracle.py — the per-frame, per-class restatement of the
reference assigner and losses, pinned by the reference's own golden — in float32 for the assignment (the kernel follows the f32
operations one for one) and in float64 for the losses; the proposal kernels claim bit equality with the torch expressions they
replace and are compared with those by torch.equal.

Tolerances: labels and regression weights exactly, regression targets 1e-6 (tests/test_target_assign_gpu.py's bound); gamma == 2 losses
5e-6 relative, gradients 2e-6 of the tensor's largest entry + 1e-5 relative (tests/test_rpn_loss_gpu.py's bounds); the powf
(gamma 1.5) and pure-L1 (beta 0) branches: twice the error of the f32 torch restatement against the float64 oracle, measured in the
test on the same inputs and device, plus that floor."""
import types

import numpy as np
import pytest
import torch

import anchor_head_cases as C

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- target assignment
class spy_method(list):
    """counts the calls of a method (one entry per call) without changing what it does; restore() puts the original back"""

    def __init__(self, cls, name):
        super().__init__()
        real = getattr(cls, name)
        self.restore = lambda: setattr(cls, name, real)
        setattr(cls, name, lambda obj, *a: (self.append(1), real(obj, *a))[1])


def fused_assign(dev, n, G, B, grid, seed, expect_fused):
    """head.assign_targets on the device -> host arrays; the route is asserted, not assumed"""
    from pcdet.models.dense_heads.target_assigner import axis_aligned_target_assigner as T
    gt, labels, targets, weights = C.assign_reference(n, G, B, grid, seed)
    head, _, _ = C.make_head(n, grid=grid)
    head = head.to(dev)
    calls = spy_method(T.AxisAlignedTargetAssigner, 'assign_targets_fused')
    try:
        assert T.FUSED
        out = head.assign_targets(torch.from_numpy(gt.copy()).to(dev))
    finally:
        calls.restore()
    assert len(calls) == (1 if expect_fused else 0)
    assert all(v.is_cuda for v in out.values()) and out['box_cls_labels'].dtype == torch.int32
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got['box_cls_labels'].shape == labels.shape and got['box_reg_targets'].shape == targets.shape
    return got, labels, targets, weights


def assert_assignment(got, labels, targets, weights):
    np.testing.assert_array_equal(got['box_cls_labels'], labels)
    np.testing.assert_array_equal(got['reg_weights'], weights)
    np.testing.assert_allclose(got['box_reg_targets'], targets, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('name', C.CLASS_COUNT_CASES)
def test_fused_assigner_class_counts(dev, name):
    n, G, B, grid, seed = C.ASSIGN_CASES[name]
    got, labels, targets, weights = fused_assign(dev, n, G, B, grid, seed, expect_fused=True)
    for c in range(1, n + 1):          # per class id: a class the kernel loses shows here by name
        want = (labels == c).sum(1)
        assert want.max() >= 3
        np.testing.assert_array_equal((got['box_cls_labels'] == c).sum(1), want, err_msg='positives of class id %d' % c)
        np.testing.assert_array_equal(got['box_cls_labels'] == c, labels == c, err_msg='positives of class id %d' % c)
    assert_assignment(got, labels, targets, weights)


@pytest.mark.parametrize('name', ['gt255', 'gt256', 'gt257', 'gt700', 'gt1024', 'anchors210', 'anchors768', 'anchors1080'])
def test_fused_assigner_table_sizes_and_anchor_tails(dev, name):
    got, labels, targets, weights = fused_assign(dev, *C.ASSIGN_CASES[name], expect_fused=True)
    assert_assignment(got, labels, targets, weights)


def test_more_ground_truths_than_the_kernel_stages_take_the_torch_route(dev):
    got, labels, targets, weights = fused_assign(dev, *C.ASSIGN_CASES['gt1025'], expect_fused=False)
    assert_assignment(got, labels, targets, weights)


@pytest.mark.parametrize('class_id,fused', [(63, True), (64, False)])
def test_class_id_at_and_past_the_presence_table(dev, class_id, fused):
    """the kernel keeps one presence flag per class id up to 63: id 63 runs fused, id 64 takes the torch route; both match the oracle"""
    from pcdet.models.dense_heads.target_assigner import axis_aligned_target_assigner as T
    gt, labels, targets, weights = C.high_id_reference(class_id)
    head, _, _ = C.make_head(C.HIGH_ID_NAMES, anchor_classes=[class_id - 1])
    head = head.to(dev)
    calls = spy_method(T.AxisAlignedTargetAssigner, 'assign_targets_fused')
    try:
        out = head.assign_targets(torch.from_numpy(gt.copy()).to(dev))
    finally:
        calls.restore()
    assert len(calls) == (1 if fused else 0)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert int((got['box_cls_labels'] == class_id).sum()) == int((labels == class_id).sum()) >= 3
    assert_assignment(got, labels, targets, weights)


def test_no_ground_truth_rows_label_everything_background(dev):
    from pcdet.models.dense_heads.target_assigner import axis_aligned_target_assigner as T
    got, labels, targets, weights = fused_assign(dev, *C.NO_BOXES, expect_fused=False)
    assert_assignment(got, labels, targets, weights)
    assert not got['box_cls_labels'].any() and not got['box_reg_targets'].any() and not got['reg_weights'].any()
    head, _, _ = C.make_head(3)
    head = head.to(dev)
    T.FUSED = False
    try:
        out = head.assign_targets(torch.zeros((3, 0, 8), device=dev))
    finally:
        T.FUSED = True
    assert_assignment({k: v.cpu().numpy() for k, v in out.items()}, labels, targets, weights)


def test_kernel_reports_what_it_does_not_support(dev):
    """the C entry point itself: more than 1,024 rows or a class id above 63 is CRB_ERR_UNSUPPORTED, no rows is CRB_ERR_ARG; nothing
    is launched in either case"""
    from crbhip import lib, ptr, cur_stream
    B, A = 1, 4
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    anchors, acls = z(A, 7), torch.ones(A, dtype=torch.int32, device=dev)
    lab, tgt, w = z(B, A, dt=torch.int32), z(B, A, 7), z(B, A)

    def call(G, n_thr):
        gt, valid, thr = z(B, max(G, 1), 8), z(B, max(G, 1), dt=torch.uint8), z(n_thr)
        wsb = lib.crb_assign_targets_workspace_bytes(B, A, max(G, 1))
        ws = z(wsb, dt=torch.uint8)
        return lib.crb_assign_targets(ptr(anchors), ptr(acls), A, ptr(gt), ptr(valid), B, G, ptr(thr), ptr(thr), n_thr, ptr(lab),
                                      ptr(tgt), ptr(w), ptr(ws), wsb, cur_stream(dev))
    assert call(1025, 2) == -4 and call(4, 65) == -4 and call(0, 2) == -1
    assert call(1024, 64) == 0
    torch.cuda.synchronize(dev)


# ------------------------------------------------------------------------------------------------------------------------ RPN loss
def device_loss(head, ref, dev, fused, reduce):
    from pcdet.models.dense_heads import anchor_head_template as aht
    leaves = {k: v.to(dev).requires_grad_(True) for k, v in ref['preds'].items()}
    head.forward_ret_dict = {'box_cls_labels': ref['labels'].to(dev), 'box_reg_targets': ref['targets'].to(dev)}
    head.forward_ret_dict.update(leaves)
    old = aht.FUSED_LOSS
    aht.FUSED_LOSS = fused
    try:
        loss, tb = head.get_loss(reduce=reduce)
    finally:
        aht.FUSED_LOSS = old
    (loss if reduce else (loss * torch.tensor(C.FRAME_WEIGHTS, device=dev))).sum().backward()
    if reduce:
        vec = torch.stack([loss.detach(), tb['rpn_loss_cls'], tb['rpn_loss_loc'], tb['rpn_loss_dir']])
        assert float(tb['rpn_loss']) == float(loss)
    else:
        vec = loss.detach()
    return vec, {k: v.grad for k, v in leaves.items()}


def loss_errors(vec, grads, ref):
    """-> relative error of every loss entry (nan where the oracle's is 0), {tensor: largest absolute gradient error}"""
    want = ref['loss'].numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.abs(vec.double().cpu().numpy() - want) / np.abs(want)
    return rel, {k: float((grads[k].double().cpu() - ref['grads'][k]).abs().max()) for k in grads}


def check_loss_case(dev, name, baseline):
    """fused losses and gradients of a case against the float64 oracle. baseline=False: the documented gamma == 2 bounds;
    baseline=True: twice the error of the f32 torch restatement (measured here) on top of them. -> the measured figures"""
    nc, nb, gamma, beta, reduce, grid = C.LOSS_CASES[name]
    ref = C.loss_reference(name)
    head, _, _ = C.make_head(nc, num_dir_bins=nb, gamma=gamma, beta=beta, grid=grid)
    head = head.to(dev)
    assert head._fused_loss_cfg() is not None
    vec, grads = device_loss(head, ref, dev, True, reduce)
    rel, gerr = loss_errors(vec, grads, ref)
    base_rel, base_gerr = np.zeros_like(rel), {k: 0.0 for k in gerr}
    if baseline:
        b_vec, b_grads = device_loss(head, ref, dev, False, reduce)
        base_rel, base_gerr = loss_errors(b_vec, b_grads, ref)
    print('\n%s: relative loss error fused %s, f32 restatement %s' % (name, rel, base_rel))
    want = ref['loss'].numpy()
    tol = (2.0 * np.nan_to_num(base_rel) + 5e-6) * np.abs(want) + 1e-9
    assert (np.abs(vec.double().cpu().numpy() - want) <= tol).all(), (rel, base_rel)
    for k in grads:
        r = ref['grads'][k].numpy()
        print('%s: %s gradient error fused %.3e, f32 restatement %.3e, scale %.3e' % (name, k, gerr[k], base_gerr[k], np.abs(r).max()))
        assert torch.isfinite(grads[k]).all()
        bad = np.abs(grads[k].double().cpu().numpy() - r) > 2.0 * base_gerr[k] + 2e-6 * np.abs(r).max() + 1e-5 * np.abs(r)
        assert not bad.any(), '%s: %d entries off, worst %.3e (scale %.3e)' % (k, bad.sum(), gerr[k], np.abs(r).max())
    # bit-reproducible
    vec2, grads2 = device_loss(head, ref, dev, True, reduce)
    assert torch.equal(vec2, vec) and all(torch.equal(grads2[k], grads[k]) for k in grads)
    return rel, gerr, base_rel, base_gerr


@pytest.mark.parametrize('name', ['nc2_nb2', 'nc5_nb3', 'nc8_nb8', 'nc3_nb1', 'nc3_strip_tail', 'nc8_nb8_per_frame'])
def test_fused_rpn_loss_class_and_bin_counts(dev, name):
    check_loss_case(dev, name, baseline=False)


def test_fused_rpn_loss_powf_branch(dev):
    """gamma = 1.5: focal_term takes powf(pt, gamma) and gamma * powf(pt, gamma - 1) instead of pt * pt and 2 pt; torch.pow and the
    device's powf are different f32 implementations, so the bound is 2 x the f32 torch restatement's own error against the float64
    oracle (same inputs, same device) + the gamma == 2 floor (5e-6 relative on the losses, 2e-6 max|ref| + 1e-5 |ref| on the
    gradients).
    Measured on an MI355X (relative error of total / cls / loc / dir loss; largest absolute gradient error):
      f32 restatement  losses 3.4e-8 / 6.0e-8 / 7.7e-8 / 9.8e-10; d cls 1.63e-7 (largest entry 0.272), d box 3.99e-9 (0.0267),
                       d dir 2.78e-10 (0.0026)
      kernel           losses 1.1e-7 / 1.4e-7 / 7.7e-8 / 9.5e-8;  d cls 1.33e-7, d box 3.30e-9, d dir 2.78e-10
      bound            cls loss 2 * 6.0e-8 + 5e-6 = 5.12e-6 relative; d cls 2 * 1.63e-7 + 2e-6 * 0.272 = 8.7e-7 (+ 1e-5 |ref|)"""
    check_loss_case(dev, 'gamma1.5', baseline=True)


def test_fused_rpn_loss_pure_l1_branch(dev):
    """beta = 0: smooth_l1 is |diff| with gradient sign(diff) (0 at 0), the branch WeightedSmoothL1Loss takes for beta < 1e-5. Bound as
    for the powf branch: 2 x the f32 torch restatement's error against the float64 oracle + the beta = 1/9 floor.
    Measured on an MI355X (relative error of total / cls / loc / dir loss; largest absolute gradient error):
      f32 restatement  losses 2.5e-8 / 6.1e-9 / 2.3e-8 / 9.8e-10; d cls 2.24e-7 (largest entry 0.282), d box 3.30e-9 (0.0267),
                       d dir 2.78e-10 (0.0026)
      kernel           losses 2.5e-8 / 6.1e-9 / 5.4e-8 / 9.5e-8;  d cls 1.94e-7, d box 3.22e-9, d dir 2.78e-10
      bound            loc loss 2 * 2.3e-8 + 5e-6 = 5.05e-6 relative; d box 2 * 3.30e-9 + 2e-6 * 0.0267 = 6.0e-8 (+ 1e-5 |ref|)"""
    check_loss_case(dev, 'beta0', baseline=True)


def test_nine_classes_take_the_torch_losses_and_match_the_oracle(dev):
    nc, nb, gamma, beta, reduce, grid = C.LOSS_CASES['nc9']
    ref = C.loss_reference('nc9')
    head, _, _ = C.make_head(nc, num_dir_bins=nb, grid=grid)
    head = head.to(dev)
    assert head._fused_loss_cfg() is None
    vec, grads = device_loss(head, ref, dev, True, reduce)
    np.testing.assert_allclose(vec.double().cpu().numpy(), ref['loss'].numpy(), rtol=5e-6, atol=1e-9)
    for k in grads:
        r = ref['grads'][k].numpy()
        assert (np.abs(grads[k].double().cpu().numpy() - r) <= 2e-6 * np.abs(r).max() + 1e-5 * np.abs(r)).all(), k


# ---------------------------------------------------------------------------------------------------------------- proposal kernels
def spy(monkeypatch, name):
    """count the calls of a C entry point without changing it"""
    from crbhip import lib
    real, calls = getattr(lib, name), []
    monkeypatch.setattr(lib, name, lambda *a: (calls.append(1), real(*a))[1])
    return calls


def quotient_sensitive_residuals(anchor_rot, period):
    """heading residuals e (f32) of an anchor with this rotation for which v = (e + rot) - DIR_OFFSET lies so close to a multiple of
    the period that floor(v / period) and floor(v * (1 / period)) differ in f32: found by scanning the 81 floats around every
    multiple -12 .. 12, with the f32 operations of the decode"""
    f = np.float32
    off, rot, inv = f(C.DIR_OFFSET), f(anchor_rot), f(1) / period
    out = []
    for m in range(-12, 13):
        e0 = np.array([f(f(f(m) * period + off) - rot)], np.float32)
        e = (e0.view(np.int32)[0] + np.arange(-40, 41)).astype(np.int32).view(np.float32)
        v = ((e + rot).astype(np.float32) - off).astype(np.float32)
        out += list(e[np.floor((v / period).astype(np.float32)) != np.floor((v * inv).astype(np.float32))])
    return out


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('k', [0, 1, 300])
@pytest.mark.parametrize('nb', [2, 4, None])
def test_decode_of_selected_anchors_equals_the_torch_expressions(dev, monkeypatch, nb, k, B):
    """crb_decode_selected_anchors through AnchorHeadTemplate.generate_predicted_boxes(anchor_idx=...) against the torch route of the
    same method. The indices hold anchor 0 and anchor A - 1; 35 of the headings (k = 300) are placed 0, 1 and 2 ulp on either side of
    a multiple of the direction period and 60 on values where floor(v / period) depends on whether the quotient is a division or a
    multiplication by the reciprocal (the two give headings a whole period apart there)."""
    from pcdet.models.dense_heads import anchor_head_template as AH
    head, _, _ = C.make_head(3, num_dir_bins=nb or 2)
    head = head.to(dev).eval()
    rs = np.random.RandomState(40 + k + B)
    preds = C.make_preds(head, B, 77 + k)
    cls, box = preds['cls_preds'].to(dev), preds['box_preds'].to(dev)
    dirs = preds['dir_cls_preds'].to(dev) if nb else None
    A = head.anchors[0].numel() // 7 * 3
    idx = rs.randint(0, A, (B, k))
    if k:
        idx[0, 0], idx[-1, -1] = 0, A - 1
    if k >= 100 and nb:
        period = np.float32(2 * np.pi / nb)
        a6 = torch.cat(head.anchors, dim=-3).reshape(-1, 7)[:, 6].cpu().numpy()
        flat = box.view(B, A, 7)
        for j in range(35):
            v = np.float32((j % 7 - 3)) * period
            for _ in range(abs(j // 7 - 2)):
                v = np.nextafter(v, np.float32(np.inf if j // 7 > 2 else -np.inf), dtype=np.float32)
            ai = idx[B - 1, 1 + j]
            flat[B - 1, ai, 6] = float(np.float32(v + np.float32(C.DIR_OFFSET)) - a6[ai])
        n_hit = 0
        for j in range(40, 100):
            ai = idx[B - 1, j]
            hits = quotient_sensitive_residuals(a6[ai], period)
            assert len(hits) >= 2
            flat[B - 1, ai, 6] = float(hits[j % len(hits)])
            n_hit += 1
        assert n_hit == 60
    idx = torch.from_numpy(idx).to(dev)
    calls = spy(monkeypatch, 'crb_decode_selected_anchors')
    assert AH.FUSED_DECODE
    f_cls, f_box = head.generate_predicted_boxes(B, cls, box, dirs, anchor_idx=idx)
    assert len(calls) == 1
    monkeypatch.setattr(AH, 'FUSED_DECODE', False)
    t_cls, t_box = head.generate_predicted_boxes(B, cls, box, dirs, anchor_idx=idx)
    assert len(calls) == 1
    assert f_box.shape == t_box.shape == (B, k, 7) and f_box.dtype == t_box.dtype == torch.float32
    assert torch.equal(f_cls, t_cls)
    if not torch.equal(f_box, t_box):
        d = (f_box != t_box).nonzero()
        raise AssertionError('%d entries differ, first %s: %r vs %r' % (d.shape[0], d[0].tolist(), float(f_box[tuple(d[0])]),
                                                                       float(t_box[tuple(d[0])])))
    if k:      # and both are the rows of the full decode at these indices
        full = head.generate_predicted_boxes(B, cls, box, dirs)[1]
        assert torch.equal(torch.gather(full, 1, idx[..., None].expand(-1, -1, 7)), t_box)


@pytest.mark.parametrize('nc', [1, 8])
def test_proposal_finish_equals_the_torch_expressions(dev, monkeypatch, nc):
    """crb_proposal_finish through RoIHeadTemplate.proposal_layer against the torch route of the same method, with the NMS result
    replaced by a hand-made keep table: frame 0 full (first and last top-k position among them), frame 1 with a -1 tail, frame 2 all
    -1 (every slot padded). B * post = 300 threads: a partial second block."""
    from pcdet.config import EasyDict
    from pcdet.models.roi_heads import roi_head_template as RH
    B, A, k, post = 3, 1000, 300, 100
    g = torch.Generator().manual_seed(5 + nc)
    cls = (torch.randn(B, A, nc, generator=g) * 2).to(dev)
    boxes = torch.randn(B, A, 7, generator=g).to(dev)
    keep = torch.full((B, post), -1, dtype=torch.int32)
    keep[0] = torch.randperm(k, generator=g)[:post].int()
    keep[0, 0], keep[0, 1] = 0, k - 1
    keep[1, :37] = torch.randperm(k, generator=g)[:37].sort()[0].int()
    keep = keep.to(dev)
    monkeypatch.setattr(RH.iou3d_nms_utils, 'nms_batched', lambda *a, **kw: (keep, None))
    cfg = EasyDict({'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.8, 'NMS_PRE_MAXSIZE': k, 'NMS_POST_MAXSIZE': post})
    calls = spy(monkeypatch, 'crb_proposal_finish')
    run = lambda: RH.RoIHeadTemplate.proposal_layer(types.SimpleNamespace(), {'batch_cls_preds': cls, 'batch_box_preds': boxes,
                                                                             'batch_size': B}, cfg)
    assert RH.FUSED_PROPOSAL
    fused = run()
    assert len(calls) == 1
    monkeypatch.setattr(RH, 'FUSED_PROPOSAL', False)
    ref = run()
    assert len(calls) == 1
    for key in ('rois', 'roi_scores', 'roi_labels', 'full_cls_scores'):
        assert fused[key].shape == ref[key].shape and fused[key].dtype == ref[key].dtype, key
        assert torch.equal(fused[key], ref[key]), key
    assert fused['has_class_labels'] == ref['has_class_labels'] == (nc > 1)
    assert fused['rois'].shape == (B, post, 7) and not fused['rois'][2].any() and not fused['rois'][1, 37:].any()
    assert (fused['roi_labels'][2] == 1).all() and not fused['roi_scores'][2].any() and not fused['full_cls_scores'][2].any()
    assert fused['rois'][0].abs().sum(-1).min() > 0
