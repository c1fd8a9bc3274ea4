"""CPU: the cases of tests/anchor_head_cases.py are what they claim, and the host routes of the anchor head — the batched torch
assigner and the torch restatement of the RPN losses, which the device path falls back to beyond the kernels' limits — agree with
oracle/anchor_head_oracle.py (the per-frame, per-class restatement of the reference, pinned by the reference's golden) on every one
of them: 1 .. 10 classes, 0 .. 1,025 ground-truth rows, four anchor counts, 1 .. 8 direction bins, gamma 1.5, beta 0.

Tolerances: labels and weights exactly, regression targets 1e-6 (tests/test_target_assign_gpu.py's bound); losses in f32 against the
float64 oracle 5e-6 relative, gradients 2e-6 of the tensor's largest entry + 1e-5 relative (tests/test_rpn_loss_gpu.py's bounds)."""
import numpy as np
import pytest
import torch

import anchor_head_cases as C
from oracle import anchor_head_oracle as aho


@pytest.mark.parametrize('n_classes,grid', [(1, C.GRID), (10, C.GRID), (3, C.GRID_UNDER_BLOCK), (3, C.GRID_BLOCK_MULTIPLE),
                                            (3, C.GRID_STRIP_TAIL)])
def test_head_anchors_are_the_oracle_anchors_and_have_the_stated_count(n_classes, grid):
    head, cfgs, names = C.make_head(n_classes, grid=grid)
    ref = C.oracle_anchors(n_classes, grid)
    assert len(head.anchors) == len(ref) == n_classes
    for a, r in zip(head.anchors, ref):
        assert torch.equal(a, r)
    A = sum(a.numel() // 7 for a in ref)
    assert A == grid[0] * grid[1] * 2 * n_classes
    if grid == C.GRID_UNDER_BLOCK:
        assert A < 256
    if grid == C.GRID_BLOCK_MULTIPLE:
        assert A % 256 == 0
    if grid == C.GRID_STRIP_TAIL:
        assert A > 1024 and 0 < A % 1024 < 256
    np.testing.assert_array_equal(C.anchor_class_ids(n_classes, grid),
                                  head.target_assigner._fused_constants(head.anchors)[1].numpy())


@pytest.mark.parametrize('name', sorted(C.ASSIGN_CASES))
def test_case_meets_the_conditions_on_the_oracle_alone(name):
    n, G, B, grid, seed = C.ASSIGN_CASES[name]
    gt, labels, targets, weights = C.assign_reference(n, G, B, grid, seed)
    A = grid[0] * grid[1] * 2 * n
    assert gt.shape == (B, G, 8) and labels.shape == (B, A) and targets.shape == (B, A, 7) and weights.shape == (B, A)
    cls_of = C.anchor_class_ids(n, grid)
    # the knobs
    assert (gt[0, 0] == gt[0, C.ROW_DUP]).all() and gt[0, 0, 7] > 0
    assert (gt[0, G // 2] == 0).all() and (gt[0, G // 2 + 1] != 0).any()                       # a zero row inside the frame
    assert (gt[1, -2:] == 0).all() and (gt[1, -3] != 0).any()                                    # ragged
    assert (gt[-1] == 0).all()                                                                   # a frame without boxes
    assert (gt[0, C.ROW_ZERO_SIZE, 3:6] == 0).all() and gt[0, C.ROW_ZERO_SIZE, 7] > 0 and gt[0, C.ROW_ZERO_SIZE].sum() != 0
    flat = torch.cat([a.reshape(-1, 7) for a in C.oracle_anchors(n, grid)])
    assert float(aho.nearest_bev_iou(flat, torch.from_numpy(gt[0, C.ROW_OUTSIDE:C.ROW_OUTSIDE + 1, :7].copy())).max()) == 0.0
    assert set(np.unique(gt[..., 7]).astype(int)) == set(range(0, n + 1))
    # every class has at least 3 positives in some frame, and positives carry their own class id
    pos = labels > 0
    assert (labels[pos] == np.broadcast_to(cls_of, labels.shape)[pos]).all()
    for c in range(1, n + 1):
        assert ((labels == c).sum(1) >= 3).any(), 'class %d' % c
    assert (labels == -1).any()
    # an anchor that is positive only because it is forced: its best overlap is below its class's matched threshold
    best = C.best_overlaps(n, grid, gt)
    matched = np.array([0.0] + [C.class_row(i)[2] for i in range(n)], np.float32)
    assert (pos & (best < matched[cls_of][None])).any()
    assert (pos & (best >= matched[cls_of][None])).any()
    # the frame without boxes: everything background
    assert (labels[-1] == 0).all() and (targets[-1] == 0).all() and (weights[-1] == 0).all()
    np.testing.assert_array_equal(weights, pos.astype(np.float32))
    assert np.isfinite(targets).all() and (targets[~pos] == 0).all()


@pytest.mark.parametrize('name', sorted(C.ASSIGN_CASES) + ['no_boxes'])
def test_batched_torch_assigner_equals_the_oracle(name):
    n, G, B, grid, seed = C.NO_BOXES if name == 'no_boxes' else C.ASSIGN_CASES[name]
    gt, labels, targets, weights = C.assign_reference(n, G, B, grid, seed)
    head, _, _ = C.make_head(n, grid=grid)
    out = head.assign_targets(torch.from_numpy(gt.copy()))
    assert out['box_cls_labels'].dtype == torch.int32 and out['box_cls_labels'].shape == labels.shape
    np.testing.assert_array_equal(out['box_cls_labels'].numpy(), labels)
    np.testing.assert_array_equal(out['reg_weights'].numpy(), weights)
    np.testing.assert_allclose(out['box_reg_targets'].numpy(), targets, rtol=1e-6, atol=1e-6)
    if name == 'no_boxes':
        assert not labels.any() and not targets.any() and not weights.any()


@pytest.mark.parametrize('class_id', [63, 64])
def test_batched_torch_assigner_equals_the_oracle_for_a_lone_high_class_id(class_id):
    gt, labels, targets, weights = C.high_id_reference(class_id)
    assert set(np.unique(gt[..., 7]).astype(int)) == {0, 2, class_id}
    assert set(np.unique(labels)) == {-1, 0, class_id} and ((labels == class_id).sum(1) >= 3).any()
    head, _, _ = C.make_head(C.HIGH_ID_NAMES, anchor_classes=[class_id - 1])
    assert head.target_assigner.max_class_id == class_id
    out = head.assign_targets(torch.from_numpy(gt.copy()))
    np.testing.assert_array_equal(out['box_cls_labels'].numpy(), labels)
    np.testing.assert_array_equal(out['reg_weights'].numpy(), weights)
    np.testing.assert_allclose(out['box_reg_targets'].numpy(), targets, rtol=1e-6, atol=1e-6)


def host_loss(head, ref, reduce):
    """get_loss of the head on the case's host tensors -> loss, tb_dict, gradients of the objective"""
    leaves = {k: v.clone().requires_grad_(True) for k, v in ref['preds'].items()}
    head.forward_ret_dict = {'box_cls_labels': ref['labels'], 'box_reg_targets': ref['targets']}
    head.forward_ret_dict.update(leaves)
    loss, tb = head.get_loss(reduce=reduce)
    (loss if reduce else (loss * torch.tensor(C.FRAME_WEIGHTS))).sum().backward()
    return loss.detach(), tb, {k: v.grad for k, v in leaves.items()}


def close_to_oracle(got, ref, what, extra=0.0):
    got, ref = got.detach().double().cpu().numpy(), ref.numpy()
    tol = 2e-6 * np.abs(ref).max() + 1e-5 * np.abs(ref) + extra
    bad = np.abs(got - ref) > tol
    assert not bad.any(), '%s: %d entries off, worst %.3e (scale %.3e)' % (what, bad.sum(), np.abs(got - ref).max(), np.abs(ref).max())


@pytest.mark.parametrize('name', sorted(C.LOSS_CASES))
def test_torch_loss_restatement_equals_the_float64_oracle(name):
    nc, nb, gamma, beta, reduce, grid = C.LOSS_CASES[name]
    ref = C.loss_reference(name)
    lab = ref['labels']
    assert int((lab > 0).sum()) > 8 and int((lab < 0).sum()) > 0 and int((lab[-1] > 0).sum()) == 0
    assert int(torch.isnan(ref['targets']).sum()) >= 3 and int((ref['preds']['cls_preds'] == 0).sum()) >= 3
    assert torch.isfinite(ref['loss']).all() and all(torch.isfinite(g).all() for g in ref['grads'].values())
    # every prediction tensor takes part (one direction bin: softmax of one logit, loss and gradient are 0)
    assert all(g.abs().max() > 0 for k, g in ref['grads'].items() if not (k == 'dir_cls_preds' and nb == 1))
    head, _, _ = C.make_head(nc, num_dir_bins=nb, gamma=gamma, beta=beta, grid=grid)
    loss, tb, grads = host_loss(head, ref, reduce)
    if reduce:
        got = [float(loss), float(tb['rpn_loss_cls']), float(tb['rpn_loss_loc']), float(tb['rpn_loss_dir'])]
        np.testing.assert_allclose(got, ref['loss'].numpy(), rtol=5e-6, atol=1e-9)
    else:
        np.testing.assert_allclose(loss.double().numpy(), ref['loss'].numpy(), rtol=5e-6)
    for k in grads:
        close_to_oracle(grads[k], ref['grads'][k], k)
