"""GPU parity of csrc/iou3d_bev.h / csrc/iou3d_nms.hip on the hand-built cases of tests/iou3d_edge_cases.py (degenerate rectangles,
boxes inside the reference's corner margin, suppressions across the words and registers of the scan's bitmap, the switch to the
prefix stage) against the oracle. tests/test_iou3d_edges_cpu.py shows that the cases are what they claim and that the oracle
itself moves by a third of the bar at most under a one-ulp change of a yaw.

Values: |hip - oracle| <= 2e-5 * max(1, oracle) per entry. NMS picks: identical.

test_pairwise_edge_cases prints the worst |hip - oracle| / bar of every family; its docstring has the figures of an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

import oracle
import iou3d_edge_cases as E

pytestmark = pytest.mark.gpu

BAR = 2e-5
NA = (1, 4, 5)
NB = (1, 63, 64, 65, 130)


def _t(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev)                      # a copy: the cases are read-only arrays


def _U():
    from pcdet.ops.iou3d_nms import iou3d_nms_utils as U
    return U


@pytest.mark.parametrize('mode', [0, 1, 2], ids=['overlap', 'iou_bev', 'iou3d'])
def test_pairwise_edge_cases(dev, mode):
    """Every pair case as entry (i, i) of full na x nb matrices, na in NA (the kernel's tile has 4 rows), nb in NB (64 columns): the
    rows are the `a` boxes of na consecutive cases, the columns the `b` boxes of the nb cases from the same start, the list taken
    cyclically; the other entries pair boxes of different cases (family 'cross'). Per entry against the oracle.

    Worst |hip - oracle| / bar per family on MI355X (overlap / BEV IoU / 3-D IoU); 0.000 = the same bits in every case:
      shift_v      0.006 / 0.006 / 0.006        near_copy    0.074 / 0.077 / 0.077
      swapped_lw   0.004 / 0.012 / 0.012        yaw_2pi      0.008 / 0.018 / 0.018
      cross        0.185 / 0.164 / 0.164 (yaw_pi x near_copy at the far centre)
      identical, shift_u, nested, nested_rot, short_edge, yaw_pi, yaw_neg, concentric, corner, straddle, zero, tiny, margin,
      z_same, z_touch, z_nested, z_flat: 0.000 / 0.000 / 0.000"""
    U = _U()
    fn = (U.boxes_overlap_bev, U.boxes_iou_bev, U.boxes_iou3d_gpu)[mode]
    cases = E.pair_cases()
    a, b = E.stack(cases)
    n = len(cases)
    da, db = _t(a, dev), _t(b, dev)
    fam = np.array([c['family'] for c in cases])
    worst = {f: 0.0 for f in list(dict.fromkeys(fam)) + ['cross']}
    worst_at = {}
    for na in NA:
        for nb in NB:
            for k in range(0, n, na):
                ia, ib = (k + np.arange(na)) % n, (k + np.arange(nb)) % n
                got = fn(da[torch.from_numpy(ia).to(dev)], db[torch.from_numpy(ib).to(dev)]).cpu().numpy()
                ref = oracle.boxes_pairwise(a[ia], b[ib], mode)
                assert got.shape == ref.shape == (na, nb)
                ratio = np.abs(got.astype(np.float64) - ref) / (BAR * np.maximum(1.0, np.abs(ref)))
                ratio[~np.isfinite(got)] = np.inf
                design = ia[:, None] == ib[None, :]
                for i, j in zip(*np.nonzero(design)):
                    f = fam[ia[i]]
                    if ratio[i, j] > worst[f]:
                        worst[f], worst_at[f] = ratio[i, j], (cases[ia[i]]['name'], na, nb, float(got[i, j]), float(ref[i, j]))
                cross = np.where(design, 0.0, ratio)
                if cross.max() > worst['cross']:
                    i, j = np.unravel_index(cross.argmax(), cross.shape)
                    worst['cross'] = cross[i, j]
                    worst_at['cross'] = (cases[ia[i]]['name'] + ' x ' + cases[ib[j]]['name'], na, nb, float(got[i, j]), float(ref[i, j]))
    for f, w in worst.items():
        print('mode %d family %-12s worst |hip - oracle| / bar = %.3f %s' % (mode, f, w, worst_at.get(f, '')))
    bad = {f: (w, worst_at[f]) for f, w in worst.items() if not w <= 1.0}
    assert not bad, bad
    # the margin pairs and the 4 mm boxes: the reference's non-zero areas, not the 0 of a geometric clipper
    sel = np.flatnonzero((fam == 'margin') | (fam == 'tiny'))
    got = np.diagonal(fn(da[torch.from_numpy(sel).to(dev)], db[torch.from_numpy(sel).to(dev)]).cpu().numpy())
    for i, v in zip(sel, got):
        assert (v == 0) == (cases[i].get('gap_mm') == 12), (cases[i]['name'], v)


def test_pairwise_writes_nothing_outside_na_x_nb(dev):
    """na = 5 is one row into the second 4-row tile, nb = 65 one column into the second 64-column tile: the threads of the padded
    tile must not write. The output lies inside a larger buffer of sentinels."""
    from crbhip import lib, check, ptr, cur_stream
    cases = E.pair_cases()
    a, b = E.stack(cases)
    for na, nb in ((5, 65), (1, 1), (4, 63), (5, 130)):
        A, B = _t(a[:na], dev), _t(b[:nb], dev)
        guard = 4096
        for mode in (0, 1, 2):
            buf = torch.full((guard + na * nb + guard,), -7.0, dtype=torch.float32, device=dev)
            out = buf[guard:guard + na * nb]
            check(lib.crb_boxes_pairwise(ptr(A), na, ptr(B), nb, ctypes.c_void_p(out.data_ptr()), mode, cur_stream(dev)),
                  'crb_boxes_pairwise')
            h = buf.cpu().numpy()
            assert (h[:guard] == -7.0).all() and (h[guard + na * nb:] == -7.0).all()
            ref = oracle.boxes_pairwise(a[:na], b[:nb], mode)
            np.testing.assert_allclose(h[guard:guard + na * nb].reshape(na, nb), ref, rtol=0, atol=BAR * max(1.0, ref.max()))


# ---------------------------------------------------------------------------------------------------------------- NMS picks
def nms_sets():
    return ([E.duplicates, E.nan_rows, E.zero_size] + [lambda n=n: E.block_edges(n) for n in E.BLOCK_EDGE_N]
            + [lambda n=n: E.thin(n) for n in E.THIN_SETS])


NMS_SET_IDS = ['duplicates', 'nan_rows', 'zero_size'] + ['block_edges_%d' % n for n in E.BLOCK_EDGE_N] + list(E.THIN_SETS)


@pytest.mark.parametrize('make', nms_sets(), ids=NMS_SET_IDS)
def test_nms_picks_on_hand_built_sets(dev, make):
    """nms_gpu / nms_normal_gpu (scores descending with the row, so the returned indices are the rows) and the fixed-size
    nms_batched output (num, the -1 tail) against the picks each set expects by construction - which the oracle confirms on the CPU
    for every set but the 32,768-box one. The thin and tiny sets hold pairs beyond their circumscribed circles that the reference
    suppresses through its corner margin: they fail on a reject that stops at the circles."""
    U = _U()
    s = make()
    b = _t(s['boxes'], dev)
    n = len(s['boxes'])
    scores = torch.arange(n, 0, -1, device=dev).float()
    for (thresh, rotated), want in s['picks'].items():
        keep, _ = (U.nms_gpu if rotated else U.nms_normal_gpu)(b, scores, thresh)
        np.testing.assert_array_equal(keep.cpu().numpy(), want, err_msg='%s thresh %r rotated %r' % (s['name'], thresh, rotated))
        kb, num = U.nms_batched(b[None], None, thresh, n, rotated=rotated)
        kb, num = kb.cpu().numpy()[0], int(num.cpu().numpy()[0])
        assert num == len(want)
        np.testing.assert_array_equal(kb[:num], want)
        assert (kb[num:] == -1).all()


def _run_prefix(dev, boxes, counts, max_keep, rotated):
    keep, num = _U().nms_batched(_t(boxes, dev), _t(counts, dev), 0.5, max_keep, rotated=rotated)
    return keep.cpu().numpy(), num.cpu().numpy()


def _check_prefix(keep, num, picks, names, what):
    for f, name in enumerate(names):
        assert num[f] == len(picks[f]), (what, name, int(num[f]), len(picks[f]))
        np.testing.assert_array_equal(keep[f, :num[f]], picks[f], err_msg='%s %s' % (what, name))
        assert (keep[f, num[f]:] == -1).all(), (what, name)


@pytest.mark.parametrize('rotated', [True, False], ids=['rotated', 'axis_aligned'])
@pytest.mark.parametrize('nmax,max_keep', E.PREFIX_CONFIGS)
def test_batched_nms_prefix_stage_at_its_edges(dev, nmax, max_keep, rotated):
    """nmax = 2 p switches the prefix stage on (p = 1,024 and p = 1,216), nmax - 1 keeps the single stage. One call holds all the
    frames of iou3d_edge_cases.prefix_frames - decided in the prefix, undecided, empty - and every frame must give the picks it
    was built for, in both configurations, alone as in the batch, and again into a workspace that another call has used."""
    boxes, counts, picks, names = E.prefix_frames(nmax, max_keep)
    assert E.prefix_len(max_keep) * 2 == nmax
    keep, num = _run_prefix(dev, boxes, counts, max_keep, rotated)
    _check_prefix(keep, num, picks, names, 'two-stage')
    # the single-stage twin: the same first max_keep picks (below its last row)
    tb, tc, tp, _ = E.prefix_twin(nmax, max_keep)
    tkeep, tnum = _run_prefix(dev, tb, tc, max_keep, rotated)
    _check_prefix(tkeep, tnum, tp, names, 'single-stage twin')
    for f in range(len(names)):
        m = int(tnum[f])
        np.testing.assert_array_equal(tkeep[f, :m], keep[f, :m])
    # decided and undecided frames do not disturb each other: every frame alone gives its row of the batch
    for f in range(len(names)):
        k1, n1 = _run_prefix(dev, boxes[f:f + 1], counts[f:f + 1], max_keep, rotated)
        assert n1[0] == num[f]
        np.testing.assert_array_equal(k1[0], keep[f])
    # the same allocation pattern again, after a call that left other masks and `done` flags in the workspace
    order = np.arange(len(names))[::-1]
    rk, rn = _run_prefix(dev, boxes[order], counts[order], max_keep, rotated)
    np.testing.assert_array_equal(rk[order], keep)
    np.testing.assert_array_equal(rn[order], num)
    keep2, num2 = _run_prefix(dev, boxes, counts, max_keep, rotated)
    np.testing.assert_array_equal(keep2, keep)
    np.testing.assert_array_equal(num2, num)


def test_nms_limits(dev):
    """nmax = 32,769 is one box more than the scan's bitmap holds (8 words per lane): CRB_ERR_UNSUPPORTED before anything is launched
    (the call gets no workspace, so it could not run anyway). nmax = 0: num 0, keep all -1."""
    from crbhip import lib, ptr, cur_stream
    B, max_keep = 2, 16
    keep = torch.full((B, max_keep), 7, dtype=torch.int32, device=dev)
    num = torch.full((B,), 7, dtype=torch.int32, device=dev)
    boxes = torch.zeros((B, 1, 7), dtype=torch.float32, device=dev)
    for rotated in (1, 0):
        rc = lib.crb_nms_batched(ptr(boxes), None, B, 32769, 0.5, rotated, max_keep, ptr(keep), ptr(num), None, 0, cur_stream(dev))
        assert rc == -4                                                          # CRB_ERR_UNSUPPORTED
    torch.cuda.synchronize(dev)
    assert (keep.cpu().numpy() == 7).all() and (num.cpu().numpy() == 7).all()
    assert lib.crb_nms_batched(ptr(boxes), None, B, 32768, 0.5, 1, max_keep, ptr(keep), ptr(num), None, 0, cur_stream(dev)) == -2
    k0, n0 = _U().nms_batched(torch.zeros((B, 0, 7), dtype=torch.float32, device=dev), None, 0.5, max_keep)
    assert (k0.cpu().numpy() == -1).all() and (n0.cpu().numpy() == 0).all()
    k0, n0 = _U().nms_batched(torch.zeros((B, 0, 7), dtype=torch.float32, device=dev),
                              torch.zeros((B,), dtype=torch.int32, device=dev), 0.5, max_keep, rotated=False)
    assert (k0.cpu().numpy() == -1).all() and (n0.cpu().numpy() == 0).all()
