"""CPU: the cases of tests/iou3d_edge_cases.py are what they claim, and the oracle (oracle/iou3d_oracle.c, the reference's rotated
overlap / IoU / NMS restated) is well-behaved on them - so that tests/test_iou3d_edges_gpu.py may hold the kernels to 2e-5 there.

Bar: 2e-5 * max(1, value) per entry, the figure of tests/test_iou3d_gpu.py (the two sides evaluate f32 sin / cos / atan2 with
different libraries)."""
import numpy as np
import pytest

import oracle
import iou3d_edge_cases as E

BAR = 2e-5
ULP_YAW = np.float32(2.0 ** -23)                  # the size of a one-ulp sinf / cosf disagreement


def bar(v):
    return BAR * np.maximum(1.0, np.abs(v))


def pair_values(a, b, mode):
    """oracle value of every pair (a[i], b[i])"""
    return np.array([oracle.boxes_pairwise(a[i:i + 1], b[i:i + 1], mode)[0, 0] for i in range(len(a))], np.float64)


def test_case_list_is_complete_and_named_once():
    fam = E.family_cases()
    assert len(fam) + len(E.UNSTABLE) == 14 * len(E.CENTRES) * len(E.YAWS) == 196
    assert len(E.UNSTABLE) <= 0.05 * 196
    names = [c['name'] for c in E.pair_cases()]
    assert len(set(names)) == len(names)
    a, b = E.stack(E.pair_cases())
    assert a.dtype == b.dtype == np.float32 and np.isfinite(a).all() and np.isfinite(b).all()
    assert (a[:, 3:6] >= 0).all() and (b[:, 3:6] >= 0).all()                     # negative sizes are out of the contract


def test_closed_forms():
    cases = [c for c in E.family_cases() if c['k'] in E.CLOSED_FAMILIES]
    assert len(cases) >= 9 * 14 - len(E.UNSTABLE)
    a, b = E.stack(cases)
    got = pair_values(a, b, 0)
    want = np.array([c['closed'] for c in cases])
    ratio = np.abs(got - want) / bar(want)
    for k in E.CLOSED_FAMILIES:
        sel = [i for i, c in enumerate(cases) if c['k'] == k]
        print('closed form, family %2d %-11s worst |oracle - closed| / bar = %.3f' % (k, E.FAMILY_NAMES[k], ratio[sel].max()))
    assert (ratio <= 1).all(), [cases[i]['name'] for i in np.flatnonzero(ratio > 1)]
    # IoU of the cases that are one rectangle written twice
    same = [c for c in cases if c['k'] in (1, 4, 8, 14)]
    a, b = E.stack(same)
    assert (np.abs(pair_values(a, b, 1) - 1.0) <= BAR).all()


def test_family_cases_are_stable_under_one_ulp_of_yaw():
    """+-2^-23 on every yaw, 60 seeded draws: overlap and IoU of every family case move by at most half the bar. A condition on the
    cases, not a tolerance: a case that misses it goes to iou3d_edge_cases.UNSTABLE."""
    cases = E.family_cases()
    a, b = E.stack(cases)
    base = {m: pair_values(a, b, m) for m in (0, 1)}
    worst = {m: np.zeros(len(cases)) for m in (0, 1)}
    rng = np.random.default_rng(2024)
    for _ in range(60):
        a2, b2 = a.copy(), b.copy()
        a2[:, 6] += rng.choice([-ULP_YAW, ULP_YAW], len(cases))
        b2[:, 6] += rng.choice([-ULP_YAW, ULP_YAW], len(cases))
        for m in (0, 1):
            worst[m] = np.maximum(worst[m], np.abs(pair_values(a2, b2, m) - base[m]) / bar(base[m]))
    print('one-ulp yaw disturbance on %d family cases: worst move / bar = %.3f (overlap), %.3f (IoU)'
          % (len(cases), worst[0].max(), worst[1].max()))
    bad = [cases[i]['name'] for i in range(len(cases)) if max(worst[0][i], worst[1][i]) > 0.5]
    assert not bad, bad


def test_margin_pairs_have_the_reference_overlap_of_disjoint_boxes():
    for c in E.margin_cases():
        ov = oracle.boxes_pairwise(c['a'][None], c['b'][None], 0)[0, 0]
        iou = oracle.boxes_pairwise(c['a'][None], c['b'][None], 1)[0, 0]
        d = np.linalg.norm(c['a'][:2].astype(np.float64) - c['b'][:2])
        assert d > c['a'][3] + 1e-3                                              # end to end: disjoint rectangles
        if c['gap_mm'] <= 9:
            assert ov > 0 and iou > 0, c['name']
            assert abs(ov - c['a'][4] * c['gap_mm'] * 1e-3) <= 1e-6             # the strip between the facing edges
        else:
            assert ov == 0 and iou == 0, c['name']
    # the table of the issue: IoU at 9 mm
    want = {'margin_4x0.2/gap9mm': 1.13e-3, 'margin_0.8x0.1/gap9mm': 5.66e-3, 'margin_2x0.15/gap9mm': 2.26e-3,
            'margin_1x0.12/gap9mm': 4.52e-3}
    for c in E.margin_cases():
        if c['name'] in want:
            assert abs(oracle.boxes_pairwise(c['a'][None], c['b'][None], 1)[0, 0] - want[c['name']]) < 1e-5
    a, b = E.tiny_pair()
    assert abs(oracle.boxes_pairwise(a[None], b[None], 1)[0, 0] - 4800.0) < 1.0
    # from 9 mm on they lie beyond the circumscribed circles (what csrc/iou3d_nms.hip's reject has to allow for), and all that
    # the reference gives an overlap lie within MARGIN * sqrt(2) of them
    for c in [c for c in E.pair_cases() if c['family'] in ('margin', 'tiny')]:
        ra, rb = 0.5 * np.hypot(c['a'][3], c['a'][4]), 0.5 * np.hypot(c['b'][3], c['b'][4])
        d = np.linalg.norm(c['a'][:2].astype(np.float64) - c['b'][:2])
        if c['family'] == 'tiny' or c['gap_mm'] >= 9:
            assert d > ra + rb, c['name']
        if c['family'] == 'tiny' or c['gap_mm'] <= 9:
            assert d < ra + rb + E.MARGIN * np.sqrt(2)


def test_z_variants_and_zero_sizes():
    cases = E.z_cases()
    a, b = E.stack(cases)
    got = pair_values(a, b, 2)
    want = np.array([c['iou3d'] for c in cases])
    assert (np.abs(got - want) <= BAR).all()
    for c in E.pair_cases():
        if c['family'] == 'zero':
            for m in (0, 1, 2):
                assert oracle.boxes_pairwise(c['a'][None], c['b'][None], m)[0, 0] == 0


@pytest.mark.skipif(not oracle.have_ref_iou3d(), reason='oracle/_ref not built (needs the reference sources)')
def test_oracle_is_bit_equal_to_the_reference_build_on_every_pair_case():
    a, b = E.stack(E.pair_cases())
    np.testing.assert_array_equal(oracle.boxes_pairwise(a, b, 1), oracle.ref_boxes_iou_bev(a, b))


# ---------------------------------------------------------------------------------------------------------------- NMS sets
def small_sets():
    return [E.duplicates(), E.nan_rows(), E.zero_size(), E.block_edges(130), E.block_edges(4160)] + [E.thin(n) for n in E.THIN_SETS]


def assert_margin_safe(boxes, thresh):
    """the rule of test_iou3d_gpu._margin_safe: no pair within 1e-4 of the threshold. -> the (i, j) with a non-zero IoU"""
    iou = oracle.boxes_pairwise(boxes, boxes, 1)
    np.fill_diagonal(iou, thresh + 1.0)
    assert not (np.abs(iou - thresh) < 1e-4).any()
    np.fill_diagonal(iou, 0.0)
    i, j = np.nonzero(iou > 0)
    return set(zip(i.tolist(), j.tolist()))


@pytest.mark.parametrize('s', small_sets(), ids=lambda s: s['name'])
def test_nms_sets_oracle_gives_the_picks_expected_by_construction(s):
    for (thresh, rotated), want in s['picks'].items():
        np.testing.assert_array_equal(oracle.nms(s['boxes'], thresh, rotated), want, err_msg='%s %r %r' % (s['name'], thresh, rotated))
    if s['name'] == 'nan_rows':
        return
    for thresh in {t for t, _ in s['picks'] if t > 0}:
        touching = assert_margin_safe(s['boxes'], thresh)
        if 'planted' in s:                                                       # every overlap at all is a planted one (or one of
            b = s['boxes']                                                       # its copies): the lattice itself is disjoint
            involved = {i for p in s['planted'] for i in p[:2]}
            same = lambda i, j: np.array_equal(b[i], b[j])                       # noqa: E731
            for i, j in touching:
                assert any(same(i, k) for k in involved) and any(same(j, k) for k in involved), (i, j)


def planted_iou_ok(kind, v):
    return {'copy': v > 0.99, 'partial': abs(v - 0.3) < 1e-3, 'chain_ab': abs(v - 0.6) < 1e-3, 'chain_bc': abs(v - 0.6) < 1e-3,
            'chain_ac': abs(v - 1 / 3) < 1e-3, 'margin': v > 1e-3 + 1e-4}[kind]


@pytest.mark.parametrize('n', E.BLOCK_EDGE_N)
def test_block_edge_sets_by_construction(n):
    """what makes the expected picks true without an n^2 oracle pass (the only check of the 32,768 set): the planted pairs have the
    IoUs they were built for, the lattice pitch exceeds the largest box diagonal plus the reject's pad, and a planted box is out
    of reach of every box but its partners"""
    s = E.block_edges(n)
    b = s['boxes']
    for i, j, kind in s['planted']:
        v = oracle.boxes_pairwise(b[i:i + 1], b[j:j + 1], 1)[0, 0]
        assert planted_iou_ok(kind, v), (i, j, kind, v)
    r = 0.5 * np.hypot(b[:, 3], b[:, 4]).astype(np.float64)
    assert E.PITCH > 2 * r.max() + 0.015
    xy = b[:, :2].astype(np.float64)
    partners = {}
    for i, j, _ in s['planted']:
        partners.setdefault(i, set()).add(j)
        partners.setdefault(j, set()).add(i)
    for i, ps in partners.items():
        d = np.linalg.norm(xy - xy[i], axis=1)
        near = np.flatnonzero(d <= r + r[i] + 0.015)
        for k in near:
            # in reach: itself, a partner, or a box that is a copy / partner of a partner (a chain, a copy of a partial)
            ok = k == i or k in ps or any(k in partners.get(q, ()) for q in ps)
            assert ok, (i, int(k))
    # rows that are not planted sit on their own lattice cell
    planted_rows = np.array(sorted(partners))
    rest = np.setdiff1d(np.arange(n), planted_rows)
    side = int(np.ceil(np.sqrt(n)))
    cell = (np.stack([rest % side, rest // side], 1) - (side - 1) / 2.0) * E.PITCH
    assert np.abs(xy[rest] - cell).max() < 1e-3
    keep = s['picks'][(0.5, True)]
    assert len(keep) == n - sum(1 for p in s['planted'] if p[2] in ('copy', 'chain_ab'))


@pytest.mark.parametrize('nmax,max_keep', E.PREFIX_CONFIGS)
@pytest.mark.parametrize('twin', [False, True], ids=['two_stage', 'single_stage_twin'])
def test_prefix_frames_oracle_gives_the_picks_expected_by_construction(nmax, max_keep, twin):
    p = E.prefix_len(max_keep)
    assert nmax == 2 * p and (max_keep, p) in ((8, 1024), (600, 1216))
    boxes, counts, picks, names = (E.prefix_twin if twin else E.prefix_frames)(nmax, max_keep)
    assert boxes.shape[1] == (nmax - 1 if twin else nmax)
    assert counts[4] == p and counts[5] == p + 1 and counts[6] == 0 and counts[7] == 1 and counts[8] == boxes.shape[1]
    assert picks[2][-1] == p - 1 and picks[3][-1] == p and len(picks[2]) == len(picks[3]) == max_keep
    assert len(picks[4]) < max_keep and picks[5][-1] == p and p + 1 not in picks[9] and p in picks[9]
    for f, name in enumerate(names):
        n = int(counts[f])
        # a greedy pick depends on the earlier rows only: rows after the max_keep-th pick need no oracle pass
        m = min(n, int(picks[f][-1]) + 2) if len(picks[f]) == max_keep else n
        for rotated in (True, False):
            got = oracle.nms(boxes[f, :m], 0.5, rotated)[:max_keep]
            np.testing.assert_array_equal(got, picks[f], err_msg='%s rotated=%r' % (name, rotated))
    assert_margin_safe(boxes[0, :E.prefix_len(max_keep) + 70], 0.5)              # one lattice under all frames; the rest are copies
