"""CPU: the hand-built cases of tests/sa_scatter_cases.py have the index patterns their names claim (decoded from the rows, in pair
order and in source-row order), their ReLU-edge cap holds, and sa_fixed_point_scale (the host arithmetic of the deterministic
scatter) gives a valid scale with a true bound on a grid of maxima."""
import math

import numpy as np
import pytest
import torch

import sa_scatter_cases as S


def _runs(a):
    """[(start, length, value)] of the runs of equal values of a 1-d array"""
    a = np.asarray(a)
    cut = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1]]))
    return [(int(s), int(e - s), int(a[s])) for s, e in zip(cut, np.concatenate([cut[1:], [len(a)]]))]


def _sorted_rows(c):
    key = S.sort_key(c)
    return key[np.argsort(key, kind='stable')]


def test_widths_and_sizes():
    hs = [S.WIDTH[n] for n in S.NAMES]
    assert all(hs.count(h) >= 2 for h in (16, 32, 64, 128)) and set(hs) == {16, 32, 64, 128}
    for name in S.NAMES:
        c = S.case(name)
        assert c['n_src'] <= 12000 and c['M'] <= 2100
        assert c['ns'] == {'padded_ns32': 32, 'padded_ns48': 48}.get(name, 16)
        assert c['grad_z'].shape == (c['n'], c['H']) and c['P'].shape == (c['n_src'], c['H'])
        for k in ('xyz', 'new_xyz', 'P', 'W1x', 'grad_z', 'mean', 'invstd', 'gamma', 'beta', 'dbeta', 'dgamma'):
            assert c[k].dtype == np.float32 and np.isfinite(c[k]).all(), (name, k)


def test_one_row():
    c = S.case('one_row')
    assert c['M'] == 515 and c['n'] % 64 != 0
    assert len(np.unique(c['row'])) == 1 and not c['empty'].any()
    assert _runs(_sorted_rows(c)) == [(0, c['n'], int(c['row'][0, 0]))]          # one run through every segment of every slab


def test_two_rows():
    c, r = S.case('two_rows'), S.reference('two_rows')
    rows, counts = np.unique(c['row'], return_counts=True)
    assert len(rows) == 2 and counts.min() > c['n'] // 3 and c['n'] % 64 != 0
    g = r['grad_P'][torch.from_numpy(rows)]
    # opposite sums (up to the f32 rounding of dbeta / dgamma and the entries zeroed at the ReLU edge), far above the rounding level
    assert float((g[0] + g[1]).abs().max()) <= 1e-2 * float(g.abs().max()) and float(g.abs().max()) > 1e-2 * float(r['mag'].max())


def test_all_distinct():
    c = S.case('all_distinct')
    assert c['M'] % 4 == 1 and len(np.unique(c['row'])) == c['n'] and c['B'] == 2


@pytest.mark.parametrize('name', ['padded', 'padded_ns32', 'padded_ns48', 'tiny', 'huge'])
def test_padded(name):
    c = S.case(name)
    js = set()
    for r in c['row']:
        j = len(np.unique(r))
        assert len(np.unique(r[:j])) == j and (r[j:] == r[0]).all()             # j distinct hits, then the first hit again
        js.add(j)
    assert 1 in js and c['ns'] in js and len(js) >= c['ns'] // 2
    assert c['n'] % 64 != 0


def test_tiny_and_huge_are_padded_scaled():
    p, t, h = S.case('padded'), S.case('tiny'), S.case('huge')
    assert t['row'].shape == p['row'].shape == h['row'].shape
    assert 0 < np.abs(t['grad_z']).max() < 1.1754944e-38                       # subnormal maxima
    assert 1e30 < np.abs(h['grad_z']).max() < 1e31
    assert 0 < np.abs(t['dbeta']).max() < 1.1754944e-38


def test_alternating():
    c = S.case('alternating')
    kinds = set()
    for r in c['row']:
        k = len(np.unique(r))
        assert k in (2, 3) and (r == r[:k][np.arange(16) % k]).all()
        assert all(r[i] != r[i + 1] for i in range(15))                         # no repeat is adjacent
        kinds.add(k)
    assert kinds == {2, 3}


def test_borders():
    c = S.case('borders')
    runs = _runs(_sorted_rows(c))
    assert [l for _, l, _ in runs[:len(S.BORDER_RUNS)]] == list(S.BORDER_RUNS)
    ends = {(s + l - 1) % 64 for s, l, _ in runs[:len(S.BORDER_RUNS)]}
    assert {14, 15, 16, 62, 63, 0} <= ends                                      # just before / at / just after a segment and a slab border
    whole = set()                                                               # whole 16-pair segments covered by one run
    two_slabs = 0
    for s, l, _ in runs:
        first, last = -(-s // 16), (s + l) // 16
        if s % 16 == 0 and (s + l) % 16 == 0:
            whole.add(last - first)
        two_slabs += s // 64 != (s + l - 1) // 64
    assert {1, 2, 3, 5} <= whole and two_slabs >= 3
    assert c['n'] % 64 != 0


def test_empties():
    c = S.case('empties')
    e, cnt = c['empty'], c['new_xyz_batch_cnt']
    assert cnt[0] == 0 and cnt[-1] == 0 and c['B'] == 5
    lo = int(cnt[:2].sum())
    assert e[lo:lo + cnt[2]].all() and cnt[2] > 0                               # a frame with queries, all empty
    assert e[8:12].all() and (8 * c['ns']) % 64 == 0                            # queries 8..11: one whole slab
    assert not e[7] and not e[12]                                               # ... between live balls
    assert any(e[i] and not e[i - 1] and not e[i + 1] for i in range(1, len(e) - 1))
    assert 0.3 < e.mean() < 0.7 and (c['idx'][e] == 0).all()


def test_outlier():
    c, r = S.case('outlier'), S.reference('outlier')
    assert int((c['row'] == 0).sum()) == 1
    assert np.abs(c['P'][0]).mean() > 500 * np.abs(c['P'][1:]).mean()
    assert float(r['xhat'].abs().max()) > 0.9 * math.sqrt(c['n'])
    assert (c['grad_z'] >= 0).all()
    d = np.abs(c['grad_z']).max()
    assert np.abs(c['dbeta']).max() / c['n'] > 0.3 * d                          # dbeta / n is of the size of max |d|
    old_R = float(d) * S.maxima(c)[1]                                           # what the parent commit took for a bound
    assert float(r['v'].abs().max()) > 20.0 * old_R


def test_exact():
    c, r = S.case('exact'), S.reference('exact')
    assert not c['xyz'].any() and not c['new_xyz'].any() and (c['beta'] == 100).all()
    g = c['grad_z'].astype(np.float64) * 1024
    assert (g == np.round(g)).all() and np.abs(g).max() <= 8
    assert (np.abs(c['P']) + 0 < 100).all()                                     # z = P + 100 > 0: the mask is all on
    assert np.array_equal(r['v'].numpy(), c['grad_z'].astype(np.float64))
    assert float(r['mag'].max()) * 1024 < 2 ** 24                                # every partial sum is an integer below 2^24 (times 2^-10)
    assert int((c['row'] == c['row'][0, 0]).sum()) >= 320


@pytest.mark.parametrize('name', S.NAMES)
def test_relu_edge_cap_and_bound(name):
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils import sa_fixed_point_scale
    c, r = S.case(name), S.reference(name)
    assert c['edge_touched'] <= S.EDGE_CAP
    # batch statistics: |xhat| <= sqrt(n), and the helper's bound holds for every case
    assert float(r['xhat'][r['live']].abs().max()) <= math.sqrt(c['n']) or name == 'exact'
    scale, bound = sa_fixed_point_scale(*S.maxima(c), c['n'])
    assert float(r['v'].abs().max()) <= bound
    assert float(r['mag'].max()) * scale < 2.0 ** 62


GRID = (0.0, 1e-45, 1e-38, 1e-30, 1.0, 1e30, 3e38)


@pytest.mark.parametrize('n', [16, 2 ** 10, 2 ** 22, 2 ** 24])
def test_scale_helper_on_a_grid(n):
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils import sa_fixed_point_scale
    for gz in GRID:
        for gi in GRID:
            for db in GRID:
                for dg in GRID:
                    m = [float(np.float32(x)) for x in (gz, gi, db, dg)]
                    scale, bound = sa_fixed_point_scale(*m, n)
                    mant, _ = math.frexp(scale)
                    assert mant == 0.5 and 2.0 ** -126 <= scale <= 2.0 ** 127, (m, scale)      # a normal f32 power of two
                    assert float(np.float32(scale)) == scale
                    assert 0.0 <= bound <= 3.4028234663852886e38
                    assert bound >= min(m[1] * (m[0] + m[2] / n + m[3] / math.sqrt(n)), 3.4028234663852886e38)
                    assert scale * bound * n < 2.0 ** 63, (m, scale, bound)
                    # the fractional bits that remain are spent: twice the scale would not fit with every pair on one row
                    assert scale == 2.0 ** 127 or 2 * scale * 2.0 ** math.frexp(bound)[1] * 2.0 ** (n - 1).bit_length() >= 2.0 ** 63


def test_outlier_at_n_pairs_on_one_row_stays_inside_int64():
    """float64 simulation of the fixed-point sum: every one of the n pairs carries the largest addend of `outlier` onto one row"""
    from pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils import sa_fixed_point_scale
    c, r = S.case('outlier'), S.reference('outlier')
    scale, bound = sa_fixed_point_scale(*S.maxima(c), c['n'])
    worst = float(r['v'].abs().max())
    assert worst <= bound
    total = sum(int(round(worst * scale)) for _ in range(64)) * (c['n'] // 64 + 1)           # python integers: no wrap
    assert total < 2 ** 63 and c['n'] * int(round(bound * scale)) < 2 ** 63
    # the parent commit's scale, 2^40 / (a power of two >= max |grad_z| max |gamma invstd|): the same sum at the RoI-grid pair count
    d, gi = S.maxima(c)[0], S.maxima(c)[1]
    old = 2.0 ** (40 - math.frexp(d * gi)[1])
    assert 7 * 2 ** 20 * int(round(worst * old)) >= 2 ** 63
