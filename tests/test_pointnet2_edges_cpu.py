"""CPU: the point-set edge cases (tests/pointnet2_edge_cases.py) are what their names claim, the C oracle equals the independent numpy
references on every one of them (indices exact, f32 values bit-exact, gradients within the rounding bound of a sum), the cases tell
deliberately wrong references apart, and crb_ball_query2_grid_workspace_bytes covers a call without points. No GPU."""
import numpy as np
import pytest

import oracle
import pointnet2_edge_cases as E

BALL = {c['name']: c for c in E.ball_cases() + E.grouped_cases()}
FPS = {c['name']: c for c in E.fps_cases()}
NN = {c['name']: c for c in E.three_nn_cases()}
INTERP = {c['name']: c for c in E.interp_cases()}
GROUP = {c['name']: c for c in E.group_cases()}


def _radii(case):
    return sorted({(r, n) for ra, na, rb, nb in case['pairs'] for r, n in ((ra, na), (rb, nb))})


def _ref(case, r, ns, mutant=None):
    return E.ref_ball_query(r, ns, case['xyz'], case['xyz_cnt'], case['new_xyz'], case['new_cnt'], mutant=mutant)


# ------------------------------------------------------------------------------------------------------------------ the cases are what they claim
def test_the_lists_cover_what_the_kernels_branch_on():
    assert {c['claims']['variant'] for c in E.fps_cases() if c['name'].startswith('ties_')} == \
        {'fps2_kernel<4>', 'fps2_kernel<8>', 'fps2_kernel<20>', 'fps_kernel<40,false>', 'fps_large_kernel'}
    for lo, hi in ((4096, 4097), (8192, 8193), (20480, 20481), (40960, 40961)):          # both sides of every dispatch boundary
        assert E.fps_variant(lo) != E.fps_variant(hi) and 'n%d' % lo in FPS and 'n%d' % hi in FPS
    frames = BALL['frames']
    assert tuple(frames['xyz_cnt']) == E.POINT_CNT and tuple(frames['new_cnt']) == E.QUERY_CNT and len(frames['new_xyz']) == 79
    assert [len(BALL['one_frame_M%d' % m]['new_xyz']) for m in E.M_TOTALS] == list(E.M_TOTALS)
    assert (BALL['frames_negative']['xyz'] < 0).all() and (BALL['frames_negative']['new_xyz'][1:6] < 0).all()
    kinds = set()
    for c in BALL.values():
        for ra, na, rb, nb in c['pairs']:
            kinds.add('lt' if ra < rb else 'gt' if ra > rb else 'eq' if na != nb else 'same')
            assert c['xyz_cnt'].sum() == len(c['xyz']) and c['new_cnt'].sum() == len(c['new_xyz'])
    assert {'lt', 'gt', 'eq'} <= kinds
    for g, c in ((c['group'], c) for c in E.grouped_cases()):
        assert all(n % g == 0 for n in c['new_cnt'])                                     # no group across a frame boundary
    assert {c['group'] for c in E.grouped_cases()} == {1, 7, 216}
    zero = [c for c in E.grouped_cases() if c['xyz_cnt'][0] == 0 and c['new_cnt'][0] >= c['group']]
    assert zero, 'a group inside a frame of zero points'


def test_frames_have_full_partial_and_empty_balls():
    for name in ('frames', 'frames_negative', 'one_frame_M79'):
        c = BALL[name]
        _, e08 = _ref(c, 0.8, 16)
        full = [E.hits_inside(c, q, 1.6) for q in range(len(c['new_xyz']))]
        assert e08.sum() >= 10 and (~e08).sum() >= 20
        assert max(full) > 65 and any(0 < h < 16 for h in (E.hits_inside(c, q, 0.8) for q in range(len(c['new_xyz']))))


def test_exact_radius_points_lie_on_the_sphere_in_f32():
    c = BALL['exact_radius']
    r2 = E.F32(1.25) * E.F32(1.25)
    q = c['new_xyz']
    assert (E.d2_f32(q, c['claims']['on_sphere'])[0] == r2).all()
    d_in = E.d2_f32(q, c['claims']['inside'])[0]
    assert (d_in < r2).all() and (d_in[:2] == np.nextafter(r2, E.F32(0))).all()          # one ulp inside
    assert (E.d2_f32(q, c['claims']['outside'])[0] > r2).all()
    for p in (c['xyz'], q):                                                              # exact in f32: the f64 expression agrees
        assert (p.astype(np.float64) * 2 ** 24 % 1 == 0).all()
    on = c['claims']['on_sphere'].astype(np.float64)
    assert (((on - q.astype(np.float64)) ** 2).sum(1) == 1.5625).all()                   # on the sphere exactly, not by rounding
    idx, empty = _ref(c, 1.25, 16)
    is_in = (c['xyz'][:, None] == c['claims']['inside'][None]).all(2).any(1)
    assert sorted(set(idx[0])) == sorted(np.flatnonzero(is_in)) and len(set(idx[0])) == 4 and not empty[0]


@pytest.mark.parametrize('ns', E.HIT_NSAMPLES)
def test_hit_count_cases_have_exactly_the_hits_they_name(ns):
    for delta in (-1, 0, 1):
        c = BALL['hits_ns%d%+d' % (ns, delta)]
        for r in (0.5, 1.0):
            assert [E.hits_inside(c, q, r) for q in range(3)] == [ns + delta, ns + delta, 0]
        at = c['claims']['hit_at']
        if ns + delta >= 64:
            assert at[0] < 64 <= at[-1]                                                  # the hits cross a 64-candidate step
        idx, empty = _ref(c, 0.5, ns)
        assert list(idx[0][:min(ns, len(at))]) == list(at[:ns]) and empty[0] == (len(at) == 0)


def test_nth_and_first_hit_positions():
    for pos in (63, 64):
        c = BALL['hit16_at_%d' % pos]
        idx, _ = _ref(c, 0.5, 16)
        assert idx[0, 15] == pos and idx[0, 14] < pos and E.hits_inside(c, 0, 0.5) == 19
        assert _ref(c, 0.5, 17)[0][0, 16] == pos + 1
    for pos in (64, 129):
        c = BALL['first_hit_at_%d' % pos]
        idx, _ = _ref(c, 0.5, 16)
        assert list(idx[0]) == [pos, pos + 3, pos + 70] + [pos] * 13


def test_cell_edge_points_are_multiples_of_the_cell():
    c = BALL['cell_edges']
    k = c['xyz'].astype(np.float64) / float(c['claims']['edge'])
    assert np.abs(k - np.round(k)).max() < 1e-6 and set(np.round(k).astype(int).ravel()) == set(range(-3, 4))
    cells = E.grid_cells_of(c['xyz'], 0.8)
    assert (np.abs(cells - np.round(k)) <= 1).all()             # f32 floor(x / edge): the point's own cell or the one below


def test_collision_case_repeats_buckets_inside_a_query():
    c = BALL['collisions']
    assert E.grid_buckets(len(c['xyz'])) == 1024
    cells = E.grid_cells_of(c['new_xyz'], 0.5)
    lo = np.array(E.COLLISION_BLOCK)
    for pts in (cells, E.grid_cells_of(c['xyz'], 0.5)):
        assert (pts >= lo).all() and (pts < lo + 4).all()
    frame = np.repeat(np.arange(2), c['new_cnt'])
    repeated = sum(len(np.unique(E.grid_bucket(frame[q], cells[q][None] + E.NEIGHBOURS, 1024))) < 27 for q in range(len(cells)))
    assert repeated >= 20, repeated


@pytest.mark.parametrize('name,path', [('grid_T4096_H1024', 'selection'), ('grid_T4096_H1025', 'fall-back by H'),
                                       ('grid_T4097_H1024', 'fall-back by T')])
def test_grid_threshold_cases_count_exactly(name, path):
    c = BALL[name]
    T, H = E.grid_candidates(c, 0, 1.0), E.hits_inside(c, 0, 1.0)
    assert (T, H) == (c['claims']['T'], c['claims']['H']) == (len(c['xyz']), H)
    took = 'fall-back by T' if T > E.BQG_MAX_CAND else 'fall-back by H' if H > E.BQG_MAX_HITS else 'selection'
    assert took == path
    assert abs(E.grid_cells_of(c['xyz'], 1.0)).max() <= 1 and (E.grid_cells_of(c['new_xyz'][:1], 1.0) == 0).all()
    assert E.hits_inside(c, 0, 0.6) > 64 and E.hits_inside(c, 1, 1.0) == 0
    idx, _ = _ref(c, 1.0, 64)
    inside = np.flatnonzero(E.d2_f32(c['new_xyz'][:1], c['xyz'])[0] < 1)
    assert list(idx[0]) == list(inside[:64]) and (np.diff(inside) > 1).any()             # the hits are scattered through the storage order


def test_grouped_threshold_cases_fill_the_candidate_list():
    for n in (E.GQ_CAP, E.GQ_CAP + 1):
        c = {k['name']: k for k in E.grouped_cases()}['group_candidates_%d' % n]
        q = c['new_xyz'].astype(np.float64)
        centre = q.mean(0)
        R = np.linalg.norm(q - centre, axis=1).max()
        dist = np.linalg.norm(c['xyz'].astype(np.float64) - centre, axis=1)
        assert len(c['xyz']) == n and (dist < R + 0.6 - 0.05).all()                      # all inside the prefilter sphere, with margin
    co = {k['name']: k for k in E.grouped_cases()}['coincident_group7']
    assert (co['new_xyz'].reshape(-1, 7, 3) == co['new_xyz'].reshape(-1, 7, 3)[:, :1]).all()


def test_fps_tie_clouds_tie():
    for c in E.fps_cases():
        copies = c['claims'].get('copies')
        if not copies:
            continue
        m = c['ms'][-1]
        sizes = E.fps_tie_sizes(c['xyz'], m)
        if c['name'].startswith('ties_'):
            assert (sizes[:, 1:] % copies == 0).all() and (sizes[:, 1:] >= copies).all()
        else:                                                   # m == n with repeated points: the tail of the run is one full tie at 0
            n = c['xyz'].shape[1]
            assert (sizes[:, -1] == n).all() and (E.ref_fps(c['xyz'], m)[:, -1] == 0).all()


def test_three_nn_cases():
    c = NN['ragged']
    assert tuple(c['kcnt']) == (0, 1, 2, 3, 4, 300) and tuple(c['ucnt']) == (2, 0, 255, 256, 257, 5)
    last = NN['ragged_empty_known_last']
    assert last['kcnt'][-1] == 0 and last['ucnt'][-1] == 2
    d2, idx = E.ref_three_nn(last['unknown'], last['ucnt'], last['known'], last['kcnt'])
    assert (idx[-2:] == len(last['known'])).all() and np.isinf(d2[-2:]).all()            # past the end: not fed to interpolation
    assert not E.nn_usable(last)[-2:].any()
    dup = NN['duplicates']
    d2, _ = E.ref_three_nn(dup['unknown'], dup['ucnt'], dup['known'], dup['kcnt'])
    assert (d2[:257, 0] == d2[:257, 1]).sum() >= 80 and (d2[:, 0] == 0).sum() >= 80


# ------------------------------------------------------------------------------------------------------------------ oracle == numpy reference
@pytest.mark.parametrize('name', list(BALL))
def test_oracle_ball_query_equals_the_reference(name):
    c = BALL[name]
    for r, ns in _radii(c):
        got = oracle.ball_query(r, ns, c['xyz'], c['xyz_cnt'], c['new_xyz'], c['new_cnt'])
        idx, empty = _ref(c, r, ns)
        np.testing.assert_array_equal(got[:, 0] == -1, empty)
        got[empty, 0] = 0
        np.testing.assert_array_equal(got, idx)


@pytest.mark.parametrize('name', list(FPS))
def test_oracle_fps_equals_the_reference(name):
    c = FPS[name]
    for m in c['ms']:
        np.testing.assert_array_equal(oracle.fps(c['xyz'], m), E.ref_fps(c['xyz'], m))


@pytest.mark.parametrize('name', list(NN))
def test_oracle_three_nn_equals_the_reference(name):
    c = NN[name]
    d2, idx = oracle.three_nn(c['unknown'], c['ucnt'], c['known'], c['kcnt'])
    rd2, ridx = E.ref_three_nn(c['unknown'], c['ucnt'], c['known'], c['kcnt'])
    np.testing.assert_array_equal(idx, ridx)
    np.testing.assert_array_equal(d2, rd2)


def _within(got, ref64, count, mag):
    bad = np.abs(got.astype(np.float64) - ref64) > E.grad_bound(count, mag)
    assert not bad.any(), (int(bad.sum()), float(np.abs(got - ref64).max()))


@pytest.mark.parametrize('name', list(INTERP))
def test_oracle_interpolation_equals_the_reference(name):
    c = INTERP[name]
    np.testing.assert_array_equal(oracle.three_interpolate(c['feat'], c['idx'], c['w']), E.ref_three_interpolate(c['feat'], c['idx'], c['w']))
    _within(oracle.three_interpolate_grad(c['grad_out'], c['idx'], c['w'], c['M']),
            *E.ref_three_interpolate_grad64(c['grad_out'], c['idx'], c['w'], c['M']))


@pytest.mark.parametrize('name', list(GROUP))
def test_oracle_grouping_equals_the_reference(name):
    c = GROUP[name]
    np.testing.assert_array_equal(oracle.group_points(c['feat'], c['feat_cnt'], c['idx'], c['idx_cnt']),
                                  E.ref_group_points(c['feat'], c['feat_cnt'], c['idx'], c['idx_cnt']))
    ref, count, mag = E.ref_group_points_grad64(c['grad_out'], c['idx'], c['idx_cnt'], c['feat_cnt'], len(c['feat']))
    _within(oracle.group_points_grad(c['grad_out'], c['idx'], c['idx_cnt'], c['feat_cnt'], len(c['feat'])), ref, count, mag)
    if 'one_row' in name:
        assert count.max() == 157 * c["idx"].shape[1]                                    # every pair of a frame on one row


def test_lds_limit_cases_sit_on_the_limit():
    ns, C = E.LDS_FIT
    assert 4 * ns * (C + 1) == 64 * 1024
    assert all(4 * n * (c + 1) > 64 * 1024 for n, c in E.LDS_OVER)


# ------------------------------------------------------------------------------------------------------------------ the cases catch wrong references
@pytest.mark.parametrize('mutant', E.BALL_MUTANTS)
def test_ball_query_cases_catch(mutant):
    caught = [c['name'] for c in BALL.values() for r, ns in _radii(c)
              if any(not np.array_equal(a, b) for a, b in zip(_ref(c, r, ns), _ref(c, r, ns, mutant=mutant)))]
    assert caught, mutant
    if mutant == 'le':
        assert 'exact_radius' in caught
    if mutant == 'wrong_start':
        assert 'frames' in caught


@pytest.mark.parametrize('mutant', E.FPS_MUTANTS)
def test_fps_cases_catch(mutant):
    caught = [c['name'] for c in E.fps_cases() if c['claims'].get('copies') and c['xyz'].shape[1] > 3
              if not np.array_equal(E.ref_fps(c['xyz'], c['ms'][-1]), E.ref_fps(c['xyz'], c['ms'][-1], mutant=mutant))]
    assert caught, mutant
    if mutant == 'tie_plain_k':                                 # every launch variant sees a tie that the bit reversal decides
        assert {FPS[n]['claims']['variant'] for n in caught} >= {E.fps_variant(n) for n in E.FPS_TIE_SIZES}, caught


@pytest.mark.parametrize('mutant', E.NN_MUTANTS)
def test_three_nn_cases_catch(mutant):
    caught = [c['name'] for c in E.three_nn_cases()
              if not np.array_equal(E.ref_three_nn(c['unknown'], c['ucnt'], c['known'], c['kcnt'])[1],
                                    E.ref_three_nn(c['unknown'], c['ucnt'], c['known'], c['kcnt'], mutant=mutant)[1])]
    assert caught, mutant
    assert ('duplicates' if mutant == 'tie_higher_index' else 'ragged') in caught


# ------------------------------------------------------------------------------------------------------------------ workspace of the grid query
def test_grid_workspace_covers_a_call_without_points():
    """crb_ball_query2_grid_stack with n_total = 0 still clears 1,025 counts and lays out 1,024 cursors and the two prefix areas of
    4,096 (+ 64) entries behind them: the size query has to say so (it said 256)"""
    import crbhip
    f = crbhip.lib.crb_ball_query2_grid_workspace_bytes
    sizes = [int(f(n)) for n in (0, 1, 2, 511, 512, 513, 5000)]
    assert sizes == sorted(sizes)
    assert sizes[0] >= 4 * (1025 + 1024 + 2 * 4096)
