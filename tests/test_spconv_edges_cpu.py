"""CPU: the hand-built tables and coordinate sets of tests/spconv_edge_cases.py are what their names claim (sizes, injective columns,
exact transposes, pair counts, empty rows, unreferenced rows, wrap traps, uncovered slice), and the oracle stays finite on the
poisoned arrays the GPU test feeds it."""
import numpy as np
import pytest

import oracle
import spconv_edge_cases as E

TABLES = ['master', 'ladder'] + ['prefix%d' % n for n in E.ROWS_SMALL + E.ROWS_CHUNK] + ['window%d' % n for n in E.ROWS_WINDOW]


def _ref_t(nbr, n_in):
    """transpose written independently of spconv_edge_cases.transpose: entry by entry"""
    t = np.full((n_in, nbr.shape[1]), -1, np.int32)
    for o in range(nbr.shape[1]):
        rows = np.flatnonzero(nbr[:, o] >= 0)
        t[nbr[rows, o], o] = rows
    return t


@pytest.mark.parametrize('name', TABLES)
def test_table_is_well_formed(name):
    c = E.table(name)
    nbr, nbr_t = c['nbr'], c['nbr_t']
    assert c['K'] == 27 and c['n_in'] >= 1 and c['n_out'] >= 1
    assert nbr.shape == (c['n_out'], 27) and nbr_t.shape == (c['n_in'], 27)
    assert nbr.dtype == np.int32 and nbr_t.dtype == np.int32
    assert nbr.min() >= -1 and nbr.max() < c['n_in'] and nbr_t.min() >= -1 and nbr_t.max() < c['n_out']
    for o in range(27):
        col = nbr[:, o][nbr[:, o] >= 0]
        assert len(np.unique(col)) == len(col), (name, o)                # injective column
    np.testing.assert_array_equal(nbr_t, _ref_t(nbr, c['n_in']))
    assert (nbr_t >= 0).sum() == (nbr >= 0).sum() >= 1                   # at least one pair


def test_master_sizes_empty_rows_and_unreferenced_rows():
    c = E.master()
    nbr = c['nbr']
    assert c['n_out'] == 4097 and c['n_in'] == 3000
    empty = np.flatnonzero((nbr < 0).all(1))
    assert 0.04 * 4097 <= len(empty) <= 0.07 * 4097                      # about 5 % (the drawn 205 plus rows empty by chance)
    unref = E.unreferenced(nbr, 3000)
    assert 0.04 * 3000 <= len(unref) <= 0.07 * 3000 and unref[0] == 0    # row 0 = the row a clamped load reads
    np.testing.assert_array_equal(np.flatnonzero((c['nbr_t'] < 0).all(1)), unref)
    assert not np.isin([0, 4094, 4095, 4096], empty).any()               # a pair in the first row, at the end of chunk 0, in chunk 1
    # the columns differ in density as stated: probabilities 0.02 .. 0.9 over the first 3,000 rows
    dens = (nbr[:3000] >= 0).mean(0) / (1.0 - np.isin(np.arange(3000), empty).mean())
    np.testing.assert_allclose(dens, E.column_prob(), atol=0.03)
    assert dens.min() < 0.04 and dens.max() > 0.85
    # mask sorting has something to sort: many distinct masks inside one 64-row tile
    masks = ((nbr[:64] >= 0) << np.arange(27)).sum(1)
    assert len(np.unique(masks)) > 32


@pytest.mark.parametrize('n', E.ROWS_SMALL + E.ROWS_CHUNK + E.ROWS_WINDOW)
def test_prefix_is_the_head_of_master(n):
    c = E.prefix(n)
    assert c['n_out'] == n and c['n_in'] == 3000
    np.testing.assert_array_equal(c['nbr'], E.master()['nbr'][:n])
    assert (c['nbr'] >= 0).any()
    assert E.window(n) is c
    assert (c['nbr'][-1] >= 0).any() or n not in (1,) + E.ROWS_CHUNK      # the seam rows themselves hold pairs


def test_ladder_pair_counts():
    c = E.ladder()
    assert c['n_in'] == c['n_out'] == 600 and len(E.LADDER) == 27
    np.testing.assert_array_equal((c['nbr'] >= 0).sum(0), E.LADDER)
    assert E.LADDER[0] == 0 and E.LADDER[14] == 0 and E.LADDER[26] == 0   # an empty offset first, in the middle, last
    for blk in (16, 32, 64, 128):                                       # every pair-block size: one below, exact, one above
        assert {blk - 1, blk, blk + 1} <= set(E.LADDER)
    for o in np.flatnonzero(np.array(E.LADDER) == 600):                 # a full column is a permutation
        np.testing.assert_array_equal(np.sort(c['nbr'][:, o]), np.arange(600))


@pytest.mark.parametrize('which', [0, 1])
def test_borders_has_corners_edges_faces_and_traps(which):
    c = E.borders(which)
    shape, coords = c['shape'], c['coords']
    D, H, W = shape
    assert shape == E.BORDER_SHAPES[which] and c['batch_size'] == 3
    assert len(np.unique(coords, axis=0)) == len(coords)
    at_ext = np.stack([(coords[:, 1 + a] == 0) | (coords[:, 1 + a] == shape[a] - 1) for a in range(3)], 1)
    n_ext = at_ext.sum(1)
    corners = coords[n_ext == 3]
    assert len(np.unique(corners[corners[:, 0] == 0][:, 1:], axis=0)) == 8
    edges = {(tuple(np.flatnonzero(~e)), tuple(s[1:][e] > 0)) for s, e in zip(coords[n_ext == 2], at_ext[n_ext == 2])}
    faces = {(tuple(np.flatnonzero(e)), tuple(s[1:][e] > 0)) for s, e in zip(coords[n_ext == 1], at_ext[n_ext == 1])}
    assert len(edges) == 12 and len(faces) == 6 and (n_ext == 0).sum() >= 20
    nbr = oracle.subm_nbr(coords, shape, [3, 3, 3])
    assert len(c['traps']) == 7
    for t in c['traps']:
        ra, rb = E.row_of(c, t['a']), E.row_of(c, t['b'])
        assert E.lin_key(t['b'], shape) - E.lin_key(t['a'], shape) == t['key_diff']
        assert rb not in nbr[ra] and ra not in nbr[rb]                  # not neighbours
        if t['offset'] is None:
            assert t['a'][1:] == t['b'][1:] and t['key_diff'] == (t['b'][0] - t['a'][0]) * D * H * W
        else:
            dz, dy, dx = t['offset']
            assert t['key_diff'] == (dz * H + dy) * W + dx              # the pair a wrapping linear index would make
            o = E.offset_index(dz, dy, dx)
            assert nbr[ra, o] == -1 and nbr[rb, 26 - o] == -1
    assert sorted(abs(t['key_diff']) for t in c['traps'])[:4] == [1, 1, 1, 1]
    assert sum(t['key_diff'] == W for t in c['traps']) == 2


def test_isolated_has_pairs_at_the_centre_offset_only():
    c = E.isolated()
    nbr = oracle.subm_nbr(c['coords'], c['shape'], [3, 3, 3])
    assert len(c['coords']) == 200
    np.testing.assert_array_equal(nbr[:, 13], np.arange(200))
    assert ((nbr >= 0).sum(0) == 0).sum() == 26


def test_solid_block_is_one_tile_with_full_rows():
    for extra in (0, 1):
        c = E.solid(extra)
        assert len(c['coords']) == 64 + extra
        nbr = oracle.subm_nbr(c['coords'], c['shape'], [3, 3, 3])
        full = ((nbr >= 0).sum(1) == 27).sum()
        assert full == 8
        if extra:
            assert ((nbr >= 0).sum(1) == 1).sum() == 1                  # the far site sees itself only


def test_line():
    c = E.line()
    co = c['coords']
    assert len(co) == 130 and len(np.unique(co[:, :3], axis=0)) == 1
    np.testing.assert_array_equal(np.sort(co[:, 3]), np.arange(co[:, 3].min(), co[:, 3].min() + 130))
    nbr = oracle.subm_nbr(co, c['shape'], [3, 3, 3])
    np.testing.assert_array_equal((nbr >= 0).sum(0)[[12, 13, 14]], [129, 130, 129])
    assert (nbr >= 0).sum() == 129 + 130 + 129


@pytest.mark.parametrize('geom', E.UNCOVERED_GEOMS)
def test_uncovered_last_slice_feeds_no_output(geom):
    c = E.uncovered()
    ks, st, pd = geom
    coords, shape = c['coords'], c['shape']
    assert shape[0] == 6 and 250 <= len(coords) <= 400
    oc, oshape = oracle.spconv_out(coords, shape, ks, st, pd)
    assert oshape[0] == 2
    nbr = oracle.spconv_nbr(coords, shape, oc, ks, st, pd)
    nbr_t = E.transpose(nbr, len(coords))
    dead = np.flatnonzero((nbr_t < 0).all(1))
    np.testing.assert_array_equal(dead, np.flatnonzero(coords[:, 1] == 5))
    assert len(dead) >= 10


def test_empty_frame():
    c = E.empty_frame()
    co = c['coords']
    assert c['shape'] == [41, 16, 16] and c['batch_size'] == 3
    assert 300 <= len(co) <= 600 and (co[:, 0] == 1).sum() == 0 and (co[:, 0] == 0).sum() > 100 and (co[:, 0] == 2).sum() > 100


@pytest.mark.parametrize('name', ['master', 'ladder'])
def test_oracle_stays_finite_on_the_poisoned_arrays(name):
    c = E.table(name)
    nbr, nbr_t = c['nbr'], c['nbr_t']
    X = E.poison(E.feats(1, c['n_in'], 16), nbr)
    dY = E.poison(E.feats(2, c['n_out'], 16), nbr_t)
    W = E.weights(3, 27, 16, 16)
    if name == 'master':
        assert np.isnan(X).all(1).sum() >= 150 and np.isnan(dY).all(1).sum() >= 205 and np.isnan(X[0]).all()
    else:
        assert not np.isnan(X).any() and not np.isnan(dY).any()          # two full columns: every row is referenced
    assert np.isfinite(oracle.conv_fwd(X, W, nbr)).all()
    assert np.isfinite(oracle.conv_dgrad(dY, W, nbr, c['n_in'])).all()
    assert np.isfinite(oracle.conv_wgrad(X, dY, nbr, 27)).all()
    # the helper names exactly the rows no entry references, and leaves the others alone
    ref = E.feats(1, c['n_in'], 16)
    keep = ~np.isnan(X).any(1)
    np.testing.assert_array_equal(X[keep], ref[keep])
    assert set(np.flatnonzero(~keep)) == set(range(c['n_in'])) - set(nbr[nbr >= 0].tolist())
