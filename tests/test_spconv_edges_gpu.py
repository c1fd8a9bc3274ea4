"""GPU parity of the sparse convolution stack on the hand-built cases of tests/spconv_edge_cases.py (what each case is: asserted on
the CPU in tests/test_spconv_edges_cpu.py): row counts around the 16- / 64-row tiles, the 128-row tile-order threshold and the
4,096-row sort chunk for every channel pair; pair counts per offset around every pair-block size of the three weight-gradient
kernels; the windowed weight gradient below and around its 32 windows; the epilogue and the inverse convolution on partial tiles;
NaN in rows no pair references; sites on grid and frame borders, an uncovered slice, an empty frame.

Reference: the double-accumulating oracle on the same table. Tolerance of tests/test_spconv_gpu.py: rtol 1e-4, atol 1e-5 max(1,
max |ref|). Tables, coordinate sets and pair lists bit for bit. Where the reference is exactly 0 (rows / offsets without pairs): == 0.

Kernel family of every channel pair (csrc/sparse_conv.hip; test_family_map_is_the_dispatch checks the map against the library):
  forward   low-channel kernel on the compact table (launch_fwd_compact: C_in 4 -> 16)                          4->16
            sparse_conv_fwd2_kernel on the compact table (launch_fwd_compact: C_in, C_out % 16 == 0, C_in <= 64)
            sparse_conv_fwd_kernel on the sorted (n, K) table (launch_fwd -> launch_fwd_subt: everything else)
  wgrad     sparse_conv_wgrad3_kernel (launch_wgrad: both % 32 == 0, <= 4 blocks of 32 x 32), sparse_conv_wgrad2_kernel (both
            % 32 == 0, more blocks), sparse_conv_wgrad_kernel (the rest)
"""
import numpy as np
import pytest
import torch

import oracle
import spconv_edge_cases as E

pytestmark = pytest.mark.gpu

# CRB_CONV_SHAPES of csrc/sparse_conv.hip
PAIRS = [(4, 16), (5, 16), (16, 4), (16, 5), (4, 64), (64, 4), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64),
         (64, 128), (128, 64), (128, 128)]
# one pair per family: forward lc / fwd / fwd2 / fwd2 / fwd2 (dgrad 128->64: fwd) / fwd; wgrad v1 / v1 / v1 / v3 / v2 / v2
FAMILY_PAIRS = [(4, 16), (5, 16), (16, 16), (32, 32), (64, 128), (128, 128)]
LADDER_PAIRS = [(16, 16), (4, 16), (32, 32), (32, 64), (64, 64), (64, 128), (128, 128)]
WINDOWED_PAIRS = [(32, 32), (32, 64), (64, 64)]


def fwd_family(cin, cout):
    if (cin, cout) == (4, 16):
        return 'lc'
    return 'fwd2' if cin % 16 == 0 and cout % 16 == 0 and cin <= 64 else 'fwd'


def wgrad_family(cin, cout):
    if cin % 32 == 0 and cout % 32 == 0:
        return 'wgrad3' if (cin // 32) * (cout // 32) <= 4 else 'wgrad2'
    return 'wgrad'


def _close(a, ref, rtol=1e-4):
    atol = 1e-5 * max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(a, ref, rtol=rtol, atol=atol)


def _t(a, dev):
    return torch.from_numpy(np.array(a, order='C', copy=True)).to(dev)        # (the cases are read-only arrays)


def _rulebook(case, dev):
    """the table as a NON-submanifold convolution: the input gradient runs the transposed table"""
    from crbhip import sparse
    return sparse.Rulebook(_t(case['nbr'], dev), _t(case['nbr_t'], dev), case['n_in'], case['n_out'], [3, 3, 3], [1, 1, 1],
                           [1, 1, 1], False, None, None, None)


def _values(case, cin, cout, base_rows=None):
    """X over the case's input rows, W, dY = the first n_out rows of one (base_rows, cout) array: the prefixes of one table share
    every value"""
    base_rows = base_rows or case['n_out']
    return (E.feats(11, case['n_in'], cin), E.weights(12, 27, cin, cout), E.feats(13, base_rows, cout)[:case['n_out']])


def _run(dev, case, X, W, dY):
    from crbhip import sparse
    rb = _rulebook(case, dev)
    x = _t(X, dev).requires_grad_(True)
    w = _t(W, dev).requires_grad_(True)
    y = sparse.sparse_conv(x, w, rb)
    y.backward(_t(dY, dev))
    return rb, y.detach().cpu().numpy(), x.grad.cpu().numpy(), w.grad.cpu().numpy()


PARTS = ('fwd', 'dgrad', 'wgrad')


def _check(case, X, W, dY, y, dx, dw, parts=PARTS):
    """against the oracle on the same table, and exactly 0 where nothing is summed: rows without pairs (both directions), offsets
    without pairs"""
    nbr = case['nbr']
    if 'fwd' in parts:
        _close(y, oracle.conv_fwd(X, W, nbr))
        assert (y[(nbr < 0).all(1)] == 0.0).all()
    if 'dgrad' in parts:
        _close(dx, oracle.conv_dgrad(dY, W, nbr, case['n_in']))
        assert (dx[(case['nbr_t'] < 0).all(1)] == 0.0).all()
    if 'wgrad' in parts:
        _close(dw, oracle.conv_wgrad(X, dY, nbr, 27))
        assert (dw[(nbr < 0).all(0)] == 0.0).all()


_LAST = [None, None]          # the 4,097-row tables are run once and checked in parts (one oracle call per test): newest run only


def _result(dev, name, cin, cout, poisoned=False):
    """-> case, rulebook, (X, W, dY, y, dx, dw) of one forward + backward on the table `name`"""
    key = (name, cin, cout, poisoned)
    if _LAST[0] != key:
        case = E.table(name)
        X, W, dY = _values(case, cin, cout, None if name == 'ladder' else E.N_OUT)
        if poisoned:
            X, dY = E.poison(X, case['nbr']), E.poison(dY, case['nbr_t'])
        rb, y, dx, dw = _run(dev, case, X, W, dY)
        _LAST[:] = [key, (case, rb, (X, W, dY, y, dx, dw))]
    return _LAST[1]


_Y_OF = {}          # (rows, cin, cout) -> y of prefix(rows): the yardstick of the prefix invariance, computed once per pair


def _y_of(dev, rows, cin, cout):
    key = (rows, cin, cout)
    if key not in _Y_OF:
        case = E.prefix(rows)
        _Y_OF[key] = _run(dev, case, *_values(case, cin, cout, E.N_OUT))[1]
    return _Y_OF[key]


@pytest.fixture(scope='module', autouse=True)
def first_use(dev):
    """what a process pays once - the device context, the library's code object, the code objects of the torch operations the
    checks use, the oracle library and the host's first pass over arrays of 3,000 x 64 - is paid here, in a set-up step, not
    inside whichever case happens to be collected first"""
    case = E.prefix(1)
    X, W, dY = _values(case, 64, 4, E.N_OUT)
    rb, y, dx, dw = _run(dev, case, X, W, dY)
    _check(case, X, W, dY, y, dx, dw)
    ct = rb.compact_table('nbr_t')
    assert sorted(ct.perm.cpu().tolist()) == list(range(case['n_in'])) and torch.equal(ct.to_nbr(), rb.nbr_t[ct.perm.long()])
    E.master(), E.ladder()
    torch.cuda.synchronize()


def test_family_map_is_the_dispatch(dev):
    """fwd_family / wgrad_family above restate launch_fwd_compact, launch_fwd and launch_wgrad; what the library answers about a
    pair agrees, every pair of CRB_CONV_SHAPES is listed, and the per-family lists hold one pair of every family"""
    from crbhip import lib
    for cin in (4, 5, 16, 32, 64, 128):
        for cout in (4, 5, 16, 32, 64, 128):
            assert bool(lib.crb_sparse_conv_supported(cin, cout)) == ((cin, cout) in PAIRS)
    for cin, cout in PAIRS:
        assert bool(lib.crb_sparse_conv_compact_supported(cin, cout)) == (fwd_family(cin, cout) in ('lc', 'fwd2'))
        assert bool(lib.crb_sparse_conv_wgrad_windowed_supported(cin, cout)) == (wgrad_family(cin, cout) == 'wgrad3')
        assert (lib.crb_sparse_conv_wgrad_occupancy(cin, cout) >= 0) == (wgrad_family(cin, cout) in ('wgrad3', 'wgrad2'))
    assert {fwd_family(*p) for p in FAMILY_PAIRS} | {fwd_family(b, a) for a, b in FAMILY_PAIRS} == {'lc', 'fwd', 'fwd2'}
    assert [fwd_family(*p) for p in FAMILY_PAIRS] == ['lc', 'fwd', 'fwd2', 'fwd2', 'fwd2', 'fwd'] and fwd_family(128, 64) == 'fwd'
    assert [wgrad_family(*p) for p in FAMILY_PAIRS] == ['wgrad', 'wgrad', 'wgrad', 'wgrad3', 'wgrad2', 'wgrad2']
    assert [wgrad_family(*p) for p in LADDER_PAIRS] == ['wgrad', 'wgrad', 'wgrad3', 'wgrad3', 'wgrad3', 'wgrad2', 'wgrad2']
    assert all(wgrad_family(*p) == 'wgrad3' for p in WINDOWED_PAIRS)


@pytest.mark.parametrize('n', E.ROWS_SMALL, ids=lambda n: 'n%d' % n)
@pytest.mark.parametrize('cin,cout', PAIRS, ids=lambda v: str(v))
def test_row_counts_every_channel_pair(dev, cin, cout, n):
    """forward, input gradient (transposed table) and weight gradient of prefix(n) against the oracle, and the prefix invariance:
    y of prefix(n) is bit for bit the head of y of prefix(193) (same per-row arithmetic, only the row -> workgroup map differs)"""
    case = E.prefix(n)
    X, W, dY = _values(case, cin, cout, E.N_OUT)
    _, y, dx, dw = _run(dev, case, X, W, dY)
    _check(case, X, W, dY, y, dx, dw)
    np.testing.assert_array_equal(y, _y_of(dev, E.ROWS_SMALL[-1], cin, cout)[:n])


@pytest.mark.parametrize('part', PARTS + ('tables',))
@pytest.mark.parametrize('n', E.ROWS_CHUNK, ids=lambda n: 'n%d' % n)
@pytest.mark.parametrize('cin,cout', FAMILY_PAIRS, ids=lambda v: str(v))
def test_chunk_boundary_every_family(dev, cin, cout, n, part):
    """the same around one sort chunk of crb_tables_finish (4,097 rows = a one-row second chunk); one run per (pair, n), checked in
    four parts: forward, input gradient, weight gradient, and `tables` = the compact tables against the (n, K) tables in kernel
    order + the prefix invariance against the 4,097-row result"""
    case, rb, res = _result(dev, 'prefix%d' % n, cin, cout)
    if part != 'tables':
        return _check(case, *res, parts=(part,))
    for which, nat in (('nbr', rb.nbr), ('nbr_t', rb.nbr_t)):
        ct = rb.compact_table(which)
        assert sorted(ct.perm.cpu().tolist()) == list(range(nat.shape[0]))
        assert torch.equal(ct.to_nbr(), nat[ct.perm.long()])
        assert ct.num_pairs() == int((case['nbr'] >= 0).sum())
    np.testing.assert_array_equal(res[3], _y_of(dev, E.N_OUT, cin, cout)[:n])


def _assert_pairs(pairs, nbr):
    pin, pout, pstart = [p.cpu().numpy() for p in pairs[:3]]
    K = nbr.shape[1]
    assert int(pstart[0]) == 0 and int(pstart[K]) == (nbr >= 0).sum()
    for o in range(K):
        rows = np.flatnonzero(nbr[:, o] >= 0)
        assert int(pstart[o + 1]) - int(pstart[o]) == len(rows)
        np.testing.assert_array_equal(pout[pstart[o]:pstart[o + 1]], rows)
        np.testing.assert_array_equal(pin[pstart[o]:pstart[o + 1]], nbr[rows, o])


@pytest.mark.parametrize('cin,cout', LADDER_PAIRS, ids=lambda v: str(v))
def test_pair_count_ladder(dev, cin, cout):
    """offsets with 0, 1, block - 1, block, block + 1 pairs for every pair-block size in use (16; 32 / 64 / 128; 32 / 64), empty
    offsets first, in the middle and last: weight gradient against the oracle, the empty offsets exactly 0, pair lists exact"""
    case = E.ladder()
    X, W, dY = _values(case, cin, cout)
    rb, y, dx, dw = _run(dev, case, X, W, dY)
    _assert_pairs(rb.pairs(), case['nbr'])
    _check(case, X, W, dY, y, dx, dw)
    for o in (0, 14, 26):
        assert E.LADDER[o] == 0 and (dw[o] == 0.0).all()


@pytest.mark.parametrize('cin,cout', WINDOWED_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize('name', ['window%d' % n for n in E.ROWS_WINDOW] + ['ladder', 'prefix4097'])
def test_windowed_wgrad_on_few_rows(dev, name, cin, cout):
    """the opt-in windowed weight gradient (32 windows of output rows) where most windows are empty, around 32 and 64 rows, on the
    ladder and over a chunk boundary: == the oracle; the window bounds partition every offset's pair list"""
    from crbhip import sparse
    case = E.table(name)
    X, _, dY = _values(case, cin, cout, E.N_OUT if name != 'ladder' else None)
    rb = _rulebook(case, dev)
    sparse.WGRAD_WINDOWED = True
    try:
        pairs = rb.pairs()
        assert len(pairs) == 4
        dw = sparse._conv_wgrad_raw(_t(X, dev), _t(dY, dev), pairs, 27).cpu().numpy()
    finally:
        sparse.WGRAD_WINDOWED = False
    ref = oracle.conv_wgrad(X, dY, case['nbr'], 27)
    _close(dw, ref)
    assert (dw[(case['nbr'] < 0).all(0)] == 0.0).all()
    _assert_pairs(pairs, case['nbr'])
    bnd, pstart = pairs[3].cpu().numpy(), pairs[2].cpu().numpy()
    assert (bnd[:, 0] == pstart[:-1]).all() and (bnd[:, -1] == pstart[1:]).all() and (np.diff(bnd, axis=1) >= 0).all()
    _close(sparse._conv_wgrad_raw(_t(X, dev), _t(dY, dev), pairs, 27).cpu().numpy(), ref)      # the default kernel, same pair lists


def _bn(cout, dev, seed):
    torch.manual_seed(seed)
    bn = torch.nn.BatchNorm1d(cout, eps=1e-3, momentum=0.01).to(dev).eval()
    with torch.no_grad():
        bn.running_mean.normal_(0, 0.5)
        bn.running_var.uniform_(0.3, 2.0)
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_(0, 0.3)
    return bn


@pytest.mark.parametrize('n', [1, 17, 65, 129], ids=lambda n: 'n%d' % n)
@pytest.mark.parametrize('cin,cout', [(4, 16), (16, 16), (64, 64)], ids=lambda v: str(v))
def test_bn_relu_epilogue_on_partial_tiles(dev, cin, cout, n):
    """sparse_conv_bn_eval (bias, BatchNorm1d of the running statistics and ReLU on the accumulator) with bias and ReLU on and off
    against the oracle convolution followed by BatchNorm1d(eps=1e-3).eval() and ReLU in float64"""
    from crbhip import sparse
    case = E.prefix(n)
    X, W, _ = _values(case, cin, cout, E.N_OUT)
    conv = torch.from_numpy(oracle.conv_fwd(X, W, case['nbr'])).double()
    rb = _rulebook(case, dev)
    bn = _bn(cout, dev, cin * 131 + cout)
    st = {k: v.detach().cpu().double() for k, v in bn.state_dict().items()}
    bias = torch.from_numpy(E.feats(14, 1, cout)[0])
    for use_bias in (False, True):
        for relu in (False, True):
            got = sparse.sparse_conv_bn_eval(_t(X, dev), _t(W, dev), rb, bias.to(dev) if use_bias else None, bn, relu)
            ref = torch.nn.functional.batch_norm(conv + bias.double() if use_bias else conv, st['running_mean'], st['running_var'],
                                                 st['weight'], st['bias'], False, 0.0, 1e-3)
            ref = torch.relu(ref) if relu else ref
            assert got.shape == (n, cout)
            _close(got.cpu().numpy(), ref.numpy())
            if relu:
                assert float(got.min()) >= 0.0


@pytest.mark.parametrize('n', [1, 17, 65, 129], ids=lambda n: 'n%d' % n)
def test_inverse_conv_on_partial_tiles(dev, n):
    """sparse_conv(..., inverse=True) on prefix(n): n coarse rows scattered over 3,000 fine rows through the transposed table,
    forward and both gradients; fine rows no pair reaches are exactly 0"""
    from crbhip import sparse
    case = E.prefix(n)
    cin = cout = 32
    nbr_t = case['nbr_t']
    Z, W, dY = E.feats(21, n, cin), E.weights(22, 27, cin, cout), E.feats(23, case['n_in'], cout)
    rb = _rulebook(case, dev)
    z = _t(Z, dev).requires_grad_(True)
    w = _t(W, dev).requires_grad_(True)
    out = sparse.sparse_conv(z, w, rb, inverse=True)
    out.backward(_t(dY, dev))
    assert out.shape == (case['n_in'], cout)
    y, dz, dw = out.detach().cpu().numpy(), z.grad.cpu().numpy(), w.grad.cpu().numpy()
    _close(y, oracle.conv_fwd(Z, W, nbr_t))
    _close(dz, oracle.conv_dgrad(dY, W, nbr_t, n))
    _close(dw, oracle.conv_wgrad(Z, dY, nbr_t, 27))
    assert (y[(nbr_t < 0).all(1)] == 0.0).all() and (dz[(case['nbr'] < 0).all(1)] == 0.0).all()
    assert (dw[(nbr_t < 0).all(0)] == 0.0).all()
    _assert_pairs(rb.pairs_t(), nbr_t)


@pytest.mark.parametrize('part', PARTS)
@pytest.mark.parametrize('cin,cout', FAMILY_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize('name', ['master', 'ladder'])
def test_nan_in_unreferenced_rows_reaches_no_output(dev, name, cin, cout, part):
    """rows no pair references hold NaN: the input rows the table never names (row 0 of master among them, the row the forward
    kernels' clamped loads read) and, for the backward, the dY rows of outputs without pairs. The kernels zero such a value by a
    select, never by a product: every output is finite and equals the oracle on the same arrays (one run per table and pair,
    checked in three parts). ladder has two full columns, so nothing to poison: it runs the same path with every row live."""
    case, _, res = _result(dev, name, cin, cout, poisoned=True)
    X, W, dY, y, dx, dw = res
    if name == 'master':
        assert np.isnan(X[0]).all() and np.isnan(X).any(1).sum() >= E.N_UNREF and np.isnan(dY).any(1).sum() >= E.N_EMPTY
    assert np.isfinite({'fwd': y, 'dgrad': dx, 'wgrad': dw}[part]).all()
    _check(case, *res, parts=(part,))


# ---------------------------------------------------------------------------------------------------------------- geometry
def _ref_transpose(nbr, n_in):
    i, o = np.nonzero(nbr >= 0)
    ref_t = np.full((n_in, nbr.shape[1]), -1, np.int32)
    ref_t[nbr[i, o], o] = i
    return ref_t


def _conv_through(dev, rb, nbr, n_in):
    """16 -> 16 and 64 -> 64 forward / backward through a rulebook the library built against the oracle on the oracle's table
    -> {cin: (dx, dw)}"""
    from crbhip import sparse
    out = {}
    K = nbr.shape[1]
    for c in (16, 64):
        X, W, dY = E.feats(31, n_in, c), E.weights(32, K, c, c), E.feats(33, len(nbr), c)
        x = _t(X, dev).requires_grad_(True)
        w = _t(W, dev).requires_grad_(True)
        y = sparse.sparse_conv(x, w, rb)
        y.backward(_t(dY, dev))
        assert y.shape == (len(nbr), c)
        dx, dw = x.grad.cpu().numpy(), w.grad.cpu().numpy()
        _close(y.detach().cpu().numpy(), oracle.conv_fwd(X, W, nbr))
        _close(dx, oracle.conv_dgrad(dY, W, nbr, n_in))
        _close(dw, oracle.conv_wgrad(X, dY, nbr, K))
        out[c] = (dx, dw)
    return out


@pytest.mark.parametrize('name', ['borders0', 'borders1', 'isolated', 'solid64', 'solid65', 'line'])
def test_subm_rulebook_on_borders_and_degenerate_sets(dev, name):
    from crbhip import sparse
    g = E.geometry(name)
    coords, shape = g['coords'], g['shape']
    nbr = oracle.subm_nbr(coords, shape, [3, 3, 3])
    with torch.enable_grad():
        rb = sparse.subm_rulebook(_t(coords, dev), shape, [3, 3, 3])
    np.testing.assert_array_equal(rb.nbr.cpu().numpy(), nbr)
    _assert_pairs(rb.pairs(), nbr)
    ct = rb.compact_table('nbr')
    assert torch.equal(ct.to_nbr(), rb.nbr[ct.perm.long()])
    grads = _conv_through(dev, rb, nbr, len(coords))
    if name == 'isolated':
        for dx, dw in grads.values():
            assert all((dw[o] == 0.0).all() for o in range(27) if o != 13) and np.abs(dw[13]).max() > 0


def _check_spconv_rulebook(rb, coords, shape, ks, st, pd):
    oc, oshape = oracle.spconv_out(coords, shape, ks, st, pd)
    assert rb.out_shape == oshape and rb.n_out == len(oc) and rb.n_in == len(coords)
    np.testing.assert_array_equal(rb.out_coords.cpu().numpy(), oc)
    nbr = oracle.spconv_nbr(coords, shape, oc, ks, st, pd)
    np.testing.assert_array_equal(rb.nbr.cpu().numpy(), nbr)
    np.testing.assert_array_equal(rb.nbr_t.cpu().numpy(), _ref_transpose(nbr, len(coords)))
    _assert_pairs(rb.pairs(), nbr)
    return oc, oshape, nbr


@pytest.mark.parametrize('name,geom', [('borders0', E.BORDER_GEOM), ('borders1', E.BORDER_GEOM), ('borders0', E.UNCOVERED_GEOMS[1]),
                                       ('uncovered', E.UNCOVERED_GEOMS[0]), ('uncovered', E.UNCOVERED_GEOMS[1])],
                         ids=['borders0-k3s2p1', 'borders1-k3s2p1', 'borders0-k3s2p011', 'uncovered-k311s211p0', 'uncovered-k3s2p011'])
def test_spconv_rulebook_on_borders_and_an_uncovered_slice(dev, name, geom):
    from crbhip import sparse
    g = E.geometry(name)
    coords, shape = g['coords'], g['shape']
    ks, st, pd = geom
    with torch.enable_grad():
        rb = sparse.spconv_rulebook(_t(coords, dev), shape, g['batch_size'], ks, st, pd)
    _, _, nbr = _check_spconv_rulebook(rb, coords, shape, ks, st, pd)
    grads = _conv_through(dev, rb, nbr, len(coords))
    if name == 'uncovered':
        last = coords[:, 1] == shape[0] - 1
        np.testing.assert_array_equal(np.flatnonzero(last), np.flatnonzero((rb.nbr_t.cpu().numpy() < 0).all(1)))
        for dx, dw in grads.values():
            assert last.sum() >= 10 and (dx[last] == 0.0).all() and np.abs(dx[~last]).max() > 0


def test_planned_chain_with_an_empty_frame(dev):
    """build_rulebooks over the eight-level chain of VoxelBackBone8x on three frames of which the middle one has no site: == the
    rulebooks built one layer at a time == the oracle, bit for bit; then 16 -> 16 and 64 -> 64 through every rulebook"""
    from crbhip import sparse
    g = E.empty_frame()
    coords, shape, B = g['coords'], g['shape'], g['batch_size']
    specs = []
    for geo in E.CHAIN_GEOMS:
        specs += [('subm', (3, 3, 3)), ('spconv',) + geo]
    c = _t(coords, dev)
    with torch.enable_grad():
        books = sparse.build_rulebooks(c, shape, B, specs, want_grad=True)
        cur, cur_shape = c, shape
        oc_np, oshape_np = coords, shape
        for k, (ks, st, pd) in enumerate(E.CHAIN_GEOMS):
            sub, b = books[2 * k], books[2 * k + 1]
            assert (oc_np[:, 0] != 1).all() and len(oc_np) > 0                   # the empty frame stays empty, the others do not
            sub_ref = oracle.subm_nbr(oc_np, oshape_np, [3, 3, 3])
            np.testing.assert_array_equal(sub.nbr.cpu().numpy(), sub_ref)
            assert torch.equal(sparse.subm_rulebook(cur, cur_shape, [3, 3, 3]).nbr, sub.nbr)
            _assert_pairs(sub.pairs(), sub_ref)
            a = sparse.spconv_rulebook(cur, cur_shape, B, ks, st, pd)
            assert a.n_out == b.n_out and a.out_shape == b.out_shape
            assert torch.equal(a.out_coords, b.out_coords) and torch.equal(a.nbr, b.nbr) and torch.equal(a.nbr_t, b.nbr_t)
            nxt, nshape, nbr_ref = _check_spconv_rulebook(b, oc_np, oshape_np, ks, st, pd)
            _conv_through(dev, sub, sub_ref, len(oc_np))
            _conv_through(dev, b, nbr_ref, len(oc_np))
            oc_np, oshape_np = nxt, nshape
            cur, cur_shape = b.out_coords.contiguous(), b.out_shape
