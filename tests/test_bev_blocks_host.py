"""CPU: the numpy restatement of the Winograd block lists (crbhip.bev_blocks.reference) against a brute-force loop over their
definition. conv-in: spatial blocks (8 tile rows over N * ceil(H / 2) x 4 tile columns) with an active pixel within one pixel of one of
their in-map pixels; conv-out: blocks that hold an active pixel; wgrad: chunks (4 x 4 tiles of one image) with an active pixel within one
pixel of theirs. tests/test_winograd_sparse_gpu.py holds the device lists to the same restatement on the same cases."""
import numpy as np
import pytest

from bev_blocks_cases import CASES, SHAPES, indices_of


def brute_force(idx, N, H, W):
    """the definition, pixel by pixel. Geometry written out here on purpose: 2 x 2 tiles, blocks of 8 x 4 tiles over the batch's tile
    rows, chunks of 4 x 4 tiles per image"""
    th, tw = (H + 1) // 2, (W + 1) // 2
    tw4 = (tw + 3) // 4
    nblocks = ((N * th + 7) // 8) * tw4
    rp, tc4 = (th + 3) // 4, (tw + 3) // 4
    nchunks = N * rp * tc4
    active = {(int(r[0]), int(r[2]), int(r[3])) for r in idx}
    c_in, c_out, wg = set(), set(), set()
    for n in range(N):
        for y in range(H):
            for x in range(W):
                blk = ((n * th + y // 2) // 8) * tw4 + (x // 2) // 4
                chk = (n * rp + (y // 2) // 4) * tc4 + (x // 2) // 4
                if (n, y, x) in active:
                    c_out.add(blk)
                if any((n, y + dy, x + dx) in active for dy in (-1, 0, 1) for dx in (-1, 0, 1)):
                    c_in.add(blk)
                    wg.add(chk)

    def arr(s):
        return np.array(sorted(s), dtype=np.int32)
    return {'conv_in': arr(c_in), 'conv_in_rest': arr(set(range(nblocks)) - c_in), 'conv_out': arr(c_out),
            'conv_out_rest': arr(set(range(nblocks)) - c_out), 'wgrad': arr(wg)}, nblocks, nchunks


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('case', CASES)
def test_reference_equals_brute_force(shape, case):
    from crbhip import bev_blocks
    N, H, W = shape
    idx = indices_of(case, N, H, W)
    want, nblocks, nchunks = brute_force(idx, N, H, W)
    g = bev_blocks.geometry(N, H, W)
    assert (g['nblocks'], g['nchunks']) == (nblocks, nchunks)
    got = bev_blocks.reference(idx, N, H, W)
    for k in want:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (k, got[k], want[k])
    if case == 'empty':
        assert got['conv_in'].size == 0 and got['wgrad'].size == 0 and got['conv_in_rest'].size == nblocks
    if case == 'full':
        assert got['conv_out'].size == nblocks and got['wgrad'].size == nchunks and got['conv_out_rest'].size == 0


def test_rows_outside_the_map_are_ignored():
    from crbhip import bev_blocks
    N, H, W = 2, 16, 24
    idx = indices_of('random', N, H, W)
    bad = np.array([[2, 0, 0, 0], [-1, 0, 3, 3], [0, 0, 16, 0], [1, 0, 0, 24], [0, 0, -1, 5]], dtype=np.int32)
    a = bev_blocks.reference(idx, N, H, W)
    b = bev_blocks.reference(np.concatenate([idx, bad]), N, H, W)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
