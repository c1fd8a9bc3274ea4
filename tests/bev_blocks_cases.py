"""Index sets shared by tests/test_bev_blocks_host.py and tests/test_winograd_sparse_gpu.py."""
import numpy as np

# (N, H, W): blocks that straddle two images (3 x 37 x 29: 19 tile rows per image), maps smaller than a block, the bench layer's aspect
SHAPES = [(3, 37, 29), (1, 5, 3), (2, 16, 24), (2, 33, 40)]
CASES = ['random', 'borders', 'two_z', 'empty', 'full']


def indices_of(case, N, H, W, seed=0):
    """(n,4) int32 rows (b, z, y, x)"""
    rng = np.random.RandomState(seed)
    if case == 'empty':
        return np.zeros((0, 4), dtype=np.int32)
    if case == 'full':
        b, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing='ij')
    elif case == 'borders':           # pixels on all four borders (corners included) of the first and last image
        pts = [(n, y, x) for n in sorted({0, N - 1}) for y, x in
               [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]]
        b, y, x = [np.array(v) for v in zip(*pts)]
    elif case == 'two_z':             # one pixel named twice, at two z levels, and a lone one
        b, y, x = np.array([N - 1, N - 1, 0]), np.array([H // 2, H // 2, H - 1]), np.array([W // 3, W // 3, 1 % W])
    else:
        keep = rng.rand(N, H, W) < 0.1
        b, y, x = np.nonzero(keep)
    z = np.arange(b.size) % 2
    rows = np.stack([b.ravel(), z.ravel(), y.ravel(), x.ravel()], 1).astype(np.int32)
    return rows[rng.permutation(rows.shape[0])]
