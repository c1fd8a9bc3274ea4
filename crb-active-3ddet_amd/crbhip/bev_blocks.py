"""Block lists of a sparse BEV map (csrc/bev_blocks.hip, crb_bev_blocks): which spatial blocks of the split-bf16 Winograd convolution
and which tile chunks of its weight gradient can see an active pixel. The first 3x3 layer of the BEV backbone walks them instead of the
whole map (crbhip.winograd: CRB_WINOGRAD_SPARSE).

`build` runs on the device and reads nothing back; `reference` restates the lists in numpy from their definition (dilate the active
pixel mask by one pixel inside the map, then ask every block whether it holds a marked pixel)."""
import ctypes
import functools

import numpy as np
import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

N_COUNTS = 8
CONV_IN, CONV_OUT, WGRAD, CONV_IN_REST, CONV_OUT_REST = range(5)


@functools.lru_cache(maxsize=64)
def _geometry(N, H, W):
    g = (ctypes.c_int32 * 12)()
    check(lib.crb_bev_blocks_geometry(N, H, W, g), 'crb_bev_blocks_geometry')
    keys = ('nblocks', 'nchunks', 'th', 'tw', 'tw4', 'rp', 'tc4', 'tile', 'tb_rows', 'tb_cols', 'ch_rows', 'ch_cols')
    return tuple(zip(keys, [int(v) for v in g])), int(lib.crb_bev_blocks_ints(N, H, W))


def geometry(N, H, W):
    """the kernels' own numbers (csrc/winograd_blocks.h) -> dict (a training step asks once per shape: the answer is kept)"""
    return dict(_geometry(int(N), int(H), int(W))[0])


class BlockLists:
    """views into the one int32 buffer crb_bev_blocks writes. counts (8,): see CONV_IN ..; every list is ascending and valid up to its
    count; `indices` are the (n,4) rows the lists were made from"""

    def __init__(self, buf, N, H, W, indices):
        g = geometry(N, H, W)
        nb, nc = g['nblocks'], g['nchunks']
        self.shape = (int(N), int(H), int(W))
        self.geom = g
        self.indices = indices
        self.buf = buf
        self.counts = buf[:N_COUNTS]
        o = N_COUNTS
        self.conv_in, self.conv_in_rest = buf[o:o + nb], buf[o + nb:o + 2 * nb]
        self.conv_out, self.conv_out_rest = buf[o + 2 * nb:o + 3 * nb], buf[o + 3 * nb:o + 4 * nb]
        self.wgrad = buf[o + 4 * nb:o + 4 * nb + nc]
        self.wgrad_count = buf[WGRAD:WGRAD + 1]
        # (the views a launch hands to the C-ABI, made once: the step's host thread is on the critical path behind the sparse backbone)
        self._conv = {'in': (self.conv_in, buf[CONV_IN:CONV_IN + 1], self.conv_in_rest, buf[CONV_IN_REST:CONV_IN_REST + 1]),
                      'out': (self.conv_out, buf[CONV_OUT:CONV_OUT + 1], self.conv_out_rest, buf[CONV_OUT_REST:CONV_OUT_REST + 1])}

    def conv(self, which):
        """(list, count, rest, rest count) of 'in' | 'out' as one-element views"""
        return self._conv[which]

    def matches(self, x):
        """x (N,C,H,W) is a map of the shape the lists were made for, on their device"""
        return x.dim() == 4 and (x.shape[0], x.shape[2], x.shape[3]) == self.shape and x.device == self.buf.device

    def pixel_mask(self, which):
        """(N,H,W) bool: the pixels of the listed conv blocks ('in' | 'out'). Reads the count back: checks only."""
        g = self.geom
        lst, cnt = self.conv(which)[:2]
        listed = torch.zeros((g['nblocks'],), dtype=torch.bool, device=self.buf.device)
        listed[lst[:int(cnt.item())].long()] = True
        N, H, W = self.shape
        dev = self.buf.device
        n = torch.arange(N, device=dev).view(N, 1, 1)
        y = torch.arange(H, device=dev).view(1, H, 1)
        x = torch.arange(W, device=dev).view(1, 1, W)
        blk = torch.div(n * g['th'] + torch.div(y, g['tile'], rounding_mode='floor'), g['tb_rows'], rounding_mode='floor') * g['tw4'] + \
            torch.div(torch.div(x, g['tile'], rounding_mode='floor'), g['tb_cols'], rounding_mode='floor')
        return listed[blk]


def build(indices, N, H, W):
    """indices (n,4) int32 device rows (b, z, y, x) -> BlockLists for an (N, ., H, W) map"""
    require_cuda(indices)
    if indices.dim() != 2 or indices.shape[1] != 4:
        raise CrbHipError('crb_bev_blocks takes (n,4) index rows (b, z, y, x)')
    idx = indices if indices.dtype == torch.int32 else indices.to(torch.int32)
    idx = idx.contiguous()
    ints = _geometry(int(N), int(H), int(W))[1]
    if ints <= 0:
        raise CrbHipError('crb_bev_blocks: no block geometry for a %d x %d x %d map' % (N, H, W))
    buf = torch.empty((ints,), dtype=torch.int32, device=idx.device)
    check(lib.crb_bev_blocks(ptr(idx), idx.shape[0], int(N), int(H), int(W), ptr(buf), ints, cur_stream(idx.device)), 'crb_bev_blocks')
    return BlockLists(buf, N, H, W, idx)


def _dilate(mask):
    """(N,H,W) bool -> true where a true pixel lies within one pixel (inside the map)"""
    p = np.pad(mask, ((0, 0), (1, 1), (1, 1)))
    out = np.zeros_like(mask)
    H, W = mask.shape[1:]
    for dy in range(3):
        for dx in range(3):
            out |= p[:, dy:dy + H, dx:dx + W]
    return out


def reference(indices, N, H, W, geom=None):
    """numpy restatement: indices (n,4) rows (b, z, y, x) -> dict of ascending int32 arrays conv_in, conv_in_rest, conv_out,
    conv_out_rest, wgrad. Rows outside the map are ignored, as the kernel ignores them."""
    g = geom or geometry(N, H, W)
    idx = np.asarray(indices).reshape(-1, 4).astype(np.int64)
    ok = (idx[:, 0] >= 0) & (idx[:, 0] < N) & (idx[:, 2] >= 0) & (idx[:, 2] < H) & (idx[:, 3] >= 0) & (idx[:, 3] < W)
    idx = idx[ok]
    active = np.zeros((N, H, W), dtype=bool)
    active[idx[:, 0], idx[:, 2], idx[:, 3]] = True
    near = _dilate(active)
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(W), indexing='ij')
    block = ((n * g['th'] + y // g['tile']) // g['tb_rows']) * g['tw4'] + (x // g['tile']) // g['tb_cols']
    chunk = (n * g['rp'] + (y // g['tile']) // g['ch_rows']) * g['tc4'] + (x // g['tile']) // g['ch_cols']

    def listed(ids, mask, total):
        f = np.zeros((total,), dtype=bool)
        f[ids[mask]] = True
        return np.flatnonzero(f).astype(np.int32), np.flatnonzero(~f).astype(np.int32)
    cin, cin_r = listed(block, near, g['nblocks'])
    cout, cout_r = listed(block, active, g['nblocks'])
    wg, _ = listed(chunk, near, g['nchunks'])
    return {'conv_in': cin, 'conv_in_rest': cin_r, 'conv_out': cout, 'conv_out_rest': cout_r, 'wgrad': wg}
