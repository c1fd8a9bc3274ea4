"""CPU: the host-visible pieces of the split-bf16 row GEMMs of the BEV up-sampling branches (csrc/rows_gemm4.hip, crbhip.rows_gemm):
prototypes and exports, which shapes have an instance, what the dispatcher answers (and why) without a device, and the weight-image
layout as the numpy restatement states it (the GPU test compares the kernel's image with that restatement bit for bit)."""
import subprocess

import numpy as np
import torch
import torch.nn as nn

NAMES = ('crb_rows_gemm4_supported', 'crb_rows_gemm4_weights_bytes', 'crb_rows_gemm4_weights', 'crb_rows_gemm4_forward',
         'crb_rows_gemm4_input_grad', 'crb_rows_gemm4_wgrad', 'crb_rows_gemm4_wgrad_workspace_bytes')


def test_prototypes_and_exports():
    import crbhip
    protos = crbhip.parse_header()
    exported = subprocess.check_output(['nm', '-D', '--defined-only', crbhip.lib_path], text=True)
    names = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    for name in NAMES:
        assert name in protos and name in names, name
    assert protos['crb_rows_gemm4_forward'] == protos['crb_rows_gemm4_input_grad']
    assert not [n for n in names if n.startswith('crb_rows_gemm4') and 'set_' in n]


def test_supported_shapes():
    from crbhip import lib, rows_gemm
    ok = lib.crb_rows_gemm4_supported
    F, I, W = rows_gemm.FORWARD, rows_gemm.INPUT_GRAD, rows_gemm.WGRAD
    # the two layers of the KITTI config
    assert ok(128, 256, 1, F) == 1 and ok(128, 256, 1, I) == 1 and ok(128, 256, 1, W) == 0
    assert ok(256, 256, 2, F) == 1 and ok(256, 256, 2, I) == 1 and ok(256, 256, 2, W) == 1
    # forward: K = cin in steps of 32, columns = cout in blocks of 128; the input gradient swaps the roles
    assert ok(32, 128, 2, F) == 1 and ok(48, 128, 2, F) == 0 and ok(64, 192, 1, F) == 0
    assert ok(128, 32, 2, I) == 1 and ok(128, 48, 2, I) == 0 and ok(192, 64, 1, I) == 0
    assert ok(512, 256, 1, W) == 1 and ok(384, 256, 2, W) == 0
    for bad in ((256, 256, 3, F), (256, 256, 0, F), (0, 256, 1, F), (256, 0, 1, I), (8192, 256, 1, F), (256, 256, 2, 3)):
        assert ok(*bad) == 0, bad
    assert lib.crb_rows_gemm4_weights_bytes(256, 256, 2) == 4 * 256 * 256 * 6
    assert lib.crb_rows_gemm4_weights_bytes(128, 256, 1) == 128 * 256 * 6
    assert lib.crb_rows_gemm4_wgrad_workspace_bytes(128, 256, 1) == 0
    n = lib.crb_rows_gemm4_wgrad_workspace_bytes(256, 256, 2)
    assert n > 0 and n % (8 * 4 * 256 * 256 * 4) == 0            # a multiple of 8 ranges of 4 taps x 256 x 256 f32 partials


def test_dispatch_says_why(monkeypatch):
    from crbhip import rows_gemm
    up2 = nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False)
    up1 = nn.ConvTranspose2d(128, 256, 1, stride=1, bias=False)
    x_cpu = torch.zeros(1, 256, 4, 4).contiguous(memory_format=torch.channels_last)
    assert rows_gemm.KERNEL == __import__('os').environ.get('CRB_ROWS_GEMM_KERNEL', 'x6')
    monkeypatch.setattr(rows_gemm, 'KERNEL', 'x6')
    path, why = rows_gemm.dispatch(up2, x_cpu)
    assert path == 'vendor' and 'device' in why
    assert rows_gemm.up_conv(up2, x_cpu) is None
    for conv in (nn.ConvTranspose2d(256, 256, 2, stride=2, bias=True), nn.ConvTranspose2d(256, 256, 3, stride=2, bias=False),
                 nn.ConvTranspose2d(256, 256, 4, stride=4, bias=False), nn.Conv2d(256, 256, 2, stride=2, bias=False),
                 nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False, groups=2), nn.Conv2d(256, 256, 3, padding=1, bias=False)):
        path, why = rows_gemm.dispatch(conv, x_cpu)
        assert path == 'vendor' and 'kernel = stride' in why, conv
    assert rows_gemm._geometry(up2) == (256, 256, 2, True) and rows_gemm._geometry(up1) == (128, 256, 1, True)
    assert rows_gemm._geometry(nn.Conv2d(128, 256, 1, bias=False)) == (128, 256, 1, False)
    monkeypatch.setattr(rows_gemm, 'KERNEL', 'vendor')
    path, why = rows_gemm.dispatch(up2, x_cpu)
    assert path == 'vendor' and 'CRB_ROWS_GEMM_KERNEL' in why
    assert not rows_gemm.use(256, 256, 2, rows_gemm.FORWARD)
    # per-launch switches: a launch that is switched off, or has no instance, is not used
    monkeypatch.setattr(rows_gemm, 'KERNEL', 'x6')
    monkeypatch.setattr(rows_gemm, 'LAUNCHES', {'2f'})
    assert rows_gemm.use(256, 256, 2, rows_gemm.FORWARD) and not rows_gemm.use(256, 256, 2, rows_gemm.INPUT_GRAD)
    monkeypatch.setattr(rows_gemm, 'LAUNCHES', {'1w', '2w'})
    assert not rows_gemm.use(128, 256, 1, rows_gemm.WGRAD) and rows_gemm.use(256, 256, 2, rows_gemm.WGRAD)
    assert set(rows_gemm.DEFAULT_LAUNCHES.split(',')) <= {'1f', '1i', '1w', '2f', '2i', '2w'}


def _bf16_to_f64(u16):
    return (u16.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def test_weight_image_layout_restated():
    """the image holds every weight exactly once per piece, the three pieces add up to the f32 weight exactly, and element
    [n / 32][k step][piece][lane][j] is Wm[k = 32 (ks / 2) + 16 (lane / 32) + 8 (ks % 2) + j][n = 32 nb + lane % 32]"""
    from crbhip import rows_gemm
    rng = np.random.default_rng(3)
    for cin, cout, s in ((64, 128, 2), (128, 256, 1), (32, 128, 2)):
        w = (rng.standard_normal((cin, cout, s, s)) * 10.0 ** rng.uniform(-3, 3, (cin, cout, s, s))).astype(np.float32)
        for direction in (rows_gemm.FORWARD, rows_gemm.INPUT_GRAD):
            if not rows_gemm.supported(cin, cout, s, direction):
                continue
            img = rows_gemm.weight_image_reference(w, s, direction)
            T = s * s
            K, N = (cin, T * cout) if direction == rows_gemm.FORWARD else (T * cout, cin)
            assert img.shape == (N // 32, K // 16, 3, 64, 8)
            assert img.size * 2 == rows_gemm.lib.crb_rows_gemm4_weights_bytes(cin, cout, s)
            total = _bf16_to_f64(img).sum(axis=2)                       # the pieces' sum, exact in f64
            for nb, ks, lane, j in ((0, 0, 0, 0), (N // 32 - 1, K // 16 - 1, 63, 7), (1, 1, 37, 5), (2, 1, 31, 2)):
                k = 32 * (ks >> 1) + 16 * (lane >> 5) + 8 * (ks & 1) + j
                n = 32 * nb + (lane & 31)
                ci, tc = (k, n) if direction == rows_gemm.FORWARD else (n, k)
                t, co = divmod(tc, cout)
                assert total[nb, ks, lane, j] == np.float64(w[ci, co, t // s, t % s]), (direction, nb, ks, lane, j)
            # every weight once: the multiset of reconstructed values is the multiset of weights
            assert np.array_equal(np.sort(total.reshape(-1)), np.sort(w.astype(np.float64).reshape(-1)))
            # a piece is below 2^-7 of the one before it (8 significant bits per piece)
            p = np.abs(_bf16_to_f64(img))
            assert np.all(p[:, :, 1] <= p[:, :, 0] * 2.0 ** -7) and np.all(p[:, :, 2] <= p[:, :, 0] * 2.0 ** -14)
