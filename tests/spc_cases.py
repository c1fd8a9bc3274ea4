"""Deterministic cases for the SPC keypoint sampling tests (tests/test_spc_cpu.py, tests/test_spc_gpu.py) and numpy restatements
of what the kernels compute: the RoI proximity mask in f64, sector_fps's bookkeeping, and the reference's stack FPS kernel.

Frame cases are margin-safe by construction. After generation every point is removed
  * whose mask decision changes within +-1e-4 m of the threshold |dims / 2| + radius,
  * whose nearest and second-nearest RoI centres are within 1e-4 m of each other,
  * whose azimuth lies within 1e-5 rad of a sector boundary (for every sector count the case is used with).
f32 rounding at 80 m range is 8e-6 m and atan2f is good to about 1e-6 rad: the margins cover the difference between libm, torch and
the device's functions and nothing coarser. At most 2 % of the generated points may go (asserted), and on the remaining points the
f32 torch expressions and the f64 numpy evaluation agree (asserted).
The two clamp-quirk points (-5, +-0.0, z) are added afterwards and listed in case['special']: their azimuth sits ON a boundary, their
sector is whatever the torch route gives on the device that runs the test, and they are excluded from the f64 comparisons."""
import math

import numpy as np

RADIUS = 1.6
SECTOR_COUNTS = (6, 1)
MAX_REMOVED = 0.02


# ---- f64 definitions -------------------------------------------------------------------------------------------------------------
def mask_f64(points, rois, radius):
    """-> (mask, nearest, slack, gap): slack = |min_dis - threshold|, gap = second-nearest distance - nearest distance"""
    p, r = points.astype(np.float64), rois.astype(np.float64)
    if len(p) == 0:
        z = np.zeros((0,))
        return z.astype(bool), z.astype(np.int64), z, z
    d = np.sqrt(((p[:, None, :] - r[None, :, 0:3]) ** 2).sum(-1))
    nearest = d.argmin(1)                                                  # (first minimum: the lowest index on a tie)
    dmin = d[np.arange(len(p)), nearest]
    thr = np.sqrt(((r[nearest, 3:6] / 2) ** 2).sum(-1)) + radius
    # (rows with the SAME centre, as the zero padding, are one centre: their distances are equal bit for bit in any arithmetic and the
    # lowest index wins everywhere; the gap guards centres that differ)
    _, first = np.unique(r[:, 0:3], axis=0, return_index=True)
    ds = np.sort(d[:, np.sort(first)], 1)
    gap = ds[:, 1] - ds[:, 0] if ds.shape[1] > 1 else np.full(len(p), np.inf)
    return dmin < thr, nearest, np.abs(dmin - thr), gap


def sector_f64(points, S):
    """-> (sector, distance of the azimuth to the nearest sector boundary in rad)"""
    p = points.astype(np.float64)
    size = np.pi * 2 / S
    a = np.arctan2(p[:, 1], p[:, 0]) + np.pi
    sec = np.clip(np.floor(a / size), 0, S).astype(np.int64)
    k = np.round(a / size)
    return sec, np.abs(a - k * size)


def quota(n_k, n, K):
    """the reference's three f64 operations (Python's ratio * num_sampled_points is not the exact rational)"""
    ratio = n_k / n
    return min(n_k, math.ceil(ratio * K))


def plan_numpy(counts, mask, sector, K, S):
    """sector_fps's bookkeeping for stacked frames, given the per-point mask and sector -> dict(src: rows of the stacked array in
    (frame, sector) segment order, input order inside a segment; seg: list of (frame, sector, n, m))"""
    src, seg, s = [], [], 0
    for b, n in enumerate(counts):
        kept = np.nonzero(mask[s:s + n])[0]
        if len(kept) == 0 and n > 0:
            kept = np.array([0])                                           # points[:1]
        sec = sector[s:s + n][kept]
        before = len(seg)
        for k in range(S):
            rows = kept[sec == k]
            if len(rows):
                src.append(rows + s)
                seg.append((b, k, len(rows), quota(len(rows), len(kept), K)))
        if len(seg) == before and len(kept):                               # every kept point fell to the clamp: one segment of all
            src.append(kept + s)
            seg.append((b, S, len(kept), min(len(kept), K)))
        s += n
    return {'src': np.concatenate(src) if src else np.zeros((0,), np.int64), 'seg': seg}


# ---- the reference's stack FPS kernel -------------------------------------------------------------------------------------------
_BREV10 = np.array([int('{:010b}'.format(i)[::-1], 2) for i in range(1024)], np.int64)


def _dist_update(p, q, temp):
    dx, dy, dz = p[:, 0] - q[0], p[:, 1] - q[1], p[:, 2] - q[2]           # f32 throughout, (dx dx + dy dy) + dz dz, no fma
    return np.minimum(dx * dx + dy * dy + dz * dz, temp)


def fps_order(xyz, cnt, m):
    """stack FPS as a total order on the candidates: larger running distance, then smaller bit-reversed (k mod 1024), then
    smaller k -> (sum m) GLOBAL indices"""
    out, s = [], 0
    for n, mk in zip(cnt, m):
        p = np.ascontiguousarray(xyz[s:s + n], np.float32)
        k = np.arange(n, dtype=np.int64)
        rank = _BREV10[k & 1023] * (1 << 32) + k
        temp = np.full(n, 1e10, np.float32)
        old, picks = 0, [0]
        for _ in range(1, min(mk, n)):
            temp = _dist_update(p, p[old], temp)
            cand = np.nonzero(temp == temp.max())[0]
            old = int(cand[np.argmin(rank[cand])])
            picks.append(old)
        out.append(np.array(picks[:min(mk, n)], np.int64) + s)
        s += n
    return np.concatenate(out) if out else np.zeros((0,), np.int64)


def fps_tree(xyz, cnt, m):
    """the same kernel thread by thread: 1024 threads scan k = tid, tid + 1024, ... and keep their first maximum (best starts at -1,
    besti at 0), then the LDS tree over 512, 256, ..., 1 pairs keeps the lower position unless the upper is strictly larger"""
    out, s = [], 0
    for n, mk in zip(cnt, m):
        p = np.ascontiguousarray(xyz[s:s + n], np.float32)
        rows = (n + 1023) // 1024
        temp = np.full(n, 1e10, np.float32)
        old, picks = 0, [0]
        for _ in range(1, min(mk, n)):
            temp = _dist_update(p, p[old], temp)
            pad = np.full(rows * 1024, -1.0, np.float32)
            pad[:n] = temp
            pad = pad.reshape(rows, 1024)
            first = pad.argmax(0)                                          # (numpy: the first maximum)
            d = pad[first, np.arange(1024)]
            i = np.where(d > -1.0, first * 1024 + np.arange(1024), 0)
            half = 512
            while half >= 1:
                take = d[half:2 * half] > d[:half]
                i[:half] = np.where(take, i[half:2 * half], i[:half])
                d[:half] = np.maximum(d[:half], d[half:2 * half])
                half //= 2
            old = int(i[0])
            picks.append(old)
        out.append(np.array(picks[:min(mk, n)], np.int64) + s)
        s += n
    return np.concatenate(out) if out else np.zeros((0,), np.int64)


# ---- frame cases ------------------------------------------------------------------------------------------------------------------
def _frame_rois(rng, miss):
    r = np.zeros((8, 7), np.float32)
    for k in range(6):
        r[k, 0:2] = rng.uniform(-45, 45, 2)
        r[k, 2] = rng.uniform(-1, 1)
        r[k, 3:6] = [rng.uniform(1.5, 5.0), rng.uniform(0.6, 2.2), rng.uniform(1.0, 2.0)]
        r[k, 6] = rng.uniform(-np.pi, np.pi)
    r[1, 0:3] = r[0, 0:3] + np.array([0.7, -0.4, 0.1], np.float32)         # two that overlap each other
    if miss:
        r[:6, 2] += 40.0                                                    # this frame's RoIs miss every point
    return r                                                                # rows 6, 7: zero padding (centre at the origin, size 0)


def _frame_points(rng, n, rois, miss):
    near = rng.integers(0, 6, n)
    centre = rois[near, 0:3].astype(np.float64)
    if miss:
        centre[:, 2] -= 40.0
    p = centre + rng.normal(0, 2.2, (n, 3))
    far = rng.random(n) < 0.3
    p[far] = np.stack([rng.uniform(-60, 60, far.sum()), rng.uniform(-60, 60, far.sum()), rng.uniform(-3, 1, far.sum())], 1)
    p[rng.random(n) < 0.02] *= 0.02                                         # a few around the origin: the zero-padded rows take part
    if miss:
        p = p[np.linalg.norm(p, axis=1) > RADIUS + 0.5]                     # ... but not in the frame that keeps nothing
    return p.astype(np.float32)


def frame_case(seed=0, counts=(1500, 37, 2300), miss_frame=1, special_frame=0):
    """-> dict(points (N, 3) f32, counts, rois (B, 8, 7) f32, radius, special: rows of the two clamp-quirk points, removed: fraction)"""
    rng = np.random.default_rng(1000 + seed)
    pts, cnt, rois, generated, removed = [], [], [], 0, 0
    for b, n in enumerate(counts):
        r = _frame_rois(rng, b == miss_frame)
        if b == special_frame:
            r[2] = [-6.0, 0.5, 0.0, 4.0, 2.0, 1.5, 0.3]                     # covers the clamp-quirk points
        p = _frame_points(rng, n, r, b == miss_frame)
        generated += len(p)
        mask, _, slack, gap = mask_f64(p, r, RADIUS)
        ok = (slack > 1e-4) & (gap > 1e-4)
        for S in SECTOR_COUNTS:
            ok &= sector_f64(p, S)[1] > 1e-5
        removed += int((~ok).sum())
        p = p[ok]
        if b == miss_frame:
            assert not mask_f64(p, r, RADIUS)[0].any()
        pts.append(p)
        cnt.append(len(p))
        rois.append(r)
    assert removed <= MAX_REMOVED * generated, (removed, generated)
    points = np.concatenate(pts)
    special = np.zeros((0,), np.int64)
    if special_frame is not None:
        s = int(np.sum(cnt[:special_frame]))
        at = s + cnt[special_frame] // 2
        quirk = np.array([[-5.0, 0.0, 0.1], [-5.0, -0.0, -0.2]], np.float32)
        points = np.concatenate([points[:at], quirk, points[at:]])
        cnt[special_frame] += 2
        special = np.array([at, at + 1])
        m, _, slack, gap = mask_f64(quirk, rois[special_frame], RADIUS)
        assert m.all() and (slack > 1e-2).all() and (gap > 1e-2).all()
    case = {'points': points, 'counts': cnt, 'rois': np.stack(rois), 'radius': RADIUS, 'special': special,
            'removed': removed / max(generated, 1)}
    _check_f32_agrees(case)
    return case


def _check_f32_agrees(case):
    """the f32 torch expressions of the reference and the f64 evaluation agree on every point that is not special"""
    import torch
    s = 0
    plain = np.ones(len(case['points']), bool)
    plain[case['special']] = False
    for b, n in enumerate(case['counts']):
        p, r = torch.from_numpy(case['points'][s:s + n]), torch.from_numpy(case['rois'][b])
        distance = (p[:, None, :] - r[None, :, 0:3]).norm(dim=-1)
        min_dis, idx = distance.min(dim=-1)
        m32 = (min_dis < (r[idx, 3:6] / 2).norm(dim=-1) + case['radius']).numpy()
        m64, near64, _, _ = mask_f64(case['points'][s:s + n], case['rois'][b], case['radius'])
        sel = plain[s:s + n]
        assert (m32 == m64)[sel].all() and (idx.numpy() == near64)[sel].all()
        for S in SECTOR_COUNTS:
            ang = torch.atan2(p[:, 1], p[:, 0]) + np.pi
            s32 = (ang / (np.pi * 2 / S)).floor().clamp(min=0, max=S).numpy().astype(np.int64)
            assert (s32 == sector_f64(case['points'][s:s + n], S)[0])[sel].all()
        s += n


def quota_case():
    """one frame, three sectors with 14 / 28 / 8 points, K = 25: (14 / 50) * 25 and (28 / 50) * 25 are integers in exact arithmetic
    (7 and 14) and land above them in f64 (quotas 8 and 15); 8 / 50 * 25 = 4 in both"""
    rng = np.random.default_rng(7)
    pts = []
    for k, n in ((0, 14), (2, 28), (4, 8)):
        a = -np.pi + (k + 0.5) * np.pi / 3 + rng.uniform(-0.3, 0.3, n)
        rad = rng.uniform(5, 40, n)
        pts.append(np.stack([rad * np.cos(a), rad * np.sin(a), rng.uniform(-1, 1, n)], 1))
    p = np.concatenate(pts).astype(np.float32)
    return {'points': p[rng.permutation(len(p))], 'K': 25, 'S': 6, 'quotas': [8, 15, 4], 'exact': [7, 14, 4]}


def fps_cases():
    """name -> (xyz (N, 3) f32, segment lengths, quotas): ties (every point three times), a segment longer than the 1024 threads, one
    beyond register residency (50,000 points, 32 picks), segments of 1 and 2 points, a segment sampled completely"""
    rng = np.random.default_rng(99)
    cloud = lambda n: np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n)], 1).astype(np.float32)
    base = cloud(230)
    ties = np.repeat(base, 3, 0)[rng.permutation(690)]
    grid = (rng.integers(0, 6, (1500, 3)) * np.float32(0.5)).astype(np.float32)          # many equal distances
    return {
        'ties': (np.concatenate([ties, grid]), [690, 1500], [48, 40]),
        'over_1024': (np.concatenate([cloud(1100), cloud(2100)]), [1100, 2100], [64, 33]),
        'large': (cloud(50000), [50000], [32]),
        'tiny': (np.concatenate([cloud(1), cloud(2), cloud(5), cloud(2)]), [1, 2, 5, 2], [1, 2, 3, 1]),
        'complete': (np.concatenate([cloud(77), grid[:40]]), [77, 40], [77, 40]),
        # every size at which the kernel takes another path: 2 / 4 / 8 / 20 points per thread in registers, then the global array
        'mid_paths': (np.concatenate([cloud(3000), cloud(5000), cloud(9000)]), [3000, 5000, 9000], [12, 12, 12]),
        'thresholds': (np.concatenate([cloud(2048), cloud(2049), cloud(4097)]), [2048, 2049, 4097], [9, 9, 9]),
        'past_registers': (np.concatenate([cloud(20480), cloud(20481)]), [20480, 20481], [8, 8]),
    }
