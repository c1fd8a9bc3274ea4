"""Hand-built boxes for the rotated BEV overlap / IoU / NMS kernels (csrc/iou3d_bev.h, csrc/iou3d_nms.hip) at the places where a
rotated-rectangle clipper and a bitmap scan go wrong: collinear edges, duplicate hull vertices, ties in the polar sort, boxes
inside the reference's 1e-2 corner margin, suppressions across the 64-box words and the 4,096-box registers of the scan, and the
switch between the single-stage and the prefix-stage batched NMS. numpy only, float32, fixed seeds, no GPU.

A box is [x, y, z, l, w, h, yaw]. u = (cos yaw, sin yaw) is a box's long-axis unit vector, v = (-sin yaw, cos yaw) the short one.

Pair cases (`pair_cases()`, a tuple of dicts: name, family, a (7,), b (7,), closed = closed-form BEV overlap or None):

  family 1 .. 14, each at CENTRES x YAWS (14 x 2 x 7 = 196 cases, `family_cases()`), base box L x W = 3.9 x 1.6:
     1 identical                               l w          8 yaw + pi                                  l w
     2 shifted by 1.0 u                        (l - 1) w    9 yaw negated                               -
     3 shifted by 0.5 v                        l (w - 0.5)  10 concentric 1.6 x 1.6 at yaw + pi/4        -
     4 the same rectangle as (w, l, yaw+pi/2)  l w          11 shares one corner (shifted l u + w v)     -
     5 nested 1 x 0.5, same yaw                0.5          12 near copy (+0.3, -0.2, 4.1 x 1.7, +0.1)   -
     6 nested 1 x 0.5, yaw + 0.4               0.5          13 1.0 x 1.6 centred on the short edge       0.5 w
     7 shares the short edge (shifted l u)     -            14 yaw + 2 pi                                l w
  'zero_zero', 'zero_car'   boxes of size 0
  'margin'                  THIN boxes end to end with a gap of 2, 5, 9 and 12 mm: disjoint, but up to 1e-2 the reference counts the
                            corners of one as inside the other and returns the area of the strip between them (family 'margin',
                            gap_mm in the case); 12 mm gives exactly 0
  'tiny'                    two 4 mm squares with centres 8 mm apart: all 8 corners lie in the other's margin zone, the "overlap"
                            exceeds both areas, the union clamps at 1e-8 and the IoU is 4,800
  'z_same', 'z_touch', 'z_nested', 'z_flat'   family 1 with the second box's z / h changed (3-D IoU only)
Boxes with a negative size are left out: the reference returns 8e8 for them and nothing is promised there.

NMS sets (dicts: boxes (n, 7) in score order, and per threshold the picks expected by construction, `picks[(thresh, rotated)]`):
duplicates(), nan_rows(), zero_size(), block_edges(n) for n in BLOCK_EDGE_N, thin(name) for name in THIN_SETS. A set's lattice is a
square grid of cars (pitch PITCH = 6 m, random yaw) that are farther apart than any two box diagonals, so every one survives;
plants replace lattice boxes:
  copy      box i = box src (src < i, src survives): i goes
  partial   box i = box src shifted by PARTIAL_SHIFT v: IoU 0.3 under the threshold 0.5, i stays
  chain     A -> B -> C: B = A + 0.4 v (IoU 0.6, goes), C = A + 0.8 v (IoU 0.6 with B, 1/3 with A): C stays
Sources of a partial or a chain have yaw 0, so the axis-aligned NMS (which ignores the yaw) sees the same rectangles.

Prefix sets (`prefix_frames(nmax, max_keep)`): the frames of one crb_nms_batched call, whose prefix stage is on for
nmax >= 2 p, p = prefix_len(max_keep). PREFIX_CONFIGS lists (nmax, max_keep); `prefix_twin` gives the single-stage twin at nmax - 1.
"""
import functools

import numpy as np

F32 = np.float32
CENTRES = ((10.0, 5.0), (69.9, -39.9))
YAWS = (0.0, np.pi / 2, np.pi, -np.pi / 2, np.pi / 4, 0.3, -2.8)
L, W, H, Z = 3.9, 1.6, 1.5, -1.0
MARGIN = 1e-2                                      # the reference's corner margin
THIN = ((4.0, 0.2), (0.8, 0.1), (2.0, 0.15), (1.0, 0.12))          # l x w of the margin pairs
THIN_YAWS = (0.0, 0.3, np.pi / 2, -2.8)
GAPS_MM = (2, 5, 9, 12)
FAMILY_NAMES = {1: 'identical', 2: 'shift_u', 3: 'shift_v', 4: 'swapped_lw', 5: 'nested', 6: 'nested_rot', 7: 'short_edge',
                8: 'yaw_pi', 9: 'yaw_neg', 10: 'concentric', 11: 'corner', 12: 'near_copy', 13: 'straddle', 14: 'yaw_2pi'}
CLOSED_FAMILIES = (1, 2, 3, 4, 5, 6, 8, 13, 14)
# family cases whose oracle value moves by more than half the 2e-5 bar under a one-ulp change of a yaw (found by
# tests/test_iou3d_edges_cpu.py::test_family_cases_are_stable_under_one_ulp_of_yaw; at most 5 % of the list may stand here)
UNSTABLE = ()

PITCH = 6.0
PARTIAL_SHIFT = W * 0.7 / 1.3                      # (w - s) / (w + s) = 0.3
BLOCK_EDGE_N = (130, 4160, 32768)
THIN_SETS = ('thin_4x0.2', 'thin_others', 'tiny')
PREFIX_CONFIGS = ((2048, 8), (2432, 600))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def box(x, y, l, w, yaw, z=Z, h=H):
    return np.array([x, y, z, l, w, h, yaw], np.float64).astype(F32)


def axes(yaw):
    return np.array([np.cos(yaw), np.sin(yaw)]), np.array([-np.sin(yaw), np.cos(yaw)])


def _family(k, c, r):
    """-> a, b, closed form of the BEV overlap (or None). Positions are computed in f64 and rounded once."""
    c = np.asarray(c, np.float64)
    u, v = axes(r)
    a = box(c[0], c[1], L, W, r)
    at = lambda d, l=L, w=W, yaw=r: box(c[0] + d[0], c[1] + d[1], l, w, yaw)      # noqa: E731
    if k == 1:
        return a, a.copy(), L * W
    if k == 2:
        return a, at(1.0 * u), (L - 1.0) * W
    if k == 3:
        return a, at(0.5 * v), L * (W - 0.5)
    if k == 4:
        return a, at(0 * u, W, L, r + np.pi / 2), L * W
    if k == 5:
        return a, at(0 * u, 1.0, 0.5), 0.5
    if k == 6:
        return a, at(0 * u, 1.0, 0.5, r + 0.4), 0.5
    if k == 7:
        return a, at(L * u), None
    if k == 8:
        return a, at(0 * u, yaw=r + np.pi), L * W
    if k == 9:
        return a, at(0 * u, yaw=-r), None
    if k == 10:
        return a, at(0 * u, 1.6, 1.6, r + np.pi / 4), None
    if k == 11:
        return a, at(L * u + W * v), None
    if k == 12:
        return a, at(np.array([0.3, -0.2]), 4.1, 1.7, r + 0.1), None
    if k == 13:
        return a, at(0.5 * L * u, 1.0, W), 0.5 * W
    if k == 14:
        return a, at(0 * u, yaw=r + 2 * np.pi), L * W
    raise KeyError(k)


def _case(name, family, a, b, closed=None, **extra):
    return _frozen(dict(name=name, family=family, a=a, b=b, closed=None if closed is None else float(closed), **extra))


@functools.lru_cache(maxsize=None)
def family_cases():
    out = []
    for k in range(1, 15):
        for ci, c in enumerate(CENTRES):
            for yi, r in enumerate(YAWS):
                name = 'f%02d_%s/c%d/y%d' % (k, FAMILY_NAMES[k], ci, yi)
                if name in UNSTABLE:
                    continue
                a, b, closed = _family(k, c, r)
                out.append(_case(name, FAMILY_NAMES[k], a, b, closed, k=k))
    return tuple(out)


def end_to_end(l, w, gap, yaw, c=CENTRES[0]):
    """two l x w boxes on one axis, `gap` between their facing short edges, symmetric about c"""
    u, _ = axes(yaw)
    d = 0.5 * (l + gap) * u
    return box(c[0] - d[0], c[1] - d[1], l, w, yaw), box(c[0] + d[0], c[1] + d[1], l, w, yaw)


def tiny_pair(c=CENTRES[0]):
    return box(c[0], c[1], 0.004, 0.004, 0.0), box(c[0] + 0.008, c[1], 0.004, 0.004, 0.0)


@functools.lru_cache(maxsize=None)
def margin_cases():
    out = []
    for (l, w), yaw in zip(THIN, THIN_YAWS):
        for g in GAPS_MM:
            a, b = end_to_end(l, w, g * 1e-3, yaw)
            out.append(_case('margin_%gx%g/gap%dmm' % (l, w, g), 'margin', a, b, gap_mm=g))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def z_cases():
    """family 1 with the second box moved / resized in z: name -> (z, h of b, expected 3-D IoU given a BEV IoU of 1)"""
    variants = {'z_same': (Z, H, 1.0), 'z_touch': (Z + H, H, 0.0), 'z_nested': (Z + 0.25, 0.5, 0.5 / H), 'z_flat': (Z, 0.0, 0.0)}
    out = []
    for name, (z, h, iou3d) in variants.items():
        for ci, c in enumerate(CENTRES):
            for yi, r in enumerate(YAWS):
                a, b, _ = _family(1, c, r)
                a, b = a.copy(), b.copy()
                b[2], b[5] = z, h
                if name == 'z_flat':
                    a[5] = 0.0
                out.append(_case('%s/c%d/y%d' % (name, ci, yi), name, a, b, L * W, iou3d=iou3d))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pair_cases():
    c = CENTRES[0]
    zero = box(c[0], c[1], 0.0, 0.0, 0.3)
    extra = [_case('zero_zero', 'zero', zero, zero.copy(), 0.0), _case('zero_car', 'zero', zero, box(c[0], c[1], L, W, 0.3), 0.0)]
    a, b = tiny_pair()
    extra.append(_case('tiny_4mm', 'tiny', a, b))
    return family_cases() + tuple(extra) + margin_cases() + z_cases()


def stack(cases):
    """-> a (n, 7), b (n, 7)"""
    return np.stack([c['a'] for c in cases]), np.stack([c['b'] for c in cases])


# ---------------------------------------------------------------------------------------------------------------- NMS sets
def lattice(n, seed, pitch=PITCH):
    """n cars on a square grid centred on the origin, random yaw, row-major in score order"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    xy = (np.stack([i % side, i // side], 1) - (side - 1) / 2.0) * pitch
    b = np.zeros((n, 7), np.float64)
    b[:, :2] = xy
    b[:, 2], b[:, 3], b[:, 4], b[:, 5] = Z, L, W, H
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b.astype(F32)


def _shift_v(b, s):
    """copy of box b moved by s along its short axis"""
    _, v = axes(float(b[6]))
    out = b.astype(np.float64)
    out[:2] += s * v
    return out.astype(F32)


def _nms_set(name, boxes, picks, **extra):
    picks = {k: np.asarray(v, np.int64) for k, v in picks.items()}
    return _frozen(dict(name=name, boxes=np.ascontiguousarray(boxes, dtype=F32), picks=picks, **extra))


@functools.lru_cache(maxsize=None)
def duplicates(k=70):
    """k copies of one car, then a far one: the copies cross a 64-box word"""
    b = np.repeat(box(10.0, 5.0, L, W, 0.3)[None], k + 1, 0)
    b[k] = box(40.0, -20.0, L, W, -1.0)
    picks = {}
    for rot in (True, False):
        picks[(0.5, rot)] = picks[(0.0, rot)] = [0, k]
        picks[(-1.0, rot)] = [0]
    return _nms_set('duplicates', b, picks)


@functools.lru_cache(maxsize=None)
def nan_rows():
    """car, the same car with a NaN centre, with a NaN yaw, two plain copies, a far car. Rotated: a NaN row overlaps nothing (every
    comparison of its corners is false), it is kept and suppresses nothing. Axis-aligned: the yaw is not read, so the NaN-yaw row
    is a plain copy and goes; fmaxf / fminf drop a NaN operand, so the NaN-centre row takes the other box's edges, has IoU 1 with
    it and goes too."""
    car = box(10.0, 5.0, L, W, 0.3)
    b = np.repeat(car[None], 6, 0)
    b[1, :2] = np.nan
    b[2, 6] = np.nan
    b[5] = box(40.0, -20.0, L, W, -1.0)
    return _nms_set('nan_rows', b, {(0.5, True): [0, 1, 2, 5], (0.5, False): [0, 5]})


@functools.lru_cache(maxsize=None)
def zero_size():
    """three boxes of size 0 (two at one place, inside a later car): overlap 0 over a union clamped at 1e-8, all kept"""
    b = np.stack([box(10.0, 5.0, 0.0, 0.0, 0.3), box(10.0, 5.0, 0.0, 0.0, 0.3), box(30.0, 5.0, 0.0, 0.0, 0.0), box(10.0, 5.0, L, W, 0.3)])
    picks = {(t, rot): [0, 1, 2, 3] for t in (0.5, 0.0) for rot in (True, False)}
    return _nms_set('zero_size', b, picks)


# n: (copies {i: src}, partials {i: src}, chains [(A, B, C)])
_PLANTS = {
    130: ({63: 5, 64: 62, 129: 65}, {65: 6, 128: 7}, [(61, 66, 70)]),
    4160: ({63: 5, 64: 62, 4095: 7, 4096: 4094, 4097: 100, 4159: 4100}, {4098: 8, 4099: 4093}, [(4092, 4101, 4102)]),
    32768: ({28672: 28671, 28673: 3, 30720: 4097, 32704: 28700, 32767: 64}, {32765: 65, 28674: 28670},
            [(32700, 32705, 32766)]),
}


@functools.lru_cache(maxsize=None)
def block_edges(n):
    copies, partials, chains = _PLANTS[n]
    b = lattice(n, 500 + n)
    for src in list(partials.values()) + [c[0] for c in chains]:
        b[src, 6] = 0.0
    for A, B, C in chains:
        b[B], b[C] = _shift_v(b[A], 0.4), _shift_v(b[A], 0.8)
    for i, src in partials.items():
        b[i] = _shift_v(b[src], PARTIAL_SHIFT)
    for i, src in sorted(copies.items()):
        assert src < i
        b[i] = b[src]
    gone = sorted(list(copies) + [c[1] for c in chains])
    keep = np.setdiff1d(np.arange(n), gone)
    planted = [(src, i, 'copy') for i, src in copies.items()] + [(src, i, 'partial') for i, src in partials.items()]
    for A, B, C in chains:
        planted += [(A, B, 'chain_ab'), (B, C, 'chain_bc'), (A, C, 'chain_ac')]
    return _nms_set('block_edges_%d' % n, b, {(0.5, True): keep, (0.5, False): keep}, planted=tuple(planted))


_THIN_SLOTS = {'thin_4x0.2': ((63, 64),), 'thin_others': ((10, 40), (62, 64), (63, 69)), 'tiny': ((63, 64),)}


@functools.lru_cache(maxsize=None)
def thin(name):
    """margin pairs (gap 9 mm) or the 4 mm pair in a 12 m lattice of 70 cars. A pair (i, j) is centred on cell i and takes the rows
    i and j (cell j stays empty); the slots straddle the first 64-box word. Under the rotated NMS box j must go; under the
    axis-aligned one (the rectangles are disjoint) it stays."""
    b = lattice(70, 600 + THIN_SETS.index(name), pitch=12.0)
    slots = _THIN_SLOTS[name]
    which = {'thin_4x0.2': (0,), 'thin_others': (1, 2, 3), 'tiny': (None,)}[name]
    thresh = {'thin_4x0.2': 1e-3, 'thin_others': 2e-3, 'tiny': 0.5}[name]
    for (i, j), k in zip(slots, which):
        c = b[i, :2].astype(np.float64)
        b[i], b[j] = tiny_pair(c) if k is None else end_to_end(THIN[k][0], THIN[k][1], 9e-3, THIN_YAWS[k], c)
    gone = [j for _, j in slots]
    return _nms_set(name, b, {(thresh, True): np.setdiff1d(np.arange(70), gone), (thresh, False): np.arange(70)},
                    thresh=thresh, planted=tuple((i, j, 'margin') for i, j in slots))


# ---------------------------------------------------------------------------------------------------------------- prefix sets
def prefix_len(max_keep):
    """length of the prefix stage of crb_nms_batched (csrc/iou3d_nms.hip, nms_prefix); it runs for nmax >= 2 * prefix_len"""
    return max(1024, (2 * max_keep + 63) // 64 * 64)


FRAME_NAMES = ('spread', 'continue_at_p', 'last_pick_p-1', 'last_pick_p', 'counts_p', 'counts_p+1', 'counts_0', 'counts_1',
               'counts_nmax', 'suppressed_beyond_p')


@functools.lru_cache(maxsize=None)
def prefix_frames(nmax, max_keep):
    """-> boxes (F, nmax, 7), counts (F,), picks (F index arrays: the first max_keep picks), FRAME_NAMES: the frames of one
    two-stage call (nmax >= 2 p, p = prefix_len(max_keep)). All frames are one lattice with rows overwritten by box 0."""
    K, p = max_keep, prefix_len(max_keep)
    assert nmax >= 2 * p and K - 1 <= p - 2 and p + K <= nmax
    base = lattice(nmax, 700 + nmax)
    frames, counts, picks = [], [], []

    def add(dup, count, expect):
        b = base.copy()
        b[np.asarray(dup, np.int64)] = base[0]
        frames.append(b)
        counts.append(count)
        e = np.asarray(expect, np.int64)
        assert len(e) <= K and (len(e) == 0 or e.max() < count)
        picks.append(e)

    r = np.arange
    add([], nmax, r(K))                                                            # decided inside the prefix
    add(r(1, p), nmax, np.r_[0, p + r(K - 1)])                                     # picks continue at p
    add(r(K - 1, p - 1), nmax, np.r_[r(K - 1), p - 1])                             # the K-th pick is the prefix's last box
    add(r(K - 1, p), nmax, np.r_[r(K - 1), p])                                     # ... is the first box after it
    add(np.setdiff1d(r(1, p), [5, p - 1]), p, [0, 5, p - 1])                       # counts = p, fewer than K survive
    add(r(1, p), p + 1, [0, p])                                                    # counts = p + 1, the last box survives
    add([], 0, [])
    add([], 1, [0])
    add(r(1, nmax - 1), nmax, [0, nmax - 1])                                       # counts = nmax, the very last box survives
    add(np.r_[r(1, p), p + 1], nmax, np.r_[0, p, p + 2 + r(K - 2)])                # p + 1 copies box 0: suppressed from inside the prefix
    boxes = np.stack(frames)
    boxes.setflags(write=False)
    return boxes, np.asarray(counts, np.int32), tuple(picks), FRAME_NAMES


def prefix_twin(nmax, max_keep):
    """the single-stage twin: the same frames without their last row (nmax - 1 < 2 p). A greedy pick depends on earlier rows only,
    so the picks are the two-stage ones below nmax - 1."""
    boxes, counts, picks, names = prefix_frames(nmax, max_keep)
    assert nmax - 1 < 2 * prefix_len(max_keep)
    return (np.ascontiguousarray(boxes[:, :nmax - 1]), np.minimum(counts, nmax - 1).astype(np.int32),
            tuple(e[e < nmax - 1] for e in picks), names)
