"""Cases and the f64 definition of the Part-A2 point head's targets and losses (csrc/part_head.hip, crbhip/part_head.py), shared by
tests/golden/make_goldens_parta2.py (which runs the reference on them) and the tests.

Targets: PointHeadTemplate.assign_stack_targets in set_ignore_flag mode with ret_part_labels=True; losses: get_cls_layer_loss with the
sigmoid focal loss + get_part_layer_loss. Points: half inside enlarged ground truths, half anywhere in range; a point closer than MARGIN
to a face plane of any box or enlarged box (zero-padded rows included, which also keeps the origin clear) is dropped, so that f32 and
f64 containment agree; the generator asserts that at most 1 % of the drawn points go (a 3.9 x 1.6 x 1.56 box has a 2e-4 m shell of
6e-3 m^3 against 9.7 m^3). Logits are uniform in [-8, 8]."""
import numpy as np

PCR = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
EXTRA = [0.2, 0.2, 0.2]                      # TARGET_CONFIG.GT_EXTRA_WIDTH of PartA2.yaml
ALPHA, GAMMA = 0.25, 2.0
LOSS_WEIGHTS = {'point_cls_weight': 1.5, 'point_part_weight': 0.75}   # (the yaml has 1.0 / 1.0: unequal values show a swapped weight)
MARGIN = 1e-4
LOSS_TILE = 1024                             # rows per workgroup of the loss kernels
BOX_CHUNK = 64                               # ground truths per LDS pass of the target kernel
SIZES = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}

# name -> (num_class, points per frame, real boxes per frame, G, seed). What each is for:
#   ragged   1,337 / 1 / 0 points; 68 real boxes of 70 rows in frame 0 (two LDS passes, the owner of some points lies in the second),
#            box 1 overlaps box 0 and box 66 overlaps box 10 (the lower index wins), frame 2 has no ground truth; 2 loss tiles
#   one      num_class = 1 (every owned point is labelled 1 whatever the box's class); one full tile + a partial one
#   tiles    3 full loss tiles + 77 rows
#   no_pos   no positive at all (normaliser 1, part loss exactly 0): boxes out of the points' reach, plus points planted in the enlarged
#            shells (label -1); one partial tile
CASES = {'ragged': (3, (1337, 1, 0), (68, 5, 0), 70, 11), 'one': (1, (700, 500), (12, 9), 12, 12),
         'tiles': (3, (2000, 1149), (20, 17), 20, 13), 'no_pos': (3, (150, 150), (3, 2), 4, 14)}


def _boxes(rng, n_real, G, x_range):
    gt = np.zeros((G, 8), np.float32)
    for g in range(n_real):
        c = int(rng.integers(1, 4))
        s = np.array(SIZES[c]) * rng.uniform(0.85, 1.15, 3)
        gt[g] = [rng.uniform(*x_range), rng.uniform(PCR[1] + 3, PCR[4] - 3), -1.0 + rng.uniform(-0.3, 0.3), *s, rng.uniform(-np.pi, np.pi), c]
    return gt


def _local(pts, box):
    """pts (n,3) f64 -> coordinates in the box frame (rotate_z(p - c, -rz))"""
    d = pts - box[None, 0:3].astype(np.float64)
    c, s = np.cos(np.float64(box[6])), np.sin(np.float64(box[6]))
    return np.stack([d[:, 0] * c + d[:, 1] * s, -d[:, 0] * s + d[:, 1] * c, d[:, 2]], 1)


def _to_world(loc, box):
    c, s = np.cos(np.float64(box[6])), np.sin(np.float64(box[6]))
    return np.stack([loc[:, 0] * c - loc[:, 1] * s + box[0], loc[:, 0] * s + loc[:, 1] * c + box[1], loc[:, 2] + box[2]], 1)


def _near_a_face(pts, gt, extra):
    """(n) bool: closer than MARGIN to a face of a row of gt (G,8) or of its enlarged twin (to the face's plane, and not farther than
    MARGIN outside the box along the other two axes)"""
    near = np.zeros(len(pts), bool)
    for box in gt:
        loc = np.abs(_local(pts.astype(np.float64), box))
        for dims in (box[3:6].astype(np.float64), (box[3:6] + np.asarray(extra, np.float32)).astype(np.float64)):
            plane = np.abs(loc - dims[None, :] / 2) < MARGIN
            within = loc < dims[None, :] / 2 + MARGIN
            for ax in range(3):
                near |= plane[:, ax] & within[:, (ax + 1) % 3] & within[:, (ax + 2) % 3]
    return near


def make_case(name):
    """-> dict: points (N,4) f32 [b,x,y,z] frame-sorted, counts, offsets (B+1) i32, gt_boxes (B,G,8) f32, num_class, cls_preds (N,C),
    part_preds (N,3)"""
    num_class, counts, n_real, G, seed = CASES[name]
    rng = np.random.default_rng(seed)
    B = len(counts)
    x_range = (42.0, 66.0) if name == 'no_pos' else (4.0, 66.0)
    gt = np.stack([_boxes(rng, n_real[b], G, x_range) for b in range(B)])
    if name == 'ragged':
        for lo, hi in ((0, 1), (10, 66)):                  # overlapping pairs, other class: the lower index owns the shared points
            gt[0, hi] = gt[0, lo]
            gt[0, hi, 0:2] += [0.6, 0.25]
            gt[0, hi, 6] += 0.3
            gt[0, hi, 7] = gt[0, lo, 7] % 3 + 1
    rows, drawn, dropped = [], 0, 0
    for b in range(B):
        want = counts[b]
        n = want + max(4, want // 25) if want else 0
        half = n // 2 if n_real[b] else 0
        if name == 'no_pos':
            any_pts = np.stack([rng.uniform(0.5, 38.0, n - half), rng.uniform(PCR[1], PCR[4], n - half), rng.uniform(PCR[2], PCR[5], n - half)], 1)
        else:
            any_pts = np.stack([rng.uniform(PCR[0], PCR[3], n - half), rng.uniform(PCR[1], PCR[4], n - half),
                                rng.uniform(PCR[2], PCR[5], n - half)], 1)
        near = []
        for k in range(half):
            box = gt[b, int(rng.integers(0, n_real[b]))]
            loc = rng.uniform(-0.5, 0.5, (1, 3)) * (box[3:6] + np.asarray(EXTRA, np.float32))
            if name == 'no_pos':                           # in the shell: beyond the box in x, inside the enlarged box
                loc[0, 0] = np.sign(loc[0, 0] + 1e-9) * (box[3] / 2 + 0.05)
            near.append(_to_world(loc, box)[0])
        pts = np.concatenate([np.asarray(near).reshape(-1, 3), any_pts]).astype(np.float32)
        pts = pts[rng.permutation(len(pts))]
        bad = _near_a_face(pts, gt[b], EXTRA)
        drawn, dropped = drawn + len(pts), dropped + int(bad.sum())
        pts = pts[~bad][:want]
        assert len(pts) == want, (name, b, len(pts))
        rows.append(np.concatenate([np.full((want, 1), b, np.float32), pts], 1))
    assert dropped <= 0.01 * drawn, (name, dropped, drawn)
    points = np.concatenate(rows).astype(np.float32)
    N = len(points)
    return {'points': points, 'counts': list(counts), 'offsets': np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
            'gt_boxes': gt, 'num_class': num_class, 'cls_preds': rng.uniform(-8, 8, (N, num_class)).astype(np.float32),
            'part_preds': rng.uniform(-8, 8, (N, 3)).astype(np.float32)}


def face_case():
    """points ON the faces of ground truths and enlarged ground truths and one f32 step to either side, B = 2 frames of equal size (the
    existing points_in_boxes_gpu route wants that) -> points (N,4), gt_boxes (2,6,8). Only for bit-equality between device routes."""
    rng = np.random.default_rng(21)
    gt = np.stack([_boxes(rng, 5, 6, (4.0, 66.0)) for _ in range(2)])
    gt[0, 0, 6], gt[1, 1, 6] = 0.0, np.float32(np.pi / 2)              # axis-aligned boxes: the face value is hit exactly
    frames = []
    for b in range(2):
        pts = []
        for box in gt[b, :5]:
            for extra in (0.0, 0.2):
                for ax in range(3):
                    for sgn in (-1.0, 1.0):
                        for eps in (0.0, 1e-5):                       # the bare half extent and the 1e-5 margin of x / y
                            loc = rng.uniform(-0.4, 0.4, (1, 3)) * box[3:6]
                            loc[0, ax] = sgn * ((np.float64(box[3 + ax]) + extra) / 2 + eps)
                            p = _to_world(loc, box)[0].astype(np.float32)
                            for q in (p, np.nextafter(p, np.float32(-1e9)), np.nextafter(p, np.float32(1e9))):
                                pts.append(q)
        frames.append(np.concatenate([np.full((len(pts), 1), b, np.float32), np.asarray(pts, np.float32)], 1))
    return np.concatenate(frames), gt


# ---- the definition, f64 ------------------------------------------------------------------------------------------------------
def _contains_f64(pts, box, dims):
    loc = np.abs(_local(pts, box))
    return (loc[:, 2] <= dims[2] / 2) & (loc[:, 0] < dims[0] / 2 + 1e-5) & (loc[:, 1] < dims[1] / 2 + 1e-5)


def targets_f64(points, gt_boxes, num_class, extra=EXTRA):
    """-> labels (N) i64, part_labels (N,3) f64, owner (N) i32"""
    N = len(points)
    labels, part, owner = np.zeros(N, np.int64), np.zeros((N, 3)), np.full(N, -1, np.int32)
    frame = points[:, 0].astype(np.int64)
    pts = points[:, 1:4].astype(np.float64)
    shell = np.zeros(N, bool)
    for b in range(gt_boxes.shape[0]):
        rows = np.nonzero(frame == b)[0]
        for g in range(gt_boxes.shape[1] - 1, -1, -1):                 # downwards: the lowest index is written last
            box = gt_boxes[b, g]
            dims = box[3:6].astype(np.float64)
            inside = _contains_f64(pts[rows], box, dims)
            owner[rows[inside]] = g
            shell[rows] |= _contains_f64(pts[rows], box, (box[3:6] + np.asarray(extra, np.float32)).astype(np.float64))
    fg = owner >= 0
    labels[shell & ~fg] = -1
    for i in np.nonzero(fg)[0]:
        box = gt_boxes[frame[i], owner[i]]
        labels[i] = 1 if num_class == 1 else int(box[7])
        part[i] = _local(pts[i:i + 1], box)[0] / box[3:6].astype(np.float64) + 0.5
    return labels, part, owner


def losses_f64(cls_preds, part_preds, labels, part_labels, alpha=ALPHA, gamma=GAMMA, weights=LOSS_WEIGHTS):
    """-> dict: loss_cls, loss_part, pos, d_cls (N,C), d_part (N,3), all f64, for unit upstream gradients"""
    x, y, t = cls_preds.astype(np.float64), part_preds.astype(np.float64), part_labels.astype(np.float64)
    C = x.shape[1]
    pos = float((labels > 0).sum())
    norm = max(pos, 1.0)
    tgt = (labels[:, None] == np.arange(1, C + 1)[None, :]).astype(np.float64)
    w = (labels >= 0).astype(np.float64)[:, None] / norm
    p = 1.0 / (1.0 + np.exp(-x))
    bce = np.maximum(x, 0) - x * tgt + np.log1p(np.exp(-np.abs(x)))
    pt = tgt * (1 - p) + (1 - tgt) * p
    aw = tgt * alpha + (1 - tgt) * (1 - alpha)
    wc, wp = weights['point_cls_weight'], weights['point_part_weight']
    dpt = np.where(tgt > 0, -1.0, 1.0) * p * (1 - p)
    d_cls = aw * (gamma * pt ** (gamma - 1) * dpt * bce + pt ** gamma * (p - tgt)) * w * wc
    m = (labels > 0).astype(np.float64)[:, None]
    q = 1.0 / (1.0 + np.exp(-y))
    pbce = np.maximum(y, 0) - y * t + np.log1p(np.exp(-np.abs(y)))
    return {'loss_cls': np.array((aw * pt ** gamma * bce * w).sum() * wc), 'loss_part': np.array((pbce * m).sum() / (3 * norm) * wp),
            'pos': np.array(pos), 'd_cls': d_cls, 'd_part': (q - t) * m / (3 * norm) * wp}


# ---- UNetV2 on a reduced grid -------------------------------------------------------------------------------------------------
# 32 x 32 x 24 cells of 0.2 m: z 25 -> 13 -> 7 -> 3 -> 1 through the four strided levels. B = 2, about 600 voxels in blobs (neighbours at
# every level). The seeded state (tests/golden/_constants.seeded_state, UNET_SEED) carries the golden's BatchNorm biases on top, which keep
# every ReLU input of the f64 forward pass farther than UNET_KINK from zero: without that margin a handful of the ~1e6 ReLU masks are
# decided by rounding and the gradients move by whole terms, in the reference's own f32 run as in any other.
UNET_GRID = (32, 32, 24)                       # x, y, z
UNET_VOXEL = [0.2, 0.2, 0.2]
UNET_PCR = [0.0, -3.2, -3.0, 6.4, 3.2, 1.8]
UNET_SEED, UNET_KINK = 47, 1e-4
# the gradients the golden stores (encoder, bottom, decoder, last lateral block) and the slice of each that is kept
UNET_GRADS = {'conv_input.0.weight': np.s_[:], 'conv4.0.0.weight': np.s_[:8], 'inv_conv3.0.weight': np.s_[:8],
              'conv_up_t1.conv1.weight': np.s_[:]}


def unet_inputs():
    """-> voxel_features (N,4) f32, voxel_coords (N,4) i32 [b,z,y,x] frame-sorted, ascending inside a frame, batch_size"""
    rng = np.random.default_rng(31)
    gx, gy, gz = UNET_GRID
    rows = []
    for b in range(2):
        cells = set()
        for _ in range(5):
            c = np.array([rng.uniform(3, gz - 3), rng.uniform(4, gy - 4), rng.uniform(4, gx - 4)])
            for _ in range(70):
                z, y, x = np.round(c + rng.normal(0, [1.5, 2.0, 2.0])).astype(int)
                if 0 <= z < gz and 0 <= y < gy and 0 <= x < gx:
                    cells.add((int(z), int(y), int(x)))
        rows += [(b,) + c for c in sorted(cells)]
    coords = np.asarray(rows, np.int32)
    return rng.normal(0, 1, (len(coords), 4)).astype(np.float32), coords, 2


def unet_probe(n_points, n_encoded):
    """the fixed directions the golden's loss is taken along: loss = sum(point_features * r1) + sum(encoded rows, ascending (b,z,y,x),
    * r2)"""
    rng = np.random.default_rng(32)
    return rng.normal(0, 1, (n_points, 16)), rng.normal(0, 1, (n_encoded, 128))


def linear_order(indices, shape):
    """argsort of (N,4) [b,z,y,x] rows by their linear index"""
    i = np.asarray(indices, np.int64)
    return np.argsort(((i[:, 0] * shape[0] + i[:, 1]) * shape[1] + i[:, 2]) * shape[2] + i[:, 3], kind='stable')


def nudge(v, margin):
    """the smallest shift s (a multiple of margin) with min|v + s| > margin"""
    for k in range(10000):
        for s in (k * margin, -k * margin):
            if np.abs(v + s).min() > margin:
                return s
    raise AssertionError('no shift found')
