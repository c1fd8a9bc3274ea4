"""Heads, ground truths and predictions for the anchor head's target, loss and proposal kernels (csrc/target_assign.hip, csrc/rpn_loss.hip,
csrc/proposal_layer.hip) away from the one shipped configuration: 1 .. 10 classes (ids 8 and above), 1 .. 8 direction bins, ground-truth
tables around the 256-row staging loop and the 1,024-row LDS table, anchor counts below one block, at a block multiple and ending
inside the loss kernel's 4 x 256 strip. numpy / torch on the host only, fixed seeds, no test functions.

Everything lives on the small range [0, -8, -3, 17.6, 8, 1]. Class i (id i + 1, name 'K01', 'K02', ...) has one anchor size, two
rotations, and its own matched / unmatched thresholds (class_row below). Lengths are >= 3.0 m and matched thresholds <= 0.49
so that on the default 22 x 20 grid (0.84 m between anchors) a box sitting on an anchor makes that anchor and its two x-neighbours
positive; the y-neighbours land between the thresholds (ignored) or below them.

make_gt rows of frame 0 (G >= 8), all other rows being ordinary boxes drawn on anchor centres of their class:
  ROW_DUP        a copy of row 0 (two ground truths attain the same best overlap on the same anchors)
  ROW_OUTSIDE    a box at (-40, 30): overlap 0 with every anchor, so it must force none
  ROW_ZERO_SIZE  a box with dx = dy = dz = 0 on an anchor centre (a valid row: its sum is not 0)
  ROW_SHRUNK     a box of half the class size on an anchor centre: best overlap ~0.25, below every matched threshold, so the
                 anchors attaining it are positive only because they are forced
  G // 2         a zero row in the middle of the frame (class 0: belongs to no class)
frame 1 is ragged (its last two rows are zero), the last frame (B >= 2) has no boxes at all.
"""
import functools

import numpy as np
import torch

RANGE = [0, -8, -3, 17.6, 8, 1]
GRID = (20, 22)                   # (ny, nx) of the golden head: 440 locations
# with 3 classes (6 anchors per location):
GRID_UNDER_BLOCK = (5, 7)         # 210 anchors: less than one 256-thread block
GRID_BLOCK_MULTIPLE = (8, 16)     # 768 = 3 * 256
GRID_STRIP_TAIL = (12, 15)        # 1,080 = 256 * 4 * 1 + 56: ends inside the first strip of the loss kernel's second block
ROW_DUP, ROW_OUTSIDE, ROW_ZERO_SIZE, ROW_SHRUNK = 1, 2, 3, 4
DIR_OFFSET = 0.78539


def class_row(i):
    """anchor size, bottom height, matched and unmatched threshold of class i (0-based)"""
    size = [3.0 + 0.27 * ((i * 5) % 7), 1.4 + 0.11 * ((i * 3) % 5), 1.5 + 0.05 * (i % 4)]
    matched = 0.40 + 0.03 * (i % 4)
    return size, -1.8 + 0.1 * (i % 3), matched, matched - 0.15 + 0.02 * (i % 3)


def class_names(n_classes):
    return ['K%02d' % (i + 1) for i in range(n_classes)]


def anchor_cfgs(n_classes, anchor_classes=None):
    """one config per class, or only for the 0-based classes listed in anchor_classes (the other names have no anchors)"""
    out = []
    for i, name in enumerate(class_names(n_classes)):
        if anchor_classes is not None and i not in anchor_classes:
            continue
        size, bottom, m, u = class_row(i)
        out.append({'class_name': name, 'anchor_sizes': [size], 'anchor_rotations': [0, 1.57], 'anchor_bottom_heights': [bottom],
                    'align_center': False, 'feature_map_stride': 1, 'matched_threshold': m, 'unmatched_threshold': u})
    return out


def make_head(n_classes, num_dir_bins=2, gamma=2.0, beta=1.0 / 9.0, grid=GRID, anchor_classes=None):
    """-> AnchorHeadSingle (host, train mode), its anchor configs and class names (what oracle.anchor_head_oracle takes)"""
    from pcdet.config import EasyDict
    from pcdet.models.dense_heads import AnchorHeadSingle
    cfgs, names = anchor_cfgs(n_classes, anchor_classes), class_names(n_classes)
    cfg = EasyDict({
        'NAME': 'AnchorHeadSingle', 'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True, 'DIR_OFFSET': DIR_OFFSET,
        'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': num_dir_bins, 'ANCHOR_GENERATOR_CONFIG': cfgs,
        'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                                   'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
        'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                         'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}})
    ny, nx = grid
    head = AnchorHeadSingle(cfg, input_channels=8, num_class=n_classes, class_names=names, grid_size=np.array([nx, ny, 1]),
                            point_cloud_range=np.array(RANGE, np.float32), predict_boxes_when_training=True)
    head.cls_loss_func.gamma = gamma
    head.reg_loss_func.beta = beta
    return head.train(), cfgs, names


def oracle_anchors(n_classes, grid=GRID, anchor_classes=None):
    from oracle import anchor_head_oracle as aho
    ny, nx = grid
    cfgs = anchor_cfgs(n_classes, anchor_classes)
    return aho.generate_anchors(RANGE, cfgs, [np.array([nx, ny])] * len(cfgs))


def make_gt(head, B, G, seed, ragged=True, hole=True, empty_frame=True, duplicate=True, outside=True, zero_size=True, shrunk=True,
            class_ids=None):
    """-> (B, G, 8) float32, zero padded. Box j of frame b has class id class_ids[(j + b) % len(class_ids)] (default: every id
    1 .. n_classes in turn), sits on an anchor centre (distinct locations while the grid has enough of them) moved by up to 5 cm,
    has the class's size scaled by 0.95 .. 1.05 and a heading near 0, near pi / 2 or anywhere in +-4 rad (beyond one period)."""
    rs = np.random.RandomState(seed)
    ids = np.asarray(class_ids if class_ids is not None else range(1, head.num_class + 1))
    a0 = head.anchors[0]
    ny, nx = a0.shape[1], a0.shape[2]
    xs, ys = a0[0, 0, :, 0, 0, 0].numpy(), a0[0, :, 0, 0, 0, 1].numpy()
    gt = np.zeros((B, G, 8), np.float32)
    special = G >= 8
    for b in range(B):
        if G == 0 or (empty_frame and B >= 2 and b == B - 1):
            continue
        rows = G - 2 if (ragged and b == 1 and G > 2) else G
        loc = rs.permutation(ny * nx)[:rows] if rows <= ny * nx else rs.randint(0, ny * nx, rows)
        jit = 0.05 if rows <= ny * nx else 0.3
        cls = ids[(np.arange(rows) + b) % len(ids)] - 1
        size = np.array([class_row(c)[0] for c in cls], np.float32)
        bottom = np.array([class_row(c)[1] for c in cls], np.float32)
        f = gt[b, :rows]
        f[:, 0] = xs[loc % nx] + rs.uniform(-jit, jit, rows)
        f[:, 1] = ys[loc // nx] + rs.uniform(-jit, jit, rows)
        f[:, 3:6] = size * rs.uniform(0.95, 1.05, (rows, 3))
        f[:, 2] = bottom + f[:, 5] / 2 + rs.uniform(-0.1, 0.1, rows)
        kind = rs.randint(0, 3, rows)
        f[:, 6] = np.where(kind == 0, rs.uniform(-0.2, 0.2, rows),
                           np.where(kind == 1, np.pi / 2 + rs.uniform(-0.2, 0.2, rows), rs.uniform(-4.0, 4.0, rows)))
        f[:, 7] = cls + 1
        if b == 0 and special:
            if duplicate:
                f[ROW_DUP] = f[0]
            if outside:
                f[ROW_OUTSIDE, 0:2] = (-40.0, 30.0)
            if zero_size:
                f[ROW_ZERO_SIZE, 3:6] = 0.0
            if shrunk:
                c = int(f[ROW_SHRUNK, 7]) - 1
                f[ROW_SHRUNK, 0], f[ROW_SHRUNK, 1] = xs[loc[ROW_SHRUNK] % nx], ys[loc[ROW_SHRUNK] // nx]
                f[ROW_SHRUNK, 3:6] = np.array(class_row(c)[0], np.float32) * 0.5
                f[ROW_SHRUNK, 6] = 0.0
            if hole:
                f[G // 2] = 0.0
    gt.setflags(write=False)
    return gt


def make_preds(head, B, seed, labels=None, targets=None):
    """-> {'cls_preds', 'box_preds', 'dir_cls_preds'} (B, ny, nx, anchors per location * {classes, 7, bins}) float32 with a few
    logits that are exactly 0.0 (where the analytic derivative of the focal term and autograd's differ); with labels / targets also
    a copy of the targets with NaN ("no target") in one of the columns 0 .. 5 of every seventh positive anchor"""
    rs = np.random.RandomState(seed)
    per = head.num_anchors_per_location
    ny, nx = head.anchors[0].shape[1], head.anchors[0].shape[2]
    mk = lambda c, s: torch.from_numpy((rs.standard_normal((B, ny, nx, per * c)) * s).astype(np.float32))
    preds = {'cls_preds': mk(head.num_class, 2.0), 'box_preds': mk(7, 0.4), 'dir_cls_preds': mk(head.model_cfg.NUM_DIR_BINS, 1.5)}
    flat = preds['cls_preds'].view(-1)
    flat[torch.from_numpy(rs.randint(0, flat.numel(), 9))] = 0.0
    if labels is None:
        return preds
    targets = targets.clone()
    pos = (labels > 0).nonzero()
    pick = pos[::7]
    targets[pick[:, 0], pick[:, 1], torch.arange(pick.shape[0]) % 6] = float('nan')
    return preds, targets


# --------------------------------------------------------------------------------------------------------------------------------
# the target-assignment cases: name -> (n_classes, G, B, grid, seed)
ASSIGN_CASES = {
    'classes1': (1, 12, 3, GRID, 101), 'classes3': (3, 12, 3, GRID, 103), 'classes7': (7, 12, 3, GRID, 108),
    'classes8': (8, 12, 3, GRID, 108), 'classes10': (10, 12, 3, GRID, 110),
    'gt255': (3, 255, 3, GRID, 255), 'gt256': (3, 256, 3, GRID, 256), 'gt257': (3, 257, 3, GRID, 257), 'gt700': (3, 700, 3, GRID, 700),
    'gt1024': (2, 1024, 3, GRID, 1031), 'gt1025': (1, 1025, 3, GRID, 1027),
    'anchors210': (3, 12, 3, GRID_UNDER_BLOCK, 210), 'anchors768': (3, 12, 3, GRID_BLOCK_MULTIPLE, 768),
    'anchors1080': (3, 12, 3, GRID_STRIP_TAIL, 1080),
}
CLASS_COUNT_CASES = ('classes1', 'classes3', 'classes7', 'classes8', 'classes10')
NO_BOXES = (3, 0, 3, GRID, 0)     # G == 0: nothing for the oracle-only conditions to hold on
# the loss cases: name -> (NC, NB, gamma, beta, reduce, grid)
LOSS_CASES = {
    'nc2_nb2': (2, 2, 2.0, 1.0 / 9.0, True, GRID), 'nc5_nb3': (5, 3, 2.0, 1.0 / 9.0, True, GRID),
    'nc8_nb8': (8, 8, 2.0, 1.0 / 9.0, True, GRID), 'nc3_nb1': (3, 1, 2.0, 1.0 / 9.0, True, GRID),
    'nc3_strip_tail': (3, 2, 2.0, 1.0 / 9.0, True, GRID_STRIP_TAIL),
    'gamma1.5': (3, 2, 1.5, 1.0 / 9.0, True, GRID), 'beta0': (3, 2, 2.0, 0.0, True, GRID),
    'nc8_nb8_per_frame': (8, 8, 2.0, 1.0 / 9.0, False, GRID), 'nc9': (9, 2, 2.0, 1.0 / 9.0, True, GRID),
}
FRAME_WEIGHTS = (0.7, -1.3, 2.1)   # of the per-frame (reduce=False) losses in the objective that is differentiated


@functools.lru_cache(maxsize=None)
def assign_reference(n_classes, G, B, grid, seed):
    """-> gt (B,G,8) ndarray and the oracle's labels (B,A) i32, targets (B,A,7), weights (B,A) ndarrays, all read-only"""
    from oracle import anchor_head_oracle as aho
    head, cfgs, names = make_head(n_classes, grid=grid)
    gt = make_gt(head, B, G, seed)
    out = aho.assign_targets(oracle_anchors(n_classes, grid), torch.from_numpy(gt.copy()), names, cfgs)
    out = tuple(o.numpy() for o in out)
    for o in out:
        o.setflags(write=False)
    return (gt,) + out


HIGH_ID_NAMES = 70               # class names of the one-anchor-class heads below


@functools.lru_cache(maxsize=None)
def high_id_reference(class_id):
    """a head with HIGH_ID_NAMES class names of which only `class_id` has anchors (the kernel's presence table ends at id 63): two
    thirds of the boxes carry that id, the others id 2, which no anchor has. -> gt and the oracle's outputs like assign_reference"""
    from oracle import anchor_head_oracle as aho
    head, cfgs, names = make_head(HIGH_ID_NAMES, anchor_classes=[class_id - 1])
    gt = make_gt(head, 3, 12, 300 + class_id, class_ids=[class_id, class_id, 2])
    out = aho.assign_targets(oracle_anchors(HIGH_ID_NAMES, GRID, [class_id - 1]), torch.from_numpy(gt.copy()), names, cfgs)
    out = tuple(o.numpy() for o in out)
    for o in out:
        o.setflags(write=False)
    return (gt,) + out


def best_overlaps(n_classes, grid, gt):
    """(B, A) best nearest-BEV overlap of every anchor with the frame's ground truths of its own class (-1 where there is none),
    in the head's anchor order; computed per frame and per class as the reference does"""
    from oracle import anchor_head_oracle as aho
    anchors = oracle_anchors(n_classes, grid)
    gt = torch.from_numpy(np.array(gt))
    out = []
    for b in range(gt.shape[0]):
        cur = gt[b]
        cnt = len(cur) - 1
        while cnt > 0 and cur[cnt].sum() == 0:
            cnt -= 1
        cur = cur[:cnt + 1]
        per = []
        for c, a in enumerate(anchors):
            sel = cur[cur[:, 7].int() == c + 1]
            flat = a.reshape(-1, 7)
            best = torch.full((flat.shape[0],), -1.0)
            if len(sel):
                best = aho.nearest_bev_iou(flat, sel[:, :7]).max(1)[0]
            per.append(best.view(*a.shape[:3], -1))
        out.append(torch.cat(per, -1).view(-1))
    return torch.stack(out).numpy()


def anchor_class_ids(n_classes, grid):
    """(A,) 1-based class id of every anchor in the head's flattened (y, x, class, rot) order"""
    ny, nx = grid
    return np.tile(np.repeat(np.arange(1, n_classes + 1), 2), ny * nx)


@functools.lru_cache(maxsize=None)
def loss_reference(name):
    """inputs of a loss case and the float64 oracle on them: dict with gt, labels, targets (with NaN entries), preds (float32 host
    tensors), loss (4,) = total, cls, loc, dir or (B,) per-frame losses, grads {name: float64 tensor} of the objective (the scalar
    loss, or sum_b FRAME_WEIGHTS[b] * loss[b])"""
    from oracle import anchor_head_oracle as aho
    nc, nb, gamma, beta, reduce, grid = LOSS_CASES[name]
    B = 3
    gt, labels, targets, _ = assign_reference(nc, 12, B, grid, 500 + nc)
    head, _, _ = make_head(nc, num_dir_bins=nb, gamma=gamma, beta=beta, grid=grid)
    labels = torch.from_numpy(np.array(labels))
    preds, targets = make_preds(head, B, 900 + nc + nb, labels, torch.from_numpy(np.array(targets)))
    anchors = oracle_anchors(nc, grid)
    leaves = {k: v.double().requires_grad_(True) for k, v in preds.items()}
    kw = dict(num_class=nc, dir_offset=DIR_OFFSET, num_bins=nb, gamma=gamma, beta=beta)
    run = lambda s: aho.rpn_loss(leaves['cls_preds'][s], leaves['box_preds'][s], leaves['dir_cls_preds'][s], labels[s],
                                 targets.double()[s], anchors, **kw)
    if reduce:
        parts = run(slice(None))
        loss = torch.stack(parts)
        parts[0].backward()
    else:
        # reduce=False of the reference: frame b's loss = its cls + loc loss + the direction loss summed over ALL frames
        frames = [run(slice(b, b + 1)) for b in range(B)]
        dir_all = sum(f[3] for f in frames)
        loss = torch.stack([f[1] + f[2] + dir_all for f in frames])
        (loss * torch.tensor(FRAME_WEIGHTS, dtype=torch.float64)).sum().backward()
    return dict(gt=gt, labels=labels, targets=targets, preds=preds, loss=loss.detach(), grads={k: v.grad for k, v in leaves.items()})
