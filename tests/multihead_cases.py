"""Heads, ground truths, predictions and selection inputs for AnchorHeadMulti, its loss kernel (csrc/multihead_loss.hip) and the per-class
selection of a batch (csrc/multiclass_nms.hip). numpy / torch on the host only, fixed seeds, no test functions. The golden file
tests/golden/ref_multihead.npz is written from these inputs by tests/golden/make_goldens_multihead.py.

Everything lives on the small range of tests/anchor_head_cases.py with its three classes K01 .. K03 (one size, two rotations each).
The main map is 21 x 13 (273 cells): 546 anchors per class, 1,638 per frame; the head boundaries 546 and 1,092 fall inside a wave and
inside a 256-thread block. The tiny map is 3 x 2.

Ground truths are ahc.make_gt's (frame 0 with its duplicate / outside / zero-size / shrunk / hole rows, frame 1 ragged, frame 2 empty);
'mixed' additionally carries a class id in the two trailing zero rows of frame 1 (garbage after the last non-zero row: the rows do not
exist for the assigner), 'noclass2' has no box of class 2.

Selection cases are margin-safe by construction; check_selection_margins asserts it."""
import os
import types

import numpy as np
import torch

import anchor_head_cases as ahc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_multihead.npz')
B = 3
GRID = (21, 13)
TINY = (3, 2)
CHANNELS = 8
NAMES = ahc.class_names(3)
LAYOUTS = {'three': ((0,), (1,), (2,)), 'two': ((0,), (1, 2)), 'one': ((0, 1, 2),)}
SEP_REG = {'NUM_MIDDLE_CONV': 1, 'NUM_MIDDLE_FILTER': 8, 'REG_LIST': ['reg:2', 'height:1', 'size:3', 'angle:1']}
LOSS_WEIGHTS = {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}


def head_cfg(layout, separate=True, use_dir=True, sep_reg=False, shared=16, head_layers=False, loss_weights=None):
    """plain dict of an AnchorHeadMulti config (the caller wraps it in its EasyDict). head_layers: every head gets a one-block
    BaseBEVBackbone of its own instead of the identity"""
    heads = []
    for group in LAYOUTS[layout]:
        h = {'HEAD_CLS_NAME': [NAMES[i] for i in group]}
        if head_layers:
            # (the reference wires a head's convolutions to the SHARED map's channels: the head's block keeps that count)
            h.update({'LAYER_NUMS': [1], 'LAYER_STRIDES': [1], 'NUM_FILTERS': [shared or CHANNELS], 'UPSAMPLE_STRIDES': [1],
                      'NUM_UPSAMPLE_FILTERS': [shared or CHANNELS]})
        heads.append(h)
    cfg = {'NAME': 'AnchorHeadMulti', 'CLASS_AGNOSTIC': False, 'DIR_OFFSET': ahc.DIR_OFFSET, 'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
           'USE_MULTIHEAD': True, 'SEPARATE_MULTIHEAD': separate, 'ANCHOR_GENERATOR_CONFIG': ahc.anchor_cfgs(3), 'RPN_HEAD_CFGS': heads,
           'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                                      'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
           'LOSS_CONFIG': {'LOSS_WEIGHTS': dict(loss_weights or LOSS_WEIGHTS)}}
    if use_dir:
        cfg['USE_DIRECTION_CLASSIFIER'] = True
    if shared:
        cfg['SHARED_CONV_NUM_FILTER'] = shared
    if sep_reg:
        cfg['SEPARATE_REG_CONFIG'] = dict(SEP_REG)
    return cfg


def head_kwargs(grid, predict_boxes_when_training=False):
    ny, nx = grid
    return dict(input_channels=CHANNELS, num_class=3, class_names=list(NAMES), grid_size=np.array([nx, ny, 1]),
                point_cloud_range=np.array(ahc.RANGE, np.float32), predict_boxes_when_training=predict_boxes_when_training)


def make_head(layout, grid=GRID, **kw):
    """this repository's AnchorHeadMulti on the host, train mode"""
    from pcdet.config import EasyDict
    from pcdet.models.dense_heads import AnchorHeadMulti
    torch.manual_seed(0)
    return AnchorHeadMulti(EasyDict(head_cfg(layout, **kw)), **head_kwargs(grid)).train()


def head_sizes(layout, separate, grid):
    """[(A_h, C_h, first class column)] of every head"""
    per_class = grid[0] * grid[1] * 2
    out, c = [], 0
    for group in LAYOUTS[layout]:
        out.append((per_class * len(group), len(group) if separate else 3, c if separate else 0))
        c += len(group)
    return out


def _grid_stub(grid):
    """what ahc.make_gt reads of a head: num_class and the anchor centres of the map (align_center off: end points on the range)"""
    ny, nx = grid
    a = torch.zeros((1, ny, nx, 1, 2, 7))
    a[0, :, :, 0, 0, 0] = torch.linspace(ahc.RANGE[0], ahc.RANGE[3], nx)[None, :]
    a[0, :, :, 0, 0, 1] = torch.linspace(ahc.RANGE[1], ahc.RANGE[4], ny)[:, None]
    return types.SimpleNamespace(num_class=3, anchors=[a])


GT_CASES = {'mixed': (GRID, 11, None), 'noclass2': (GRID, 12, (1, 3)), 'tiny': (TINY, 13, None)}


def make_gt(name):
    grid, seed, ids = GT_CASES[name]
    special = grid != TINY
    gt = np.array(ahc.make_gt(_grid_stub(grid), B, 12 if special else 4, seed, class_ids=ids, duplicate=special, outside=special,
                              zero_size=special, shrunk=special, hole=special))
    if name == 'mixed':
        assert (gt[1, -2:, :7] == 0).all()
        gt[1, -2:, 7] = 2.0                      # garbage behind the last non-zero row
    gt.setflags(write=False)
    return gt


# ------------------------------------------------------------------------------------------------------------------------ losses
# name -> (layout, SEPARATE_MULTIHEAD, direction classifier, grid); every layout with both switches, one tiny map
LOSS_CASES = {'%s_%s_%s' % (lay, 'sep' if sep else 'all', 'dir' if d else 'nodir'): (lay, sep, d, GRID)
              for lay in LAYOUTS for sep in (True, False) for d in (True, False)}
LOSS_CASES['tiny_three_sep_dir'] = ('three', True, True, TINY)
OUTSIDE_ANCHOR = 20          # frame 0: an anchor of class 1's head relabelled as a positive of class 3
GRAD_ROWS = 7                # every GRAD_ROWS-th anchor row of the f64 gradients is stored in the golden


def plant_targets(labels, targets, grid):
    """labels (B,A) / targets (B,A,7) of the 'mixed' (or 'tiny') assignment -> copies with, on the main map: ignored anchors across
    both head boundaries, a positive whose class lies outside its head's columns, and a NaN ("no target") in one of the columns 0 .. 5
    of every seventh positive. The last frame keeps zero positives."""
    labels, targets = np.array(labels, np.int32), np.array(targets, np.float32)
    per_class = grid[0] * grid[1] * 2
    if grid == GRID:
        labels[:, per_class - 2:per_class + 3] = -1
        labels[:, 2 * per_class - 1:2 * per_class + 2] = -1
        labels[0, OUTSIDE_ANCHOR] = 3
        targets[0, OUTSIDE_ANCHOR] = [0.3, -0.2, 0.1, 0.05, -0.1, 0.2, 0.7]
    pos = np.argwhere(labels > 0)[::7]
    targets[pos[:, 0], pos[:, 1], np.arange(len(pos)) % 6] = np.nan
    assert (labels[-1] > 0).sum() == 0 and (labels[0] > 0).sum() > 0
    return labels, targets


def make_preds(case):
    """-> (cls, box, dir) lists over the heads of float32 arrays (B,A_h,C_h), (B,A_h,7), (B,A_h,2) (dir None without the classifier);
    nine class logits are exactly 0 (where autograd's derivative of the focal term and the analytic one differ)"""
    layout, separate, use_dir, grid = LOSS_CASES[case]
    rs = np.random.RandomState(abs(hash_name(case)) % (2 ** 31))
    cls, box, dirs = [], [], []
    for n, c, _ in head_sizes(layout, separate, grid):
        x = (rs.standard_normal((B, n, c)) * 2.0).astype(np.float32)
        x.reshape(-1)[rs.randint(0, x.size, 9)] = 0.0
        cls.append(x)
        box.append((rs.standard_normal((B, n, 7)) * 0.4).astype(np.float32))
        dirs.append((rs.standard_normal((B, n, 2)) * 1.5).astype(np.float32))
    return cls, box, (dirs if use_dir else None)


def hash_name(s):
    h = 7
    for ch in s:
        h = (h * 131 + ord(ch)) % 1000003
    return h


# --------------------------------------------------------------------------------------------------------------------- selection
# name -> layout, grid, SCORE_THRESH, NMS_TYPE, NMS_THRESH, PRE, POST, hot[frame][segment] = anchors planted above the threshold
# (None: every anchor of the frame stays below it), seed. Segments in (head, class) order.
SEL_CASES = {
    # no candidate / one / more than PRE (64: the cut falls on a wave edge); a frame with none at all
    'base': dict(layout='three', grid=GRID, thresh=0.1, nms='nms_gpu', iou=0.1, pre=64, post=10, hot=[[0, 1, 80], [30, 70, 5], None], seed=1),
    # a two-class head (4 anchors per location), PRE 100, more than PRE candidates
    'two_pre100': dict(layout='two', grid=GRID, thresh=0.1, nms='nms_gpu', iou=0.3, pre=100, post=500, hot=[[130, 101, 7], [64, 100, 99], [1, 0, 128]], seed=32),
    # every anchor passes (546 or 1,092 candidates for 64 places: the radix select)
    # (its cold logits are positive too: the best 64 of a segment are reported whatever they are)
    'all_pass': dict(layout='two', grid=GRID, thresh=-0.5, nms='nms_gpu', iou=0.1, pre=64, post=500, hot=[[9, 9, 9], [0, 0, 0], [3, 70, 2]], seed=13,
                     cold=(0.7, 2.4), hot_from=2.6),
    'normal': dict(layout='three', grid=GRID, thresh=0.1, nms='nms_normal_gpu', iou=0.2, pre=64, post=500, hot=[[40, 64, 65], [63, 2, 0], [0, 0, 90]], seed=4),
    # NMS_POST_MAXSIZE cuts the segments
    'post_cut': dict(layout='one', grid=GRID, thresh=0.1, nms='nms_gpu', iou=0.7, pre=100, post=3, hot=[[50, 120, 2], [3, 4, 100], [0, 0, 0]], seed=5),
    # fewer anchors than PRE
    'tiny': dict(layout='three', grid=TINY, thresh=0.1, nms='nms_gpu', iou=0.1, pre=64, post=500, hot=[[12, 0, 5], [1, 11, 0], None], seed=6),
    # SCORE_THRESH 0.5 with the planted logits 0.0 (f32 sigmoid exactly 0.5: a candidate) and -2^-20 (0.49999976: none)
    'half': dict(layout='three', grid=GRID, thresh=0.5, nms='nms_gpu', iou=0.1, pre=64, post=500, hot=[[20, 3, 0], [0, 66, 1], [5, 5, 5]], seed=7,
                 planted=True),
    # two equal logits in one segment, both candidates, boxes far apart: the smaller anchor index comes first
    'tie': dict(layout='three', grid=GRID, thresh=0.1, nms='nms_gpu', iou=0.1, pre=64, post=500, hot=[[10, 0, 0], [0, 0, 0], [0, 0, 0]], seed=8, tie=True),
}
PLANT_AT, PLANT_BELOW = 100, 200        # anchors of segment 0, frame 0 of 'half'
TIE_A, TIE_B = 31, 400                  # anchors of segment 0, frame 0 of 'tie'
MARGIN = 1e-4


EXP_STEPS = 2        # f32 steps by which an exp implementation may miss the correctly rounded value (libm bounds are 1)


def sigmoid_f32(x, shift=0):
    """torch.sigmoid of f32 logits as its three f32 operations, 1 / (1 + exp(-x)): the add and the divide are exactly rounded ones on
    every machine, exp is not. shift: the exp result moved by that many f32 steps off the correctly rounded value"""
    e = np.exp(-x.astype(np.float64)).astype(np.float32)
    for _ in range(abs(shift)):
        e = np.nextafter(e, np.float32(np.inf if shift > 0 else -np.inf))
    return np.float32(1.0) / (np.float32(1.0) + e)


def sigmoid_stable(x):
    """True where the f32 sigmoid of x is the same number for every exp result within EXP_STEPS f32 steps of the correctly rounded
    one: there the add or the divide rounds the difference away, and the score is the same bits on the host that writes the golden
    and on the device, whichever exp each of them has"""
    ref = sigmoid_f32(x)
    ok = np.ones(x.shape, bool)
    for s in range(-EXP_STEPS, EXP_STEPS + 1):
        ok &= sigmoid_f32(x, s) == ref
    return ok


def stabilise(x, keep=None):
    """every logit (but those under the mask `keep`) moved up by as few f32 steps as it takes to make its sigmoid stable"""
    x = x.copy()
    free = (x > 0) if keep is None else (x > 0) & ~keep        # (no logit below 0 has a stable sigmoid: the cases report none)
    for _ in range(4000):
        bad = ~sigmoid_stable(x) & free
        if not bad.any():
            break
        x[bad] = np.nextafter(x[bad], np.float32(np.inf))
    assert (sigmoid_stable(x) | ~free).all()
    return x


def make_selection(name):
    """-> dict(cls [ (B,A_h,C_h) ], box [ (B,A_h,7) ], dir [ (B,A_h,2) ]) float32 arrays per head. Cold logits are distinct values of
    [-9, -3.5] (scores below 0.03), hot ones distinct values of [0.7, 6] (scores above 0.66; below 0.6 no logit is stable against two steps). Every logit above 0 - every one whose score
    a case reports - is moved by a few f32 steps to a value whose f32 sigmoid does not depend on the exp implementation (sigmoid_stable)."""
    c = SEL_CASES[name]
    rs = np.random.RandomState(100 + c['seed'])
    sizes = head_sizes(c['layout'], True, c['grid'])
    lo = c.get('hot_from', 0.7)
    cold = c.get('cold', (-9.0, -3.5))
    cls, box, dirs, seg = [], [], [], 0
    for n, C, _ in sizes:
        x = np.empty((B, n, C), np.float32)
        for b in range(B):
            for k in range(C):
                col = np.linspace(cold[0], cold[1], n)[rs.permutation(n)]
                hot = c['hot'][b]
                m = 0 if hot is None else min(hot[seg + k], n)
                if m:
                    col[rs.permutation(n)[:m]] = np.linspace(lo, 6.0, m + 2)[1:-1][rs.permutation(m)]
                x[b, :, k] = col
        if seg == 0 and c.get('planted'):
            x[0, PLANT_AT, 0], x[0, PLANT_BELOW, 0] = 0.0, -2.0 ** -20
        if seg == 0 and c.get('tie'):
            x[0, TIE_A, 0] = x[0, TIE_B, 0] = 2.5
        keep = np.zeros(x.shape, bool)
        if seg == 0 and c.get('planted'):
            # (exp(-0.0) is 1 in every libm; the logit below the threshold is no candidate, its score is never reported)
            keep[0, [PLANT_AT, PLANT_BELOW], 0] = True
        moved = stabilise(x, keep)
        assert np.abs(moved.astype(np.float64) - x).max() <= 1e-3
        x = moved
        cls.append(x)
        bx = (rs.standard_normal((B, n, 7)) * 0.3).astype(np.float32)
        # size residuals 0: exp(0) is the decode's only operation that is not an exactly rounded one (every other is a single add, multiply,
        # divide, floor or square root of torch), so the decoded boxes are the same bits on the host that wrote the golden and on the device
        bx[..., 3:6] = 0.0
        box.append(bx)
        dirs.append((rs.standard_normal((B, n, 2)) * 1.5).astype(np.float32))
        seg += C
    return dict(cls=cls, box=box, dir=dirs)


def nms_cfg(name):
    c = SEL_CASES[name]
    return {'MULTI_CLASSES_NMS': True, 'NMS_TYPE': c['nms'], 'NMS_THRESH': c['iou'], 'NMS_PRE_MAXSIZE': c['pre'], 'NMS_POST_MAXSIZE': c['post']}


def candidates_definition(col, thresh, pre):
    """the definition of crb_multiclass_candidates for one segment in float64: anchors whose score is >= thresh, best first, equal
    scores by ascending index, at most min(pre, len) of them -> indices. (The margins make the f32 order the f64 order.)"""
    p = 1.0 / (1.0 + np.exp(-col.astype(np.float64)))
    idx = np.nonzero(p >= thresh)[0]
    order = np.lexsort((idx, -p[idx]))
    return idx[order][:min(pre, len(col))]


def _aligned_iou(b):
    """pairwise axis-aligned BEV IoU of (n,7) boxes as nms_normal_gpu sees them"""
    x1, x2 = b[:, 0] - b[:, 3] / 2, b[:, 0] + b[:, 3] / 2
    y1, y2 = b[:, 1] - b[:, 4] / 2, b[:, 1] + b[:, 4] / 2
    w = np.clip(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), 0, None)
    h = np.clip(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), 0, None)
    area = (x2 - x1) * (y2 - y1)
    return w * h / np.maximum(area[:, None] + area[None] - w * h, 1e-8)


def check_selection_margins(name, boxes):
    """asserts the margins of a selection case; boxes [(B,A_h,7)] decoded boxes per head (host arrays). -> the candidates of every
    (frame, head, class) by the definition"""
    import oracle
    c, d = SEL_CASES[name], make_selection(name)
    assert all((bx[..., 3:6] == 0).all() for bx in d['box'])           # the decode has no exp to round
    out = {}
    for h, x in enumerate(d['cls']):
        assert np.abs(x).max() <= 12.0
        for b in range(B):
            for k in range(x.shape[2]):
                col = x[b, :, k]
                p = 1.0 / (1.0 + np.exp(-col.astype(np.float64)))
                near = np.abs(p - c['thresh']) < MARGIN
                if c.get('planted') and h == 0 and b == 0 and k == 0:
                    assert set(np.nonzero(near)[0]) == {PLANT_AT, PLANT_BELOW}
                    s = torch.sigmoid(torch.from_numpy(col[[PLANT_AT, PLANT_BELOW]])).numpy()
                    assert s[0] == np.float32(0.5) and s[1] < np.float32(0.5)
                else:
                    assert not near.any(), (name, h, b, k)
                u, counts = np.unique(col, return_counts=True)
                if c.get('tie') and h == 0 and b == 0 and k == 0:
                    assert (counts > 1).sum() == 1 and col[TIE_A] == col[TIE_B] == u[counts > 1][0]
                else:
                    assert (counts == 1).all(), (name, h, b, k)
                    # (the planted pair of 'half' is 4 f32 steps apart on purpose; the lower one is no candidate)
                    ps = np.sort(np.delete(p, PLANT_BELOW) if c.get('planted') and h == 0 and b == 0 and k == 0 else p)
                    assert ((ps[1:] - ps[:-1]) / ps[1:]).min() > 1e-5      # no two scores that f32 rounding could swap
                idx = candidates_definition(col, c['thresh'], c['pre'])
                out[(b, h, k)] = idx
                # every reported score is the same f32 number under any exp within EXP_STEPS steps, and torch's on this host is that number
                # (the planted logit 0.0: exp(-0.0) is exactly 1 in every libm, its score 0.5 needs no margin)
                assert sigmoid_stable(col[idx][col[idx] != 0]).all(), (name, h, b, k)
                assert np.array_equal(torch.sigmoid(torch.from_numpy(col[idx].copy())).numpy(), sigmoid_f32(col[idx])), (name, h, b, k)
                bx = boxes[h][b][idx]
                if len(idx) > 1:
                    iou = _aligned_iou(bx) if c['nms'] == 'nms_normal_gpu' else oracle.boxes_pairwise(bx, bx, 1)
                    off = iou[~np.eye(len(idx), dtype=bool)]
                    assert (np.abs(off - c['iou']) >= MARGIN).all(), (name, h, b, k)
                if c.get('tie') and h == 0 and b == 0 and k == 0:
                    pos = {int(a): i for i, a in enumerate(idx)}
                    assert pos[TIE_A] + 1 == pos[TIE_B] and iou[pos[TIE_A], pos[TIE_B]] == 0
    return out


# ------------------------------------------------------------------------------------------- csrc/rpn_loss.hip, single head
def rpn_single_outputs(L=None):
    """the outputs of crb_rpn_loss_forward / _backward (device) on the single-head loss cases of tests/anchor_head_cases.py that the
    kernel takes -> {case_loss (B,3), case_npos (B), case_sha_cls / _box / _dir: SHA-256 of the gradients' bytes}. L: a ctypes handle of
    another build of the library (the parent commit's, when the golden is written); None: this build."""
    import ctypes
    import hashlib
    import crbhip
    from crbhip import rpn_loss as rl
    if L is None:
        L = crbhip.lib
    else:
        protos = crbhip.parse_header()
        for fn in ('crb_rpn_loss_workspace_bytes', 'crb_rpn_loss_forward', 'crb_rpn_loss_backward'):
            getattr(L, fn).restype, getattr(L, fn).argtypes = protos[fn]
    dev = torch.device('cuda', 0)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    out = {}
    for name, (nc, nb, gamma, beta, _, grid) in ahc.LOSS_CASES.items():
        if nc > 8:
            continue
        ref = ahc.loss_reference(name)
        n = int(ref['labels'].shape[0])
        anchors = torch.cat(ahc.oracle_anchors(nc, grid), dim=-3).reshape(-1, 7).float().contiguous().to(dev)
        A = int(anchors.shape[0])
        cls, box, dirs = (ref['preds'][k].reshape(n, A, -1).contiguous().to(dev) for k in ('cls_preds', 'box_preds', 'dir_cls_preds'))
        labels, tgt = ref['labels'].int().contiguous().to(dev), ref['targets'].float().contiguous().to(dev)
        cfg = rl.make_cfg(nc, nb, [1.0] * 7, 1.0, 2.0, 0.2, ahc.DIR_OFFSET, gamma=gamma, beta=beta)
        loss, npos = torch.empty((n, 3), device=dev), torch.empty((n,), device=dev)
        wsb = L.crb_rpn_loss_workspace_bytes(n, A)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.crb_rpn_loss_forward(p(cls), p(box), p(dirs), p(labels), p(tgt), p(anchors), n, A, ctypes.byref(cfg), p(loss), p(npos), p(ws),
                                    wsb, st)
        assert rc == 0, (name, rc)
        g = torch.tensor(ahc.FRAME_WEIGHTS, device=dev)[:, None] * torch.tensor([1.0, 0.5, -2.0], device=dev)[None, :]
        g = g.contiguous()
        d = [torch.empty_like(t) for t in (cls, box, dirs)]
        rc = L.crb_rpn_loss_backward(p(cls), p(box), p(dirs), p(labels), p(tgt), p(anchors), n, A, ctypes.byref(cfg), p(npos), p(g),
                                     p(d[0]), p(d[1]), p(d[2]), st)
        assert rc == 0, (name, rc)
        torch.cuda.synchronize()
        out[name + '_loss'], out[name + '_npos'] = loss.cpu().numpy(), npos.cpu().numpy()
        for key, t in zip(('cls', 'box', 'dir'), d):
            out['%s_sha_%s' % (name, key)] = np.frombuffer(hashlib.sha256(t.cpu().numpy().tobytes()).digest(), np.uint8).copy()
    return out


# ----------------------------------------------------------------------------------------------------------------- head forward
FORWARD_CASES = {'two_sep': dict(layout='two'), 'three_all_sep_reg': dict(layout='three', separate=False, sep_reg=True),
                 'one_layers_nodir': dict(layout='one', head_layers=True, use_dir=False)}
FORWARD_SEED, FORWARD_ROWS = 77, 5


def forward_input():
    return np.random.RandomState(FORWARD_SEED).standard_normal((B, CHANNELS, GRID[0], GRID[1])).astype(np.float32)


# ------------------------------------------------------------------------------------- candidates alone: the cut and the full sort
# crb_multiclass_candidates against candidates_definition, without NMS and without the loop route (torch.topk leaves the order of equal
# scores open, so a cut inside a run of equal scores has no loop-route answer). name -> anchors, classes, PRE and per (frame, class) the
# triple (distinct hot logits, anchors sharing ONE logit below all of them, that logit or None); every other anchor is cold.
CUT_THRESH = 0.1
CUT_CASES = {
    # the cut falls inside the run (34 of 100 taken), just behind its first anchor (1 of 40), exactly in front of it (64 distinct), and
    # the whole run fits (10 + 50 < 64: no select)
    'tie_cut': dict(A=546, C=2, pre=64, seg=[[(30, 100, 2.0), (63, 40, 1.5)], [(64, 50, 2.0), (10, 50, 1.0)]]),
    # PRE = 4,096, the whole LDS sort: 5,000 pass; exactly 4,096 pass (no select); 4,097 pass; all 6,000 pass with a run of 300 across the cut
    'full_pre': dict(A=6000, C=2, pre=4096, seg=[[(5000, 0, None), (4096, 0, None)], [(4097, 0, None), (3900, 300, 0.65)]],
                     all_hot=(1, 1)),
}


def make_cut_case(name):
    """-> (2, A, C) float32 logits"""
    c = CUT_CASES[name]
    rs = np.random.RandomState(hash_name(name) % (2 ** 31))
    x = np.empty((2, c['A'], c['C']), np.float32)
    for b in range(2):
        for k in range(c['C']):
            hot, run, val = c['seg'][b][k]
            col = np.linspace(-9.0, -3.5, c['A'])[rs.permutation(c['A'])]
            if c.get('all_hot') == (b, k):                       # no cold anchor: the rest passes too, below the run
                col = np.linspace(-2.0, 0.5, c['A'])[rs.permutation(c['A'])]
            where = rs.permutation(c['A'])
            col[where[:hot]] = np.linspace(0.7 if val is None else val + 0.5, 6.0, hot)[rs.permutation(hot)]
            if run:
                col[where[hot:hot + run]] = val
            x[b, :, k] = col
    # distinct scores are far enough apart that f32 rounding cannot swap them
    for b in range(2):
        for k in range(c['C']):
            p = np.unique(1.0 / (1.0 + np.exp(-np.unique(x[b, :, k]).astype(np.float64))))
            assert ((p[1:] - p[:-1]) / p[1:]).min() > 1e-6 and np.abs(p - CUT_THRESH).min() > MARGIN
    return x
