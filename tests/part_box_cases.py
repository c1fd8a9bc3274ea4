"""Cases and the f64 definitions of the point heads' box branch (csrc/point_box.hip, crbhip/point_box.py), shared by
tests/golden/make_goldens_parta2_free.py (which runs the reference on them) and the tests.

The cases are those of tests/part_cases.py (`ragged`: frames of 1,337 / 1 / 0 rows and 68 boxes = two LDS passes; `tiles`: 3 full loss
tiles + 77 rows; `no_pos`: normaliser 1, a box loss of exactly 0) plus the yaml's mean sizes, box predictions, unequal code weights and
unequal loss weights; and `one`: num_class = 1 with every ground truth's class column forced to 1 (part_cases' own `one` draws classes
1 .. 3, which the reference's coder asserts on with a single mean size).

box_preds (N,8): on positive rows the f64 label plus a difference of magnitude 0 .. 1 (0 .. 0.6 on the cos / sin pair, so that the pair
keeps a norm >= 0.15 for the decode), either sign, which spans both smooth-L1 branches around beta = 1/9; a row where any |diff * w|
lies within BETA_MARGIN of beta is redrawn (at most 1 % of the rows, asserted). Other rows: uniform codes in [-1, 1] and a cos / sin
pair of norm 0.5 .. 1.5. Class logits have no ties (asserted)."""
import functools

import numpy as np

import part_cases as cases

MEAN_SIZE = [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]              # BOX_CODER_CONFIG.mean_size of PartA2_free.yaml
CODE_WEIGHTS = [1.0, 0.9, 1.1, 0.8, 1.2, 0.7, 1.3, 0.6]                          # (the yaml has ones: unequal values show a swapped weight)
LOSS_WEIGHTS = {'point_cls_weight': 1.5, 'point_part_weight': 0.75, 'point_box_weight': 1.25}
BETA = 1.0 / 9.0
BETA_MARGIN = 1e-4
CASES = ('ragged', 'one', 'tiles', 'no_pos')
NAN_CODE = 2                                  # the code of the NaN label of `tiles` (direct loss test only)


def mean_size(num_class):
    """(K,3) f64 holding the f32 values: the coder keeps its mean sizes in f32, also in an f64 run"""
    return np.asarray(MEAN_SIZE[:1] if num_class == 1 else MEAN_SIZE, np.float32).astype(np.float64)


# ---- the definitions, f64 -----------------------------------------------------------------------------------------------------
def box_targets_f64(points, gt_boxes, num_class, mean):
    """-> labels (N) i64, owner (N) i32, box_labels (N,8) f64, part_labels (N,3) f64: PointResidualCoder.encode_torch with
    use_mean_size against the owning ground truth, the anchor size taken by the ground truth's class column; zeros without an owner"""
    labels, part, owner = cases.targets_f64(points, gt_boxes, num_class)
    mean = np.asarray(mean, np.float64)
    box = np.zeros((len(points), 8))
    frame = points[:, 0].astype(np.int64)
    for i in np.nonzero(owner >= 0)[0]:
        g = gt_boxes[frame[i], owner[i]].astype(np.float64)
        a = mean[int(g[7]) - 1]
        diag = np.sqrt(a[0] ** 2 + a[1] ** 2)
        p = points[i, 1:4].astype(np.float64)
        d = np.maximum(g[3:6], 1e-5)
        box[i] = [(g[0] - p[0]) / diag, (g[1] - p[1]) / diag, (g[2] - p[2]) / a[2], np.log(d[0] / a[0]), np.log(d[1] / a[1]),
                  np.log(d[2] / a[2]), np.cos(g[6]), np.sin(g[6])]
    return labels, owner, box, part


def box_loss_f64(cls_preds, part_preds, box_preds, labels, part_labels, box_labels, code_weights=CODE_WEIGHTS, beta=BETA,
                 weights=LOSS_WEIGHTS):
    """-> dict: loss_cls, loss_part, loss_box, pos, d_cls (N,C), d_part (N,3), d_box (N,8), all f64, for unit upstream gradients.
    part_preds None: no part branch (loss_part 0, d_part zeros). WeightedSmoothL1Loss: a NaN label is replaced by the prediction."""
    N = len(labels)
    has_part = part_preds is not None
    r = cases.losses_f64(cls_preds, part_preds if has_part else np.zeros((N, 3)), labels, part_labels if has_part else np.zeros((N, 3)),
                         weights={'point_cls_weight': weights['point_cls_weight'],
                                  'point_part_weight': weights['point_part_weight'] if has_part else 0.0})
    x, t = box_preds.astype(np.float64), box_labels.astype(np.float64)
    t = np.where(np.isnan(t), x, t)
    w = np.asarray(code_weights, np.float64)[None, :]
    diff = (x - t) * w
    n = np.abs(diff)
    if beta < 1e-5:
        src, dsrc = n, np.sign(diff)
    else:
        src = np.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
        dsrc = np.where(n < beta, diff / beta, np.sign(diff))
    row = (labels > 0).astype(np.float64)[:, None] / max(float((labels > 0).sum()), 1.0)
    r['loss_box'] = np.array((src * row).sum() * weights['point_box_weight'])
    r['d_box'] = dsrc * w * row * weights['point_box_weight']
    return r


def decode_f64(points, cls_preds, box_preds, mean):
    """generate_predicted_boxes: -> boxes (N,7) f64 decoded with the mean size of the argmax class (first maximum), classes (N)"""
    mean = np.asarray(mean, np.float64)
    cls = np.argmax(cls_preds, axis=1)
    a = mean[cls]
    e, p = box_preds.astype(np.float64), points[:, 1:4].astype(np.float64)
    diag = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)
    return np.stack([e[:, 0] * diag + p[:, 0], e[:, 1] * diag + p[:, 1], e[:, 2] * a[:, 2] + p[:, 2], np.exp(e[:, 3]) * a[:, 0],
                     np.exp(e[:, 4]) * a[:, 1], np.exp(e[:, 5]) * a[:, 2], np.arctan2(e[:, 7], e[:, 6])], 1), cls


def pack_dense(counts, rows, fill):
    """stacked rows (N,D) of frames with `counts` rows -> (B,Amax,D) padded with `fill`"""
    B, amax = len(counts), max(counts) if len(counts) else 0
    out = np.full((B, amax, rows.shape[1]), fill, rows.dtype)
    o = 0
    for b, n in enumerate(counts):
        out[b, :n] = rows[o:o + n]
        o += n
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def make_case(name):
    """part_cases.make_case(name) + mean_size (K,3) f64, box_preds (N,8) f32, box_labels_f64 (N,8), labels, owner, part_labels_f64"""
    c = cases.make_case(name)
    if name == 'one':
        c['gt_boxes'][..., 7] = np.where(c['gt_boxes'][..., 7] > 0, np.float32(1), np.float32(0))
    c['mean_size'] = mean_size(c['num_class'])
    labels, owner, box, part = box_targets_f64(c['points'], c['gt_boxes'], c['num_class'], c['mean_size'])
    rng = np.random.default_rng(cases.CASES[name][4] + 100)
    N = len(labels)
    w = np.asarray(CODE_WEIGHTS)
    span = np.array([1.0] * 6 + [0.6, 0.6])

    def draw(n):
        return rng.uniform(0.0, 1.0, (n, 8)) * span * rng.choice([-1.0, 1.0], (n, 8))
    ang, rad = rng.uniform(-np.pi, np.pi, N), rng.uniform(0.5, 1.5, N)
    preds = np.concatenate([rng.uniform(-1, 1, (N, 6)), (rad * np.cos(ang))[:, None], (rad * np.sin(ang))[:, None]], 1)
    pos = np.nonzero(labels > 0)[0]
    diff = draw(len(pos))
    redrawn = 0
    for _ in range(100):
        x32 = (box[pos] + diff).astype(np.float32).astype(np.float64)
        bad = (np.abs(np.abs((x32 - box[pos].astype(np.float32)) * w) - BETA) < BETA_MARGIN).any(1)
        if not bad.any():
            break
        redrawn += int(bad.sum())
        diff[bad] = draw(int(bad.sum()))
    else:
        raise AssertionError('beta margin not met')
    assert redrawn <= 0.01 * max(len(pos), 100), (name, redrawn, len(pos))
    preds[pos] = box[pos] + diff
    c['box_preds'] = preds.astype(np.float32)
    assert (np.hypot(c['box_preds'][:, 6], c['box_preds'][:, 7]) >= 0.1).all()
    srt = np.sort(c['cls_preds'], axis=1)
    assert c['cls_preds'].shape[1] == 1 or (np.diff(srt, axis=1) > 0).all()                    # no ties between the class logits
    c.update(labels=labels, owner=owner, box_labels_f64=box, part_labels_f64=part)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """make_case(name), built once per process and shared: read it, do not write to it"""
    return make_case(name)


def nan_row(c):
    """the positive row of a case that carries the NaN box label in the direct loss test"""
    return int(np.nonzero(c['labels'] > 0)[0][7])


# ---- stacked proposals --------------------------------------------------------------------------------------------------------
PROPOSAL_COUNTS = (420, 150, 0)                # one frame above NMS_PRE_MAXSIZE, one below, one empty
PROPOSAL_NMS = {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 300, 'NMS_POST_MAXSIZE': 64, 'NMS_THRESH': 0.8}
PROPOSAL_IOU_MARGIN = 1e-4


def proposal_case(seed):
    """per-point boxes in clusters (so that the NMS has something to remove): points (N,4) frame-sorted, cls_preds (N,3) logits
    without ties and with distinct row maxima, box_preds (N,8) codes whose decoded boxes scatter around their cluster's box.
    The maker picks the seed at which no pair of candidates of a frame has a BEV IoU within PROPOSAL_IOU_MARGIN of NMS_THRESH."""
    rng = np.random.default_rng(seed)
    mean = np.asarray(MEAN_SIZE)
    pts, cls, codes = [], [], []
    for b, n in enumerate(PROPOSAL_COUNTS):
        if n == 0:
            continue
        n_clusters = max(1, n // 12)
        centres = np.stack([rng.uniform(5, 65, n_clusters), rng.uniform(-35, 35, n_clusters), rng.uniform(-1.3, -0.7, n_clusters)], 1)
        kind = rng.integers(0, 3, n_clusters)
        heading = rng.uniform(-np.pi, np.pi, n_clusters)
        which = rng.integers(0, n_clusters, n)
        k = kind[which]
        a = mean[k]
        diag = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)
        p = centres[which] + rng.uniform(-0.5, 0.5, (n, 3)) * a
        target = centres[which] + rng.normal(0, 0.06, (n, 3)) * a                   # where the decoded box lands
        p32 = p.astype(np.float32).astype(np.float64)
        rz = heading[which] + rng.normal(0, 0.05, n)
        rad = rng.uniform(0.7, 1.3, n)
        codes.append(np.concatenate([(target[:, 0:2] - p32[:, 0:2]) / diag[:, None], ((target[:, 2] - p32[:, 2]) / a[:, 2])[:, None],
                                     rng.normal(0, 0.05, (n, 3)), (rad * np.cos(rz))[:, None], (rad * np.sin(rz))[:, None]], 1))
        logits = rng.uniform(-6, 2, (n, 3))
        logits[np.arange(n), k] = rng.uniform(2.5, 8, n)                            # the cluster's class wins
        pts.append(np.concatenate([np.full((n, 1), b), p], 1))
        cls.append(logits)
    points, cls_preds = np.concatenate(pts).astype(np.float32), np.concatenate(cls).astype(np.float32)
    top = np.sort(cls_preds.max(1))
    assert (np.diff(top) > 0).all()
    return {'points': points, 'cls_preds': cls_preds, 'box_preds': np.concatenate(codes).astype(np.float32),
            'counts': list(PROPOSAL_COUNTS), 'batch_size': len(PROPOSAL_COUNTS)}


# ---- the detector on the reduced U-Net grid -----------------------------------------------------------------------------------
# PartA2_free.yaml's PointRCNN on part_cases.unet_inputs() (B = 2, about 600 voxels, 32 x 32 x 24 cells of 0.2 m), reduced where the
# yaml's sizes only cost time: a 6^3 RoI grid (12^3 gives a 57 M-parameter first FC layer), 16 sampled RoIs per frame, 64 / 32
# proposals. DP_RATIO 0 leaves nothing random but the RoI sampler, whose draws the golden records.
NET_SEED = 53
NET_GT = 6                                      # rows of gt_boxes per frame
NET_GRADS = {'backbone_3d.conv_input.0.weight': np.s_[:], 'backbone_3d.conv_up_t1.conv1.weight': np.s_[:],
             'point_head.cls_layers.0.weight': np.s_[:8], 'point_head.part_reg_layers.0.weight': np.s_[:8],
             'point_head.box_layers.0.weight': np.s_[:8], 'point_head.box_layers.6.weight': np.s_[:],
             'roi_head.conv_rpn.0.0.weight': np.s_[:], 'roi_head.shared_fc_layer.0.weight': np.s_[:16, :384]}
NET_SMALL = ('point_head.box_layers.6.weight', 'point_head.box_layers.6.bias')    # scaled by 0.1: proposals of sane sizes near their points


def net_overrides(model_cfg):
    """the reductions above, on the MODEL section of the yaml / of parta2_free_cfg()"""
    r = model_cfg.ROI_HEAD
    r.DP_RATIO = 0.0
    r.ROI_AWARE_POOL.POOL_SIZE = 6
    r.TARGET_CONFIG.ROI_PER_IMAGE = 16
    r.NMS_CONFIG.TRAIN.NMS_POST_MAXSIZE = 64
    r.NMS_CONFIG.TEST.NMS_POST_MAXSIZE = 32
    return model_cfg


def net_batch():
    """-> voxels (N,1,4) f32, voxel_num_points (N) f32, voxel_coords (N,4) f32 [b,z,y,x], batch_size: one point per voxel, so that
    MeanVFE hands UNetV2 the rows of part_cases.unet_inputs(); points (N,5) [b,x,y,z,0]: the voxel centres (what the eval pass
    counts inside its predictions)"""
    feats, coords, B = cases.unet_inputs()
    centres = (coords[:, [3, 2, 1]] + 0.5) * np.asarray(cases.UNET_VOXEL) + np.asarray(cases.UNET_PCR[:3])
    points = np.concatenate([coords[:, 0:1], centres, np.zeros((len(coords), 1))], 1).astype(np.float32)
    return {'voxels': feats[:, None, :].copy(), 'voxel_num_points': np.ones(len(feats), np.float32),
            'voxel_coords': coords.astype(np.float32), 'points': points, 'batch_size': B}
