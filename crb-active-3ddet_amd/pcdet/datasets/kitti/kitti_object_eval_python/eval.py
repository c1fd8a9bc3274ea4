"""KITTI object AP (image box / BEV / 3D / AOS) with the reference's definitions and its public surface
(pcdet/datasets/kitti/kitti_object_eval_python/eval.py): get_official_eval_result, do_eval, eval_class, calculate_iou_partly.

Two routes compute the same quantities from the same packed arrays:
  route='device'  crbhip.kitti_eval: the HIP kernels of csrc/kitti_eval.hip (overlaps of all frames in one launch, one wave per
                  (frame, combination) for the greedy matchings with lane = score threshold), one read-back at the end.
  route='host'    plain numpy, written here: f64 convex clipping for the rotated overlaps, the greedy matching vectorised over the
                  detections and the thresholds of a (frame, combination). Used without a GPU, by the CPU tests and as the second
                  opinion on random inputs.
route=None reads CRB_KITTI_EVAL_ROUTE, and without it takes the device when one is present.

A combination is (metric, class, difficulty, overlap row) = (m, c, l, k); the ignore flags depend on (c, l) only, the minimum
overlap is min_overlaps[k, m, c]. Scores are carried in f64, in which f32 detector scores and scores read from label files are
both exact. Not provided: get_coco_eval_result."""
import io as sysio
import os

import numpy as np

CLASS_NAMES = ['car', 'pedestrian', 'cyclist', 'van', 'person_sitting', 'truck']
MIN_HEIGHT = [40, 25, 25]
MAX_OCCLUSION = [0, 1, 2]
MAX_TRUNCATION = [0.15, 0.3, 0.5]
N_SAMPLE_PTS = 41
OTHER_CLASS = 7
NO_DETECTION = -10000000


def default_route(route=None):
    route = route or os.environ.get('CRB_KITTI_EVAL_ROUTE')
    if route is None:
        import torch
        route = 'device' if torch.cuda.is_available() else 'host'
    assert route in ('device', 'host'), route
    return route


# ------------------------------------------------------------------------------------------------------------------ packing
def _cat(annos, key, width, dtype=np.float64):
    parts = [np.asarray(a[key], dtype=dtype).reshape(-1, width) for a in annos if len(a['name'])]
    return np.concatenate(parts, 0) if parts else np.zeros((0, width), dtype)


def _class_ids(annos):
    parts = [np.asarray(a['name']).astype(str) for a in annos if len(a['name'])]
    names = np.concatenate(parts) if parts else np.zeros(0, dtype=str)
    lower = np.char.lower(names) if len(names) else names
    ids = np.full(len(names), OTHER_CLASS, dtype=np.int32)
    for k, n in enumerate(CLASS_NAMES):
        ids[lower == n] = k
    return ids, (names == 'DontCare').astype(np.uint8)


def pack_annos(gt_annos, dt_annos):
    """lists of anno dicts -> flat arrays with per-frame prefix sums (vectorised; no loop over boxes)"""
    assert len(gt_annos) == len(dt_annos)
    p = {'num_frames': len(gt_annos)}
    for side, annos in (('gt', gt_annos), ('dt', dt_annos)):
        n = np.array([len(a['name']) for a in annos], dtype=np.int64)
        p[side + '_off'] = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        p[side + '_bbox'] = _cat(annos, 'bbox', 4)
        p[side + '_alpha'] = _cat(annos, 'alpha', 1)[:, 0]
        p[side + '_cam'] = np.concatenate([_cat(annos, 'location', 3), _cat(annos, 'dimensions', 3), _cat(annos, 'rotation_y', 1)], 1)
        p[side + '_cls'], dc = _class_ids(annos)
        if side == 'gt':
            p['gt_dc'] = dc
            p['gt_occ'] = _cat(annos, 'occluded', 1)[:, 0]
            p['gt_trunc'] = _cat(annos, 'truncated', 1)[:, 0]
        else:
            p['dt_score'] = _cat(annos, 'score', 1)[:, 0]
    p['pair_off'] = np.concatenate([[0], np.cumsum(np.diff(p['gt_off']) * np.diff(p['dt_off']))]).astype(np.int64)
    return p


def ignore_flags(p, current_class, difficulty):
    """clean_data for every box at once -> (ignored_gt (G) i8, ignored_dt (D) i8)"""
    c, d = current_class, difficulty
    cls = p['gt_cls']
    valid = np.where(cls == c, 1, np.where(((c == 1) & (cls == 4)) | ((c == 0) & (cls == 3)), 0, -1))
    height = p['gt_bbox'][:, 3] - p['gt_bbox'][:, 1]
    ignore = (p['gt_occ'] > MAX_OCCLUSION[d]) | (p['gt_trunc'] > MAX_TRUNCATION[d]) | (height <= MIN_HEIGHT[d])
    gf = np.where((valid == 1) & ~ignore, 0, np.where((valid == 0) | (ignore & (valid == 1)), 1, -1)).astype(np.int8)
    dheight = np.abs(p['dt_bbox'][:, 3] - p['dt_bbox'][:, 1])
    df = np.where(dheight < MIN_HEIGHT[d], 1, np.where(p['dt_cls'] == c, 0, -1)).astype(np.int8)
    return gf, df


# ------------------------------------------------------------------------------------------------------- host route: overlaps
def _corners(b):
    """(P, 5) [x, y, dx, dy, angle], a positive angle turns clockwise (rotate_iou.py::rbbox_to_corners) -> (P, 4, 2)"""
    c, s = np.cos(b[:, 4:5]), np.sin(b[:, 4:5])
    cx = b[:, 2:3] / 2 * np.array([[-1., -1., 1., 1.]])
    cy = b[:, 3:4] / 2 * np.array([[-1., 1., 1., -1.]])
    return np.stack([c * cx + s * cy + b[:, 0:1], -s * cx + c * cy + b[:, 1:2]], -1)


def _signed_area(poly, cnt):
    idx = np.arange(poly.shape[1])[None, :]
    nxt = np.take_along_axis(poly, np.where(idx + 1 < cnt[:, None], idx + 1, 0)[:, :, None].repeat(2, 2), 1)
    t = np.where(idx < cnt[:, None], poly[..., 0] * nxt[..., 1] - nxt[..., 0] * poly[..., 1], 0.0)
    return 0.5 * t.sum(1)


def rotated_intersection(a, b):
    """intersection area of P pairs of rotated rectangles (P, 5), f64: Sutherland-Hodgman clipping of a by the edges of b, all pairs
    at once with a vertex count per pair (a quadrilateral cut by four half planes has at most 8 vertices)"""
    P = a.shape[0]
    if P == 0:
        return np.zeros(0)
    clip = _corners(b)
    orient = np.sign(_signed_area(clip, np.full(P, 4)))[:, None]
    poly = np.zeros((P, 8, 2))
    poly[:, :4] = _corners(a)
    cnt = np.full(P, 4)
    idx = np.arange(8)[None, :]
    for e in range(4):
        p0, p1 = clip[:, e], clip[:, (e + 1) % 4]
        ex, ey = (p1 - p0)[:, 0:1], (p1 - p0)[:, 1:2]
        valid = idx < cnt[:, None]
        nxt = np.take_along_axis(poly, np.where(idx + 1 < cnt[:, None], idx + 1, 0)[:, :, None].repeat(2, 2), 1)
        dc = orient * (ex * (poly[..., 1] - p0[:, 1:2]) - ey * (poly[..., 0] - p0[:, 0:1]))
        dn = orient * (ex * (nxt[..., 1] - p0[:, 1:2]) - ey * (nxt[..., 0] - p0[:, 0:1]))
        keep, cross = valid & (dc >= 0), valid & ((dc >= 0) != (dn >= 0))
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.where(cross, dc / (dc - dn), 0.0)
        x = poly + t[..., None] * (nxt - poly)
        slots = np.stack([keep, cross], 2).reshape(P, 16)
        pts = np.stack([poly, x], 2).reshape(P, 16, 2)
        pos = np.cumsum(slots, 1) - 1
        new = np.zeros((P, 8, 2))
        r, c = np.nonzero(slots)
        new[r, pos[r, c]] = pts[r, c]
        poly, cnt = new, slots.sum(1)
    return np.abs(_signed_area(poly, cnt))


def _pair_index(p):
    """(P) dt row and gt row of every (detection, ground truth) pair of a frame; the pairs of frame f lie at pair_off[f] in [dt, gt]
    row-major order"""
    ng, nd = np.diff(p['gt_off']), np.diff(p['dt_off'])
    P = int(p['pair_off'][-1])
    frame = np.repeat(np.arange(p['num_frames']), ng * nd)
    local = np.arange(P) - p['pair_off'][frame]
    g = ng[frame]
    safe = np.maximum(g, 1)
    return p['dt_off'][frame] + local // safe, p['gt_off'][frame] + local % safe


def host_overlaps(p):
    """-> (4, P) f64: image IoU, BEV IoU, 3D IoU, image intersection over the detection's area (the DontCare criterion)"""
    di, gi = _pair_index(p)
    out = np.zeros((4, len(di)))
    db, gb = p['dt_bbox'][di], p['gt_bbox'][gi]
    iw = np.minimum(db[:, 2], gb[:, 2]) - np.maximum(db[:, 0], gb[:, 0])
    ih = np.minimum(db[:, 3], gb[:, 3]) - np.maximum(db[:, 1], gb[:, 1])
    hit = (iw > 0) & (ih > 0)
    da = (db[:, 2] - db[:, 0]) * (db[:, 3] - db[:, 1])
    ga = (gb[:, 2] - gb[:, 0]) * (gb[:, 3] - gb[:, 1])
    with np.errstate(divide='ignore', invalid='ignore'):
        out[0] = np.where(hit, iw * ih / (da + ga - iw * ih), 0.0)
        out[3] = np.where(hit, iw * ih / da, 0.0)
    dc, gc = p['dt_cam'][di], p['gt_cam'][gi]
    near = np.hypot(dc[:, 0] - gc[:, 0], dc[:, 2] - gc[:, 2]) <= \
        0.5 * (np.hypot(dc[:, 3], dc[:, 5]) + np.hypot(gc[:, 3], gc[:, 5]))
    inter = np.zeros(len(di))
    inter[near] = rotated_intersection(gc[near][:, [0, 2, 3, 5, 6]], dc[near][:, [0, 2, 3, 5, 6]])
    with np.errstate(divide='ignore', invalid='ignore'):
        out[1] = np.where(inter > 0, inter / (dc[:, 3] * dc[:, 5] + gc[:, 3] * gc[:, 5] - inter), 0.0)
        ih3 = np.minimum(dc[:, 1], gc[:, 1]) - np.maximum(dc[:, 1] - dc[:, 4], gc[:, 1] - gc[:, 4])
        inc = ih3 * inter
        ok = (inter > 0) & (ih3 > 0)
        out[2] = np.where(ok, inc / (dc[:, 3] * dc[:, 4] * dc[:, 5] + gc[:, 3] * gc[:, 4] * gc[:, 5] - inc), 0.0)
    return out


# ------------------------------------------------------------------------------------------------------- host route: matching
def _match_frame(ov, ovdc, gf, df, gdc, score, galpha, dalpha, min_overlap, thresholds, metric, compute_aos):
    """compute_statistics_jit of one frame for T thresholds at once (thresholds None: the compute_fp=False pass, T = 1).
    ov, ovdc (D, G). The walk over the detections of a ground-truth box has a closed form: among the candidates (not of another
    class, not assigned, not below the threshold, overlap above the minimum) the first one of the largest overlap whose flag is 0
    (first of the highest score in the compute_fp=False pass, any flag), otherwise the first one whose flag is 1.
    -> tp, fp, fn (T) i64, similarity (T) f64, tp score per ground-truth box (G) f64 or None"""
    D, G = ov.shape
    fp_mode = thresholds is not None
    T = len(thresholds) if fp_mode else 1
    below = (score[None, :] < thresholds[:, None]) if fp_mode else np.zeros((1, D), bool)
    assigned = np.zeros((T, D), bool)
    tp, fp, fn, sim = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T)
    tp_score = None if fp_mode else np.full(G, -np.inf)
    rows = np.arange(T)
    if D == 0:
        return tp, fp, fn + int((gf == 0).sum()), sim, tp_score
    for i in np.nonzero(gf != -1)[0]:
        cand = ((df != -1) & (ov[:, i] > min_overlap))[None, :] & ~assigned & ~below
        if fp_mode:
            zero = cand & (df == 0)[None, :]
            det = np.where(zero.any(1), np.argmax(np.where(zero, ov[None, :, i], -1.0), 1), np.argmax(cand, 1))
            found = cand.any(1)
        else:
            cand &= (score > NO_DETECTION)[None, :]
            det = np.argmax(np.where(cand, score[None, :], -np.inf), 1)
            found = cand.any(1)
        nothing = found & ((gf[i] == 1) | (df[det] == 1))
        hit = found & ~nothing
        fn += (~found) & (gf[i] == 0)
        tp += hit
        assigned[rows[found], det[found]] = True
        if compute_aos:
            sim += np.where(hit, (1.0 + np.cos(galpha[i] - dalpha[det])) / 2.0, 0.0)
        if not fp_mode and hit[0]:
            tp_score[i] = score[det[0]]
    if fp_mode:
        open_ = ~assigned & (df == 0)[None, :] & ~below
        fp = open_.sum(1)
        if metric == 0:
            for i in np.nonzero(gdc)[0]:
                stuff = open_ & (ovdc[:, i] > min_overlap)[None, :]
                fp = fp - stuff.sum(1)
                open_ &= ~stuff
    return tp, fp, fn, sim, tp_score


def get_thresholds(scores, num_gt, num_sample_pts=N_SAMPLE_PTS):
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    current_recall = 0
    thresholds = []
    for i, score in enumerate(scores):
        l_recall = (i + 1) / num_gt
        r_recall = (i + 2) / num_gt if i < (len(scores) - 1) else l_recall
        if ((r_recall - current_recall) < (current_recall - l_recall)) and (i < (len(scores) - 1)):
            continue
        thresholds.append(score)
        current_recall += 1 / (num_sample_pts - 1.0)
    return thresholds


def _host_evaluate(p, current_classes, min_overlaps, metrics, aos_flags):
    C, K, M, F = len(current_classes), len(min_overlaps), len(metrics), p['num_frames']
    ov = host_overlaps(p)
    thr = np.zeros((M, C, 3, K, N_SAMPLE_PTS))
    nthr = np.zeros((M, C, 3, K), np.int64)
    pr = np.zeros((M, C, 3, K, N_SAMPLE_PTS, 4))
    tp_scores = {}
    num_valid = np.zeros((C, 3), np.int64)
    frames = []
    for f in range(F):
        g0, g1, d0, d1, q0 = p['gt_off'][f], p['gt_off'][f + 1], p['dt_off'][f], p['dt_off'][f + 1], p['pair_off'][f]
        shape = (d1 - d0, g1 - g0)
        frames.append((slice(g0, g1), slice(d0, d1), [ov[m, q0:q0 + shape[0] * shape[1]].reshape(shape) for m in range(4)]))
    for c, cls in enumerate(current_classes):
        for l in range(3):
            gf, df = ignore_flags(p, cls, l)
            num_valid[c, l] = int((gf == 0).sum())
            for mi, m in enumerate(metrics):
                for k in range(K):
                    mo = min_overlaps[k, m, c]
                    args = [(o[m], o[3], gf[gs], df[ds], p['gt_dc'][gs], p['dt_score'][ds], p['gt_alpha'][gs],
                             p['dt_alpha'][ds]) for gs, ds, o in frames]
                    slots = np.concatenate([_match_frame(*a, mo, None, m, False)[4] for a in args]) if F else np.zeros(0)
                    scores = np.sort(slots[slots > -np.inf])[::-1]
                    tp_scores[(mi, c, l, k)] = scores
                    t = np.array(get_thresholds(scores, num_valid[c, l]))
                    nthr[mi, c, l, k] = len(t)
                    thr[mi, c, l, k, :len(t)] = t
                    if len(t):
                        for a in args:
                            tp, fp, fn, sim, _ = _match_frame(*a, mo, t, m, aos_flags[mi])
                            pr[mi, c, l, k, :len(t)] += np.stack([tp, fp, fn, sim], 1)
    return {'overlaps': ov, 'thresholds': thr, 'num_thresholds': nthr, 'pr': pr, 'tp_scores': tp_scores, 'num_valid_gt': num_valid}


# --------------------------------------------------------------------------------------------------------------- both routes
def evaluate_packed(p, current_classes, min_overlaps, metrics=(0, 1, 2), aos_flags=None, route=None, detail=False):
    """all matchings of the given metrics -> dict: 'thresholds' (M, C, 3, K, 41) f64 with 'num_thresholds' (M, C, 3, K),
    'pr' (M, C, 3, K, 41, 4) f64 [tp, fp, fn, similarity] (integers are exact) and the final 'recall' / 'precision' / 'orientation'
    tables (M, C, 3, K, 41) taken from 'pr' in f64 as the reference takes them; with detail=True (always on the host route) also
    'tp_scores' {(mi, c, l, k): descending f64}, 'num_valid_gt' (C, 3) and 'overlaps' (4, P) f64"""
    metrics = list(metrics)
    aos_flags = list(aos_flags) if aos_flags is not None else [False] * len(metrics)
    min_overlaps = np.asarray(min_overlaps, dtype=np.float64)
    current_classes = [int(c) for c in current_classes]
    if default_route(route) == 'device':
        from crbhip import kitti_eval as dev
        r = dev.evaluate(p, current_classes, min_overlaps, metrics, aos_flags, detail=detail)
    else:
        r = _host_evaluate(p, current_classes, min_overlaps, metrics, aos_flags)
    pr, nthr = r['pr'], r['num_thresholds']
    live = np.arange(N_SAMPLE_PTS) < nthr[..., None]
    with np.errstate(divide='ignore', invalid='ignore'):
        tables = {'recall': pr[..., 0] / (pr[..., 0] + pr[..., 2]), 'precision': pr[..., 0] / (pr[..., 0] + pr[..., 1]),
                  'orientation': pr[..., 3] / (pr[..., 0] + pr[..., 1])}
    for name, t in tables.items():
        t = np.where(live, t, 0.0)
        # value i becomes the maximum of values i .. 40 for the live entries (NaN propagates, as np.max does)
        run = np.flip(np.maximum.accumulate(np.flip(t, -1), -1), -1)
        r[name] = np.where(live, run, 0.0)
    for mi in range(len(metrics)):
        if not aos_flags[mi]:
            r['orientation'][mi] = 0.0
    return r


def calculate_iou_partly(gt_annos, dt_annos, metric, num_parts=50, route=None):
    """-> overlaps (per frame (n_first, n_second) f64), parted_overlaps, total_gt_num, total_dt_num as the reference returns them.
    Only pairs of the same frame are computed: a part's matrix holds its frames' blocks on the diagonal and zeros elsewhere."""
    assert len(gt_annos) == len(dt_annos)
    if metric not in (0, 1, 2):
        raise ValueError("unknown metric")
    p = pack_annos(dt_annos, gt_annos)                  # rows = first argument
    if default_route(route) == 'device':
        from crbhip import kitti_eval as dev
        ov = dev.overlaps(p).cpu().numpy()[metric]
    else:
        ov = host_overlaps(p)[metric]
    n_first, n_second = np.diff(p['dt_off']), np.diff(p['gt_off'])
    overlaps = [ov[p['pair_off'][f]:p['pair_off'][f + 1]].reshape(n_first[f], n_second[f]) for f in range(len(gt_annos))]
    parted, idx = [], 0
    for num_part in get_split_parts(len(gt_annos), num_parts):
        a, b = p['dt_off'][idx:idx + num_part + 1] - p['dt_off'][idx], p['gt_off'][idx:idx + num_part + 1] - p['gt_off'][idx]
        part = np.zeros((a[-1], b[-1]))
        for i in range(num_part):
            part[a[i]:a[i + 1], b[i]:b[i + 1]] = overlaps[idx + i]
        parted.append(part)
        idx += num_part
    return overlaps, parted, n_first, n_second


def get_split_parts(num, num_part):
    same_part = num // num_part
    remain_num = num % num_part
    if same_part == 0:
        return [num]
    if remain_num == 0:
        return [same_part] * num_part
    return [same_part] * num_part + [remain_num]


def eval_class(gt_annos, dt_annos, current_classes, difficultys, metric, min_overlaps, compute_aos=False, num_parts=100, route=None):
    """-> {'recall', 'precision', 'orientation'}: (num_class, num_difficulty, num_minoverlap, 41). difficultys is a subset of
    [0, 1, 2]; all three are always computed and the requested ones returned."""
    r = evaluate_packed(pack_annos(gt_annos, dt_annos), current_classes, min_overlaps, [metric], [compute_aos], route)
    return {k: r[k][0][:, list(difficultys)] for k in ('recall', 'precision', 'orientation')}


def get_mAP(prec):
    sums = 0
    for i in range(0, prec.shape[-1], 4):
        sums = sums + prec[..., i]
    return sums / 11 * 100


def get_mAP_R40(prec):
    sums = 0
    for i in range(1, prec.shape[-1]):
        sums = sums + prec[..., i]
    return sums / 40 * 100


def print_str(value, *arg, sstream=None):
    if sstream is None:
        sstream = sysio.StringIO()
    sstream.truncate(0)
    sstream.seek(0)
    print(value, *arg, file=sstream)
    return sstream.getvalue()


def do_eval(gt_annos, dt_annos, current_classes, min_overlaps, compute_aos=False, PR_detail_dict=None, route=None, detail=None):
    """-> mAP_bbox, mAP_bev, mAP_3d, mAP_aos, mAP_bbox_R40, mAP_bev_R40, mAP_3d_R40, mAP_aos_R40, each (num_class, 3, num_minoverlap).
    The three metrics share one pass. detail: a dict that receives the thresholds, counts and true-positive scores."""
    r = evaluate_packed(pack_annos(gt_annos, dt_annos), current_classes, min_overlaps, (0, 1, 2), (compute_aos, False, False), route,
                        detail=detail is not None)
    if detail is not None:
        detail.update(r)
    prec = r['precision']
    mAP_aos = mAP_aos_R40 = None
    if PR_detail_dict is not None:
        PR_detail_dict['bbox'] = prec[0]
    if compute_aos:
        mAP_aos, mAP_aos_R40 = get_mAP(r['orientation'][0]), get_mAP_R40(r['orientation'][0])
        if PR_detail_dict is not None:
            PR_detail_dict['aos'] = r['orientation'][0]
    if PR_detail_dict is not None:
        PR_detail_dict['bev'] = prec[1]
        PR_detail_dict['3d'] = prec[2]
    return (get_mAP(prec[0]), get_mAP(prec[1]), get_mAP(prec[2]), mAP_aos,
            get_mAP_R40(prec[0]), get_mAP_R40(prec[1]), get_mAP_R40(prec[2]), mAP_aos_R40)


def get_official_eval_result(gt_annos, dt_annos, current_classes, PR_detail_dict=None, route=None, detail=None):
    overlap_0_7 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7], [0.7, 0.5, 0.5, 0.7, 0.5, 0.7]])
    overlap_0_5 = np.array([[0.7, 0.5, 0.5, 0.7, 0.5, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5], [0.5, 0.25, 0.25, 0.5, 0.25, 0.5]])
    min_overlaps = np.stack([overlap_0_7, overlap_0_5], axis=0)
    class_to_name = {0: 'Car', 1: 'Pedestrian', 2: 'Cyclist', 3: 'Van', 4: 'Person_sitting', 5: 'Truck'}
    name_to_class = {v: n for n, v in class_to_name.items()}
    if not isinstance(current_classes, (list, tuple)):
        current_classes = [current_classes]
    current_classes = [name_to_class[c] if isinstance(c, str) else c for c in current_classes]
    min_overlaps = min_overlaps[:, :, current_classes]
    result = ''
    compute_aos = False                                   # the first detection of the first non-empty frame decides, as there
    for anno in dt_annos:
        if anno['alpha'].shape[0] != 0:
            if anno['alpha'][0] != -10:
                compute_aos = True
            break
    mAPbbox, mAPbev, mAP3d, mAPaos, mAPbbox_R40, mAPbev_R40, mAP3d_R40, mAPaos_R40 = do_eval(
        gt_annos, dt_annos, current_classes, min_overlaps, compute_aos, PR_detail_dict=PR_detail_dict, route=route, detail=detail)

    ret_dict = {}
    for j, curcls in enumerate(current_classes):
        name = class_to_name[curcls]
        for i in range(min_overlaps.shape[0]):
            for tag, bbox, bev, d3, aos in (('AP', mAPbbox, mAPbev, mAP3d, mAPaos), ('AP_R40', mAPbbox_R40, mAPbev_R40, mAP3d_R40, mAPaos_R40)):
                result += print_str(f"{name} " + (tag + "@{:.2f}, {:.2f}, {:.2f}:").format(*min_overlaps[i, :, j]))
                result += print_str(f"bbox AP:{bbox[j, 0, i]:.4f}, {bbox[j, 1, i]:.4f}, {bbox[j, 2, i]:.4f}")
                result += print_str(f"bev  AP:{bev[j, 0, i]:.4f}, {bev[j, 1, i]:.4f}, {bev[j, 2, i]:.4f}")
                result += print_str(f"3d   AP:{d3[j, 0, i]:.4f}, {d3[j, 1, i]:.4f}, {d3[j, 2, i]:.4f}")
                if compute_aos:
                    result += print_str(f"aos  AP:{aos[j, 0, i]:.2f}, {aos[j, 1, i]:.2f}, {aos[j, 2, i]:.2f}")
            if i == 0:
                for key, table in (('aos', mAPaos_R40), ('3d', mAP3d_R40), ('bev', mAPbev_R40), ('image', mAPbbox_R40)):
                    if table is None:
                        continue
                    for l, level in enumerate(('easy', 'moderate', 'hard')):
                        ret_dict['%s_%s/%s_R40' % (name, key, level)] = table[j, l, 0]
    return result, ret_dict
