"""Generate ref_kitti_eval.npz from the reference's own KITTI evaluator (companion of make_goldens.py, whose import recipe it reuses).

Runs ONLY where the reference tree is mounted; the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_kitti_eval.py

The reference's eval.py is numba.jit and its rotate_iou.py numba.cuda; both run here as plain Python. After import_reference() the
numba stub gets float32 / int32 and numba.cuda a local.array / shared.array that return numpy arrays of the run's precision, and
rotate_iou_gpu_eval is replaced in both modules by a double loop (ours) that calls the reference's devRotateIoUEval(query_box, box,
criterion) per pair, in the argument order of its kernel, output [N, K], with a centre-distance early-out. Nothing of the reference
is copied.

Cases (tests/kitti_eval_cases.py draws the annos; every frame is margin-safe against the REFERENCE's f32 and f64 overlaps, and no
minimum overlap lies between the two):
  small           24 frames, 0..12 gt, all seven names, three noise levels, wrong classes, low boxes, false positives; frame 3 has no
                  gt, frame 4 no detections, frame 5 neither
  small_noalpha   the same frames with every detection's alpha = -10: the reference leaves AOS out (result text and dict only)
  dense           64 frames of easy objects with tight detections and no Cyclist at all: some combination reaches 41 thresholds, some
                  stays below, and the Cyclist rows have no valid ground truth
Stored per case, under '<case>/': gt/<key>, dt/<key> (flat annos, 'n' per frame), result_str, ret_keys / ret_vals, pr_detail/<key>,
  recall / precision / orientation (3 metrics, C, 3, K, 41) from eval_class, overlaps_f32 / overlaps_f64 (3, P): the per-frame [dt, gt]
  matrices flattened in frame order, from a run with f32 local arrays and inputs (the reference's) and one with f64; thresholds
  (54, 41) + num_thresholds (54), pr (54, 41, 4) [tp, fp, fn, similarity], tp_scores (flat, descending per combination) +
  num_tp (54); combination index = ((metric * C + class) * 3 + difficulty) * K + overlap row.
e_ref (3): max |f32 - f64| overlap per metric over the cases, the project's unit for the overlap bars."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402
import kitti_eval_cases as kc  # noqa: E402

CLASSES = ['Car', 'Pedestrian', 'Cyclist']
LOCAL = {'dtype': np.float32}
REC = {}


def install():
    mg.import_reference()
    nb = sys.modules['numba']
    nb.float32, nb.int32 = np.float32, np.int32
    array = lambda shape, dtype=None: np.zeros(shape, dtype=LOCAL['dtype'])
    nb.cuda.local = types.SimpleNamespace(array=array)
    nb.cuda.shared = types.SimpleNamespace(array=array)
    from pcdet.datasets.kitti.kitti_object_eval_python import eval as ref_eval, rotate_iou as ref_riou

    def rotate_iou_eval(boxes, query_boxes, criterion=-1, device_id=0):
        dt = LOCAL['dtype']
        boxes, query_boxes = boxes.astype(dt), query_boxes.astype(dt)
        iou = np.zeros((boxes.shape[0], query_boxes.shape[0]), dtype=dt)
        reach_b, reach_q = 0.5 * np.hypot(boxes[:, 2], boxes[:, 3]), 0.5 * np.hypot(query_boxes[:, 2], query_boxes[:, 3])
        with np.errstate(all='ignore'):
            for n in range(boxes.shape[0]):
                for k in range(query_boxes.shape[0]):
                    if np.hypot(boxes[n, 0] - query_boxes[k, 0], boxes[n, 1] - query_boxes[k, 1]) > reach_b[n] + reach_q[k]:
                        continue
                    iou[n, k] = ref_riou.devRotateIoUEval(query_boxes[k], boxes[n], criterion)
        return iou

    ref_eval.rotate_iou_gpu_eval = ref_riou.rotate_iou_gpu_eval = rotate_iou_eval

    get_thresholds, fused, eval_class = ref_eval.get_thresholds, ref_eval.fused_compute_statistics, ref_eval.eval_class

    def rec_thresholds(scores, num_gt, num_sample_pts=41):
        r = get_thresholds(scores, num_gt, num_sample_pts)                   # sorts `scores` in place (ascending)
        REC['tp'].append(np.array(scores, dtype=np.float64)[::-1].copy())
        REC['thr'].append(np.array(r, dtype=np.float64))
        return r

    def rec_fused(overlaps, pr, *a, **k):
        fused(overlaps, pr, *a, **k)
        if not REC['pr'] or REC['pr'][-1] is not pr:
            REC['pr'].append(pr)

    def rec_eval_class(*a, **k):
        r = eval_class(*a, **k)
        REC['tables'].append(r)
        return r

    ref_eval.get_thresholds, ref_eval.fused_compute_statistics, ref_eval.eval_class = rec_thresholds, rec_fused, rec_eval_class
    return ref_eval


def frame_overlaps(ref_eval, gt_annos, dt_annos, dtype):
    """-> (3, P): the reference's overlaps of every frame, [dt, gt] row-major, in frame order"""
    LOCAL['dtype'] = dtype
    cast = lambda annos: [{k: (v.astype(dtype) if k in ('dimensions', 'location', 'rotation_y') else v) for k, v in a.items()} for a in annos]
    try:
        out = [np.concatenate([o.reshape(-1).astype(np.float64) for o in
                               ref_eval.calculate_iou_partly(cast(dt_annos), cast(gt_annos), m, 100)[0]] + [np.zeros(0)])
               for m in range(3)]
    finally:
        LOCAL['dtype'] = np.float32
    return np.stack(out)


def run_case(ref_eval, gt_annos, dt_annos, full=True):
    REC.update({'tp': [], 'thr': [], 'pr': [], 'tables': []})
    detail = {}
    result_str, ret = ref_eval.get_official_eval_result(gt_annos, dt_annos, CLASSES, PR_detail_dict=detail)
    out = {'result_str': np.array(result_str), 'ret_keys': np.array(list(ret.keys())), 'ret_vals': np.array([ret[k] for k in ret])}
    for k, v in kc.pack(gt_annos, False).items():
        out['gt/' + k] = v
    for k, v in kc.pack(dt_annos, True).items():
        out['dt/' + k] = v
    if not full:
        return out
    for k, v in detail.items():
        out['pr_detail/' + k] = v
    assert len(REC['tables']) == 3 and len(REC['thr']) == len(REC['pr']) == 54
    for name in ('recall', 'precision', 'orientation'):
        out[name] = np.stack([t[name] for t in REC['tables']])
    thr, pr = np.zeros((54, 41)), np.zeros((54, 41, 4))
    for q in range(54):
        n = len(REC['thr'][q])
        assert n <= 41 and REC['pr'][q].shape == (n, 4)
        thr[q, :n], pr[q, :n] = REC['thr'][q], REC['pr'][q]
    out.update({'thresholds': thr, 'num_thresholds': np.array([len(t) for t in REC['thr']]), 'pr': pr,
                'tp_scores': np.concatenate(REC['tp'] + [np.zeros(0)]), 'num_tp': np.array([len(t) for t in REC['tp']])})
    out['overlaps_f32'] = frame_overlaps(ref_eval, gt_annos, dt_annos, np.float32)
    out['overlaps_f64'] = frame_overlaps(ref_eval, gt_annos, dt_annos, np.float64)
    return out


def check_inputs(ref_eval, gt_annos, dt_annos, ov32):
    """the conditions the cases must meet, on the stored inputs -> set of the conditions met"""
    met, q0 = set(), 0
    for g, d in zip(gt_annos, dt_annos):
        ng, nd = len(g['name']), len(d['name'])
        met.add('no gt' if ng == 0 and nd else 'no dt' if nd == 0 and ng else 'neither' if ng == 0 and nd == 0 else 'both')
        o3 = ov32[2, q0:q0 + ng * nd].reshape(nd, ng)
        q0 += ng * nd
        for j in range(nd):
            if abs(d['bbox'][j, 3] - d['bbox'][j, 1]) < 25 and d['name'][j] in CLASSES:
                met.add('low detection')
            for i in range(ng):
                if g['name'][i] == 'Van' and d['name'][j] == 'Car' and o3[j, i] > 0.7:
                    met.add('Van matched by Car')
                if g['name'][i] == 'Person_sitting' and d['name'][j] == 'Pedestrian' and o3[j, i] > 0.5:
                    met.add('Person_sitting matched by Pedestrian')
        assert len(set(d['score'].tolist())) == nd and d['score'].dtype == np.float32
    assert not kc.near_threshold([ov32])
    names = np.concatenate([g['name'] for g in gt_annos])
    for n in ('Van', 'Person_sitting', 'DontCare'):
        if n in names:
            met.add('name ' + n)
    return met


def main():
    ref_eval = install()

    def overlap_fn(g, d):
        # the margin rule on the reference's f32 overlaps AND on its f64 ones, and no minimum overlap between the two: the reference's
        # f32 clipper is up to 1e-3 off on some pairs (e_ref below), more than the margin
        a, b = frame_overlaps(ref_eval, [g], [d], np.float32), frame_overlaps(ref_eval, [g], [d], np.float64)
        flip = any(np.any((a > t) != (b > t)) for t in kc.MIN_OVERLAPS)
        return [a, b, np.full(1, kc.MIN_OVERLAPS[0]) if flip else np.zeros(0)]

    out, met = {}, set()
    small_gt, small_dt, again = kc.make_annos(2024, 24, kc.SMALL, overlap_fn, forced={3: (0, 4), 4: (5, 0), 5: (0, 0)})
    print('small: %d frames drawn again for the margin rule' % again)
    out['small'] = run_case(ref_eval, small_gt, small_dt)
    # nstuff > 0: with the DontCare regions moved off the image some image-metric false-positive count must change
    moved = [dict(g, bbox=np.where((g['name'] == 'DontCare')[:, None], g['bbox'] - 5000.0, g['bbox'])) for g in small_gt]
    REC.update({'tp': [], 'thr': [], 'pr': [], 'tables': []})
    ref_eval.get_official_eval_result(moved, small_dt, CLASSES)
    assert any(not np.array_equal(REC['pr'][q][:, 1], out['small']['pr'][q, :len(REC['pr'][q]), 1]) for q in range(18)), \
        'no false positive is absorbed by a DontCare region'
    met |= check_inputs(ref_eval, small_gt, small_dt, out['small']['overlaps_f32'])
    o = out['small']
    assert any(k.endswith('_aos/easy_R40') for k in o['ret_keys']) and len(o['ret_keys']) == 36

    noalpha = [dict(d, alpha=np.full(len(d['name']), -10.0)) for d in small_dt]
    out['small_noalpha'] = run_case(ref_eval, small_gt, noalpha, full=False)
    assert len(out['small_noalpha']['ret_keys']) == 27

    dense_gt, dense_dt, again = kc.make_annos(77, 64, kc.DENSE, overlap_fn)
    print('dense: %d frames drawn again for the margin rule' % again)
    out['dense'] = run_case(ref_eval, dense_gt, dense_dt)
    met |= check_inputs(ref_eval, dense_gt, dense_dt, out['dense']['overlaps_f32'])
    nthr = out['dense']['num_thresholds'].reshape(3, 3, 3, 2)
    print('dense: thresholds per combination', nthr.reshape(-1).tolist())
    assert nthr.max() == 41 and nthr[:, :2].min() < 41 and (nthr[:, 2] == 0).all(), 'dense must reach 41, stay below 41, and have no Cyclist'
    assert 'Cyclist' not in np.concatenate([g['name'] for g in dense_gt])

    want = {'no gt', 'no dt', 'neither', 'both', 'low detection', 'Van matched by Car', 'Person_sitting matched by Pedestrian',
            'name Van', 'name Person_sitting', 'name DontCare'}
    assert want <= met, want - met
    out['e_ref'] = np.max([np.abs(out[c]['overlaps_f32'] - out[c]['overlaps_f64']).max(axis=1) for c in ('small', 'dense')], axis=0)
    print('e_ref per metric', out['e_ref'])
    for c in ('small', 'dense'):
        print(c, 'gt %d dt %d pairs %d' % (out[c]['gt/n'].sum(), out[c]['dt/n'].sum(), out[c]['overlaps_f32'].shape[1]))
    mg.save('ref_kitti_eval.npz', out)


if __name__ == '__main__':
    main()
