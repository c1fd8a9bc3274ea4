"""GPU: the device route of the KITTI evaluator (csrc/kitti_eval.hip behind get_official_eval_result(route='device')) against the
reference's recorded run (tests/golden/ref_kitti_eval.npz) and, on seeded random annos, against the host route.

Bars. Rotated overlaps: FACTOR x e_ref of the golden's f64 values, e_ref = the reference's own max |f32 - f64| per metric recorded
there. Image-box IoU: 1e-12 (the same f64 expression). True-positive scores, thresholds (values and count) and the tp / fp / fn
counts of all 54 combinations: EQUAL. Similarity 1e-9 (a few hundred f64 cos terms of <= 1 ulp each). Tables 1e-12 (f64 ratios of
equal integers), orientation 1e-9; the dict's AP values 1e-12 and its AOS values 1e-7 (100 x the mean of 40 orientation entries of
1e-9 each is 1e-7 at most). Result text equal.
Frame order: the counts are integer sums and do not depend on it; the similarity is added in frame order, so a permutation of the
frames may move it inside the 1e-9 bar.
The functions below are also what tools/kitti_eval_host_check.py runs on the host build of the kernels."""
import os

import numpy as np
import pytest

import kitti_eval_cases as kc
from pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_eval

FACTOR = 4
CLASSES = ['Car', 'Pedestrian', 'Cyclist']
CASES = ('small', 'dense')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_kitti_eval.npz')
_cache = {}


def golden():
    if 'z' not in _cache:
        _cache['z'] = np.load(GOLDEN)
    return _cache['z']


def annos(case):
    z = golden()
    return kc.unpack(z, case + '/gt/', False), kc.unpack(z, case + '/dt/', True)


def run(gt, dt, classes=CLASSES, route='device'):
    detail, pr_detail = {}, {}
    text, ret = kitti_eval.get_official_eval_result(gt, dt, classes, PR_detail_dict=pr_detail, route=route, detail=detail)
    return {'text': text, 'ret': ret, 'detail': detail, 'pr_detail': pr_detail}


def run_case(case):
    return run(*annos(case))


def same_bits(a, b):
    da, db = a['detail'], b['detail']
    return a['text'] == b['text'] and all(np.array_equal(da[k], db[k], equal_nan=True) for k in
                                           ('overlaps', 'thresholds', 'num_thresholds', 'pr', 'recall', 'precision', 'orientation'))


def check_against(z, case, r, full=True):
    """-> list of misses; prints every figure before it is judged"""
    bad = []

    def judge(name, value, bar):
        print('%s %s: %s (bar %s)' % (case, name, value, bar))
        if not value <= bar:
            bad.append('%s %s: %s > %s' % (case, name, value, bar))

    def equal(name, a, b):
        ok = np.array_equal(np.asarray(a), np.asarray(b))
        print('%s %s equal: %s' % (case, name, ok))
        if not ok:
            bad.append('%s %s differs' % (case, name))

    equal('result text', r['text'], str(z[case + '/result_str']))
    equal('dict keys', list(r['ret'].keys()), [str(k) for k in z[case + '/ret_keys']])
    for k, v in zip(z[case + '/ret_keys'], z[case + '/ret_vals']):
        got = r['ret'].get(str(k), np.inf)
        if not (np.isnan(v) and np.isnan(got)):
            judge('dict ' + str(k), abs(got - v), 1e-7 if '_aos/' in str(k) else 1e-12)
    if not full:
        return bad
    d, e_ref = r['detail'], z['e_ref']
    judge('image IoU', np.abs(d['overlaps'][0] - z[case + '/overlaps_f64'][0]).max(), 1e-12)
    for m, name in ((1, 'BEV IoU'), (2, '3D IoU')):
        judge(name + ' vs f64', np.abs(d['overlaps'][m] - z[case + '/overlaps_f64'][m]).max(), FACTOR * e_ref[m])
    equal('true-positive scores', np.concatenate([d['tp_scores'][k] for k in sorted(d['tp_scores'])]), z[case + '/tp_scores'])
    equal('true positives per combination', [len(d['tp_scores'][k]) for k in sorted(d['tp_scores'])], z[case + '/num_tp'])
    equal('number of thresholds', d['num_thresholds'].reshape(-1), z[case + '/num_thresholds'])
    equal('thresholds', d['thresholds'].reshape(54, 41), z[case + '/thresholds'])
    pr = d['pr'].reshape(54, 41, 4)
    equal('tp / fp / fn', pr[..., :3], z[case + '/pr'][..., :3])
    judge('similarity', np.abs(pr[..., 3] - z[case + '/pr'][..., 3]).max(), 1e-9)
    for name, bar in (('recall', 1e-12), ('precision', 1e-12), ('orientation', 1e-9)):
        a, b = d[name], z[case + '/' + name]
        equal(name + ' NaN pattern', np.isnan(a), np.isnan(b))
        judge(name, np.nanmax(np.abs(a - b)) if np.isfinite(a).any() else 0.0, bar)
    for key, bar in (('bbox', 1e-12), ('bev', 1e-12), ('3d', 1e-12), ('aos', 1e-9)):
        a, b = r['pr_detail'][key], z[case + '/pr_detail/' + key]
        judge('PR_detail_dict ' + key, np.nanmax(np.abs(a - b)), bar)
    return bad


def check_case(case, r):
    return check_against(golden(), case, r)


# ---------------------------------------------------------------------------------------------------------------- size cases
def _limits():
    from crbhip import kitti_eval as dev
    return dev.stage_limits()


def size_annos(name):
    """seeded margin-safe (against the host route's f64 overlaps) random annos -> gt_annos, dt_annos, classes"""
    if name == 'one_frame':
        return kc.make_annos(11, 1, kc.SMALL, kc.host_overlap_fn, forced={0: (9, 12)})[:2] + (CLASSES,)
    if name in ('65_frames', '129_frames'):
        return kc.make_annos(12, int(name.split('_')[0]), dict(kc.SMALL, max_gt=5, max_fp=2), kc.host_overlap_fn)[:2] + (CLASSES,)
    if name == 'empty_sides':
        return kc.make_annos(13, 5, kc.SMALL, kc.host_overlap_fn, forced={0: (0, 70), 1: (30, 0), 2: (1, 1), 3: (0, 0)})[:2] + (CLASSES,)
    if name == 'stage_limit':
        max_gt, max_dt, max_pairs = _limits()                       # 64, 512, 2048
        forced = {0: (32, max_pairs // 32), 1: (32, max_pairs // 32 + 1), 2: (max_gt, 20), 3: (max_gt + 1, 20), 4: (3, max_dt),
                  5: (3, max_dt + 1)}
        return kc.make_annos(14, 7, kc.SMALL, kc.host_overlap_fn, forced=forced)[:2] + (CLASSES,)
    if name == 'cyclist_only':
        return kc.make_annos(15, 12, kc.SMALL, kc.host_overlap_fn)[:2] + (['Cyclist'],)
    raise KeyError(name)


SIZE_CASES = ('one_frame', '65_frames', '129_frames', 'empty_sides', 'stage_limit', 'cyclist_only')


def compare_routes(name, dev, host):
    bad = []
    a, b = dev['detail'], host['detail']
    for k in ('num_thresholds', 'thresholds'):
        if not np.array_equal(a[k], b[k]):
            bad.append('%s: %s differs between the routes' % (name, k))
    if not np.array_equal(a['pr'][..., :3], b['pr'][..., :3]):
        bad.append('%s: tp / fp / fn differ between the routes' % name)
    sim = np.abs(a['pr'][..., 3] - b['pr'][..., 3]).max() if a['pr'].size else 0.0
    print('%s: thresholds %d .. %d, tp sum %d, similarity difference %.3g' % (name, a['num_thresholds'].min(), a['num_thresholds'].max(),
                                                                             a['pr'][..., 0].sum(), sim))
    if not sim <= 1e-9:
        bad.append('%s: similarity differs by %g' % (name, sim))
    if dev['text'] != host['text']:
        bad.append('%s: result text differs between the routes' % name)
    return bad


def check_sizes(name):
    gt, dt, classes = size_annos(name)
    return compare_routes(name, run(gt, dt, classes, 'device'), run(gt, dt, classes, 'host'))


# --------------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope='module')
def device_runs():
    return {case: run_case(case) for case in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_device_route_against_reference(device_runs, case):
    bad = check_case(case, device_runs[case])
    assert not bad, bad


@pytest.mark.gpu
def test_alpha_switched_off_leaves_aos_out():
    gt, dt = annos('small_noalpha')
    assert dt[0]['alpha'][0] == -10
    r = run(gt, dt)
    bad = check_against(golden(), 'small_noalpha', r, full=False)
    assert not bad and 'aos' not in r['text'] and len(r['ret']) == 27, bad


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_two_runs_bit_equal(device_runs, case):
    assert same_bits(device_runs[case], run_case(case))


@pytest.mark.gpu
def test_frame_order_changes_no_count(device_runs):
    gt, dt = annos('small')
    perm = np.random.default_rng(3).permutation(len(gt))
    a, b = device_runs['small']['detail'], run([gt[i] for i in perm], [dt[i] for i in perm])['detail']
    assert np.array_equal(a['thresholds'], b['thresholds']) and np.array_equal(a['pr'][..., :3], b['pr'][..., :3])
    assert np.abs(a['pr'][..., 3] - b['pr'][..., 3]).max() <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize('name', SIZE_CASES)
def test_sizes_against_host_route(name):
    bad = check_sizes(name)
    assert not bad, bad


@pytest.mark.gpu
def test_public_functions_return_shapes():
    gt, dt = annos('small')
    overlaps, parted, n_first, n_second = kitti_eval.calculate_iou_partly(dt, gt, 2, route='device')
    assert len(overlaps) == len(gt) and all(o.shape == (len(d['name']), len(g['name'])) for o, g, d in zip(overlaps, gt, dt))
    assert parted[0].shape == (n_first.sum(), n_second.sum())
    flat = np.concatenate([o.reshape(-1) for o in overlaps])
    assert np.abs(flat - golden()['small/overlaps_f64'][2]).max() <= FACTOR * golden()['e_ref'][2]
    mo = np.stack([np.full((3, 3), 0.7), np.full((3, 3), 0.5)])
    r = kitti_eval.eval_class(gt, dt, [0, 1, 2], [0, 1, 2], 1, mo, route='device')
    assert r['precision'].shape == (3, 3, 2, 41) and not r['orientation'].any()


@pytest.mark.gpu
def test_eval_one_epoch_second():
    """model -> pred_dicts -> AP on 8 synthetic frames; both routes on the detector's own boxes agree on every count"""
    import torch
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.model_cfgs import second_cfg
    from pcdet.models import build_network
    from pcdet.utils.eval_utils import eval_one_epoch
    torch.manual_seed(0)
    ds = SyntheticDataset(num_frames=8, training=False)
    cfg = second_cfg('kitti')
    cfg.MODEL.POST_PROCESSING.SCORE_THRESH = 0.0            # seeded weights: keep what the NMS keeps
    model = build_network(cfg.MODEL, 3, ds).cuda()
    loader = build_synthetic_dataloader(ds, batch_size=4)
    seen = []
    keep = ds.generate_prediction_dicts
    ds.generate_prediction_dicts = lambda *a, **k: seen.append(keep(*a, **k)) or seen[-1]
    det_dev = {}
    ret = eval_one_epoch(cfg, model, loader, route='device', detail=det_dev)
    for t in (0.3, 0.5, 0.7):
        assert 'recall/roi_%s' % t in ret and 'recall/rcnn_%s' % t in ret
    ap_keys = ['%s_%s/%s_R40' % (c, m, l) for c in ds.class_names for m in ('3d', 'bev', 'image') for l in ('easy', 'moderate', 'hard')]
    assert all(k in ret and (np.isfinite(ret[k]) or np.isnan(ret[k])) for k in ap_keys)
    det_annos = [a for batch in seen for a in batch]
    assert len(det_annos) == 8 and sum(len(a['name']) for a in det_annos) > 0
    det_host = {}
    ds.evaluation(det_annos, ds.class_names, route='host', detail=det_host)
    assert np.array_equal(det_dev['num_thresholds'], det_host['num_thresholds'])
    assert np.array_equal(det_dev['pr'][..., :3], det_host['pr'][..., :3])


@pytest.mark.gpu
def test_ground_truth_fed_back_scores_100_on_device():
    """identical boxes: every corner of one lies exactly on the other's boundary, which the f32 clipper must still count as inside
    (the corner margin of csrc/kitti_eval.hip); 256 frames so that every class / difficulty has the 40 valid boxes AP 100 needs"""
    from pcdet.datasets import SyntheticDataset
    ds = SyntheticDataset(num_frames=256, n_points=500)
    gt = [info['annos'] for info in ds.kitti_infos]
    dt = [dict(g, score=np.ones(len(g['name']), dtype=np.float32)) for g in gt]
    dev, host = {}, {}
    _, ap = ds.evaluation(dt, ds.class_names, route='device', detail=dev)
    ds.evaluation(dt, ds.class_names, route='host', detail=host)
    p = kitti_eval.pack_annos(gt, dt)
    dt_row, gt_row = kitti_eval._pair_index(p)
    diagonal = dt_row == gt_row                                                          # the pairs of identical boxes
    worst = np.abs(dev['overlaps'][1:3, diagonal] - 1.0).max()
    print('identical boxes: BEV / 3D IoU at most %.3g from 1' % worst)
    # bar: the margin the project keeps between an overlap and a decision (kitti_eval_cases.MARGIN); f32 clipping of a box of
    # >= 0.5 m with coordinates below 10 m is good to about 1e-6
    assert worst <= kc.MARGIN and diagonal.sum() == p['gt_off'][-1]
    assert all(v == 100.0 for v in ap.values()), ap
    assert np.array_equal(dev['pr'][..., :3], host['pr'][..., :3]) and np.array_equal(dev['thresholds'], host['thresholds'])
