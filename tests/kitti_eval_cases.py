"""Seeded KITTI annos for the evaluator's tests and goldens: generator, margin rule, (un)packing into flat arrays.

A frame is drawn from (seed, frame index, attempt). The margin rule of the project (README, NMS): a frame is drawn again with the
next attempt while any overlap of any metric lies within MARGIN of a minimum overlap (0.25, 0.5, 0.7), so no stored decision is a
near-tie; the caller passes the function that gives the frame's overlaps (the reference's for the goldens, the host route's for
random cases). Scores are distinct f32 values within a frame.

Ground truth of a frame: names from Car / Pedestrian / Cyclist / Van / Person_sitting / Truck / DontCare, occlusion 0..3,
truncation 0..0.6, image-box heights 20..90 px (`easy` frames: occlusion 0, truncation 0, heights 45..90). Detections: jittered
copies of the ground truth at the noise levels of the spec, some with the wrong class, some with a box below the height limits,
plus pure false positives, half of them inside a DontCare region when the frame has one."""
import numpy as np

MARGIN = 1e-4
MIN_OVERLAPS = (0.25, 0.5, 0.7)
DIMS = {'Car': (3.9, 1.56, 1.6), 'Van': (5.0, 2.2, 1.9), 'Truck': (8.0, 3.0, 2.5), 'Pedestrian': (0.8, 1.73, 0.6),
        'Person_sitting': (0.8, 1.3, 0.6), 'Cyclist': (1.76, 1.73, 0.6)}          # l, h, w
DETECTED_AS = {'Van': 'Car', 'Person_sitting': 'Pedestrian'}
SMALL = dict(names=('Car', 'Pedestrian', 'Cyclist', 'Van', 'Person_sitting', 'Truck'), weights=(5, 3, 3, 2, 2, 1), max_gt=12, max_dc=2,
             noise=(0.03, 0.12, 0.35), p_det=0.8, p_wrong=0.1, p_low=0.08, max_fp=5, easy=False)
DENSE = dict(names=('Car', 'Pedestrian', 'Van', 'Person_sitting'), weights=(6, 4, 1, 1), max_gt=8, max_dc=1,
             noise=(0.01, 0.02, 0.03), p_det={'Car': 1.0, 'Van': 1.0, 'default': 0.8}, p_wrong=0.0, p_low=0.0, max_fp=2, easy=True)


def empty_anno(with_score):
    a = {'name': np.zeros(0, dtype='<U14'), 'truncated': np.zeros(0), 'occluded': np.zeros(0, dtype=np.int64), 'alpha': np.zeros(0),
         'bbox': np.zeros((0, 4)), 'dimensions': np.zeros((0, 3)), 'location': np.zeros((0, 3)), 'rotation_y': np.zeros(0)}
    if with_score:
        a['score'] = np.zeros(0, dtype=np.float32)
    return a


def _anno(rows, with_score):
    a = empty_anno(with_score)
    if rows:
        for k in a:
            a[k] = np.array([r.get(k, 0.0) for r in rows], dtype=a[k].dtype)
    return a


def _object(rng, name, easy):
    l, h, w = np.array(DIMS[name]) * rng.uniform(0.9, 1.1, 3)
    x, z = rng.uniform(-25, 25), rng.uniform(6, 60)
    ry = rng.uniform(-np.pi, np.pi)
    hpx = rng.uniform(45, 90) if easy else rng.uniform(20, 90)
    wpx = hpx * rng.uniform(0.6, 2.0)
    u, v = rng.uniform(80, 1150), rng.uniform(150, 300)
    return {'name': name, 'truncated': 0.0 if easy else float(rng.choice([0.0, 0.1, 0.2, 0.4, 0.6])),
            'occluded': 0 if easy else int(rng.integers(0, 4)), 'alpha': ry - np.arctan2(x, z),
            'bbox': [u - wpx / 2, v - hpx / 2, u + wpx / 2, v + hpx / 2], 'dimensions': [l, h, w],
            'location': [x, rng.uniform(1.4, 1.9), z], 'rotation_y': ry}


def _dontcare(rng):
    u, v, wpx, hpx = rng.uniform(150, 1000), rng.uniform(150, 300), rng.uniform(80, 200), rng.uniform(40, 100)
    return {'name': 'DontCare', 'truncated': -1.0, 'occluded': -1, 'alpha': -10.0, 'bbox': [u - wpx / 2, v - hpx / 2, u + wpx / 2, v + hpx / 2],
            'dimensions': [-1.0, -1.0, -1.0], 'location': [-1000.0, -1000.0, -1000.0], 'rotation_y': -10.0}


def draw_frame(rng, spec, n_gt=None, n_dt=None):
    """-> gt anno, dt anno (scores still to be set by the caller). n_gt / n_dt force the counts (n_dt: false positives fill up)."""
    names, w = spec['names'], np.array(spec['weights'], dtype=np.float64)
    count = int(rng.integers(0, spec['max_gt'] + 1)) if n_gt is None else n_gt
    n_dc = min(int(rng.integers(0, spec['max_dc'] + 1)), count)
    gts = [_object(rng, str(rng.choice(names, p=w / w.sum())), spec['easy']) for _ in range(count - n_dc)] + \
        [_dontcare(rng) for _ in range(n_dc)]
    order = rng.permutation(len(gts))
    gts = [gts[i] for i in order]
    dts = []
    for g in gts:
        if g['name'] == 'DontCare':
            continue
        p_det = spec['p_det'] if not isinstance(spec['p_det'], dict) else spec['p_det'].get(g['name'], spec['p_det']['default'])
        if rng.uniform() >= p_det:
            continue
        s = float(rng.choice(spec['noise']))
        hpx = g['bbox'][3] - g['bbox'][1]
        d = dict(g)
        d['name'] = DETECTED_AS.get(g['name'], g['name']) if rng.uniform() < 0.7 else g['name']
        if rng.uniform() < spec['p_wrong']:
            d['name'] = str(rng.choice(['Car', 'Pedestrian', 'Cyclist']))
        d['location'] = list(np.array(g['location']) + rng.normal(0, s, 3) * [1, 0.3, 1])
        d['dimensions'] = list(np.array(g['dimensions']) * (1 + rng.normal(0, s / 4, 3)))
        d['rotation_y'] = g['rotation_y'] + rng.normal(0, s / 2)
        d['alpha'] = g['alpha'] + rng.normal(0, s)
        d['bbox'] = list(np.array(g['bbox']) + rng.normal(0, s * hpx * 0.3, 4))
        if rng.uniform() < spec['p_low']:                                  # a box below the height limits: ignored, not wrong
            mid, low = (d['bbox'][1] + d['bbox'][3]) / 2, rng.uniform(10, 24)
            d['bbox'][1], d['bbox'][3] = mid - low / 2, mid + low / 2
        dts.append(d)
    dcs = [g for g in gts if g['name'] == 'DontCare']
    n_fp = int(rng.integers(0, spec['max_fp'] + 1)) if n_dt is None else max(n_dt - len(dts), 0)
    for i in range(n_fp):
        d = _object(rng, str(rng.choice(['Car', 'Pedestrian', 'Cyclist'])), True)
        if dcs and i % 2 == 0:
            x1, y1, x2, y2 = dcs[i // 2 % len(dcs)]['bbox']
            cx, cy = rng.uniform(x1 + 15, x2 - 15), (y1 + y2) / 2
            half = (y2 - y1) / 2 * rng.uniform(0.5, 0.9)             # hangs over the region's edge when it is narrow
            d['bbox'] = [cx - 14, cy - half, cx + 14, cy + half]
        dts.append(d)
    if n_dt is not None:
        dts = dts[:n_dt]
    return _anno(gts, False), _anno(dts, True)


def near_threshold(overlaps, margin=MARGIN):
    return any(np.any(np.abs(np.asarray(o, dtype=np.float64) - t) < margin) for o in overlaps for t in MIN_OVERLAPS)


def make_annos(seed, num_frames, spec, overlap_fn, forced=None, alpha_off=False):
    """forced: {frame: (n_gt, n_dt)}; overlap_fn(gt_anno, dt_anno) -> the frame's overlap matrices of the three metrics.
    alpha_off: every detection's alpha is -10 (the reference then leaves AOS out). -> gt_annos, dt_annos, frames drawn again"""
    gt_annos, dt_annos, again = [], [], 0
    for f in range(num_frames):
        attempt = 0
        while True:
            rng = np.random.default_rng([seed, f, attempt])
            g, d = draw_frame(rng, spec, *(forced or {}).get(f, (None, None)))
            n = len(d['name'])
            d['score'] = ((rng.permutation(20000)[:n] + 1) / 20001.0).astype(np.float32)
            if alpha_off:
                d['alpha'] = np.full(n, -10.0)
            if not near_threshold(overlap_fn(g, d)):
                break
            attempt += 1
            again += 1
        gt_annos.append(g)
        dt_annos.append(d)
    return gt_annos, dt_annos, again


def host_overlap_fn(g, d):
    from pcdet.datasets.kitti.kitti_object_eval_python import eval as kitti_eval
    return kitti_eval.host_overlaps(kitti_eval.pack_annos([g], [d]))[:3]


def pack(annos, with_score):
    """annos -> flat arrays for an .npz ('n' per frame + every key stacked)"""
    out = {'n': np.array([len(a['name']) for a in annos], dtype=np.int64)}
    e = empty_anno(with_score)
    for k in e:
        out[k] = np.concatenate([np.asarray(a[k], dtype=e[k].dtype).reshape((-1,) + e[k].shape[1:]) for a in annos], 0)
    return out


def unpack(z, prefix, with_score):
    n = z[prefix + 'n']
    off = np.concatenate([[0], np.cumsum(n)])
    return [{k: z[prefix + k][off[i]:off[i + 1]] for k in empty_anno(with_score)} for i in range(len(n))]
