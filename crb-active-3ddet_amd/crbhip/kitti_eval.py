"""KITTI AP on the device: binding of csrc/kitti_eval.hip (crb_kitti_* in include/crb_hip.h).

evaluate() uploads the packed annos of pcdet.datasets.kitti.kitti_object_eval_python.eval.pack_annos once, launches
overlaps -> ignore flags -> true-positive scores -> (torch.sort) -> thresholds -> precision / recall counts on the current stream and
reads back ONE buffer at the end: per (combination, threshold) the rows [tp, fp, fn, similarity, threshold] and the number of
thresholds per combination. The (class, difficulty, overlap, 41) tables of the three metrics are ratios of those exact integers and
are taken from them in f64 by the caller, the same way on both routes. detail=True reads the overlaps and the true-positive scores
back as well (tests, tools).

Host tensors are accepted only when the library has been replaced by a host build (tools/kitti_eval_host_check.py sets DEVICE)."""
import numpy as np
import torch

from ._lib import lib, check, ptr, cur_stream

N_SAMPLE_PTS = 41
DEVICE = None                # None: the current cuda device


def _dev():
    if DEVICE is not None:
        return torch.device(DEVICE)
    if not torch.cuda.is_available():
        from ._lib import CrbHipError
        raise CrbHipError('crbhip.kitti_eval needs a GPU: the HIP path has no CPU fallback (the evaluator has route="host")')
    return torch.device('cuda', torch.cuda.current_device())


def stage_limits():
    """(n_gt, n_dt, n_gt * n_dt) up to which crb_kitti_match_pr stages a frame in LDS"""
    return tuple(int(lib.crb_kitti_stage_limit(i)) for i in range(3))


class _Frames(object):
    """the packed annos on the device"""

    def __init__(self, p):
        dev = _dev()
        self.dev = dev
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dtype=dt).to(dev)
        self.F = int(p['num_frames'])
        self.G, self.D, self.P = int(p['gt_off'][-1]), int(p['dt_off'][-1]), int(p['pair_off'][-1])
        for k in ('gt_off', 'dt_off', 'pair_off'):
            setattr(self, k, up(p[k], torch.int64))
        for k in ('gt_bbox', 'dt_bbox', 'gt_cam', 'dt_cam', 'gt_alpha', 'dt_alpha', 'gt_occ', 'gt_trunc', 'dt_score'):
            setattr(self, k, up(p[k], torch.float64))
        self.gt_cls, self.dt_cls = up(p['gt_cls'], torch.int32), up(p['dt_cls'], torch.int32)
        self.gt_dc = up(p['gt_dc'], torch.uint8)
        nd, ng = np.diff(p['dt_off']), np.diff(p['gt_off'])
        words = (nd + 31) // 32
        lim = stage_limits()
        big = (ng > lim[0]) | (nd > lim[1]) | (ng * nd > lim[2])
        self.asg_words, self.big_words = int(words.sum()), int(words[big].sum())
        self.asg_off = up(np.concatenate([[0], np.cumsum(words)]), torch.int64)
        self.big_off = up(np.concatenate([[0], np.cumsum(np.where(big, words, 0))]), torch.int64)
        self.stream = cur_stream(dev) if dev.type == 'cuda' else None

    def overlaps(self):
        ov = torch.empty((4, self.P), dtype=torch.float64, device=self.dev)
        check(lib.crb_kitti_overlaps(ptr(self.gt_off), ptr(self.dt_off), ptr(self.pair_off), self.F, self.P, ptr(self.gt_bbox),
                                     ptr(self.dt_bbox), ptr(self.gt_cam), ptr(self.dt_cam), ptr(ov), self.stream), 'crb_kitti_overlaps')
        return ov


def overlaps(p):
    """-> (4, P) f64 device tensor: image IoU, BEV IoU, 3D IoU, image intersection over the detection's area; the pairs of frame f at
    p['pair_off'][f] as a row-major [n_dt, n_gt] matrix"""
    return _Frames(p).overlaps()


def evaluate(p, current_classes, min_overlaps, metrics, aos_flags, detail=False):
    """p: pack_annos(...); current_classes ints; min_overlaps (K, 3, C) f64; metrics list of 0..2; aos_flags per metric.
    -> {'thresholds' (M, C, 3, K, 41), 'num_thresholds' (M, C, 3, K), 'pr' (M, C, 3, K, 41, 4), 'num_valid_gt' (C, 3)} as numpy
    (+ 'overlaps' (4, P), 'tp_scores' {(mi, c, l, k): descending scores} with detail=True)"""
    fr = _Frames(p)
    dev, st = fr.dev, fr.stream
    M, C, K = len(metrics), len(current_classes), int(min_overlaps.shape[0])
    NC = M * C * 3 * K
    mi, c, l, k = [a.reshape(-1) for a in np.meshgrid(np.arange(M), np.arange(C), np.arange(3), np.arange(K), indexing='ij')]
    metric_of = np.asarray(metrics, dtype=np.int64)[mi]
    aos_slot = np.full(NC, -1, dtype=np.int64)
    with_aos = np.asarray(aos_flags, dtype=bool)[mi]
    aos_slot[with_aos] = np.arange(int(with_aos.sum()))
    num_aos = int(with_aos.sum())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    combo_metric, combo_flags, combo_aos = i32(metric_of), i32(c * 3 + l), i32(aos_slot)
    combo_min = torch.from_numpy(np.ascontiguousarray(min_overlaps[k, metric_of, c], dtype=np.float64)).to(dev)
    classes = i32(current_classes)

    ov = fr.overlaps()
    gt_flag = torch.empty((C * 3, fr.G), dtype=torch.int8, device=dev)
    dt_flag = torch.empty((C * 3, fr.D), dtype=torch.int8, device=dev)
    check(lib.crb_kitti_ignore_flags(ptr(fr.gt_cls), ptr(fr.gt_occ), ptr(fr.gt_trunc), ptr(fr.gt_bbox), fr.G, ptr(fr.dt_cls),
                                     ptr(fr.dt_bbox), fr.D, ptr(classes), C, ptr(gt_flag), ptr(dt_flag), st), 'crb_kitti_ignore_flags')
    num_valid = (gt_flag == 0).sum(dim=1).to(torch.int32)                          # (C * 3)
    tp_scores = torch.empty((NC, fr.G), dtype=torch.float64, device=dev)
    asg = torch.empty(max(fr.asg_words * NC, 1), dtype=torch.int32, device=dev)
    check(lib.crb_kitti_match_scores(ptr(fr.gt_off), ptr(fr.dt_off), ptr(fr.pair_off), ptr(fr.asg_off), fr.F, fr.G, fr.D, fr.P, ptr(ov),
                                     ptr(gt_flag), ptr(dt_flag), ptr(fr.dt_score), ptr(combo_metric), ptr(combo_flags), ptr(combo_min),
                                     NC, ptr(asg), ptr(tp_scores), st), 'crb_kitti_match_scores')
    sorted_scores = torch.sort(tp_scores, dim=1, descending=True).values.contiguous()
    num_scores = (tp_scores > float('-inf')).sum(dim=1).to(torch.int32)
    thresholds = torch.empty((NC, N_SAMPLE_PTS), dtype=torch.float64, device=dev)
    num_thresholds = torch.empty(NC, dtype=torch.int32, device=dev)
    combo_valid = num_valid[combo_flags.long()].contiguous()
    check(lib.crb_kitti_thresholds(ptr(sorted_scores), ptr(num_scores), ptr(combo_valid), NC, fr.G, ptr(thresholds),
                                   ptr(num_thresholds), st), 'crb_kitti_thresholds')
    asg_big = torch.empty(max(fr.big_words * NC * 64, 1), dtype=torch.int32, device=dev)
    counts = torch.empty((NC, N_SAMPLE_PTS, 3), dtype=torch.int32, device=dev)
    sim_part = torch.empty((max(fr.F * num_aos, 1), N_SAMPLE_PTS), dtype=torch.float64, device=dev)
    result = torch.empty(NC * N_SAMPLE_PTS * 5 + NC, dtype=torch.float64, device=dev)
    check(lib.crb_kitti_match_pr(ptr(fr.gt_off), ptr(fr.dt_off), ptr(fr.pair_off), ptr(fr.big_off), fr.F, fr.G, fr.D, fr.P, ptr(ov),
                                 ptr(gt_flag), ptr(dt_flag), ptr(fr.dt_score), ptr(fr.gt_dc), ptr(fr.gt_alpha), ptr(fr.dt_alpha),
                                 ptr(combo_metric), ptr(combo_flags), ptr(combo_min), ptr(combo_aos), NC, num_aos, ptr(thresholds),
                                 ptr(num_thresholds), ptr(asg_big), ptr(counts), ptr(sim_part), ptr(result), st), 'crb_kitti_match_pr')
    host = result.cpu().numpy()                                                    # the one read-back
    rows = host[:NC * N_SAMPLE_PTS * 5].reshape(M, C, 3, K, N_SAMPLE_PTS, 5)
    out = {'thresholds': rows[..., 4].copy(), 'pr': rows[..., :4].copy(),
           'num_thresholds': host[NC * N_SAMPLE_PTS * 5:].astype(np.int64).reshape(M, C, 3, K)}
    if detail:
        out['overlaps'] = ov.cpu().numpy()
        out['num_valid_gt'] = num_valid.cpu().numpy().astype(np.int64).reshape(C, 3)
        s, n = sorted_scores.cpu().numpy(), num_scores.cpu().numpy()
        out['tp_scores'] = {(int(mi[q]), int(c[q]), int(l[q]), int(k[q])): s[q, :n[q]] for q in range(NC)}
    return out
