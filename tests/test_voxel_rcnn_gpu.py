"""GPU: Voxel R-CNN. csrc/voxel_pool.hip (voxel query on the site hash, moments of the relative positions, fused pooling forward and
backward) against the numpy restatement, the f64 pooling definition and the torch route; VoxelRCNNHead against the golden written by
the reference's own head; VoxelRCNN training / eval steps on synthetic frames and the entropy strategy on it.

Bars. Query indices: exact (the case builder asserts the margins that make every correct f32 evaluation agree). Pooling forward:
max|fused - pool_f64| <= 4 * e_ref, e_ref = max|reference f32 - pool_f64| read from the golden (the folded affine A d + b sums in
another order than conv-then-BatchNorm). Backward and running statistics of mlps_pos: max|fused - torch route in f64 on this device|
<= 4 * e_ref of the same quantity, e_ref = max|reference f32 - reference f64| recorded alongside in the golden. Figures of the MI355X run: DESIGN.md
section 6."""
import warnings

import numpy as np
import pytest
import torch

import test_voxel_rcnn_cpu as cpu
import voxel_rcnn_cases as cases

pytestmark = pytest.mark.gpu
FACTOR = 4.0


class no_fallback(warnings.catch_warnings):
    """the HIP route must not announce the torch route"""
    def __enter__(self):
        r = super().__enter__()
        warnings.filterwarnings('error', message='.*torch route.*')
        return r


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope='module')
def level():
    out = {}
    for name in cases.LEVEL_CASES:
        p = cases.level_case(name)
        out[name] = (p, cases.case_query_inputs(p))
    return out


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _query(dev, p, q, coords, xyz=None):
    from crbhip import sparse, voxel_pool
    c = _t(coords, dev)
    hkeys, hvals, cap = sparse.build_hash(c, list(cases.SHAPE))
    idx, cnt = voxel_pool.voxel_query(_t(q[0] if xyz is None else xyz, dev), _t(q[1], dev), _t(q[2], dev), cases.B, cases.SHAPE, p['ranges'],
                                      p['radius'], p['nsample'], hkeys, hvals, cap)
    return idx.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize('name', list(cases.LEVEL_CASES))
def test_query_indices_equal_the_restatement(dev, gold, level, name):
    """idx and empty_ball_mask with no tolerance, rows in the case's own order (a: ascending (b,z,y,x); b: shuffled inside the
    frames) and in a full shuffle across the frames (the hash takes any row order; idx holds global rows)"""
    p, q = level[name]
    idx, cnt = _query(dev, p, q, p['coords'])
    np.testing.assert_array_equal(idx, gold['q_%s_idx' % name])
    np.testing.assert_array_equal(cnt == 0, gold['q_%s_empty' % name])
    want_cnt = np.array([0 if e else len(set(r.tolist())) for r, e in zip(gold['q_%s_idx' % name], gold['q_%s_empty' % name])])   # hits kept
    np.testing.assert_array_equal(cnt, want_cnt)
    perm = np.random.default_rng(7).permutation(len(p['coords']))
    idx2, cnt2 = _query(dev, p, q, p['coords'][perm], q[0][perm])
    np.testing.assert_array_equal(cnt2, cnt)
    np.testing.assert_array_equal(perm[idx2][cnt > 0], idx[cnt > 0])
    assert (idx2[cnt == 0] == 0).all()


def test_query_frame_index_out_of_range_is_an_empty_ball(dev, level):
    p, q = level['b']
    coords = q[2].copy()
    coords[:5, 0] = [-1, 2, 7, -100, 2 ** 20]
    idx, cnt = _query(dev, p, (q[0], q[1], coords), p['coords'])
    assert (cnt[:5] == 0).all() and (idx[:5] == 0).all() and cnt[5:].max() > 0


def test_boundary_grid_coordinates_equal_torch(dev):
    """grid points exactly on voxel faces (k * voxel_size + range minimum formed in f32), one ulp to either side and at negative
    coordinates: the head's integer coordinates are torch's two-step float `//` on this device, for every stride. The two steps are
    kept as torch ops in the head, so this comparison holds by construction and guards against a later edit of the head (a kernel
    with floorf(a / b), say); the independent part is the check away from the faces against the floor of the f64 quotient.
    test_boundary_points_through_the_query hands such coordinates on to crb_voxel_query."""
    head = cpu.make_head().to(dev)
    lo, vs = np.asarray(cases.HEAD_PCR[:3], np.float32), np.asarray(cases.VOXEL, np.float32)
    k = np.arange(-40, 200, dtype=np.float32)[:, None]
    face = (k * vs + lo).astype(np.float32)
    pts = np.concatenate([face, np.nextafter(face, np.float32(1e9)), np.nextafter(face, np.float32(-1e9)),
                          (np.random.default_rng(3).uniform(-45, 205, (500, 3)) * vs + lo).astype(np.float32)])
    xyz = _t(pts, dev).view(1, -1, 3)
    got = head.grid_voxel_coords(xyz)
    bidx = torch.zeros_like(xyz[..., :1])
    for stride in (1, 2, 4, 8):
        want = torch.cat([bidx] + [((xyz[:, :, a:a + 1] - cases.HEAD_PCR[a]) // cases.VOXEL[a]) // stride for a in range(3)], dim=-1).int()
        lvl = head.level_coords(got, bidx, stride)
        assert lvl.dtype == torch.int32 and torch.equal(lvl, want)
        q = (pts.astype(np.float64) - lo.astype(np.float64)) / vs.astype(np.float64)
        away = np.abs(q - np.round(q)) > 1e-4
        f64 = np.floor(np.floor(q) / stride).astype(np.int64)
        assert np.array_equal(lvl[0, :, 1:].cpu().numpy()[away], f64[away])
    assert int(lvl[0, :, 1:].min()) < 0


def test_boundary_points_through_the_query(dev, level):
    """grid points on and next to voxel faces, negative coordinates among them: integer coordinates formed on the device by the
    head's two float steps as [b, x, y, z], re-ordered as the module re-orders them, through crb_voxel_query; equal to the restatement
    on the same integers (the radius is off every distance these lattice-aligned points have to a voxel centre)"""
    from crbhip import sparse, voxel_pool
    p, _ = level['b']
    s, pcr = p['stride'], p['pcr']
    lo, vs = np.asarray(pcr[:3], np.float32), np.asarray(cases.VOXEL, np.float32) * s
    k = np.stack(np.meshgrid(np.arange(-3, 6), np.arange(-2, 5), np.arange(-1, 4), indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    face = (k * vs + lo).astype(np.float32)
    pts = np.concatenate([face, np.nextafter(face, np.float32(1e9)), np.nextafter(face, np.float32(-1e9))])
    pts = np.concatenate([pts, pts])                                  # both frames
    b = np.repeat(np.arange(2, dtype=np.float32), len(pts) // 2)[:, None]
    xyz_d = _t(pts, dev)
    steps = torch.cat([_t(b, dev)] + [((xyz_d[:, a:a + 1] - pcr[a]) // cases.VOXEL[a]) // s for a in range(3)], dim=-1).int()
    bzyx = torch.cat([steps[:, :1], steps[:, 1:].flip(1)], dim=1).contiguous()
    assert int(bzyx[:, 1:].min()) < 0
    radius = float(np.float32(1.37 * p['radius'] / 1.6))
    centres = cases.voxel_centers(p['coords'][:, 1:4], s, pcr)
    d2 = ((centres[None].astype(np.float64) - pts[:, None].astype(np.float64)) ** 2).sum(-1)
    assert np.abs(d2 - float(np.float32(radius)) ** 2).min() > 1e-5 * radius ** 2
    c = _t(p['coords'], dev)
    hkeys, hvals, cap = sparse.build_hash(c, list(cases.SHAPE))
    idx, cnt = voxel_pool.voxel_query(_t(centres, dev), xyz_d, bzyx, cases.B, cases.SHAPE, p['ranges'], radius, p['nsample'], hkeys, hvals, cap)
    want_idx, want_empty = cases.voxel_query_np(p['ranges'], radius, p['nsample'], centres, pts, bzyx.cpu().numpy(), cases.dense_index(p['coords']))
    np.testing.assert_array_equal(idx.cpu().numpy(), want_idx)
    np.testing.assert_array_equal(cnt.cpu().numpy() == 0, want_empty)
    assert want_empty.any() and not want_empty.all()


def _fused_pool(dev, p, q, pool, training, mod=None):
    """the fused pooling body of a module on its own mlps_in output -> pooled (M,C), features_in, the module"""
    import spconv.pytorch as spconv
    mod = (mod or cpu.make_module(p, pool)).to(dev).train(training)
    coords = _t(p['coords'], dev)
    sp = spconv.SparseConvTensor(torch.zeros((len(coords), 1), device=dev), coords, list(cases.SHAPE), cases.B)
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import _rows
    with torch.no_grad():
        fin = _rows(mod.mlps_in[0], _t(p['feats'], dev))
    assert mod.fused_route(0, fin, sp) is None
    pooled = mod._pool_fused(0, fin, _t(q[0], dev), _t(q[1], dev), _t(q[2], dev), sp)
    return pooled, fin, mod


@pytest.mark.parametrize('name', list(cases.LEVEL_CASES))
@pytest.mark.parametrize('pool', cases.POOLS)
@pytest.mark.parametrize('training', [True, False])
def test_pool_forward_against_the_f64_definition(dev, gold, level, name, pool, training):
    p, q = level[name]
    tag = 'm_%s_%s_%s' % (name, pool, 'train' if training else 'eval')
    ref_mod = cpu.make_module(p, pool)
    bn = ref_mod.mlps_pos[0][1]
    stats = {} if training else {'mean': bn.running_mean.numpy().copy(), 'var': bn.running_var.numpy().copy()}
    with torch.no_grad():
        pooled, fin, mod = _fused_pool(dev, p, q, pool, training)
    idx, empty = gold['q_%s_idx' % name], gold['q_%s_empty' % name]
    f64, _, bm, bv = cases.pool_f64(fin.cpu().numpy(), q[0], q[1], idx, empty, ref_mod.mlps_pos[0][0].weight.detach().numpy(),
                                    bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.eps, pool, **stats)
    e_ref = float(gold[tag + '_pooled_e_ref'][0])
    err = float(np.abs(pooled.cpu().numpy().astype(np.float64) - f64).max())
    print('%s: fused pooling error %.3g against f64, e_ref %.3g, ratio %.2f (bar %.0f)' % (tag, err, e_ref, err / e_ref, FACTOR))
    assert pooled.shape == (len(q[1]), p['c']) and err <= FACTOR * e_ref
    # the quirk: an empty ball yields relu(b), b the folded BatchNorm's bias, not zero
    m_, v_ = (bm, bv) if training else (stats['mean'], stats['var'])
    relu_b = np.maximum(bn.bias.detach().numpy() - bn.weight.detach().numpy() * m_ / np.sqrt(v_ + bn.eps), 0)
    rows = pooled.cpu().numpy()[empty]
    assert empty.any() and np.abs(rows - relu_b).max() <= FACTOR * e_ref and relu_b.max() > 1e-2
    if training:
        n = idx.size
        got_bn = mod.mlps_pos[0][1]
        mom = got_bn.momentum
        want_mean = (1 - mom) * bn.running_mean.numpy() + mom * bm
        want_var = (1 - mom) * bn.running_var.numpy() + mom * bv * n / (n - 1)
        for key, got, want in (('running_mean', got_bn.running_mean, want_mean), ('running_var', got_bn.running_var, want_var)):
            e = float(gold['%s_e_ref_buf/mlps_pos.0.1.%s' % (tag, key)][0])
            d = float(np.abs(got.cpu().numpy() - want).max())
            print('  %s: %.3g against f64 (e_ref %.3g)' % (key, d, e))
            assert d <= FACTOR * e
        assert int(got_bn.num_batches_tracked) == 1


NAMED = ('grad/features', 'grad/mlps_pos.0.0.weight', 'grad/mlps_pos.0.1.weight', 'grad/mlps_pos.0.1.bias',
         'buf/mlps_pos.0.1.running_mean', 'buf/mlps_pos.0.1.running_var')


@pytest.mark.parametrize('name', list(cases.LEVEL_CASES))
@pytest.mark.parametrize('pool', cases.POOLS)
@pytest.mark.parametrize('training', [True, False])
def test_module_step_against_the_torch_route(dev, gold, level, name, pool, training):
    """forward + backward of the whole module on the HIP route (handed the sparse tensor) against the torch route (handed the dense
    index) on the same device, in training mode (batch statistics from the moments, running statistics updated) and in eval mode
    (mlps_pos folded from its running statistics with autograd into W, gamma, beta: the frozen-BatchNorm fine-tuning path). The
    torch route runs in f64, so that the bar measures the HIP route's error alone, as the forward's does: d features_in, dW / dgamma /
    dbeta of mlps_pos and (training) its running statistics within FACTOR * e_ref, e_ref = the reference's own f32 error of the same
    quantity against its f64 run (golden). The other gradients and statistics pass through plain torch layers on both routes: they
    are printed, and everything is held against the golden at the ordinary f32 agreement."""
    p, q = level[name]
    tag = 'm_%s_%s_%s' % (name, pool, 'train' if training else 'eval')
    with no_fallback():
        fused = cpu.run_module(cpu.make_module(p, pool).to(dev), p, cpu.module_inputs(p, q, dev=dev, sparse=True), training)
    ref = cpu.run_module(cpu.make_module(p, pool).double().to(dev), p, cpu.module_inputs(p, q, dev=dev, dtype=torch.float64), training)
    torch.cuda.synchronize()
    assert cpu.assert_matches_golden(gold, tag, fused) == (20 if training else 11)
    bad, seen = [], 0
    for key in ref:
        a, b = fused[key], ref[key]
        if not a.dtype.is_floating_point:
            assert torch.equal(a, b), key
            continue
        e_ref = float(gold['%s_e_ref_%s' % (tag, key)][0])
        err = float((a.double() - b).abs().max())
        print('%s %-32s |fused - torch route f64| %.3g, e_ref %.3g, ratio %.2f%s' % (tag, key, err, e_ref, err / e_ref,
                                                                                     ' (asserted)' if key in NAMED else ''))
        seen += key in NAMED
        if key in NAMED and err > FACTOR * e_ref:
            bad.append((key, err, e_ref))
    assert seen == (6 if training else 4) and not bad, bad


def test_backward_compact_route_equals_the_atomic_route(dev, level):
    """the deterministic scatter (selected row + gradient through index_add_) against the atomic scatter: same gradient up to the
    summation order, bit-identical from call to call"""
    p, q = level['a']
    grads = {}
    for det in (False, True, True):
        torch.use_deterministic_algorithms(det)
        try:
            _, fin, mod = _fused_pool(dev, p, q, 'max_pool', True)
            fin = fin.clone().requires_grad_(True)
            import spconv.pytorch as spconv
            sp = spconv.SparseConvTensor(torch.zeros((len(p['coords']), 1), device=dev), _t(p['coords'], dev), list(cases.SHAPE), cases.B)
            out = mod._pool_fused(0, fin, _t(q[0], dev), _t(q[1], dev), _t(q[2], dev), sp)
            w = _t(cpu.out_weights(p, tuple(out.shape)).astype(np.float32), dev)
            (out * w).sum().backward()
        finally:
            torch.use_deterministic_algorithms(False)
        grads.setdefault(det, []).append(fin.grad.clone())
    scale = float(grads[False][0].abs().max())
    assert float((grads[True][0] - grads[False][0]).abs().max()) <= 1e-5 * scale
    assert torch.equal(grads[True][0], grads[True][1])


def test_unsupported_width_takes_the_torch_route_and_says_so(dev, level):
    p, q = level['b']
    p = dict(p, c=48)
    mods = [cpu.make_module(p, 'max_pool').to(dev).train() for _ in range(2)]
    with pytest.warns(UserWarning, match='torch route'):
        a = mods[0](**cpu.module_inputs(p, q, dev=dev, sparse=True))
    b = mods[1](**cpu.module_inputs(p, q, dev=dev, sparse=False))
    assert a.shape == (len(q[1]), p['c_out']) and torch.isfinite(a).all()
    assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_kernel_argument_checks(dev, level):
    import crbhip
    from crbhip import sparse, voxel_pool
    p, q = level['b']
    c = _t(p['coords'], dev)
    hkeys, hvals, cap = sparse.build_hash(c, list(cases.SHAPE))
    args = (_t(q[0], dev), _t(q[1], dev), _t(q[2], dev), cases.B, cases.SHAPE)
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_UNSUPPORTED'):
        voxel_pool.voxel_query(*args, [1, 2, 5], p['radius'], 5, hkeys, hvals, cap)
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_UNSUPPORTED'):
        voxel_pool.voxel_query(*args, [1, 2, 4], p['radius'], 33, hkeys, hvals, cap)
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_ARG'):
        voxel_pool.voxel_query(*args, [1, 2, 4], p['radius'], 5, hkeys, hvals, cap - 1)
    idx, cnt = voxel_pool.voxel_query(*args, p['ranges'], p['radius'], p['nsample'], hkeys, hvals, cap)
    f = torch.zeros((len(p['coords']), 48), device=dev)
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_UNSUPPORTED'):
        voxel_pool.voxel_pool(f, torch.zeros(48, 3, device=dev), torch.zeros(48, device=dev), args[0], args[1], idx, cnt, 'max_pool')


# ---- head and detector ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dp', [('dp0', 0.0), ('dp3', 0.3)])
def test_head_eval_matches_the_reference(dev, gold, tag, dp):
    head = cpu.make_head(dp).to(dev).eval()
    with torch.no_grad(), no_fallback():
        bd = head(cpu.head_batch(dev))
    np.testing.assert_allclose(bd['batch_cls_preds'].cpu().numpy(), gold['head_eval_cls_' + tag], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(bd['batch_box_preds'].cpu().numpy(), gold['head_eval_box_' + tag], rtol=1e-4, atol=1e-5)


def test_head_train_step_matches_the_reference(dev, gold):
    with no_fallback():
        head = cpu.head_train_step(dev)
    cpu.check_head_train_step(gold, head)


def test_head_training_step_is_reproducible_under_deterministic_algorithms(dev):
    """two identical training steps of the head under torch.use_deterministic_algorithms(True): bit-identical loss and gradients"""
    runs = []
    torch.use_deterministic_algorithms(True)
    try:
        for _ in range(2):
            with no_fallback():                                    # the max_pool level stays on the HIP route ...
                warnings.filterwarnings('ignore', message='.*avg_pool under deterministic.*')    # ... the avg_pool level says it does not
                head = cpu.head_train_step(dev)
            loss, _ = head.get_loss()
            head.zero_grad()
            loss.backward()
            runs.append((loss.detach().clone(), {n: t.grad.clone() for n, t in head.named_parameters()}))
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.isfinite(runs[0][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


POINTS = 8000


def _detector(dev, dp_ratio=0.3):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import voxel_rcnn_cfg
    from pcdet.models import build_network
    cfg = voxel_rcnn_cfg()
    cfg.MODEL.ROI_HEAD.DP_RATIO = dp_ratio
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 1, SyntheticDataset(num_frames=2, n_points=POINTS, class_names=cfg.CLASS_NAMES))
    return cfg, model.to(dev)


def _det_batch(dev):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, gt = kitti_batch(40, 2, POINTS)
    gt = gt.copy()
    gt[..., 7] = (gt[..., 3] > 0)                                    # one class: every box is a Car
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    return {'points': _t(np.concatenate([bidx[:, None], pts], 1), dev), 'point_frame_offsets': _t(off, dev), 'batch_size': 2,
            'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': _t(gt, dev), 'frame_id': np.array(['000040', '000041'])}


def test_detector_training_step(dev):
    _, model = _detector(dev)
    model.train()
    with no_fallback():
        ret, tb, _ = model(_det_batch(dev))
    loss = ret['loss']
    model.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for k in ('rpn_loss', 'rcnn_loss', 'rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner'):
        assert k in tb and isinstance(tb[k], torch.Tensor) and not tb[k].requires_grad, k
    np.testing.assert_allclose(float(loss), float(tb['rpn_loss']) + float(tb['rcnn_loss']), rtol=1e-6)
    missing = [n for n, t in model.named_parameters() if t.grad is None or not torch.isfinite(t.grad).all()]
    assert not missing, missing
    pos = [m for lay in model.roi_head.roi_grid_pool_layers for m in lay.mlps_pos]
    assert len(pos) == 3 and all(int(m[1].num_batches_tracked) == 1 for m in pos)


def test_detector_eval_pass_returns_the_pred_dict_contract(dev):
    cfg, model = _detector(dev)
    cfg.MODEL.POST_PROCESSING.SCORE_THRESH = 0.0                       # (random weights: keep whatever the NMS keeps)
    model.eval()
    with torch.no_grad():
        pred, recall = model(_det_batch(dev))
    assert len(pred) == 2 and any(len(p['pred_scores']) > 0 for p in pred)
    for p in pred:
        assert set(p.keys()) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_logits'}
        n = len(p['pred_scores'])
        assert p['pred_boxes'].shape == (n, 7) and p['pred_labels'].shape == (n,) and p['pred_logits'].shape == (n, 1)
        assert bool((p['pred_labels'] == 1).all()) and bool(((p['pred_scores'] >= 0) & (p['pred_scores'] <= 1)).all())
    assert 'gt' in recall and all(('roi_%s' % t) in recall and ('rcnn_%s' % t) in recall for t in (0.3, 0.5, 0.7))


def test_entropy_strategy_selects_frames(dev):
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.query_strategies import build_strategy
    cfg, model = _detector(dev)
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': 'entropy', 'AGGREGATION': 'mean', 'SELECT_NUMS': 3})
    pool = SyntheticDataset(num_frames=8, first_frame=300, n_points=POINTS, class_names=cfg.CLASS_NAMES)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=POINTS, class_names=cfg.CLASS_NAMES)
    strat = build_strategy('entropy', model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 4), 0, '/tmp', cfg)
    picked = strat.query(cur_epoch=0)
    assert len(picked) == 3 and len(set(picked)) == 3 and set(picked) <= set(pool.sample_id_list), picked


# ---- memory ---------------------------------------------------------------------------------------------------------------
def test_fused_route_builds_no_dense_index_and_no_grouped_tensor(dev):
    """B = 2, R = 128, G = 6, C = 32, nsample = 16 (M = 55,296) on the KITTI x_conv2 level shape (21, 800, 704): the peak-allocation
    increase across one NeighborVoxelSAModuleMSG forward + backward stays below M * C * nsample * 4 bytes (one grouped tensor, 113 MB)
    and below B * Z * Y * X * 4 bytes (the dense index, 94.6 MB)"""
    import spconv.pytorch as spconv
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    B, R, G, C, ns = 2, 128, 6, 32, 16
    Z, Y, X = 21, 800, 704
    stride, n_vox = 2, 15000
    rng = np.random.default_rng(11)
    pcr = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
    rois = np.stack([rng.uniform(5, 65, (B, R)), rng.uniform(-35, 35, (B, R)), rng.uniform(-1.6, -0.4, (B, R)), rng.uniform(3.2, 4.4, (B, R)),
                     rng.uniform(1.4, 1.9, (B, R)), rng.uniform(1.4, 1.8, (B, R)), rng.uniform(-3.1, 3.1, (B, R))], -1).astype(np.float32)
    new_xyz = cases.grid_points(rois.reshape(-1, 7), G).reshape(-1, 3)
    coords = []
    for b in range(B):                                               # voxels around the grid points, so that the balls are not empty
        pick = new_xyz[b * R * G ** 3:(b + 1) * R * G ** 3][rng.integers(0, R * G ** 3, n_vox)] + rng.normal(0, 0.15, (n_vox, 3))
        c = np.floor((pick - np.array(pcr[:3])) / (np.array(cases.VOXEL) * stride)).astype(np.int64)[:, ::-1]
        c = np.unique(c[(c >= 0).all(1) & (c < [Z, Y, X]).all(1)], axis=0)
        coords.append(np.concatenate([np.full((len(c), 1), b), c], 1))
    coords = np.concatenate(coords).astype(np.int32)
    M = B * R * G ** 3
    grid = np.floor(np.floor((new_xyz - np.array(pcr[:3], np.float32)) / np.array(cases.VOXEL, np.float32)) / stride)
    new_coords = np.concatenate([np.repeat(np.arange(B), R * G ** 3)[:, None], grid], 1).astype(np.int32)        # [b, x, y, z]
    torch.manual_seed(0)
    mod = NeighborVoxelSAModuleMSG(query_ranges=[[4, 4, 4]], radii=[0.4], nsamples=[ns], mlps=[[C, C, C]], pool_method='max_pool').to(dev).train()
    c_dev = _t(coords, dev)
    sp = spconv.SparseConvTensor(torch.zeros((len(coords), 1), device=dev), c_dev, [Z, Y, X], B)
    kw = dict(xyz=_t(cases.voxel_centers(coords[:, 1:4], stride, pcr), dev), xyz_batch_cnt=_t(np.bincount(coords[:, 0], minlength=B).astype(np.int32), dev),
              new_xyz=_t(new_xyz, dev), new_xyz_batch_cnt=torch.full((B,), R * G ** 3, dtype=torch.int32, device=dev),
              new_coords=_t(new_coords, dev), features=torch.randn(len(coords), C, device=dev).requires_grad_(True), voxel2point_indices=sp)
    with no_fallback():
        mod(**kw).sum().backward()                                   # warm-up: library workspaces, allocator pools
        mod.zero_grad()
        kw['features'].grad = None
        sp._crb_site_hash = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        out = mod(**kw)
        out.sum().backward()
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    grouped, dense = M * C * ns * 4, B * Z * Y * X * 4
    print('M = %d, N = %d: peak allocation increase %.1f MB; one grouped tensor %.1f MB, the dense index %.1f MB' % (
        M, len(coords), peak / 2 ** 20, grouped / 2 ** 20, dense / 2 ** 20))
    assert M == 55296 and out.shape == (M, C) and float(out.abs().max()) > 0
    assert peak < grouped and peak < dense
