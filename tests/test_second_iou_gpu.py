"""GPU: SECOND-IoU. csrc/roi_bev_pool.hip against the f64 definition with the reference's own f32 error as the yardstick, the IoU loss
kernel of csrc/rcnn_loss.hip against the torch expression, SECONDNetIoU against the detector golden written by the reference
(tests/golden/make_goldens_second_iou.py), the entropy / random strategies on it, and a checkpoint round trip.

Pool bound: max|kernel - pool_f64| <= 2 * e_ref, e_ref = max|reference f32 - pool_f64| read from the golden (kernel and reference
each form the sampling coordinate with a handful of differently ordered roundings on values up to W; nothing else differs)."""
import io

import numpy as np
import pytest
import torch

import second_iou_cases as cases
from golden._constants import pv_seeded_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def _pool(bev, rois, G, geo=None):
    from crbhip import roi_bev_pool
    return roi_bev_pool.as_nchw(roi_bev_pool.roi_bev_pool(bev, rois, G, *(geo or cases.pool_geometry())), G)


@pytest.mark.parametrize('G', cases.POOL_GRIDS)
@pytest.mark.parametrize('stride', [7, 9])
def test_pool_against_the_reference(dev, gold, G, stride):
    rois = gold['pool_rois'] if stride == 7 else np.concatenate([gold['pool_rois'], gold['pool_rois_extra']], -1)
    got = _pool(torch.from_numpy(gold['pool_bev']).to(dev), torch.from_numpy(rois).to(dev), G)
    assert got.shape == (cases.POOL_B * cases.POOL_R, cases.POOL_C, G, G)
    got = got.cpu().numpy()
    e_ref = float(gold['pool_e_ref_g%d' % G][0])
    err = float(np.abs(got.astype(np.float64) - gold['pool_f64_g%d' % G]).max())
    print('pool G=%d stride %d: kernel error %.3g against f64, e_ref %.3g' % (G, stride, err, e_ref))
    assert err <= 2 * e_ref
    # padding and exclusion: the RoI off the map gives exact zeros, the all-zero padding row is pooled like any other row
    R = cases.POOL_R
    for b in range(cases.POOL_B):
        assert np.all(got[b * R + cases.ROW_OUTSIDE] == 0)
        pad, want = got[b * R + cases.ROW_PADDING], gold['pool_ref_g%d' % G][b * R + cases.ROW_PADDING]
        assert np.abs(pad).max() > 1e-2 and float(np.abs(pad - want).max()) <= 2 * e_ref


@pytest.mark.parametrize('C', [4, 132, 512])
def test_pool_channel_and_layout_tails(dev, gold, C):
    """R = 3 (fewer RoIs than any tile), one / 33 / 128 channel quads, against the torch path on the same device tensors; the
    logical (B*R, C, G, G) view indexes channel c, grid row j, grid column i"""
    from pcdet.models.roi_heads.second_head import roi_grid_pool_torch
    rng = np.random.default_rng(C)
    G, B, R = 7, cases.POOL_B, 3
    bev = torch.from_numpy(rng.normal(0, 1, (B, cases.POOL_H, cases.POOL_W, C)).astype(np.float32)).to(dev)
    rois = torch.from_numpy(gold['pool_rois'][:, [0, 5, cases.ROW_BIG_ANGLE]]).to(dev)
    got = _pool(bev, rois, G)
    ref = roi_grid_pool_torch(bev.permute(0, 3, 1, 2), rois, G, *cases.pool_geometry())
    assert got.shape == ref.shape == (B * R, C, G, G)
    e_ref = float(gold['pool_e_ref_g7'][0])
    err = float((got - ref).abs().max())
    print('pool C=%d: kernel against the torch path on the device %.3g (bound %.3g)' % (C, err, 2 * e_ref))
    assert err <= 2 * e_ref
    f64 = cases.pool_f64(bev.cpu().numpy(), rois.cpu().numpy(), G, *cases.pool_geometry())
    for n, c, j, i in ((0, 0, 0, 0), (B * R - 1, C - 1, G - 1, 0), (2, C // 2, 1, 5), (4, 3, 6, 2)):
        assert abs(float(got[n, c, j, i]) - f64[n, c, j, i]) <= 2 * e_ref


def test_pool_is_bit_reproducible(dev, gold):
    bev, rois = torch.from_numpy(gold['pool_bev']).to(dev), torch.from_numpy(gold['pool_rois']).to(dev)
    assert torch.equal(_pool(bev, rois, 7), _pool(bev, rois, 7))


def test_pool_argument_checks(dev, gold):
    import crbhip
    from crbhip import roi_bev_pool
    bev, rois = torch.from_numpy(gold['pool_bev']).to(dev), torch.from_numpy(gold['pool_rois']).to(dev)
    geo = cases.pool_geometry()
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_ARG'):
        roi_bev_pool.roi_bev_pool(bev[..., :6].contiguous(), rois, 7, *geo)           # C = 6
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_ARG'):
        roi_bev_pool.roi_bev_pool(bev, rois, 0, *geo)                                 # G = 0
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_ARG'):
        roi_bev_pool.roi_bev_pool(bev, rois, 7, geo[0], geo[1], 0.0, geo[3])          # a cell of no size
    with pytest.raises(crbhip.CrbHipError, match='CRB_ERR_UNSUPPORTED'):
        roi_bev_pool.roi_bev_pool(bev, rois, 17, *geo)
    with pytest.raises(crbhip.CrbHipError):
        roi_bev_pool.roi_bev_pool(bev.cpu(), rois.cpu(), 7, *geo)                     # host tensors: no fall-back
    torch.cuda.synchronize()


def _iou_loss_torch(x, y, kind, weight):
    from pcdet.utils import loss_utils
    if kind == 'BinaryCrossEntropy':
        l = torch.nn.functional.binary_cross_entropy_with_logits(x, y, reduction='none')
    elif kind == 'L2':
        l = torch.nn.functional.mse_loss(x, y, reduction='none')
    else:
        l = loss_utils.WeightedSmoothL1Loss.smooth_l1_loss(x - y, 1.0 / 9.0)
    valid = (y >= 0).float()
    return (l * valid).sum() / torch.clamp(valid.sum(), min=1.0) * weight


@pytest.mark.parametrize('kind', cases.LOSS_KINDS)
@pytest.mark.parametrize('n,ignored', [(2048, 'some'), (77, 'some'), (1500, 'none'), (130, 'all')])
def test_iou_loss_kernel(dev, kind, n, ignored):
    """crb_rcnn_iou_loss against the torch expression and its autograd: loss 2e-6 relative, gradient 2e-5 of the largest entry
    (the bars of crb_rcnn_loss); rows with the label -1, no ignored row, and the all-ignored batch; bit-equal re-runs"""
    import crbhip
    from crbhip import rcnn_loss
    rng = np.random.default_rng(n)
    x = torch.from_numpy(rng.normal(0, 2, (n, 1)).astype(np.float32)).to(dev)
    x[::9] = 40.0
    x[1::9] = -40.0
    y = torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32)).to(dev)
    y[::4], y[1::4] = 0.0, 1.0
    if ignored == 'some':
        y[2::5] = -1.0
    elif ignored == 'all':
        y[:] = -1.0
    weight = 1.3
    xa = x.clone().requires_grad_(True)
    want = _iou_loss_torch(xa.view(-1), y, kind, weight)
    (want * 1.7).backward()
    xb = x.clone().requires_grad_(True)
    got, valid = rcnn_loss.rcnn_iou_loss(xb, y, kind, weight)
    (got * 1.7).backward()
    assert int(valid) == int((y >= 0).sum())
    assert abs(float(got) - float(want)) <= 2e-6 * max(1.0, abs(float(want))), (float(got), float(want))
    scale = max(float(xa.grad.abs().max()), 1e-12)
    assert xb.grad.shape == x.shape and float((xb.grad - xa.grad).abs().max()) <= 2e-5 * scale
    if ignored == 'all':
        assert float(got) == 0.0 and float(xb.grad.abs().max()) == 0.0
    again, _ = rcnn_loss.rcnn_iou_loss(x, y, kind, weight)
    assert torch.equal(again, got.detach())
    with pytest.raises(crbhip.CrbHipError):
        rcnn_loss.rcnn_iou_loss(x, y, 'focalbce', weight)


def _detector(dev, dp_ratio=0.0, seeded=True):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_iou_cfg
    from pcdet.models import build_network
    cfg = second_iou_cfg()
    cfg.MODEL.ROI_HEAD.DP_RATIO = dp_ratio
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, n_points=cases.DET_POINTS))
    if seeded:
        model.load_state_dict(pv_seeded_state(model))
    return cfg, model.to(dev)


def _det_batch(dev, gold):
    from pcdet.datasets.synthetic import kitti_batch
    pts, off, _ = kitti_batch(cases.DET_FIRST_FRAME, 2, cases.DET_POINTS)
    bidx = np.repeat(np.arange(2, dtype=np.float32), np.diff(off))
    return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev), 'point_frame_offsets': torch.from_numpy(off).to(dev),
            'batch_size': 2, 'point_frame_counts_host': np.diff(off).tolist(), 'gt_boxes': torch.from_numpy(gold['det_gt']).to(dev),
            'frame_id': np.array(['%06d' % (cases.DET_FIRST_FRAME + i) for i in range(2)])}


def test_train_step_matches_the_reference_detector(dev, gold):
    """ONE training step of SECONDNetIoU against the reference's own SECONDNetIoU (second_iou.yaml, DP_RATIO 0; CPU, spconv answered
    by the oracle): same seeded weights by parameter name, same two synthetic frames, the reference's recorded RoI-sampler picks
    injected as boxes. First-stage proposals 1e-5 of their largest coordinate, losses and tb_dict entries 1e-5 relative; pooled
    features 3e-4 of the largest entry (the maps themselves differ by the backbones' f32 rounding, so the pool's own bar does not
    apply), second-stage logits 2e-3 of their largest magnitude and parameter gradients 2e-2 of their largest entry: the bars of
    tests/test_pvrcnn_gpu.py for the same quantities."""
    _, model = _detector(dev)
    assert sorted(model.state_dict().keys()) == [str(k) for k in gold['det_keys']]
    model.train()
    ref_sampled = np.take_along_axis(gold['det_proposals'], gold['det_sampled'][:, :, None], axis=1)
    model.roi_head.proposal_target_layer.injected_rois = torch.from_numpy(ref_sampled)
    inter = {}
    head = model.roi_head
    orig_pl, orig_pool = head.proposal_layer, head.roi_grid_pool

    def pl(bd, nms_config):
        t = orig_pl(bd, nms_config=nms_config)
        inter['proposals'] = bd['rois'].detach().clone()
        return t

    def pool(bd):
        inter['pooled'] = orig_pool(bd)
        return inter['pooled']
    head.proposal_layer, head.roi_grid_pool = pl, pool
    ret, tb, _ = model(_det_batch(dev, gold))
    head.proposal_layer, head.roi_grid_pool = orig_pl, orig_pool
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    torch.cuda.synchronize()
    pr, want_pr = inter['proposals'].cpu().numpy(), gold['det_proposals']
    tol = 1e-5 * float(np.abs(want_pr).max())
    for f in range(2):
        dist = np.abs(pr[f][:, None, :] - want_pr[f][None, :, :]).max(-1)          # as a set per frame: equal scores have no order
        print('frame %d proposals: %.3g / %.3g (bound %.3g)' % (f, dist.min(0).max(), dist.min(1).max(), tol))
        assert dist.min(0).max() <= tol and dist.min(1).max() <= tol
    np.testing.assert_allclose(head.forward_ret_dict['rois'].cpu().numpy(), gold['det_rois'], rtol=0, atol=tol)
    _rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    e = _rel(inter['pooled'].cpu().numpy()[cases.DET_POOLED], gold['det_pooled'])
    print('pooled features: %.3g of the largest entry' % e)
    assert e <= 3e-4
    print('loss %.7g (reference %.7g)' % (float(ret['loss']), float(gold['det_loss'][0])))
    for k, want in zip(gold['det_tb_keys'], gold['det_tb_vals']):
        print('  %-14s %.7g (reference %.7g)' % (k, float(tb[str(k)]), want))
    assert sorted(tb.keys()) == [str(k) for k in gold['det_tb_keys']]
    np.testing.assert_allclose(float(ret['loss']), float(gold['det_loss'][0]), rtol=1e-5)
    for k, want in zip(gold['det_tb_keys'], gold['det_tb_vals']):
        np.testing.assert_allclose(float(tb[str(k)]), want, rtol=1e-5, err_msg=str(k))
    np.testing.assert_allclose(head.forward_ret_dict['rcnn_cls_labels'].cpu().numpy(), gold['det_rcnn_labels'], rtol=0, atol=1e-4)
    got, want = head.forward_ret_dict['rcnn_iou'].detach().cpu().numpy(), gold['det_rcnn_iou']
    assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max(), (np.abs(got - want).max(), np.abs(want).max())
    params = dict(model.named_parameters())
    for n, sl in cases.DET_GRADS.items():
        got, want = params[n].grad.cpu().numpy()[sl], gold['det_grad/' + n]
        err = float(np.abs(got - want).max()) / float(gold['det_gradmax/' + n][0])
        print('%-48s gradient error %.2e of its largest entry' % (n, err))
        assert err <= 2e-2, (n, err)


@pytest.mark.parametrize('tag', ['iou', 'weighted'])
def test_eval_pass_matches_the_reference_detector(dev, gold, tag):
    from pcdet.config import EasyDict
    cfg, model = _detector(dev)
    model.eval()
    if tag == 'weighted':
        cfg.MODEL.POST_PROCESSING.NMS_CONFIG.SCORE_TYPE = 'weighted_iou_cls'
        cfg.MODEL.POST_PROCESSING.NMS_CONFIG.SCORE_WEIGHTS = EasyDict(cases.DET_SCORE_WEIGHTS)
    with torch.no_grad():
        pred, recall = model(_det_batch(dev, gold))
    assert [len(p['pred_scores']) for p in pred] == gold['ev_%s_counts' % tag].tolist()
    if tag == 'iou':
        assert sorted(recall.keys()) == [str(k) for k in gold['ev_recall_keys']]
        assert [recall[str(k)] for k in gold['ev_recall_keys']] == gold['ev_recall_vals'].tolist()
    p = pred[0]
    assert set(p.keys()) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores', 'pred_logits'}
    assert p['pred_logits'].shape == (len(p['pred_scores']), 3)
    np.testing.assert_array_equal(p['pred_labels'].cpu().numpy(), gold['ev_%s_pred_labels' % tag])
    np.testing.assert_allclose(p['pred_boxes'].cpu().numpy(), gold['ev_%s_pred_boxes' % tag], rtol=0,
                               atol=1e-5 * float(np.abs(gold['ev_%s_pred_boxes' % tag]).max()))
    for key in ('pred_scores', 'pred_cls_scores', 'pred_iou_scores'):
        want = gold['ev_%s_%s' % (tag, key)]
        assert np.abs(p[key].cpu().numpy() - want).max() <= 2e-3 * np.abs(want).max(), key


@pytest.mark.parametrize('name', ['entropy', 'random'])
def test_strategies_run_on_second_iou(dev, name):
    from pcdet.config import EasyDict
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.query_strategies import build_strategy
    cfg, model = _detector(dev, dp_ratio=0.3, seeded=False)
    cfg.DATA_CONFIG = EasyDict({'DATASET': 'KittiDataset'})
    cfg.ACTIVE_TRAIN = EasyDict({'METHOD': name, 'AGGREGATION': 'mean', 'SELECT_NUMS': 3})
    pool = SyntheticDataset(num_frames=8, first_frame=300, n_points=cases.DET_POINTS)
    lab = SyntheticDataset(num_frames=2, first_frame=0, n_points=cases.DET_POINTS)
    strat = build_strategy(name, model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 4), 0, '/tmp', cfg)
    picked = strat.query(cur_epoch=0)
    assert len(picked) == 3 and len(set(picked)) == 3 and set(picked) <= set(pool.sample_id_list), picked


def test_checkpoint_round_trip(dev, gold):
    """a checkpoint saved from the model loads back with strict=True and the eval output is unchanged"""
    _, model = _detector(dev, dp_ratio=0.3)
    model.eval()
    with torch.no_grad():
        a, _ = model(_det_batch(dev, gold))
    buf = io.BytesIO()
    torch.save({'model_state': model.state_dict()}, buf)
    buf.seek(0)
    _, other = _detector(dev, dp_ratio=0.3, seeded=False)
    other.load_state_dict(torch.load(buf, map_location=dev)['model_state'], strict=True)
    other.eval()
    with torch.no_grad():
        b, _ = other(_det_batch(dev, gold))
    assert len(a) == len(b) == 2 and len(a[0]['pred_scores']) > 0
    for pa, pb in zip(a, b):
        for k in pa:
            assert torch.equal(pa[k], pb[k]), k
