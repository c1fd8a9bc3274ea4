"""CPU: SECOND-IoU (SECONDHead, SECONDNetIoU) against goldens written by the reference's own modules
(tests/golden/make_goldens_second_iou.py). The pooling runs through its torch restatement here; the final NMS of the post-processing
is answered by the oracle (the device op has no host twin). The GPU tests run the same checks through the HIP kernels."""
import numpy as np
import pytest
import torch

import oracle
import second_iou_cases as cases
from golden._constants import seeded_state


def _t(a):
    return torch.from_numpy(np.array(a))


@pytest.fixture(scope='module')
def gold():
    return np.load(cases.GOLDEN)


def _head(dp_ratio=0.0, iou_loss='BinaryCrossEntropy'):
    from pcdet.config import EasyDict
    from pcdet.models.roi_heads import SECONDHead
    torch.manual_seed(3)
    head = SECONDHead(input_channels=cases.POOL_C, model_cfg=EasyDict(cases.head_cfg(dp_ratio, iou_loss)), num_class=1)
    head.load_state_dict(seeded_state(head, cases.HEAD_SEED))
    return head


def _pool_batch(gold, channels_last=True):
    from pcdet.config import EasyDict
    feats = _t(gold['pool_bev']).permute(0, 3, 1, 2)              # the backbone's layout: (B,C,H,W) view of the NHWC map
    return {'batch_size': cases.POOL_B, 'rois': _t(gold['pool_rois']),
            'spatial_features_2d': feats if channels_last else feats.contiguous(), 'dataset_cfg': EasyDict(cases.dataset_cfg_dict())}


@pytest.fixture(scope='module')
def detector():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import second_iou_cfg
    from pcdet.models import build_network
    from pcdet.models.detectors import build_detector
    cfg = second_iou_cfg()
    torch.manual_seed(0)
    ds = SyntheticDataset(num_frames=2)
    model = build_detector(cfg.MODEL, 3, ds)
    assert type(build_network(cfg.MODEL, 3, ds)) is type(model)
    return cfg, model


def test_build_detector_accepts_second_iou_cfg(detector, gold):
    from pcdet.models.detectors import SECONDNetIoU
    from pcdet.models.roi_heads import SECONDHead
    cfg, model = detector
    assert isinstance(model, SECONDNetIoU) and isinstance(model.roi_head, SECONDHead)
    r = cfg.MODEL.ROI_HEAD
    assert (r.NMS_CONFIG.TRAIN.NMS_PRE_MAXSIZE, r.NMS_CONFIG.TRAIN.NMS_POST_MAXSIZE, r.NMS_CONFIG.TRAIN.NMS_THRESH) == (9000, 512, 0.8)
    assert (r.NMS_CONFIG.TEST.NMS_PRE_MAXSIZE, r.NMS_CONFIG.TEST.NMS_POST_MAXSIZE, r.NMS_CONFIG.TEST.NMS_THRESH) == (1024, 100, 0.7)
    assert (r.ROI_GRID_POOL.GRID_SIZE, r.ROI_GRID_POOL.IN_CHANNEL, r.ROI_GRID_POOL.DOWNSAMPLE_RATIO) == (7, 512, 8)
    assert r.TARGET_CONFIG.CLS_SCORE_TYPE == 'roi_iou' and r.TARGET_CONFIG.ROI_PER_IMAGE == 128
    assert r.LOSS_CONFIG.IOU_LOSS == 'BinaryCrossEntropy' and r.LOSS_CONFIG.LOSS_WEIGHTS['rcnn_iou_weight'] == 1.0
    # the reference detector's parameter / buffer names and shapes (the golden's detector has DP_RATIO 0, like the GPU test's)
    from pcdet.models import build_network
    cfg.MODEL.ROI_HEAD.DP_RATIO = 0.0
    try:
        sd = build_network(cfg.MODEL, 3, model.dataset).state_dict()
    finally:
        cfg.MODEL.ROI_HEAD.DP_RATIO = 0.3
    assert sorted(sd.keys()) == [str(k) for k in gold['det_keys']]
    assert [','.join(str(v) for v in sd[k].shape) for k in sorted(sd.keys())] == [str(s) for s in gold['det_shapes']]
    assert tuple(sd['roi_head.shared_fc_layer.0.weight'].shape) == (256, 512 * 49, 1)


def test_record_layout_follows_the_config(detector):
    from pcdet.query_strategies import scoring
    L = scoring.RecordLayout.for_model(detector[1])
    assert (L.max_box, L.num_class) == (100, 3)                  # the RoI head hands 100 boxes per frame to post-processing


@pytest.mark.parametrize('tag,dp', [('dp0', 0.0), ('dp3', 0.3)])
def test_state_dict_keys_and_shapes_equal_the_reference(gold, tag, dp):
    sd = _head(dp).state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['head_keys_' + tag]]
    assert [','.join(str(v) for v in t.shape) for t in sd.values()] == [str(s) for s in gold['head_shapes_' + tag]]
    G2 = 49
    assert tuple(sd['shared_fc_layer.0.weight'].shape) == (cases.HEAD_SHARED_FC[0], cases.POOL_C * G2, 1)


@pytest.mark.parametrize('G', cases.POOL_GRIDS)
@pytest.mark.parametrize('channels_last', [True, False])
def test_torch_pool_matches_the_reference(gold, G, channels_last):
    """the torch path of roi_grid_pool: within the reference's own f32 error e_ref of the f64 definition, (B*R, C, G, G)"""
    head = _head()
    head.model_cfg.ROI_GRID_POOL.GRID_SIZE = G
    got = head.roi_grid_pool(_pool_batch(gold, channels_last)).numpy()
    f64, e_ref = gold['pool_f64_g%d' % G], float(gold['pool_e_ref_g%d' % G][0])
    assert got.shape == (cases.POOL_B * cases.POOL_R, cases.POOL_C, G, G)
    err = float(np.abs(got.astype(np.float64) - f64).max())
    print('torch path G=%d: error %.3g against f64, e_ref %.3g' % (G, err, e_ref))
    assert err <= e_ref
    assert float(np.abs(got - gold['pool_ref_g%d' % G]).max()) <= e_ref
    for b in range(cases.POOL_B):
        assert np.all(got[b * cases.POOL_R + cases.ROW_OUTSIDE] == 0)
        assert np.abs(got[b * cases.POOL_R + cases.ROW_PADDING]).max() > 1e-2


def test_f64_definition_is_the_formula_of_torch(gold):
    """pool_f64 (the yardstick of the kernel) against affine_grid / grid_sample in f64"""
    from pcdet.models.roi_heads.second_head import roi_grid_pool_torch
    bev, rois = _t(gold['pool_bev']).double().permute(0, 3, 1, 2), _t(gold['pool_rois']).double()
    for G in cases.POOL_GRIDS:
        ref = roi_grid_pool_torch(bev, rois, G, *cases.pool_geometry()).numpy()
        assert float(np.abs(ref - cases.pool_f64(gold['pool_bev'], gold['pool_rois'], G, *cases.pool_geometry())).max()) <= 1e-12
        np.testing.assert_array_equal(cases.pool_f64(gold['pool_bev'], gold['pool_rois'], G, *cases.pool_geometry()), gold['pool_f64_g%d' % G])


@pytest.mark.parametrize('tag,dp', [('dp0', 0.0), ('dp3', 0.3)])
def test_head_eval_output(gold, tag, dp):
    head = _head(dp).eval()
    with torch.no_grad():
        bd = head(_pool_batch(gold))
    assert bd['batch_cls_preds'].shape == (cases.POOL_B, cases.POOL_R, 1)
    np.testing.assert_allclose(bd['batch_cls_preds'].numpy(), gold['head_eval_' + tag], rtol=1e-4, atol=1e-5)
    assert bd['batch_box_preds'] is bd['rois'] and bd['cls_preds_normalized'] is False


def _train_step(gold, kind):
    head = _head(0.0, kind).train()
    sample = tuple(_t(a) for a in cases.head_sample())
    head.proposal_target_layer.sample_rois_for_rcnn = lambda bd, u=None: tuple(a.clone() for a in sample)
    bd = _pool_batch(gold)
    bd['gt_boxes'] = sample[1]
    head(bd)
    return head


@pytest.mark.parametrize('kind', cases.LOSS_KINDS)
def test_head_losses(gold, kind):
    head = _train_step(gold, kind)
    loss, tb = head.get_loss()
    assert sorted(tb.keys()) == ['rcnn_loss', 'rcnn_loss_iou']
    got = np.array([float(loss.detach()), float(tb['rcnn_loss_iou']), float(tb['rcnn_loss'])])
    np.testing.assert_allclose(got, gold['head_loss_' + kind], rtol=2e-5)


def test_head_train_step_logits_and_gradients(gold):
    head = _train_step(gold, 'BinaryCrossEntropy')
    ret = head.forward_ret_dict
    np.testing.assert_allclose(ret['rcnn_cls_labels'].numpy(), gold['head_labels'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(ret['rcnn_iou'].detach().numpy(), gold['head_rcnn_iou'], rtol=1e-4, atol=1e-5)
    loss, _ = head.get_loss()
    head.zero_grad()
    loss.backward()
    params = dict(head.named_parameters())
    names = [k[len('head_grad/'):] for k in gold.files if k.startswith('head_grad/')]
    assert 'shared_fc_layer.0.weight' in names and 'iou_layers.7.weight' in names and len(names) == 9
    for n in names:
        np.testing.assert_allclose(params[n].grad.numpy(), gold['head_grad/' + n], rtol=1e-3, atol=1e-6, err_msg=n)


@pytest.mark.parametrize('training', [True, False])
def test_grid_point_major_rows_give_the_same_logits(gold, training):
    """the kernel hands back (grid point, channel)-ordered rows as a permuted view: the first FC layer then contracts against the
    re-ordered columns of its weight (a view in training, the cached folded copy in eval); same logits, the parameter untouched"""
    head = _head(0.0)
    head.train(training)
    with torch.set_grad_enabled(training):
        nchw = head.roi_grid_pool(_pool_batch(gold))
        view = nchw.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not view.is_contiguous() and head._first_weight_rows(view)[1] and not head._first_weight_rows(nchw)[1]
        w0 = head.shared_fc_layer[0].weight.detach().clone()
        a, b = head._iou_branch(nchw), head._iou_branch(view)
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert torch.equal(head.shared_fc_layer[0].weight.detach(), w0)


def test_focalbce_and_num_pts_iou_cls_raise(gold, detector):
    head = _train_step(gold, 'BinaryCrossEntropy')
    head.model_cfg.LOSS_CONFIG.IOU_LOSS = 'focalbce'
    with pytest.raises(NotImplementedError):
        head.get_loss()
    _, model = detector
    nms = model.model_cfg.POST_PROCESSING.NMS_CONFIG
    x = torch.rand(2, 5)
    for kind in ('num_pts_iou_cls',):
        nms.SCORE_TYPE = kind
        try:
            with pytest.raises(NotImplementedError):
                model.nms_scores(x, x, torch.ones(2, 5, dtype=torch.long))
        finally:
            nms.pop('SCORE_TYPE')
    for key, where in (('MULTI_CLASSES_NMS', nms), ('OUTPUT_RAW_SCORE', model.model_cfg.POST_PROCESSING)):
        where[key] = True
        try:
            with pytest.raises(NotImplementedError):
                model.post_processing({'batch_size': 1})
        finally:
            where[key] = False


def _oracle_nms_batched(boxes_sorted, counts, thresh, max_keep, rotated=True):
    B = boxes_sorted.shape[0]
    keep = torch.full((B, max_keep), -1, dtype=torch.int32)
    num = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        n = int(counts[b]) if counts is not None else boxes_sorted.shape[1]
        k = oracle.nms(boxes_sorted[b, :n].numpy(), float(thresh), rotated=rotated)[:max_keep]
        keep[b, :len(k)] = torch.from_numpy(k.astype(np.int32))
        num[b] = len(k)
    return keep, num


@pytest.mark.parametrize('tag', ['iou', 'weighted'])
def test_post_processing_picks_and_scores(gold, detector, monkeypatch, tag):
    from pcdet.config import EasyDict
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    monkeypatch.setattr(iou3d_nms_utils, 'nms_batched', _oracle_nms_batched)
    _, model = detector
    nms = model.model_cfg.POST_PROCESSING.NMS_CONFIG
    if tag == 'weighted':
        nms.SCORE_TYPE, nms.SCORE_WEIGHTS = 'weighted_iou_cls', EasyDict(cases.DET_SCORE_WEIGHTS)
    try:
        bd = {'batch_size': 2, 'batch_box_preds': _t(gold['ev_rois']), 'batch_cls_preds': _t(gold['ev_iou_logits']),
              'roi_scores': _t(gold['ev_roi_scores']), 'roi_labels': _t(gold['ev_roi_labels']), 'has_class_labels': True,
              'cls_preds_normalized': False, 'full_cls_scores': torch.arange(2 * 100 * 3, dtype=torch.float32).view(2, 100, 3)}
        pred, recall = model.post_processing(bd)
    finally:
        nms.pop('SCORE_TYPE', None)
        nms.pop('SCORE_WEIGHTS', None)
    assert recall == {} and [len(p['pred_scores']) for p in pred] == gold['ev_%s_counts' % tag].tolist()
    p = pred[0]
    assert set(p.keys()) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_cls_scores', 'pred_iou_scores', 'pred_logits'}
    np.testing.assert_array_equal(p['pred_boxes'].numpy(), gold['ev_%s_pred_boxes' % tag])
    np.testing.assert_array_equal(p['pred_labels'].numpy(), gold['ev_%s_pred_labels' % tag])
    for key in ('pred_scores', 'pred_cls_scores', 'pred_iou_scores'):
        np.testing.assert_allclose(p[key].numpy(), gold['ev_%s_%s' % (tag, key)], rtol=1e-6, atol=1e-7)
    # pred_logits: the full_cls_scores rows of the kept boxes
    rows = (p['pred_logits'][:, 0] / 3).long()
    np.testing.assert_array_equal(_t(gold['ev_rois'])[0][rows].numpy(), gold['ev_%s_pred_boxes' % tag])
