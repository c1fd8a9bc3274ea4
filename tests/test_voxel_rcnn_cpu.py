"""CPU: Voxel R-CNN (voxel_query, NeighborVoxelSAModuleMSG, VoxelRCNNHead, VoxelRCNN) against goldens written by the reference's own
modules (tests/golden/make_goldens_voxel_rcnn.py). Everything runs through the torch route here (dense index, materialised groups);
the GPU tests run the same cases through the HIP kernels."""
import numpy as np
import pytest
import torch

import voxel_rcnn_cases as cases
from golden._constants import seeded_state


def _t(a):
    return torch.from_numpy(np.array(a))


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


def make_module(p, pool):
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import NeighborVoxelSAModuleMSG
    mod = NeighborVoxelSAModuleMSG(query_ranges=[p['ranges']], radii=[p['radius']], nsamples=[p['nsample']],
                                   mlps=[[p['c_in'], p['c'], p['c_out']]], pool_method=pool)
    mod.load_state_dict(seeded_state(mod, cases.MODULE_SEED))
    return mod


def module_inputs(p, q, dev='cpu', dtype=torch.float32, sparse=False):
    """keyword arguments of NeighborVoxelSAModuleMSG.forward for a level case; the features require a gradient"""
    xyz, new_xyz, new_coords = q
    G = p['grid']
    coords = _t(p['coords']).to(dev)
    if sparse:
        import spconv.pytorch as spconv
        index = spconv.SparseConvTensor(torch.zeros((len(coords), 1), device=dev), coords, list(cases.SHAPE), cases.B)
    else:
        index = _t(cases.dense_index(p['coords'])).to(dev)
    return dict(xyz=_t(xyz).to(dev, dtype), xyz_batch_cnt=_t(np.bincount(p['coords'][:, 0], minlength=cases.B).astype(np.int32)).to(dev),
                new_xyz=_t(new_xyz).to(dev, dtype), new_xyz_batch_cnt=torch.full((cases.B,), cases.R * G ** 3, dtype=torch.int32, device=dev),
                new_coords=_t(new_coords[:, [0, 3, 2, 1]].copy()).to(dev), features=_t(p['feats']).to(dev, dtype).requires_grad_(True),
                voxel2point_indices=index)


def out_weights(p, shape):
    return np.random.default_rng(p['seed'] + 9).normal(0, 1, shape)


@pytest.mark.parametrize('name', list(cases.LEVEL_CASES))
def test_restatement_equals_brute_force_and_golden(gold, level, name):
    p, (xyz, new_xyz, new_coords) = level[name]
    cases.assert_radius_margin(p['ranges'], p['radius'], xyz, new_xyz, new_coords, p['coords'], p['radius_margin'])
    idx, empty = cases.voxel_query_np(p['ranges'], p['radius'], p['nsample'], xyz, new_xyz, new_coords, cases.dense_index(p['coords']))
    bidx, bempty = cases.voxel_query_brute(p['ranges'], p['radius'], p['nsample'], xyz, new_xyz, new_coords, p['coords'])
    np.testing.assert_array_equal(idx, bidx)
    np.testing.assert_array_equal(empty, bempty)
    np.testing.assert_array_equal(idx, gold['q_%s_idx' % name])
    np.testing.assert_array_equal(empty, gold['q_%s_empty' % name])
    G3 = p['grid'] ** 3
    per_roi = (~empty).reshape(-1, G3).sum(1)
    assert per_roi[cases.ROI_EMPTY] == 0 and per_roi[cases.ROI_CLUSTER] == G3 and 0 < per_roi[cases.ROI_BIG] < G3
    assert 0 < per_roi[cases.ROI_CORNER] < G3 and new_coords[:, 1:].min() < 0
    # the cluster decides by the first-hits rule: a ball there holds more voxels than nsample
    r2 = np.float32(p['radius']) ** 2
    m = cases.ROI_CLUSTER * G3 + G3 // 2
    assert (cases._dist2_f32(xyz[p['coords'][:, 0] == 0], new_xyz[m]) <= r2).sum() > p['nsample']
    # and somewhere a ball holds fewer: the fill rule decides
    partial = [i for i in range(len(idx)) if not empty[i] and len(set(idx[i].tolist())) < p['nsample']]
    assert partial and all((idx[i][len(set(idx[i].tolist())):] == idx[i][0]).all() for i in partial[:50])
    if p['shuffled']:
        c = p['coords']
        key = ((c[:, 0].astype(np.int64) * 100 + c[:, 1]) * 100 + c[:, 2]) * 100 + c[:, 3]
        assert (np.diff(key) < 0).any() and (np.diff(c[:, 0]) >= 0).all()


@pytest.mark.parametrize('name', list(cases.LEVEL_CASES))
@pytest.mark.parametrize('sparse', [False, True])
def test_torch_query_equals_restatement(gold, level, name, sparse):
    from pcdet.ops.pointnet2.pointnet2_stack import voxel_query_utils
    p, q = level[name]
    kw = module_inputs(p, q, sparse=sparse)
    idx, empty = voxel_query_utils.voxel_query(p['ranges'], p['radius'], p['nsample'], kw['xyz'], kw['new_xyz'], _t(q[2]),
                                               kw['voxel2point_indices'])
    assert idx.dtype == torch.int32 and empty.dtype == torch.bool
    np.testing.assert_array_equal(idx.numpy(), gold['q_%s_idx' % name])
    np.testing.assert_array_equal(empty.numpy(), gold['q_%s_empty' % name])


def test_generate_voxel2pinds(level):
    import spconv.pytorch as spconv
    from pcdet.utils import common_utils
    p, _ = level['b']
    sp = spconv.SparseConvTensor(torch.zeros(len(p['coords']), 1), _t(p['coords']), list(cases.SHAPE), cases.B)
    got = common_utils.generate_voxel2pinds(sp)
    assert got.dtype == torch.int32
    np.testing.assert_array_equal(got.numpy(), cases.dense_index(p['coords']))


def run_module(mod, p, kw, training):
    """-> out and the gradients (both modes), in training also the buffers, keyed like the golden"""
    mod.train(training)
    out = mod(**kw)
    res = {'out': out.detach()}
    w = _t(out_weights(p, tuple(out.shape))).to(out.device, out.dtype)
    mod.zero_grad()
    ((out * w).sum() / out.shape[0]).backward()          # eval mode too: the frozen-BatchNorm fine-tuning path
    res['grad/features'] = kw['features'].grad.detach()
    for n, t in mod.named_parameters():
        res['grad/' + n] = t.grad.detach()
    if training:
        for n, t in mod.named_buffers():
            res['buf/' + n] = t.detach().clone()
    return res


def assert_matches_golden(gold, tag, res, factor=None):
    """every recorded quantity of a module run against the golden. factor None: the ordinary f32 agreement of two evaluations of the
    same graph (rtol 1e-4 + 1e-5 of the largest entry); a number: within factor * e_ref, the reference's own f32 error"""
    checked = 0
    for key, val in res.items():
        ref = gold['%s_%s' % (tag, key)]
        got = val.cpu().numpy()
        if key in ('out', 'grad/features'):
            got = got[cases.ROWS]
        if not np.issubdtype(ref.dtype, np.floating):
            np.testing.assert_array_equal(got, ref, err_msg=key)
        elif factor is None:
            np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5 * float(np.abs(ref).max()), err_msg=key)
        else:
            e_ref = float(gold['%s_e_ref_%s' % (tag, key)][0])
            err = float(np.abs(got.astype(np.float64) - ref).max())
            print('%s %s: |got - ref f32| %.3g, e_ref %.3g (ratio %.2f)' % (tag, key, err, e_ref, err / max(e_ref, 1e-30)))
            assert err <= factor * e_ref, (key, err, e_ref)
        checked += 1
    return checked


@pytest.mark.parametrize('name', list(cases.LEVEL_CASES))
@pytest.mark.parametrize('pool', cases.POOLS)
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('sparse', [False, True])
def test_torch_route_module_matches_the_reference(gold, level, name, pool, training, sparse):
    p, q = level[name]
    tag = 'm_%s_%s_%s' % (name, pool, 'train' if training else 'eval')
    res = run_module(make_module(p, pool), p, module_inputs(p, q, sparse=sparse), training)
    assert res['out'].shape == (len(q[1]), p['c_out'])
    assert assert_matches_golden(gold, tag, res) == (1 + 1 + 9 + 9 if training else 1 + 1 + 9)


@pytest.mark.parametrize('pool', cases.POOLS)
def test_f64_definition_is_the_torch_route(level, pool):
    """cases.pool_f64 (the yardstick of the kernel) against the torch route's pooling body in f64, batch statistics included"""
    p, q = level['b']
    mod = make_module(p, pool).double().train()
    kw = module_inputs(p, q, dtype=torch.float64)
    idx, empty = cases.voxel_query_np(p['ranges'], p['radius'], p['nsample'], *q, cases.dense_index(p['coords']))
    fin = torch.randn(len(p['coords']), p['c'], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = mod._pool_torch(0, fin, kw['xyz'], kw['xyz_batch_cnt'], kw['new_xyz'], kw['new_xyz_batch_cnt'], _t(q[2]), kw['voxel2point_indices'])
    conv, bn = mod.mlps_pos[0][0], mod.mlps_pos[0][1]
    ref = cases.pool_f64(fin.numpy(), q[0], q[1], idx, empty, seeded_state(mod, cases.MODULE_SEED)['mlps_pos.0.0.weight'].numpy(),
                         bn.weight.detach().numpy(), bn.bias.detach().numpy(), bn.eps, pool)[0]
    assert float(np.abs(got.detach().numpy() - ref).max()) < 1e-11
    assert conv.weight.shape == (p['c'], 3, 1, 1)


def test_folded_position_branch_equals_batchnorm2d(level):
    """fold_pos_bn from the nine moments of d against nn.BatchNorm2d on the materialised (1, 3, M, nsample) tensor: values, the
    gradients of W / gamma / beta (the variance's dependence on W included), running statistics and num_batches_tracked"""
    from pcdet.ops.pointnet2.pointnet2_stack.voxel_pool_modules import fold_pos_bn
    p, q = level['b']
    idx, empty = cases.voxel_query_np(p['ranges'], p['radius'], p['nsample'], *q, cases.dense_index(p['coords']))
    d = q[0][idx] - q[1][:, None, :]
    d[empty] = 0
    d = _t(d).double()                                                        # (M, ns, 3)
    flat = d.reshape(-1, 3)
    mu = flat.mean(0)
    sigma = (flat.t() @ flat) / flat.shape[0] - mu[:, None] * mu[None, :]
    mods = [make_module(p, 'max_pool').double().train().mlps_pos[0] for _ in range(2)]
    wsum = torch.randn(d.shape[0], d.shape[1], p['c'], dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    ref = mods[0](d.permute(2, 0, 1).unsqueeze(0))[0].permute(1, 2, 0)        # (M, ns, C)
    (ref * wsum).sum().backward()
    A, b = fold_pos_bn(mods[1][0], mods[1][1], mu, sigma, float(flat.shape[0]))
    got = d @ A.double().t() + b.double()
    (got * wsum).sum().backward()
    assert float((got - ref).detach().abs().max()) < 1e-5                               # (A, b are handed over in f32)
    for a, c in zip(mods[0].parameters(), mods[1].parameters()):
        np.testing.assert_allclose(c.grad.numpy(), a.grad.numpy(), rtol=1e-4, atol=1e-5 * float(a.grad.abs().max()))
    for a, c in zip(mods[0].buffers(), mods[1].buffers()):
        np.testing.assert_allclose(c.numpy(), a.numpy(), rtol=1e-9)
    assert int(mods[1][1].num_batches_tracked) == 1


# ---- head ---------------------------------------------------------------------------------------------------------------
def make_head(dp_ratio=0.0):
    from pcdet.config import EasyDict
    from pcdet.models.roi_heads import VoxelRCNNHead
    torch.manual_seed(3)
    head = VoxelRCNNHead(backbone_channels=dict(cases.HEAD_CHANNELS), model_cfg=EasyDict(cases.head_cfg(dp_ratio)),
                         point_cloud_range=np.array(cases.HEAD_PCR, np.float32), voxel_size=list(cases.VOXEL), num_class=1)
    head.load_state_dict(seeded_state(head, cases.HEAD_SEED))
    return head


def head_batch(dev='cpu'):
    import spconv.pytorch as spconv
    rois, levels = cases.head_inputs()
    feats = {n: spconv.SparseConvTensor(_t(f).to(dev), _t(c).to(dev), list(cases.head_level_shape(cases.HEAD_STRIDES[n])), cases.B)
             for n, (c, f) in levels.items()}
    return {'batch_size': cases.B, 'rois': _t(rois).to(dev), 'roi_labels': torch.ones(rois.shape[:2], dtype=torch.long, device=dev),
            'roi_scores': torch.zeros(rois.shape[:2], device=dev), 'multi_scale_3d_features': feats,
            'multi_scale_3d_strides': dict(cases.HEAD_STRIDES)}


def head_train_step(dev='cpu'):
    head = make_head(0.0).to(dev).train()
    sample = tuple(_t(a).to(dev) for a in cases.head_sample())
    head.proposal_target_layer.sample_rois_for_rcnn = lambda bd, u=None: tuple(a.clone() for a in sample)
    bd = head_batch(dev)
    bd['gt_boxes'] = sample[1]
    head(bd)
    return head


def check_head_train_step(gold, head, grad_rtol=1e-3):
    ret = head.forward_ret_dict
    np.testing.assert_allclose(ret['rcnn_cls_labels'].cpu().numpy(), gold['head_cls_labels'], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(ret['reg_valid_mask'].cpu().numpy(), gold['head_reg_valid'])
    np.testing.assert_allclose(ret['rcnn_cls'].detach().cpu().numpy(), gold['head_rcnn_cls'], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ret['rcnn_reg'].detach().cpu().numpy(), gold['head_rcnn_reg'], rtol=1e-4, atol=1e-5)
    loss, tb = head.get_loss()
    assert sorted(tb.keys()) == [str(k) for k in gold['head_tb_keys']]
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in tb.values())
    np.testing.assert_allclose(float(loss.detach()), gold['head_loss'][0], rtol=2e-5)
    np.testing.assert_allclose([float(tb[k]) for k in sorted(tb.keys())], gold['head_tb_vals'], rtol=2e-5)
    head.zero_grad()
    loss.backward()
    names = [k[len('head_grad/'):] for k in gold.files if k.startswith('head_grad/')]
    params = dict(head.named_parameters())
    assert sorted(names) == sorted(params.keys())
    for n in names:
        g = params[n].grad.cpu().numpy()
        ref = gold['head_grad/' + n]
        np.testing.assert_allclose(g[:8] if n == 'shared_fc_layer.0.weight' else g, ref, rtol=grad_rtol, atol=1e-5 * float(np.abs(ref).max()),
                                   err_msg=n)
    for k in gold.files:
        if k.startswith('head_buf/'):
            got = dict(head.named_buffers())[k[len('head_buf/'):]].cpu().numpy()
            np.testing.assert_allclose(got, gold[k], rtol=1e-4, atol=1e-6, err_msg=k)


@pytest.mark.parametrize('tag,dp', [('dp0', 0.0), ('dp3', 0.3)])
def test_state_dict_keys_and_shapes_equal_the_reference(gold, tag, dp):
    sd = make_head(dp).state_dict()
    assert list(sd.keys()) == [str(k) for k in gold['head_keys_' + tag]]
    assert [','.join(str(v) for v in t.shape) for t in sd.values()] == [str(s) for s in gold['head_shapes_' + tag]]
    assert tuple(sd['shared_fc_layer.0.weight'].shape) == (cases.HEAD_FC[0], cases.HEAD_GRID ** 3 * 64)
    assert tuple(sd['roi_grid_pool_layers.1.mlps_pos.0.0.weight'].shape) == (64, 3, 1, 1)


@pytest.mark.parametrize('tag,dp', [('dp0', 0.0), ('dp3', 0.3)])
def test_head_eval_output(gold, tag, dp):
    head = make_head(dp).eval()
    with torch.no_grad():
        bd = head(head_batch())
    np.testing.assert_allclose(bd['batch_cls_preds'].numpy(), gold['head_eval_cls_' + tag], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(bd['batch_box_preds'].numpy(), gold['head_eval_box_' + tag], rtol=1e-4, atol=1e-5)
    assert bd['cls_preds_normalized'] is False and bd['batch_cls_preds'].shape == (cases.B, cases.R, 1)


def test_head_train_step_loss_and_gradients(gold):
    check_head_train_step(gold, head_train_step())


def test_head_config_is_left_as_it_is():
    """the reference prepends the backbone width to ROI_GRID_POOL.POOL_LAYERS.*.MLPS in place; a second head built from the same
    config then fails there. Here the config keeps its values."""
    from pcdet.config import EasyDict
    from pcdet.models.roi_heads import VoxelRCNNHead
    cfg = EasyDict(cases.head_cfg())
    for _ in range(2):
        VoxelRCNNHead(backbone_channels=dict(cases.HEAD_CHANNELS), model_cfg=cfg, point_cloud_range=cases.HEAD_PCR, voxel_size=cases.VOXEL)
    assert cfg.ROI_GRID_POOL.POOL_LAYERS.x_conv4.MLPS == [[64, 32]]


# ---- detector -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def detector():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import voxel_rcnn_cfg
    from pcdet.models import build_network
    cfg = voxel_rcnn_cfg()
    torch.manual_seed(0)
    ds = SyntheticDataset(num_frames=2, class_names=cfg.CLASS_NAMES)
    return cfg, build_network(cfg.MODEL, len(cfg.CLASS_NAMES), ds)


def test_voxel_rcnn_cfg_builds_the_detector(detector):
    from pcdet.models.detectors import VoxelRCNN
    from pcdet.models.roi_heads import VoxelRCNNHead
    from pcdet.query_strategies import scoring
    cfg, model = detector
    assert isinstance(model, VoxelRCNN) and isinstance(model.roi_head, VoxelRCNNHead)
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'BaseBEVBackbone',
                                                             'AnchorHeadSingle', 'VoxelRCNNHead']
    assert cfg.CLASS_NAMES == ['Car'] and len(cfg.MODEL.DENSE_HEAD.ANCHOR_GENERATOR_CONFIG) == 1
    b2 = cfg.MODEL.BACKBONE_2D
    assert (b2.LAYER_NUMS, b2.NUM_FILTERS, b2.NUM_UPSAMPLE_FILTERS) == ([5, 5], [64, 128], [128, 128])
    r = cfg.MODEL.ROI_HEAD
    assert r.ROI_GRID_POOL.FEATURES_SOURCE == ['x_conv2', 'x_conv3', 'x_conv4'] and r.ROI_GRID_POOL.GRID_SIZE == 6
    assert [r.ROI_GRID_POOL.POOL_LAYERS[k].POOL_RADIUS for k in r.ROI_GRID_POOL.FEATURES_SOURCE] == [[0.4], [0.8], [1.6]]
    assert (r.NMS_CONFIG.TEST.NMS_PRE_MAXSIZE, r.NMS_CONFIG.TEST.NMS_POST_MAXSIZE, r.NMS_CONFIG.TEST.NMS_THRESH) == (2048, 100, 0.7)
    assert cfg.MODEL.POST_PROCESSING.SCORE_THRESH == 0.3 and cfg.MODEL.POST_PROCESSING.NMS_CONFIG.NMS_THRESH == 0.1
    aug = cfg.DATA_CONFIG.DATA_AUGMENTOR.AUG_CONFIG_LIST
    assert [a.NAME for a in aug] == ['gt_sampling', 'random_world_flip', 'random_world_rotation', 'random_world_scaling']
    assert aug[0].SAMPLE_GROUPS == ['Car:15'] and aug[0].USE_ROAD_PLANE is False and aug[1].ALONG_AXIS_LIST == ['x']
    sd = model.state_dict()
    assert tuple(sd['roi_head.shared_fc_layer.0.weight'].shape) == (256, 216 * 96)
    assert tuple(sd['roi_head.roi_grid_pool_layers.2.mlps_in.0.0.weight'].shape) == (32, 64, 1)
    assert tuple(sd['roi_head.reg_pred_layer.weight'].shape) == (7, 256) and tuple(sd['roi_head.cls_pred_layer.weight'].shape) == (1, 256)
    L = scoring.RecordLayout.for_model(model)
    assert (L.max_box, L.num_class) == (100, 1)


def test_injected_roi_targets_dict_is_used(gold):
    """batch_dict['roi_targets_dict'] replaces the sampler: a head whose sampler would fail reproduces the step of the head that sampled"""
    first = head_train_step()
    targets = {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in first.forward_ret_dict.items()
               if k not in ('rcnn_cls', 'rcnn_reg')}
    head = make_head(0.0).train()

    def no_sampler(*a, **k):
        raise AssertionError('the sampler ran although a RoI sample was injected')
    head.assign_targets = no_sampler
    bd = head_batch()
    bd['rois'] = torch.zeros_like(bd['rois'])                     # what the proposal stage left is replaced by the sample's RoIs
    bd['roi_targets_dict'] = targets
    head(bd)
    assert head.forward_ret_dict is targets and torch.equal(bd['rois'], targets['rois'])
    check_head_train_step(gold, head)


def _oracle_nms_batched(boxes_sorted, counts, thresh, max_keep, rotated=True):
    import oracle
    B = boxes_sorted.shape[0]
    keep = torch.full((B, max_keep), -1, dtype=torch.int32)
    num = torch.zeros((B,), dtype=torch.int32)
    for b in range(B):
        n = int(counts[b]) if counts is not None else boxes_sorted.shape[1]
        k = oracle.nms(boxes_sorted[b, :n].numpy(), float(thresh), rotated=rotated)[:max_keep]
        keep[b, :len(k)] = torch.from_numpy(k.astype(np.int32))
        num[b] = len(k)
    return keep, num


@pytest.mark.parametrize('has_class_labels', [True, False])
def test_post_processing_contract_and_labels(detector, monkeypatch, has_class_labels):
    """pred_boxes / pred_scores / pred_labels / pred_logits of the kept boxes; the labels are the first stage's roi_labels when it
    produced class labels (a multi-class first stage under the class-agnostic head), else the head's own arg-max + 1"""
    from pcdet.ops.iou3d_nms import iou3d_nms_utils
    monkeypatch.setattr(iou3d_nms_utils, 'nms_batched', _oracle_nms_batched)
    _, model = detector
    rng = np.random.default_rng(5)
    n = 12
    boxes = np.zeros((2, n, 7), np.float32)
    boxes[..., 0] = 5 + 4 * np.arange(n)                          # far apart: the NMS keeps every box above the score threshold
    boxes[..., 3:6] = [3.9, 1.6, 1.5]
    logits = rng.normal(0, 2, (2, n, 1)).astype(np.float32)
    labels = rng.integers(1, 4, (2, n)).astype(np.int64)
    bd = {'batch_size': 2, 'batch_box_preds': _t(boxes), 'batch_cls_preds': _t(logits), 'roi_labels': _t(labels),
          'has_class_labels': has_class_labels, 'cls_preds_normalized': False,
          'full_cls_scores': torch.arange(2 * n * 3, dtype=torch.float32).view(2, n, 3)}
    pred, recall = model.post_processing(bd)
    assert recall == {}
    scores = 1 / (1 + np.exp(-logits[..., 0].astype(np.float64)))
    for b, p in enumerate(pred):
        assert set(p.keys()) == {'pred_boxes', 'pred_scores', 'pred_labels', 'pred_logits'}
        keep = np.nonzero(scores[b] > model.model_cfg.POST_PROCESSING.SCORE_THRESH)[0]
        keep = keep[np.argsort(-scores[b][keep], kind='stable')]
        assert len(keep) >= 2
        np.testing.assert_array_equal(p['pred_boxes'].numpy(), boxes[b][keep])
        np.testing.assert_allclose(p['pred_scores'].numpy(), scores[b][keep], rtol=1e-6)
        np.testing.assert_array_equal(p['pred_labels'].numpy(), labels[b][keep] if has_class_labels else np.ones(len(keep), np.int64))
        np.testing.assert_array_equal((p['pred_logits'][:, 0] / 3).long().numpy() - b * n, keep)


def test_unsupported_options_raise(detector, level):
    from pcdet.config import EasyDict
    from pcdet.models.roi_heads import VoxelRCNNHead
    _, model = detector
    post = model.model_cfg.POST_PROCESSING
    for key, where in (('MULTI_CLASSES_NMS', post.NMS_CONFIG), ('OUTPUT_RAW_SCORE', post)):
        where[key] = True
        try:
            with pytest.raises(NotImplementedError):
                model.post_processing({'batch_size': 1})
        finally:
            where[key] = False
    cfg = EasyDict(cases.head_cfg())
    cfg.LOSS_CONFIG.GRID_3D_IOU_LOSS = True
    with pytest.raises(NotImplementedError):
        VoxelRCNNHead(backbone_channels=dict(cases.HEAD_CHANNELS), model_cfg=cfg, point_cloud_range=cases.HEAD_PCR, voxel_size=cases.VOXEL)
    p, q = level['b']
    with pytest.raises(NotImplementedError):
        make_module(p, 'median_pool')(**module_inputs(p, q))


def test_c_abi_refuses_host_tensors(level):
    import crbhip
    from crbhip import voxel_pool
    p, q = level['b']
    with pytest.raises(crbhip.CrbHipError):
        voxel_pool.voxel_query(_t(q[0]), _t(q[1]), _t(q[2]), cases.B, cases.SHAPE, p['ranges'], p['radius'], p['nsample'],
                               torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int32), 8)
    assert crbhip.lib.crb_voxel_pool_supported(32, 16) == 1 and crbhip.lib.crb_voxel_pool_supported(64, 32) == 1
    assert crbhip.lib.crb_voxel_pool_supported(48, 16) == 0 and crbhip.lib.crb_voxel_pool_supported(32, 33) == 0
