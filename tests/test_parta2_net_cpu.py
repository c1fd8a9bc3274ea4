"""CPU: the numpy definition of the sparse RoI-aware pooling (tests/roiaware_cases.py) against the reference's own PartA2FCHead pooling
(tests/golden/ref_partA2.npz), the premises of the seeded cases, and PartA2Net as build_network assembles it from parta2_net_cfg()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import roiaware_cases as cases  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_definition_scattered_densely_is_the_reference_pooling():
    """the rows of the definition, written into dense grids, are the reference's pooled tensors: max exact, avg to 1e-6"""
    c, d = cases.get_case('golden')
    g = np.load(os.path.join(GOLD, 'ref_partA2.npz'))
    part, feat = cases.scatter_dense(c, d)
    np.testing.assert_array_equal(feat, g['pa2_pooled_rpn'])
    np.testing.assert_allclose(part, g['pa2_pooled_part'], rtol=1e-6, atol=1e-6)
    idx = np.argwhere(g['pa2_pooled_part'].sum(-1) != 0)                 # the reference's sparse rows, lexicographic
    np.testing.assert_array_equal(d['coords'], idx.astype(np.int32))


@pytest.mark.parametrize('name', cases.CASE_NAMES)
def test_case_premises_hold(name):
    c, d = cases.get_case(name)                                          # get_case asserts the premise when it builds the case
    cases.check_premise(name, c, d)
    assert d['coords'].shape[0] == len(d['kept']) and c['part'].dtype == np.float32
    if len(d['coords']) > 1:                                             # rows in lexicographic order
        o = c['o']
        key = ((d['coords'][:, 0].astype(np.int64) * o + d['coords'][:, 1]) * o + d['coords'][:, 2]) * o + d['coords'][:, 3]
        assert (np.diff(key) > 0).all()


def test_gradient_definition_conserves_the_upstream_gradient():
    c, d = cases.get_case('odd')
    rng = np.random.default_rng(1)
    T, C = len(d['coords']), c['feat'].shape[1]
    gp, gf = rng.normal(0, 1, (T, 4)).astype(np.float32), rng.normal(0, 1, (T, C)).astype(np.float32)
    r = cases.grad_definition(c, d, gp, gf)
    np.testing.assert_allclose(r['grad_part'].sum(0), gp.astype(np.float64).sum(0), rtol=1e-9, atol=1e-9)   # avg: the weights of a row sum to 1
    np.testing.assert_allclose(r['grad_feat'].sum(0), gf.astype(np.float64).sum(0), rtol=1e-9, atol=1e-9)   # max: one point per (row, channel)
    assert (r['n_feat'].sum(0) == T).all() and r['n_part'].sum() == 4 * sum(len(k) for k in d['kept'])


@pytest.fixture(scope='module')
def kitti_model():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import parta2_net_cfg
    from pcdet.models import build_network
    return build_network(parta2_net_cfg().MODEL, 3, SyntheticDataset(num_frames=2))


def test_build_network_gives_the_reference_module_chain(kitti_model):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import parta2_net_cfg
    from pcdet.models import build_network
    from pcdet.models.detectors import PartA2Net
    m = kitti_model
    assert type(m) is PartA2Net
    assert [type(x).__name__ for x in m.module_list] == ['MeanVFE', 'UNetV2', 'HeightCompression', 'BaseBEVBackbone', 'AnchorHeadSingle',
                                                         'PointIntraPartOffsetHead', 'PartA2FCHead']
    assert m.roi_head.roiaware_pool3d_layer.out_size == 12 and m.roi_head.roiaware_pool3d_layer.max_pts_each_voxel == 128
    sd = m.state_dict()
    # every parameter and buffer of the reference's own PartA2Net, name and shape (tests/golden/make_goldens_parta2_net.py)
    net = np.load(os.path.join(GOLD, 'ref_parta2_net.npz'))
    assert sorted(sd) == list(net['keys_yaml'])                           # the yaml as it stands (dropout layers in the FC stacks)
    assert [str(tuple(sd[k].shape)) for k in sorted(sd)] == list(net['shapes_yaml'])
    cfg0 = parta2_net_cfg().MODEL
    cfg0.ROI_HEAD.DP_RATIO = 0.0                                         # the golden step's configuration
    sd0 = build_network(cfg0, 3, SyntheticDataset(num_frames=2)).state_dict()
    assert sorted(sd0) == list(net['keys']) and [str(tuple(sd0[k].shape)) for k in sorted(sd0)] == list(net['shapes'])
    # the 3-D backbone's parameters are the reference UNetV2's (names and shapes written by the reference's own module)
    g = np.load(os.path.join(GOLD, 'ref_unetv2.npz'))
    own = {k[len('backbone_3d.'):]: str(tuple(v.shape)) for k, v in sd.items() if k.startswith('backbone_3d.')}
    assert sorted(own) == list(g['keys']) and [own[k] for k in sorted(own)] == list(g['shapes'])
    # the RoI head's sparse stacks carry the reference PartA2FCHead's parameter names (the FC stacks' indices move with the yaml's
    # dropout layers and widths); the shapes follow the yaml
    roi = {k[len('roi_head.'):]: tuple(v.shape) for k, v in sd.items() if k.startswith('roi_head.')}
    conv = lambda keys: sorted(k for k in keys if k.startswith('conv_'))
    assert conv(roi) == conv(str(k) for k in np.load(os.path.join(GOLD, 'ref_partA2.npz'))['pa2_keys'])
    assert roi['shared_fc_layer.0.weight'] == (256, 128 * 12 ** 3, 1) and roi['conv_rpn.0.0.weight'][-1] == 16
    assert [k for k in roi if k.startswith('shared_fc_layer.') and k.endswith('.weight') and len(roi[k]) == 3] == \
        ['shared_fc_layer.0.weight', 'shared_fc_layer.4.weight', 'shared_fc_layer.8.weight']      # Conv, BN, ReLU, Dropout x 2, then 3
    last = lambda p: roi[max((k for k in roi if k.startswith(p) and k.endswith('.weight')), key=lambda k: int(k.split('.')[1]))]
    assert last('cls_layers.') == (1, 256, 1) and last('reg_layers.') == (7, 256, 1)
    # point head: one linear layer per branch on UNetV2's 16 point features (CLS_FC [], PART_FC [], class agnostic)
    ph = {k[len('point_head.'):]: tuple(v.shape) for k, v in sd.items() if k.startswith('point_head.')}
    assert ph == {'cls_layers.0.weight': (1, 16), 'cls_layers.0.bias': (1,), 'part_reg_layers.0.weight': (3, 16),
                  'part_reg_layers.0.bias': (3,)}


def test_record_layout_is_100_boxes_of_3_classes(kitti_model):
    from pcdet.query_strategies import scoring
    lay = scoring.RecordLayout.for_model(kitti_model)
    assert (lay.max_box, lay.num_class) == (100, 3) and lay == scoring.RecordLayout(100, 3)


def test_waymo_configuration_builds():
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import parta2_net_cfg
    from pcdet.models import build_network
    cfg = parta2_net_cfg('waymo')
    m = build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2, kind='waymo', n_points=20000))
    assert type(m).__name__ == 'PartA2Net' and m.roi_head.roiaware_pool3d_layer.out_size == 10
    assert cfg.MODEL.ROI_HEAD.NMS_CONFIG.TEST.NMS_POST_MAXSIZE == 300 and cfg.CLASS_NAMES[0] == 'Vehicle'
    assert m.dense_head.model_cfg.ANCHOR_GENERATOR_CONFIG[0]['anchor_bottom_heights'] == [0]
