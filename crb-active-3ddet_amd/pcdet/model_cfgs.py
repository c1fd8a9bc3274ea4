"""Model configs as data (the values of tools/cfgs/kitti_models/second.yaml, tools/cfgs/waymo_models/second.yaml and
tools/cfgs/active-kitti_models/pv_rcnn_active_crb.yaml), so the GPU box needs no YAML tree. cfg_from_yaml_file in
pcdet.config reads the reference's own YAMLs when they are available."""
from .config import EasyDict


def _anchor(cls, size, bottom, matched, unmatched, stride=8):
    return {'class_name': cls, 'anchor_sizes': [size], 'anchor_rotations': [0, 1.57],
            'anchor_bottom_heights': [bottom], 'align_center': False, 'feature_map_stride': stride,
            'matched_threshold': matched, 'unmatched_threshold': unmatched}


def _dense_head(anchors, predict_when_training_cfg=None):
    return {
        'NAME': 'AnchorHeadSingle', 'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True,
        'DIR_OFFSET': 0.78539, 'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2,
        'ANCHOR_GENERATOR_CONFIG': anchors,
        'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                                   'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
        'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2,
                                         'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}},
    }


KITTI_ANCHORS = [_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45),
                 _anchor('Pedestrian', [0.8, 0.6, 1.73], -0.6, 0.5, 0.35),
                 _anchor('Cyclist', [1.76, 0.6, 1.73], -0.6, 0.5, 0.35)]
WAYMO_ANCHORS = [_anchor('Vehicle', [4.7, 2.1, 1.7], 0, 0.55, 0.4),
                 _anchor('Pedestrian', [0.91, 0.86, 1.73], 0, 0.5, 0.35),
                 _anchor('Cyclist', [1.78, 0.84, 1.78], 0, 0.5, 0.35)]

_BEV = {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [5, 5], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [128, 256],
        'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [256, 256]}


def second_cfg(kind='kitti'):
    anchors = KITTI_ANCHORS if kind == 'kitti' else WAYMO_ANCHORS
    names = ['Car', 'Pedestrian', 'Cyclist'] if kind == 'kitti' else ['Vehicle', 'Pedestrian', 'Cyclist']
    nms_thresh = 0.01 if kind == 'kitti' else 0.7
    return EasyDict({
        'CLASS_NAMES': names,
        'MODEL': {
            'NAME': 'SECONDNet',
            'VFE': {'NAME': 'MeanVFE'},
            'BACKBONE_3D': {'NAME': 'VoxelBackBone8x'},
            'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
            'BACKBONE_2D': dict(_BEV),
            'DENSE_HEAD': _dense_head(anchors),
            'POST_PROCESSING': {
                'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                'EVAL_METRIC': 'kitti',
                'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': nms_thresh,
                               'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
        },
        'OPTIMIZATION': {'BATCH_SIZE_PER_GPU': 4, 'NUM_EPOCHS': 80, 'OPTIMIZER': 'adam_onecycle', 'LR': 0.003,
                         'WEIGHT_DECAY': 0.01, 'MOMENTUM': 0.9, 'MOMS': [0.95, 0.85], 'PCT_START': 0.4,
                         'DIV_FACTOR': 10, 'GRAD_NORM_CLIP': 10},
    })


def second_iou_cfg():
    """values of tools/cfgs/kitti_models/second_iou.yaml: the KITTI SECOND trunk + SECONDHead (7 x 7 BEV grid pooling on the
    512-channel stride-8 map, IoU branch), boxes re-scored by the predicted IoU"""
    c = second_cfg('kitti')
    m = c.MODEL
    m.NAME = 'SECONDNetIoU'
    m.ROI_HEAD = EasyDict({
        'NAME': 'SECONDHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [256, 256], 'IOU_FC': [256, 256], 'DP_RATIO': 0.3,
        'NMS_CONFIG': {
            'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                      'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
            'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                     'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
        'ROI_GRID_POOL': {'GRID_SIZE': 7, 'IN_CHANNEL': 512, 'DOWNSAMPLE_RATIO': 8},
        'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5,
                          'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                          'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
        'LOSS_CONFIG': {'IOU_LOSS': 'BinaryCrossEntropy',
                        'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.0, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}})
    c.OPTIMIZATION.update({'DECAY_STEP_LIST': [35, 45], 'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001, 'LR_WARMUP': False, 'WARMUP_EPOCH': 1})
    return c


def second_multihead_cfg():
    """values of tools/cfgs/kitti_models/second_multihead.yaml: the KITTI SECOND trunk + AnchorHeadMulti (a 64-filter shared 3 x 3
    convolution, one identity head per class with its own class column, every anchor bottom at -1.6) and per-class NMS"""
    c = second_cfg('kitti')
    m = c.MODEL
    anchors = [_anchor('Car', [3.9, 1.6, 1.56], -1.6, 0.6, 0.45), _anchor('Pedestrian', [0.8, 0.6, 1.73], -1.6, 0.5, 0.35),
               _anchor('Cyclist', [1.76, 0.6, 1.73], -1.6, 0.5, 0.35)]
    head = _dense_head(anchors)
    head.update({'NAME': 'AnchorHeadMulti', 'USE_MULTIHEAD': True, 'SEPARATE_MULTIHEAD': True, 'SHARED_CONV_NUM_FILTER': 64,
                 'RPN_HEAD_CFGS': [{'HEAD_CLS_NAME': ['Car']}, {'HEAD_CLS_NAME': ['Pedestrian']}, {'HEAD_CLS_NAME': ['Cyclist']}]})
    m.DENSE_HEAD = EasyDict(head)
    m.POST_PROCESSING = EasyDict({
        'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'MULTI_CLASSES_NMS': True, 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
        'EVAL_METRIC': 'kitti',
        'NMS_CONFIG': {'MULTI_CLASSES_NMS': True, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1, 'NMS_PRE_MAXSIZE': 4096,
                       'NMS_POST_MAXSIZE': 500}})
    c.DATA_CONFIG = EasyDict({'DATASET': 'KittiDataset'})
    c.OPTIMIZATION.update({'DECAY_STEP_LIST': [35, 45], 'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001, 'LR_WARMUP': False, 'WARMUP_EPOCH': 1})
    return c


def voxel_rcnn_cfg():
    """values of tools/cfgs/kitti_models/voxel_rcnn_car.yaml: class Car only, the SECOND trunk with the narrow BEV backbone
    ([64, 128] filters, [128, 128] up-sampling) + VoxelRCNNHead (6^3 grid, voxel-neighbourhood pooling of x_conv2 / x_conv3 /
    x_conv4). DATA_CONFIG.DATA_AUGMENTOR carries the model's own queue: gt_sampling Car:15 (no LIMIT_WHOLE_SCENE), flip about x,
    rotation, scaling; USE_ROAD_PLANE is off for synthetic frames, as in kitti_augmentor_cfg."""
    c = second_cfg('kitti')
    c.CLASS_NAMES = ['Car']
    aug = kitti_augmentor_cfg()
    aug[0].PREPARE = EasyDict({'filter_by_min_points': ['Car:5'], 'filter_by_difficulty': [-1]})
    aug[0].SAMPLE_GROUPS = ['Car:15']
    aug[0].LIMIT_WHOLE_SCENE = False
    c.DATA_CONFIG = EasyDict({'DATASET': 'KittiDataset', 'DATA_AUGMENTOR': {'DISABLE_AUG_LIST': ['placeholder'], 'AUG_CONFIG_LIST': aug}})
    m = c.MODEL
    m.NAME = 'VoxelRCNN'
    m.BACKBONE_2D = EasyDict(dict(_BEV, NUM_FILTERS=[64, 128], NUM_UPSAMPLE_FILTERS=[128, 128]))
    m.DENSE_HEAD = EasyDict(_dense_head(KITTI_ANCHORS[:1]))
    level = lambda radius: {'MLPS': [[32, 32]], 'QUERY_RANGES': [[4, 4, 4]], 'POOL_RADIUS': [radius], 'NSAMPLE': [16],
                            'POOL_METHOD': 'max_pool'}
    m.ROI_HEAD = EasyDict({
        'NAME': 'VoxelRCNNHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [256, 256], 'CLS_FC': [256, 256], 'REG_FC': [256, 256],
        'DP_RATIO': 0.3,
        'NMS_CONFIG': {
            'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                      'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
            'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'USE_FAST_NMS': False, 'SCORE_THRESH': 0.0,
                     'NMS_PRE_MAXSIZE': 2048, 'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
        'ROI_GRID_POOL': {'FEATURES_SOURCE': ['x_conv2', 'x_conv3', 'x_conv4'], 'PRE_MLP': True, 'GRID_SIZE': 6,
                          'POOL_LAYERS': {'x_conv2': level(0.4), 'x_conv3': level(0.8), 'x_conv4': level(1.6)}},
        'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5,
                          'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                          'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
        'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                        'GRID_3D_IOU_LOSS': False,
                        'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                         'rcnn_iou3d_weight': 1.0, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}})
    m.POST_PROCESSING.SCORE_THRESH = 0.3
    m.POST_PROCESSING.NMS_CONFIG.NMS_THRESH = 0.1
    c.OPTIMIZATION.update({'BATCH_SIZE_PER_GPU': 2, 'LR': 0.01, 'DECAY_STEP_LIST': [35, 45], 'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001,
                           'LR_WARMUP': False, 'WARMUP_EPOCH': 1})
    return c


def pointpillar_cfg():
    """values of tools/cfgs/kitti_models/pointpillar.yaml: PillarVFE (one 64-filter PFN layer) on 0.16 x 0.16 x 4 m pillars of at most
    32 points over [0, -39.68, -3, 69.12, 39.68, 1] (a 432 x 496 x 1 grid, 16,000 / 40,000 pillars), PointPillarScatter, the three-block
    BEV backbone and the KITTI anchors at feature_map_stride 2. DATA_CONFIG carries the range and the voxel generator's values (what
    SyntheticDataset(point_cloud_range=, voxel_size=, max_points_per_voxel=, max_num_voxels=) takes) and kitti_augmentor_cfg()'s queue."""
    c = second_cfg('kitti')
    c.DATA_CONFIG = EasyDict({
        'DATASET': 'KittiDataset', 'POINT_CLOUD_RANGE': [0, -39.68, -3, 69.12, 39.68, 1],
        'DATA_PROCESSOR': [
            {'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
            {'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': {'train': True, 'test': False}},
            {'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.16, 0.16, 4], 'MAX_POINTS_PER_VOXEL': 32,
             'MAX_NUMBER_OF_VOXELS': {'train': 16000, 'test': 40000}}],
        'DATA_AUGMENTOR': {'DISABLE_AUG_LIST': ['placeholder'], 'AUG_CONFIG_LIST': kitti_augmentor_cfg()}})
    m = c.MODEL
    m.NAME = 'PointPillar'
    m.VFE = EasyDict({'NAME': 'PillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [64]})
    m.pop('BACKBONE_3D')
    m.MAP_TO_BEV = EasyDict({'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 64})
    m.BACKBONE_2D = EasyDict({'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [3, 5, 5], 'LAYER_STRIDES': [2, 2, 2], 'NUM_FILTERS': [64, 128, 256],
                              'UPSAMPLE_STRIDES': [1, 2, 4], 'NUM_UPSAMPLE_FILTERS': [128, 128, 128]})
    m.DENSE_HEAD = EasyDict(_dense_head([_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45, stride=2),
                                         _anchor('Pedestrian', [0.8, 0.6, 1.73], -0.6, 0.5, 0.35, stride=2),
                                         _anchor('Cyclist', [1.76, 0.6, 1.73], -0.6, 0.5, 0.35, stride=2)]))
    c.OPTIMIZATION.update({'DECAY_STEP_LIST': [35, 45], 'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001, 'LR_WARMUP': False, 'WARMUP_EPOCH': 1})
    return c


def centerpoint_cfg(kind='kitti'):
    """values of tools/cfgs/waymo_models/centerpoint_without_resnet.yaml: the SECOND trunk + CenterHead (one head for the three
    classes, 64 shared channels, two-convolution branches, stride-8 targets with at most 500 objects). kind='waymo': the yaml as it
    stands. kind='kitti': the same model section with the KITTI class names on the KITTI geometry of second_cfg('kitti');
    POST_CENTER_LIMIT_RANGE is the KITTI point-cloud range."""
    assert kind in ('kitti', 'waymo')
    names = ['Car', 'Pedestrian', 'Cyclist'] if kind == 'kitti' else ['Vehicle', 'Pedestrian', 'Cyclist']
    limit = [0, -40, -3, 70.4, 40, 1] if kind == 'kitti' else [-75.2, -75.2, -2, 75.2, 75.2, 4]
    return EasyDict({
        'CLASS_NAMES': names,
        'DATA_CONFIG': {'DATASET': 'KittiDataset' if kind == 'kitti' else 'WaymoDataset'},
        'MODEL': {
            'NAME': 'CenterPoint',
            'VFE': {'NAME': 'MeanVFE'},
            'BACKBONE_3D': {'NAME': 'VoxelBackBone8x'},
            'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
            'BACKBONE_2D': dict(_BEV),
            'DENSE_HEAD': {
                'NAME': 'CenterHead', 'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': [list(names)],
                'SHARED_CONV_CHANNEL': 64, 'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
                'SEPARATE_HEAD_CFG': {
                    'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'],
                    'HEAD_DICT': {'center': {'out_channels': 2, 'num_conv': 2}, 'center_z': {'out_channels': 1, 'num_conv': 2},
                                  'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}},
                'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 8, 'NUM_MAX_OBJS': 500, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
                'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0,
                                                 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}},
                'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': limit, 'MAX_OBJ_PER_SAMPLE': 500,
                                    'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096,
                                                   'NMS_POST_MAXSIZE': 500}}},
            'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'EVAL_METRIC': 'kitti' if kind == 'kitti' else 'waymo'},
        },
        'OPTIMIZATION': {'BATCH_SIZE_PER_GPU': 4, 'NUM_EPOCHS': 30, 'OPTIMIZER': 'adam_onecycle', 'LR': 0.003, 'WEIGHT_DECAY': 0.01,
                         'MOMENTUM': 0.9, 'MOMS': [0.95, 0.85], 'PCT_START': 0.4, 'DIV_FACTOR': 10, 'DECAY_STEP_LIST': [35, 45],
                         'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001, 'LR_WARMUP': False, 'WARMUP_EPOCH': 1, 'GRAD_NORM_CLIP': 10},
    })


def centerpoint_dyn_pillar_cfg():
    """values of tools/cfgs/waymo_models/centerpoint_dyn_pillar_1x.yaml: DynPillarVFE (two PFN layers, dynamic voxelization: no cap on
    points per pillar or on pillars) on 0.32 x 0.32 x 6 m pillars over [-74.88, -74.88, -2, 74.88, 74.88, 4] (a 468 x 468 x 1 grid),
    PointPillarScatter, the three-block BEV backbone with a stride-1 first block and CenterHead at FEATURE_MAP_STRIDE 1."""
    c = centerpoint_cfg('waymo')
    c.DATA_CONFIG = EasyDict({
        'DATASET': 'WaymoDataset', 'POINT_CLOUD_RANGE': [-74.88, -74.88, -2, 74.88, 74.88, 4.0],
        'DATA_PROCESSOR': [
            {'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
            {'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': {'train': True, 'test': True}},
            {'NAME': 'transform_points_to_voxels_placeholder', 'VOXEL_SIZE': [0.32, 0.32, 6.0]}]})
    m = c.MODEL
    m.VFE = EasyDict({'NAME': 'DynPillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [64, 64]})
    m.pop('BACKBONE_3D')
    m.MAP_TO_BEV = EasyDict({'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 64})
    m.BACKBONE_2D = EasyDict({'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [3, 5, 5], 'LAYER_STRIDES': [1, 2, 2], 'NUM_FILTERS': [64, 128, 256],
                              'UPSAMPLE_STRIDES': [1, 2, 4], 'NUM_UPSAMPLE_FILTERS': [128, 128, 128]})
    m.DENSE_HEAD.TARGET_ASSIGNER_CONFIG.FEATURE_MAP_STRIDE = 1
    m.DENSE_HEAD.POST_PROCESSING.POST_CENTER_LIMIT_RANGE = [-80, -80, -10.0, 80, 80, 10.0]
    c.OPTIMIZATION.BATCH_SIZE_PER_GPU = 2
    return c


def centerpoint_dyn_pillar_dataset_args(cfg=None):
    """the keyword arguments that make a SyntheticDataset produce centerpoint_dyn_pillar_cfg()'s grid (Waymo-like frames, 5 features)"""
    d = (cfg or centerpoint_dyn_pillar_cfg()).DATA_CONFIG
    v = [p for p in d.DATA_PROCESSOR if p['NAME'] == 'transform_points_to_voxels_placeholder'][0]
    return {'kind': 'waymo', 'point_cloud_range': list(d.POINT_CLOUD_RANGE), 'voxel_size': list(v['VOXEL_SIZE'])}


def pointpillar_dataset_args(cfg=None):
    """the keyword arguments that make a SyntheticDataset produce pointpillar_cfg()'s grid"""
    d = (cfg or pointpillar_cfg()).DATA_CONFIG
    v = [p for p in d.DATA_PROCESSOR if p['NAME'] == 'transform_points_to_voxels'][0]
    return {'point_cloud_range': list(d.POINT_CLOUD_RANGE), 'voxel_size': list(v['VOXEL_SIZE']),
            'max_points_per_voxel': int(v['MAX_POINTS_PER_VOXEL']), 'max_num_voxels': dict(v['MAX_NUMBER_OF_VOXELS'])}


def pv_rcnn_cfg(kind='kitti'):
    """values of tools/cfgs/active-kitti_models/pv_rcnn_active_crb.yaml; kind='waymo': the differences of
    tools/cfgs/active-waymo_models/pv_rcnn_active_crb.yaml applied on top (anchors, 4096 keypoints, bev/x_conv3/x_conv4/
    raw_points feature sources, NMS sizes and thresholds, K1=3 / K2=2 / SELECT_NUMS=400)"""
    assert kind in ('kitti', 'waymo')
    if kind == 'waymo':
        c = pv_rcnn_cfg('kitti')
        c.CLASS_NAMES = ['Vehicle', 'Pedestrian', 'Cyclist']
        c.DATA_CONFIG.DATASET = 'WaymoDataset'
        m = c.MODEL
        m.DENSE_HEAD = EasyDict(_dense_head(WAYMO_ANCHORS))
        m.PFE.NUM_KEYPOINTS = 4096
        m.PFE.FEATURES_SOURCE = ['bev', 'x_conv3', 'x_conv4', 'raw_points']
        m.POINT_HEAD.NUM_KEYPOINTS = 4096
        m.ROI_HEAD.NMS_CONFIG.TEST.NMS_PRE_MAXSIZE = 4096
        m.ROI_HEAD.NMS_CONFIG.TEST.NMS_THRESH = 0.85
        m.POST_PROCESSING.EVAL_METRIC = 'waymo'
        m.POST_PROCESSING.NMS_CONFIG.NMS_THRESH = 0.7
        c.OPTIMIZATION.WEIGHT_DECAY = 0.001
        c.ACTIVE_TRAIN.update({'PRE_TRAIN_SAMPLE_NUMS': 400, 'SELECT_NUMS': 400, 'TOTAL_BUDGET_NUMS': 2000})
        c.ACTIVE_TRAIN.ACTIVE_CONFIG.update({'K1': 3, 'K2': 2})
        return c
    sa = lambda f, mlp, r, ns: {'DOWNSAMPLE_FACTOR': f, 'MLPS': [list(mlp), list(mlp)], 'POOL_RADIUS': list(r),
                                'NSAMPLE': list(ns)}
    return EasyDict({
        'CLASS_NAMES': ['Car', 'Pedestrian', 'Cyclist'],
        'DATA_CONFIG': {'DATASET': 'KittiDataset'},
        'MODEL': {
            'NAME': 'PVRCNN',
            'VFE': {'NAME': 'MeanVFE'},
            'BACKBONE_3D': {'NAME': 'VoxelBackBone8x'},
            'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
            'BACKBONE_2D': dict(_BEV),
            'DENSE_HEAD': _dense_head(KITTI_ANCHORS),
            'PFE': {
                'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 2048,
                'NUM_OUTPUT_FEATURES': 128, 'SAMPLE_METHOD': 'FPS',
                'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'raw_points'],
                'SA_LAYER': {
                    'raw_points': {'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]},
                    'x_conv1': sa(1, (16, 16), (0.4, 0.8), (16, 16)),
                    'x_conv2': sa(2, (32, 32), (0.8, 1.2), (16, 32)),
                    'x_conv3': sa(4, (64, 64), (1.2, 2.4), (16, 32)),
                    'x_conv4': sa(8, (64, 64), (2.4, 4.8), (16, 32)),
                }},
            'POINT_HEAD': {
                'NAME': 'PointHeadSimple', 'CLS_FC': [256, 256], 'CLASS_AGNOSTIC': True,
                'USE_POINT_FEATURES_BEFORE_FUSION': True, 'NUM_KEYPOINTS': 2048,
                'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]},
                'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0}}},
            'ROI_HEAD': {
                'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True, 'SAMPLING_ROUND': 5, 'SHARED_FC': [256, 256],
                'CLS_FC': [256, 256], 'REG_FC': [256, 256], 'DP_RATIO': 0.3,
                'NMS_CONFIG': {
                    'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                              'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                    'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                             'NMS_POST_MAXSIZE': 128, 'NMS_THRESH': 0.7}},
                'ROI_GRID_POOL': {'GRID_SIZE': 6, 'MLPS': [[64, 64], [64, 64]], 'POOL_RADIUS': [0.8, 1.6],
                                  'NSAMPLE': [16, 16], 'POOL_METHOD': 'max_pool'},
                'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5,
                                  'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                                  'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8,
                                  'REG_FG_THRESH': 0.55},
                'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1',
                                'CORNER_LOSS_REGULARIZATION': True,
                                'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0,
                                                 'rcnn_corner_weight': 1.0,
                                                 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}},
            'POST_PROCESSING': {
                'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                'EVAL_METRIC': 'kitti',
                'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1,
                               'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
        },
        'OPTIMIZATION': {'OPTIMIZER': 'adam_onecycle', 'LR': 0.01, 'WEIGHT_DECAY': 0.01, 'MOMENTUM': 0.9,
                         'MOMS': [0.95, 0.85], 'PCT_START': 0.4, 'DIV_FACTOR': 10, 'GRAD_NORM_CLIP': 10},
        'ACTIVE_TRAIN': {'METHOD': 'crb', 'AGGREGATION': 'mean', 'PRE_TRAIN_SAMPLE_NUMS': 100,
                         'PRE_TRAIN_EPOCH_NUMS': 40, 'TRAIN_RESUME': True, 'SELECT_NUMS': 100,
                         'SELECT_LABEL_EPOCH_INTERVAL': 40, 'TOTAL_BUDGET_NUMS': 600,
                         'ACTIVE_CONFIG': {'K1': 5, 'K2': 3, 'BANDWIDTH': 5, 'CLUSTERING': 'kmeans++'}},
    })


def _vector_pool(kind, reduced, msg, groups, **extra):
    """one VectorPoolAggregationModuleMSG section; groups: (NUM_LOCAL_VOXEL, MAX_NEIGHBOR_DISTANCE, NEIGHBOR_NSAMPLE, POST_MLPS)"""
    d = dict(extra)
    d.update({'NAME': 'VectorPoolAggregationModuleMSG', 'NUM_GROUPS': len(groups), 'LOCAL_AGGREGATION_TYPE': kind,
              'NUM_REDUCED_CHANNELS': reduced, 'NUM_CHANNELS_OF_LOCAL_AGGREGATION': 32, 'MSG_POST_MLPS': list(msg)})
    for k, (grid, dist, nsample, post) in enumerate(groups):
        d['GROUP_CFG_%d' % k] = {'NUM_LOCAL_VOXEL': list(grid), 'MAX_NEIGHBOR_DISTANCE': dist, 'NEIGHBOR_NSAMPLE': nsample,
                                 'POST_MLPS': list(post)}
    return d


def pv_rcnn_plusplus_vector_pool_sections(raw_reduced=2):
    """the four VectorPoolAggregationModuleMSG sections of tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml: SA_LAYER raw_points /
    x_conv3 / x_conv4 (local_interpolation) and ROI_GRID_POOL (voxel_random_choice)"""
    g3 = (3, 3, 3)
    sa = {'raw_points': _vector_pool('local_interpolation', raw_reduced, [32], [((2, 2, 2), 0.2, -1, (32, 32)), (g3, 0.4, -1, (32, 32))],
                                     FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=2.4),
          'x_conv3': _vector_pool('local_interpolation', 32, [128], [(g3, 1.2, -1, (64, 64)), (g3, 2.4, -1, (64, 64))], DOWNSAMPLE_FACTOR=4,
                                  INPUT_CHANNELS=64, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=4.0),
          'x_conv4': _vector_pool('local_interpolation', 32, [128], [(g3, 2.4, -1, (64, 64)), (g3, 4.8, -1, (64, 64))], DOWNSAMPLE_FACTOR=8,
                                  INPUT_CHANNELS=64, FILTER_NEIGHBOR_WITH_ROI=True, RADIUS_OF_NEIGHBOR_WITH_ROI=6.4)}
    pool = _vector_pool('voxel_random_choice', 30, [128], [(g3, 0.8, 32, (64, 64)), (g3, 1.6, 32, (64, 64))], GRID_SIZE=6)
    return sa, pool


def pv_rcnn_plusplus_cfg(kind='kitti', aggregation='sa'):
    """pv_rcnn_cfg(kind) with the PFE section and the RoI-head NMS sizes of tools/cfgs/waymo_models/pv_rcnn_plusplus.yaml: keypoints by
    sectorized proposal-centric sampling (SPC, 6 sectors, 1.6 m around the proposals), feature sources bev / x_conv3 / x_conv4 /
    raw_points with their neighbours filtered by the RoIs (2.4 / 4.0 / 6.4 m), 90 fused features, 100 test RoIs.
    aggregation='sa' (the default): the set-abstraction layers and the RoI grid pool are PV-RCNN's StackSAModuleMSG.
    aggregation='vector_pool': the yaml's four VectorPoolAggregationModuleMSG sections as they stand there; kind='kitti' reduces the
    raw points to 1 channel instead of 2 (KITTI clouds carry one feature, and the layer asserts divisibility)."""
    assert aggregation in ('sa', 'vector_pool')
    c = pv_rcnn_cfg(kind)
    m = c.MODEL
    m.NAME = 'PVRCNNPlusPlus'
    m.PFE.SAMPLE_METHOD = 'SPC'
    m.PFE.SPC_SAMPLING = EasyDict({'NUM_SECTORS': 6, 'SAMPLE_RADIUS_WITH_ROI': 1.6})
    m.PFE.NUM_OUTPUT_FEATURES = 90
    m.PFE.FEATURES_SOURCE = ['bev', 'x_conv3', 'x_conv4', 'raw_points']
    for src, radius in (('raw_points', 2.4), ('x_conv3', 4.0), ('x_conv4', 6.4)):
        m.PFE.SA_LAYER[src].update({'FILTER_NEIGHBOR_WITH_ROI': True, 'RADIUS_OF_NEIGHBOR_WITH_ROI': radius})
    for src in ('x_conv1', 'x_conv2'):
        m.PFE.SA_LAYER.pop(src)
    if aggregation == 'vector_pool':
        sa, pool = pv_rcnn_plusplus_vector_pool_sections(raw_reduced=1 if kind == 'kitti' else 2)
        m.PFE.SA_LAYER = EasyDict(sa)
        m.ROI_HEAD.ROI_GRID_POOL = EasyDict(pool)
    m.ROI_HEAD.pop('SAMPLING_ROUND', None)
    m.ROI_HEAD.NMS_CONFIG.TRAIN.update({'NMS_PRE_MAXSIZE': 9000, 'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8})
    m.ROI_HEAD.NMS_CONFIG.TEST.update({'NMS_PRE_MAXSIZE': 1024, 'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7, 'SCORE_THRESH': 0.1})
    c.ACTIVE_TRAIN.METHOD = 'random'
    c.ACTIVE_TRAIN.pop('ACTIVE_CONFIG', None)
    return c


def parta2_net_cfg(kind='kitti'):
    """values of tools/cfgs/kitti_models/PartA2.yaml; kind='waymo': tools/cfgs/waymo_models/PartA2.yaml (anchors, 4096 / 300 test
    RoIs at 0.85, POOL_SIZE 10, final NMS 0.7). The yamls' anchors differ from the other models': every KITTI class sits at a bottom
    height of -1.78."""
    assert kind in ('kitti', 'waymo')
    waymo = kind == 'waymo'
    if waymo:
        anchors = [_anchor('Vehicle', [4.7, 2.1, 1.7], 0, 0.55, 0.4), _anchor('Pedestrian', [0.91, 0.86, 1.73], 0, 0.5, 0.35),
                   _anchor('Cyclist', [1.78, 0.84, 1.78], 0, 0.5, 0.35)]
    else:
        anchors = [_anchor('Car', [3.9, 1.6, 1.56], -1.78, 0.6, 0.45), _anchor('Pedestrian', [0.8, 0.6, 1.73], -1.78, 0.5, 0.35),
                   _anchor('Cyclist', [1.76, 0.6, 1.73], -1.78, 0.5, 0.35)]
    test_nms = {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 4096 if waymo else 1024,
                'NMS_POST_MAXSIZE': 300 if waymo else 100, 'NMS_THRESH': 0.85 if waymo else 0.7}
    return EasyDict({
        'CLASS_NAMES': ['Vehicle' if waymo else 'Car', 'Pedestrian', 'Cyclist'],
        'DATA_CONFIG': {'DATASET': 'WaymoDataset' if waymo else 'KittiDataset'},
        'MODEL': {
            'NAME': 'PartA2Net',
            'VFE': {'NAME': 'MeanVFE'},
            'BACKBONE_3D': {'NAME': 'UNetV2'},
            'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
            'BACKBONE_2D': dict(_BEV),
            'DENSE_HEAD': _dense_head(anchors),
            'POINT_HEAD': {
                'NAME': 'PointIntraPartOffsetHead', 'CLS_FC': [], 'PART_FC': [], 'CLASS_AGNOSTIC': True,
                'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]},
                'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_part_weight': 1.0}}},
            'ROI_HEAD': {
                'NAME': 'PartA2FCHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [256, 256, 256], 'CLS_FC': [256, 256],
                'REG_FC': [256, 256], 'DP_RATIO': 0.3, 'SEG_MASK_SCORE_THRESH': 0.3,
                'NMS_CONFIG': {
                    'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                              'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                    'TEST': test_nms},
                'ROI_AWARE_POOL': {'POOL_SIZE': 10 if waymo else 12, 'NUM_FEATURES': 128, 'MAX_POINTS_PER_VOXEL': 128},
                'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5,
                                  'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                                  'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.65},
                'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                                'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                                 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}},
            'POST_PROCESSING': {
                'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                'EVAL_METRIC': 'waymo' if waymo else 'kitti',
                'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7 if waymo else 0.1,
                               'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
        },
        'OPTIMIZATION': {'BATCH_SIZE_PER_GPU': 2 if waymo else 4, 'NUM_EPOCHS': 30 if waymo else 80, 'OPTIMIZER': 'adam_onecycle',
                         'LR': 0.01, 'WEIGHT_DECAY': 0.01, 'MOMENTUM': 0.9, 'MOMS': [0.95, 0.85], 'PCT_START': 0.4,
                         'DIV_FACTOR': 10, 'DECAY_STEP_LIST': [35, 45], 'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001,
                         'LR_WARMUP': False, 'WARMUP_EPOCH': 1, 'GRAD_NORM_CLIP': 10},
        'ACTIVE_TRAIN': {'METHOD': 'random', 'PRE_TRAIN_SAMPLE_NUMS': 100, 'SELECT_NUMS': 100, 'TOTAL_BUDGET_NUMS': 600},
    })


def parta2_free_cfg():
    """values of tools/cfgs/kitti_models/PartA2_free.yaml, the anchor-free Part-A2 (MODEL.NAME: PointRCNN): MeanVFE -> UNetV2 without
    the encoded tensor -> PointIntraPartOffsetHead with a box per point -> PartA2FCHead with DISABLE_PART. No BEV backbone, no anchors."""
    return EasyDict({
        'CLASS_NAMES': ['Car', 'Pedestrian', 'Cyclist'],
        'DATA_CONFIG': {'DATASET': 'KittiDataset'},
        'MODEL': {
            'NAME': 'PointRCNN',
            'VFE': {'NAME': 'MeanVFE'},
            'BACKBONE_3D': {'NAME': 'UNetV2', 'RETURN_ENCODED_TENSOR': False},
            'POINT_HEAD': {
                'NAME': 'PointIntraPartOffsetHead', 'CLS_FC': [128, 128], 'PART_FC': [128, 128], 'REG_FC': [128, 128],
                'CLASS_AGNOSTIC': False, 'USE_POINT_FEATURES_BEFORE_FUSION': False,
                'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2], 'BOX_CODER': 'PointResidualCoder',
                                  'BOX_CODER_CONFIG': {'use_mean_size': True,
                                                       'mean_size': [[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]]}},
                'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss',
                                'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_box_weight': 1.0, 'point_part_weight': 1.0,
                                                 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}},
            'ROI_HEAD': {
                'NAME': 'PartA2FCHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [256, 256, 256], 'CLS_FC': [256, 256],
                'REG_FC': [256, 256], 'DP_RATIO': 0.3, 'DISABLE_PART': True, 'SEG_MASK_SCORE_THRESH': 0.0,
                'NMS_CONFIG': {
                    'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                              'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                    'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                             'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.85}},
                'ROI_AWARE_POOL': {'POOL_SIZE': 12, 'NUM_FEATURES': 128, 'MAX_POINTS_PER_VOXEL': 128},
                'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5,
                                  'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                                  'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.65},
                'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                                'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                                 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}},
            'POST_PROCESSING': {
                'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False, 'EVAL_METRIC': 'kitti',
                'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1,
                               'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
        },
        'OPTIMIZATION': {'BATCH_SIZE_PER_GPU': 4, 'NUM_EPOCHS': 80, 'OPTIMIZER': 'adam_onecycle', 'LR': 0.003, 'WEIGHT_DECAY': 0.01,
                         'MOMENTUM': 0.9, 'MOMS': [0.95, 0.85], 'PCT_START': 0.4, 'DIV_FACTOR': 10, 'DECAY_STEP_LIST': [35, 45],
                         'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001, 'LR_WARMUP': False, 'WARMUP_EPOCH': 1, 'GRAD_NORM_CLIP': 10},
    })


def pv_rcnn_llal_cfg():
    """values of tools/cfgs/active-kitti_models/pv_rcnn_active_llal.yaml: the KITTI PV-RCNN with the LLAL loss-prediction module
    (ROI_HEAD.LOSS_NET), no MC-dropout rounds, the loss net frozen during detector training (OPTIMIZATION.LOSS_NET_SKIP) and
    trained for LOSS_NET_TRAIN_EPOCH epochs per selection round"""
    c = pv_rcnn_cfg('kitti')
    h = c.MODEL.ROI_HEAD
    h.pop('SAMPLING_ROUND')
    h.LOSS_NET = EasyDict({'SHARED_FC': [256, 256]})
    h.EMBEDDING_REQUIRED = False
    c.OPTIMIZATION.NUM_EPOCHS = 60
    c.OPTIMIZATION.LOSS_NET_SKIP = True
    c.ACTIVE_TRAIN.METHOD = 'llal'
    c.ACTIVE_TRAIN.LOSS_NET_TRAIN_EPOCH = 10
    c.ACTIVE_TRAIN.pop('ACTIVE_CONFIG')
    return c


def kitti_augmentor_cfg(db_info_path=None, use_road_plane=False, num_point_features=4):
    """DATA_AUGMENTOR of tools/cfgs/dataset_configs/kitti_dataset.yaml:18-44 as a list of step configs: gt_sampling (Car:20,
    Pedestrian:15, Cyclist:15, at least 5 points per object, LIMIT_WHOLE_SCENE), world flip about x, rotation, scaling.
    db_info_path: the DB_INFO_PATH pickles under the augmentor's root_path (None: the database is handed over as db_infos=).
    use_road_plane: the reference's True needs the road planes and the calibration of the real dataset, which synthetic frames do
    not have; data_dict['road_plane'] / ['calib'] are read when it is set."""
    return [
        EasyDict({'NAME': 'gt_sampling', 'USE_ROAD_PLANE': bool(use_road_plane),
                  'DB_INFO_PATH': list(db_info_path) if db_info_path else [],
                  'PREPARE': {'filter_by_min_points': ['Car:5', 'Pedestrian:5', 'Cyclist:5'], 'filter_by_difficulty': [-1]},
                  'SAMPLE_GROUPS': ['Car:20', 'Pedestrian:15', 'Cyclist:15'], 'NUM_POINT_FEATURES': int(num_point_features),
                  'DATABASE_WITH_FAKELIDAR': False, 'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': True}),
        EasyDict({'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']}),
        EasyDict({'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.78539816, 0.78539816]}),
        EasyDict({'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}),
    ]
