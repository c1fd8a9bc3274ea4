"""Shared inputs and the f64 definition for the SECOND-IoU tests (tests/test_second_iou_cpu.py, tests/test_second_iou_gpu.py) and
their golden generator (tests/golden/make_goldens_second_iou.py). No reference import here: this module travels with the tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_second_iou.npz')

# pool case: a deliberately non-square map (an H / W swap fails), 0.4 m cells = VOXEL_SIZE 0.05 x DOWNSAMPLE_RATIO 8
POOL_B, POOL_H, POOL_W, POOL_C, POOL_R = 2, 25, 22, 8, 16
POOL_PCR = [0.0, -5.0, -3.0, 8.8, 5.0, 1.0]            # 22 x 25 cells of 0.4 m
POOL_VOXEL = [0.05, 0.05, 0.1]
POOL_RATIO = 8
POOL_GRIDS = (7, 4)
# rows of a frame's RoI list with a fixed role (pool_case_rois)
ROW_OUTSIDE, ROW_PADDING, ROW_BIG_ANGLE, ROW_ANGLE_0, ROW_ANGLE_HALF_PI, ROW_TINY = 9, 10, 11, 12, 13, 14

HEAD_SHARED_FC, HEAD_IOU_FC, HEAD_ROI_PER_IMAGE = [32, 32], [32, 32], 16
HEAD_SEED = 83
LOSS_KINDS = ('BinaryCrossEntropy', 'L2', 'smoothL1')

DET_FIRST_FRAME, DET_POINTS = 40, 8000
DET_GRADS = {'backbone_3d.conv_input.0.weight': np.s_[:], 'backbone_2d.blocks.0.1.weight': np.s_[:8],
             'roi_head.shared_fc_layer.0.weight': np.s_[:, :128], 'roi_head.iou_layers.7.weight': np.s_[:],
             'roi_head.iou_layers.7.bias': np.s_[:]}
DET_POOLED = np.s_[::4, ::64]
DET_SCORE_WEIGHTS = {'iou': 0.7, 'cls': 0.3}


def pool_geometry():
    """x_min, y_min, cell_x, cell_y of the pool case"""
    return POOL_PCR[0], POOL_PCR[1], POOL_VOXEL[0] * POOL_RATIO, POOL_VOXEL[1] * POOL_RATIO


def pool_case_rois(rng):
    """(B, 16, 7) f32 RoIs fixed by construction: rows 0-4 fully inside the map; 5-8 straddle the x-min / x-max / y-min / y-max
    border; 9 fully outside; 10 an all-zero padding row; 11 |rz| > pi; 12 rz = 0; 13 rz = pi/2; 14 smaller than one cell; 15 inside
    with rz < -pi"""
    x0, y0, x1, y1 = POOL_PCR[0], POOL_PCR[1], POOL_PCR[3], POOL_PCR[4]
    rois = np.zeros((POOL_B, POOL_R, 7), np.float32)
    for b in range(POOL_B):
        def inside(rz=None, dx=None, dy=None):
            return [rng.uniform(x0 + 2.5, x1 - 2.5), rng.uniform(y0 + 2.5, y1 - 2.5), rng.uniform(-1.5, -0.5),
                    rng.uniform(0.8, 2.0) if dx is None else dx, rng.uniform(0.5, 1.5) if dy is None else dy, rng.uniform(1.4, 1.8),
                    rng.uniform(-np.pi, np.pi) if rz is None else rz]
        rows = [inside() for _ in range(5)]
        for cx, cy in ((x0 + 0.1, None), (x1 - 0.1, None), (None, y0 + 0.05), (None, y1 - 0.1)):
            r = inside()
            r[0] = r[0] if cx is None else cx
            r[1] = r[1] if cy is None else cy
            rows.append(r)
        out = inside()
        out[0], out[1] = x1 + 11.0, y1 + 15.0
        rows.append(out)
        rows.append([0.0] * 7)
        rows.append(inside(rz=4.0 + 0.1 * b))
        rows.append(inside(rz=0.0))
        rows.append(inside(rz=float(np.float32(np.pi / 2))))
        rows.append(inside(dx=0.1, dy=0.15))
        rows.append(inside(rz=-3.5 - 0.1 * b))
        rois[b] = np.array(rows, np.float32)
    return rois


def pool_case_inputs():
    """bev (B,H,W,C) NHWC random normal, rois (B,16,7), two more RoI columns for the row-stride-9 variant"""
    rng = np.random.default_rng(HEAD_SEED + 1)
    bev = rng.normal(0, 1, (POOL_B, POOL_H, POOL_W, POOL_C)).astype(np.float32)
    rois = pool_case_rois(rng)
    extra = rng.normal(0, 1, (POOL_B, POOL_R, 2)).astype(np.float32)
    return bev, rois, extra


def pool_f64(bev, rois, G, x_min, y_min, cell_x, cell_y):
    """the pooling's definition in f64: bev (B,H,W,C), rois (B,R,7+) -> (B*R, C, G, G). affine_grid / grid_sample with
    align_corners=False, bilinear, zero padding, theta as SECONDHead.roi_grid_pool writes it (the W - 1 convention)."""
    bev, rois = np.asarray(bev, np.float64), np.asarray(rois, np.float64)
    B, H, W, C = bev.shape
    R = rois.shape[1]
    out = np.zeros((B * R, C, G, G), np.float64)
    idx = np.arange(G)
    u = ((2 * idx + 1) / G - 1)[None, :].repeat(G, 0)            # (j, i): column i
    v = ((2 * idx + 1) / G - 1)[:, None].repeat(G, 1)            # (j, i): row j
    for b in range(B):
        for r in range(R):
            x, y, dx, dy, rz = rois[b, r, 0], rois[b, r, 1], rois[b, r, 3], rois[b, r, 4], rois[b, r, 6]
            x1, x2 = (x - dx / 2 - x_min) / cell_x, (x + dx / 2 - x_min) / cell_x
            y1, y2 = (y - dy / 2 - y_min) / cell_y, (y + dy / 2 - y_min) / cell_y
            c, s = np.cos(rz), np.sin(rz)
            W1, H1 = W - 1, H - 1
            gx = (x2 - x1) / W1 * c * u + (x2 - x1) / W1 * (-s) * v + (x1 + x2 - W + 1) / W1
            gy = (y2 - y1) / H1 * s * u + (y2 - y1) / H1 * c * v + (y1 + y2 - H + 1) / H1
            ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
            fx, fy = np.floor(ix), np.floor(iy)
            acc = np.zeros((G, G, C))
            for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
                cx, cy = fx + ox, fy + oy
                w = (1 - np.abs(ix - cx)) * (1 - np.abs(iy - cy))
                ok = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
                xi, yi = np.clip(cx, 0, W - 1).astype(np.int64), np.clip(cy, 0, H - 1).astype(np.int64)
                acc += np.where(ok, w, 0.0)[..., None] * bev[b, yi, xi]
            out[b * R + r] = acc.transpose(2, 0, 1)
    return out


def head_cfg(dp_ratio=0.0, iou_loss='BinaryCrossEntropy', in_channel=POOL_C, grid=7):
    """ROI_HEAD of kitti_models/second_iou.yaml scaled down to the pool case (plain dicts: each side wraps them in its own EasyDict)"""
    return {'NAME': 'SECONDHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': list(HEAD_SHARED_FC), 'IOU_FC': list(HEAD_IOU_FC),
            'DP_RATIO': dp_ratio,
            'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                     'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                           'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                                    'NMS_POST_MAXSIZE': 100, 'NMS_THRESH': 0.7}},
            'ROI_GRID_POOL': {'GRID_SIZE': grid, 'IN_CHANNEL': in_channel, 'DOWNSAMPLE_RATIO': POOL_RATIO},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': HEAD_ROI_PER_IMAGE, 'FG_RATIO': 0.5,
                              'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75,
                              'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
            'LOSS_CONFIG': {'IOU_LOSS': iou_loss,
                            'LOSS_WEIGHTS': {'rcnn_iou_weight': 1.0, 'code_weights': [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}}}


def dataset_cfg_dict():
    return {'POINT_CLOUD_RANGE': list(POOL_PCR), 'DATA_PROCESSOR': [{'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': list(POOL_VOXEL)}]}


def head_sample():
    """the injected RoI sample of the head's training step: what ProposalTargetLayer.sample_rois_for_rcnn returns for the pool
    case's RoIs (rois, gt_of_rois (B,P,8), max IoUs in [0, 1], roi scores, roi labels)"""
    rng = np.random.default_rng(HEAD_SEED + 2)
    _, rois, _ = pool_case_inputs()
    gt = np.concatenate([rois + rng.normal(0, 0.1, rois.shape).astype(np.float32),
                         rng.integers(1, 4, rois.shape[:2] + (1,)).astype(np.float32)], -1)
    ious = rng.uniform(0, 1, rois.shape[:2]).astype(np.float32)
    scores = rng.normal(0, 1, rois.shape[:2]).astype(np.float32)
    labels = rng.integers(1, 4, rois.shape[:2]).astype(np.int64)
    return rois, gt, ious, scores, labels
