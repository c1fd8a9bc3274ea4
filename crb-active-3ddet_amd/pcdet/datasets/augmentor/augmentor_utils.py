"""World augmentation arithmetic on host arrays (pcdet/datasets/augmentor/augmentor_utils.py:8-81,124-175 of the reference).

This file is the arithmetic definition that crbhip.augment (csrc/augment.hip) reproduces bit for bit. Everything is f32 with
one rounding per operation: every scalar that meets an array is an np.float32, and numpy rounds each elementwise product, sum
and difference on its own. The random draws are separate functions (`draw_*`) so that the device route
(DeviceDataAugmentor) consumes np.random with the same calls in the same order and only the arithmetic moves to the GPU.

A step at its identity value is skipped rather than computed ((c, s) = (1, 0), scale 1, offset 0): x + 0.0 turns -0.0 into
+0.0, and identity parameters are required to leave every bit of a frame alone.

gt_boxes (G, 7 + C): [x, y, z, dx, dy, dz, heading, (vx, vy), ...]; points (N, 3 + C). The flips, the scaling and the
translation update their arguments in place and return them; the rotation returns a new points array (as the reference does)."""
import numpy as np

PI_F = np.float32(np.pi)
TWO_PI_F = np.float32(2 * np.pi)


# ---- draws: the reference's np.random calls -----------------------------------------------------------------------------------
def draw_flip():
    return bool(np.random.choice([False, True], replace=False, p=[0.5, 0.5]))


def draw_uniform(lo, hi):
    return float(np.random.uniform(lo, hi))


def scaling_is_drawn(scale_range):
    """a range narrower than 1e-3 means no scaling and NO draw (augmentor_utils.py:75-76)"""
    return not (scale_range[1] - scale_range[0] < 1e-3)


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------
def rotation_cs(angle):
    """f64 angle -> (c, s) = (f32(cos a), f32(sin a))"""
    return np.float32(np.cos(np.float64(angle))), np.float32(np.sin(np.float64(angle)))


def _rot_xy(x, y, c, s):
    return x * c - y * s, x * s + y * c


def flip_along_x(gt_boxes, points):
    gt_boxes[:, 1] = -gt_boxes[:, 1]
    gt_boxes[:, 6] = -gt_boxes[:, 6]
    points[:, 1] = -points[:, 1]
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 8] = -gt_boxes[:, 8]
    return gt_boxes, points


def flip_along_y(gt_boxes, points):
    gt_boxes[:, 0] = -gt_boxes[:, 0]
    gt_boxes[:, 6] = -(gt_boxes[:, 6] + PI_F)
    points[:, 0] = -points[:, 0]
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 7] = -gt_boxes[:, 7]
    return gt_boxes, points


def rotate(gt_boxes, points, angle):
    c, s = rotation_cs(angle)
    points = points.copy()
    if c == 1 and s == 0:
        return gt_boxes, points
    points[:, 0], points[:, 1] = _rot_xy(points[:, 0].copy(), points[:, 1].copy(), c, s)
    gt_boxes[:, 0], gt_boxes[:, 1] = _rot_xy(gt_boxes[:, 0].copy(), gt_boxes[:, 1].copy(), c, s)
    gt_boxes[:, 6] += np.float32(angle)
    if gt_boxes.shape[1] > 7:
        gt_boxes[:, 7], gt_boxes[:, 8] = _rot_xy(gt_boxes[:, 7].copy(), gt_boxes[:, 8].copy(), c, s)
    return gt_boxes, points


def scale(gt_boxes, points, factor):
    k = np.float32(factor)
    if k != 1:
        points[:, :3] *= k
        gt_boxes[:, :6] *= k
    return gt_boxes, points


def translate(gt_boxes, points, axis, offset):
    t = np.float32(offset)
    if t != 0:
        col = 'xyz'.index(axis)
        points[:, col] += t
        gt_boxes[:, col] += t
    return gt_boxes, points


def limit_heading(heading):
    """limit_period(heading, offset=0.5, period=2 pi) as h - floor(h / f32(2 pi) + 0.5) * f32(2 pi)"""
    return heading - np.floor(heading / TWO_PI_F + np.float32(0.5)) * TWO_PI_F


# ---- the reference's entry points: draw, then apply ---------------------------------------------------------------------------
def random_flip_along_x(gt_boxes, points):
    return flip_along_x(gt_boxes, points) if draw_flip() else (gt_boxes, points)


def random_flip_along_y(gt_boxes, points):
    return flip_along_y(gt_boxes, points) if draw_flip() else (gt_boxes, points)


def global_rotation(gt_boxes, points, rot_range):
    return rotate(gt_boxes, points, draw_uniform(rot_range[0], rot_range[1]))


def global_scaling(gt_boxes, points, scale_range):
    if not scaling_is_drawn(scale_range):
        return gt_boxes, points
    return scale(gt_boxes, points, draw_uniform(scale_range[0], scale_range[1]))


def random_translation_along_x(gt_boxes, points, offset_range):
    return translate(gt_boxes, points, 'x', draw_uniform(offset_range[0], offset_range[1]))


def random_translation_along_y(gt_boxes, points, offset_range):
    return translate(gt_boxes, points, 'y', draw_uniform(offset_range[0], offset_range[1]))


def random_translation_along_z(gt_boxes, points, offset_range):
    return translate(gt_boxes, points, 'z', draw_uniform(offset_range[0], offset_range[1]))


# ---- the box range test with the device kernel's corner expression -------------------------------------------------------------
_CORNER_SIGNS = np.array([[0.5, 0.5, -0.5], [0.5, -0.5, -0.5], [-0.5, -0.5, -0.5], [-0.5, 0.5, -0.5],
                          [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [-0.5, -0.5, 0.5], [-0.5, 0.5, 0.5]], dtype=np.float32)


def box_corners_f32(boxes):
    """(G, 7+) f32 -> (G, 8, 3): box_utils.boxes_to_corners_3d with the rotation written out as separately rounded f32 products
    and c = f32(cos(f64 heading)), s = f32(sin(f64 heading)) (boxes_to_corners_3d goes through torch.cos and a matmul, which
    may fuse or reorder; this is the expression crb_augment_boxes evaluates)"""
    boxes = np.asarray(boxes, dtype=np.float32)
    c = np.cos(boxes[:, 6].astype(np.float64)).astype(np.float32)[:, None]
    s = np.sin(boxes[:, 6].astype(np.float64)).astype(np.float32)[:, None]
    lx = boxes[:, 3:4] * _CORNER_SIGNS[None, :, 0]
    ly = boxes[:, 4:5] * _CORNER_SIGNS[None, :, 1]
    lz = boxes[:, 5:6] * _CORNER_SIGNS[None, :, 2]
    cx = (lx * c - ly * s) + boxes[:, 0:1]
    cy = (lx * s + ly * c) + boxes[:, 1:2]
    cz = lz + boxes[:, 2:3]
    return np.stack([cx, cy, cz], axis=-1)


def mask_boxes_outside_range_f32(boxes, limit_range, min_num_corners=1):
    """box_utils.mask_boxes_outside_range_numpy's rule on box_corners_f32's corners"""
    if boxes.shape[0] == 0:
        return np.zeros((0,), dtype=bool)
    corners = box_corners_f32(boxes)
    lr = np.asarray(limit_range, dtype=np.float32)
    inside = ((corners >= lr[0:3]) & (corners <= lr[3:6])).all(axis=2)
    return inside.sum(axis=1) >= min_num_corners
