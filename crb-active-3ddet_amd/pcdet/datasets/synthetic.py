"""Seeded synthetic inputs shared by tests, smoke() and bench.py.
KITTI-shaped LiDAR clouds: 64 beams, +-45 deg azimuth, ground plane + random walls + boxes, cropped to the KITTI range
and resampled to exactly n points. Pure numpy so the CPU box and the GPU box generate identical data."""
import numpy as np

KITTI_RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
KITTI_VOXEL = [0.05, 0.05, 0.1]
WAYMO_RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
WAYMO_VOXEL = [0.1, 0.1, 0.15]
CLASS_SIZES = {1: (3.9, 1.6, 1.56), 2: (0.8, 0.6, 1.73), 3: (1.76, 0.6, 1.73)}   # second.yaml:41,51,61


def _boxes(rng, n_car, n_ped, n_cyc, xr, yr, ground_z):
    out = []
    for cls, cnt in ((1, n_car), (2, n_ped), (3, n_cyc)):
        dx, dy, dz = CLASS_SIZES[cls]
        for _ in range(cnt):
            x = rng.uniform(*xr)
            y = rng.uniform(*yr)
            yaw = rng.uniform(-np.pi, np.pi)
            out.append([x, y, ground_z + dz / 2, dx, dy, dz, yaw, cls])
    return np.asarray(out, dtype=np.float32)


def _ray_box(o, d, box):
    """nearest positive ray/box hit distance (inf if none); o (3,), d (n,3)"""
    cx, cy, cz, dx, dy, dz, yaw = box[:7]
    c, s = np.cos(-yaw), np.sin(-yaw)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    ol = R @ (o - np.array([cx, cy, cz]))
    dl = d @ R.T
    h = np.array([dx, dy, dz]) / 2
    with np.errstate(divide='ignore', invalid='ignore'):
        t1 = (-h - ol) / dl
        t2 = (h - ol) / dl
    lo, hi = np.minimum(t1, t2), np.maximum(t1, t2)
    # NaN-ignoring max / min over the 3 slabs as elementwise fmax / fmin of the columns: the same values as
    # np.nanmax(.., axis=1) / np.nanmin (a max picks one of its inputs), without numpy's slow reduce over a length-3 axis
    # (25 of the 45 ms a frame took)
    tmin = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), lo[:, 2])
    tmax = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), hi[:, 2])
    hit = (tmax >= tmin) & (tmax > 0)
    return np.where(hit, np.maximum(tmin, 0.0), np.inf)


def _box_columns(box, az, margin=2e-3):
    """indices of the azimuth samples inside the azimuth hull of the box footprint (+ margin), or None when the hull is not
    an interval that can be trusted (the sensor is inside / next to the footprint)"""
    cx, cy, _, dx, dy, _, yaw = box[:7]
    c, s = np.cos(yaw), np.sin(yaw)
    hx, hy = dx / 2, dy / 2
    corners = np.array([[cx + sx * hx * c - sy * hy * s, cy + sx * hx * s + sy * hy * c] for sx in (-1, 1) for sy in (-1, 1)])
    if np.hypot(cx, cy) < np.hypot(hx, hy) + 1.0:
        return None
    ac = np.arctan2(cy, cx)
    rel = np.arctan2(corners[:, 1], corners[:, 0]) - ac
    rel = (rel + np.pi) % (2 * np.pi) - np.pi                      # footprint seen from outside: |rel| < pi / 2
    lo, hi = rel.min() - margin, rel.max() + margin
    ra = (az - ac + np.pi) % (2 * np.pi) - np.pi
    return np.nonzero((ra >= lo) & (ra <= hi))[0]


def kitti_frame(frame_idx, n_points=20000, waymo=False):
    """-> points (n,4|5) f32, gt_boxes (G,8) f32 [x,y,z,dx,dy,dz,yaw,cls]"""
    rng = np.random.default_rng(np.random.PCG64(20230501 + int(frame_idx)))
    if waymo:
        rngx = WAYMO_RANGE
        az_lo, az_hi, n_az = -np.pi, np.pi, 2650
        boxes = _boxes(rng, 18, 6, 6, (-65, 65), (-65, 65), -1.73)
        nfeat = 5
    else:
        rngx = KITTI_RANGE
        az_lo, az_hi, n_az = -np.pi / 4, np.pi / 4, 512
        boxes = _boxes(rng, 6, 3, 3, (5, 65), (-30, 30), -1.73)
        nfeat = 4
    elev = np.deg2rad(np.linspace(-24.8, 2.0, 64))
    az = rng.uniform(az_lo, az_hi, n_az)
    wall = np.where(rng.uniform(size=n_az) < 0.5, rng.uniform(8, 70, n_az), np.inf)
    E, A = np.meshgrid(elev, az, indexing='ij')
    d = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    o = np.zeros(3)
    with np.errstate(divide='ignore'):
        t_ground = np.where(d[:, 2] < 0, -1.73 / d[:, 2], np.inf)
    t_wall = np.tile(wall[None, :], (64, 1)).reshape(-1) / np.maximum(np.cos(E).reshape(-1), 1e-6)
    t = np.minimum(t_ground, t_wall)
    # a box can only be hit by rays whose azimuth lies inside the azimuth hull of its footprint: run the ray/box test on
    # those columns of the (elevation, azimuth) grid only. Same arithmetic on the same rows for the rays that are tested,
    # "no hit" (inf) for the others, which is what the full test returns for them — the generated frames are bit-identical
    # (checked against the exhaustive loop on 150 KITTI / Waymo frames), a frame costs 2-3x less.
    d_grid = d.reshape(64, n_az, 3)
    for b in boxes:
        cols = _box_columns(b.astype(np.float64), az)
        if cols is None:
            t = np.minimum(t, _ray_box(o, d, b.astype(np.float64)))
        elif len(cols):
            tb = _ray_box(o, d_grid[:, cols].reshape(-1, 3), b.astype(np.float64)).reshape(64, len(cols))
            tg = t.reshape(64, n_az)
            tg[:, cols] = np.minimum(tg[:, cols], tb)
    ok = np.isfinite(t) & (t < 120)
    t = t[ok] + rng.normal(0, 0.02, ok.sum())
    pts = d[ok] * t[:, None]
    m = ((pts[:, 0] >= rngx[0]) & (pts[:, 0] < rngx[3]) & (pts[:, 1] >= rngx[1]) & (pts[:, 1] < rngx[4]) &
         (pts[:, 2] >= rngx[2]) & (pts[:, 2] < rngx[5]))
    pts = pts[m]
    if len(pts) == 0:
        pts = np.zeros((1, 3))
    sel = rng.choice(len(pts), size=n_points, replace=len(pts) < n_points)
    pts = pts[sel]
    if len(sel) > len(np.unique(sel)):          # duplicated samples get a little jitter
        pts = pts + rng.normal(0, 0.01, pts.shape)
    feats = [rng.uniform(0, 1, (n_points, 1))]
    if nfeat == 5:
        feats.append(rng.uniform(0, 1.5, (n_points, 1)))
    out = np.concatenate([pts] + feats, axis=1).astype(np.float32)
    return out, boxes


def kitti_batch(first_frame, batch_size, n_points=20000, waymo=False):
    """-> points (B*n, C) f32, frame_offsets (B+1) i32, gt_boxes (B,G,8) f32"""
    ps, bs = [], []
    for i in range(batch_size):
        p, b = kitti_frame(first_frame + i, n_points, waymo)
        ps.append(p)
        bs.append(b)
    off = np.concatenate([[0], np.cumsum([len(p) for p in ps])]).astype(np.int32)
    return np.concatenate(ps), off, np.stack(bs)


def random_sparse_coords(rng, n, batch_size, shape_dhw, clustered=True):
    """unique active sites (n,4) i32 [b,z,y,x], in random row order"""
    D, H, W = shape_dhw
    if clustered:
        centers = np.stack([rng.integers(0, batch_size, 64), rng.integers(0, D, 64), rng.integers(0, H, 64),
                            rng.integers(0, W, 64)], axis=1)
        c = centers[rng.integers(0, 64, n * 2)]
        off = np.round(rng.normal(0, 2.5, (n * 2, 3))).astype(np.int64)
        pts = np.concatenate([c[:, :1], c[:, 1:] + off], axis=1)
        ok = ((pts[:, 1] >= 0) & (pts[:, 1] < D) & (pts[:, 2] >= 0) & (pts[:, 2] < H) & (pts[:, 3] >= 0) &
              (pts[:, 3] < W))
        pts = pts[ok]
    else:
        pts = np.stack([rng.integers(0, batch_size, n * 2), rng.integers(0, D, n * 2), rng.integers(0, H, n * 2),
                        rng.integers(0, W, n * 2)], axis=1)
    _, first = np.unique(pts, axis=0, return_index=True)
    pts = pts[np.sort(first)][:n]
    return np.ascontiguousarray(pts.astype(np.int32))


# --- evaluation side of the synthetic KITTI frames: one fixed KITTI-like calibration and the frames' ground truth in KITTI form ---
KITTI_P2 = [[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]
KITTI_R0 = [[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]]
KITTI_TR_VELO2CAM = [[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                     [0.9998621, 0.00752379, 0.01480755, -0.2717806]]
KITTI_IMAGE_SHAPE = (375, 1242)                     # (height, width)
KITTI_CLASS_NAMES = ('Car', 'Pedestrian', 'Cyclist')    # class ids 1, 2, 3 of kitti_frame's boxes
TRUNCATION_LEVELS = (0.0, 0.2, 0.4, 0.6)


class Calibration(object):
    """the reference Calibration's coordinate changes (pcdet/utils/calibration_kitti.py) for matrices P2 (3, 4), R0 (3, 3),
    Tr_velo2cam (3, 4); f64 unless the matrices are given in another type. Without arguments: the synthetic frames' calibration."""

    def __init__(self, calib=None):
        calib = calib or {'P2': np.array(KITTI_P2), 'R0': np.array(KITTI_R0), 'Tr_velo2cam': np.array(KITTI_TR_VELO2CAM)}
        self.P2, self.R0, self.V2C = calib['P2'], calib['R0'], calib['Tr_velo2cam']
        self.cu, self.cv, self.fu, self.fv = self.P2[0, 2], self.P2[1, 2], self.P2[0, 0], self.P2[1, 1]
        self.tx, self.ty = self.P2[0, 3] / (-self.fu), self.P2[1, 3] / (-self.fv)

    @staticmethod
    def cart_to_hom(pts):
        return np.hstack((pts, np.ones((pts.shape[0], 1), dtype=pts.dtype)))

    def lidar_to_rect(self, pts_lidar):
        return self.cart_to_hom(pts_lidar) @ (self.V2C.T @ self.R0.T)

    def rect_to_lidar(self, pts_rect):
        m = np.eye(4, dtype=self.R0.dtype)
        m[:3, :3] = self.R0
        v = np.eye(4, dtype=self.V2C.dtype)
        v[:3] = self.V2C
        return (self.cart_to_hom(pts_rect) @ np.linalg.inv((m @ v).T))[:, 0:3]

    def rect_to_img(self, pts_rect):
        """-> pixel coordinates (N, 2), depth in the rect camera frame (N)"""
        hom = self.cart_to_hom(pts_rect) @ self.P2.T
        return hom[:, 0:2] / pts_rect[:, 2:3], hom[:, 2] - self.P2[2, 3]

    def lidar_to_img(self, pts_lidar):
        return self.rect_to_img(self.lidar_to_rect(pts_lidar))

    def img_to_rect(self, u, v, depth_rect):
        x = ((u - self.cu) * depth_rect) / self.fu + self.tx
        y = ((v - self.cv) * depth_rect) / self.fv + self.ty
        return np.stack([x, y, depth_rect], axis=1)


def kitti_frame_boxes(frame_idx):
    """the gt_boxes of kitti_frame(frame_idx) without its points (the boxes are the generator's first draws)"""
    rng = np.random.default_rng(np.random.PCG64(20230501 + int(frame_idx)))
    return _boxes(rng, 6, 3, 3, (5, 65), (-30, 30), -1.73)


def kitti_frame_annos(frame_idx):
    """ground truth of a synthetic KITTI frame as a KITTI anno dict, from its lidar boxes through the calibration above:
    location / dimensions (l, h, w) / rotation_y in the rect camera frame, bbox the clipped projection, alpha = -atan2(-y, x) + ry
    (lidar x, y). Occlusion and truncation are not in the scene; they follow the indices so that every difficulty occurs:
    Boxes the camera does not see are left out ('index': the rows of kitti_frame's gt_boxes that are kept).
    occluded = (frame + box) % 4 and truncated = TRUNCATION_LEVELS[occluded], so a quarter of the boxes can count as easy, a quarter
    from moderate on, a quarter as hard only and a quarter never (the image-box height decides the rest)."""
    from ..utils import box_utils
    boxes = kitti_frame_boxes(frame_idx).astype(np.float64)
    calib = Calibration()
    cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes[:, :7], calib)
    bbox = box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=KITTI_IMAGE_SHAPE)
    # KITTI labels what the camera sees: a box whose clipped projection has no area (beside or behind the image) is left out
    seen = np.nonzero((cam[:, 2] > 0) & (bbox[:, 2] > bbox[:, 0]) & (bbox[:, 3] > bbox[:, 1]))[0]
    boxes, cam, bbox = boxes[seen], cam[seen], bbox[seen]
    level = (int(frame_idx) + seen) % 4
    return {'name': np.array(KITTI_CLASS_NAMES)[boxes[:, 7].astype(np.int64) - 1], 'truncated': np.array(TRUNCATION_LEVELS)[level],
            'occluded': level.astype(np.int64), 'alpha': -np.arctan2(-boxes[:, 1], boxes[:, 0]) + cam[:, 6], 'bbox': bbox,
            'dimensions': cam[:, 3:6], 'location': cam[:, 0:3], 'rotation_y': cam[:, 6], 'score': -np.ones(len(boxes)),
            'gt_boxes_lidar': boxes[:, :7], 'index': seen}


class FrameInfo(dict):
    """an entry of kitti_infos; info['annos'] of a KITTI frame is made on first use and kept"""

    def __missing__(self, key):
        if key != 'annos' or self.get('kind', 'kitti') != 'kitti':
            raise KeyError(key)
        self['annos'] = kitti_frame_annos(self['frame_id'])
        return self['annos']
