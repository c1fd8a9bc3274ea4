"""VectorPool aggregation: case generators, numpy restatements of the three reference kernels (pointnet2_stack/src/
vector_pool_gpu.cu) in f32 with their operation order, and an f64 definition of the interpolation. numpy only: the golden
generator imports this beside the reference, the tests beside the port.

Restatements, one new point ("thread") at a time:
  query_neighbors   query_stacked_local_neighbor_idxs_kernel: the frame walk, local = support - new, the cube / ball test, the list in
                    ascending row order cut after nsample (> 0) and after 1000 (temp_idxs[1000])
  three_nn          query_three_nn_by_stacked_local_idxs_kernel over that list: d = (cx-x)^2 + (cy-y)^2 + (cz-z)^2 in f32, strict <
                    against best1 / best2 / best3 (f64 1e40 at the start), missing slots repeat the first; sqrt as the Python wrapper
  voxel_pool        vector_pool_kernel_stack, pooling_type 1 (random choice), with the launcher's f32 grid sizes; `pick` is the row
                    grouped_idxs records for the cell
  voxel_pool_grad   vector_pool_grad_kernel_stack with the contributions of a row added in ascending (new point, cell) order
"""
import numpy as np

F = np.float32
MAX_CANDIDATES = 1000


def frame_of(m, new_cnt):
    """the kernels' walk: -> frame index of new point m (past the sum: the last frame)"""
    bs, covered = 0, int(new_cnt[0])
    for k in range(1, len(new_cnt)):
        if m < covered:
            break
        covered += int(new_cnt[k])
        bs = k
    return bs


def _in_range(local, dist, neighbor_type):
    """local (n, 3) f32 -> (n) bool kept"""
    lx, ly, lz = local[:, 0], local[:, 1], local[:, 2]
    if neighbor_type == 1:
        return ~((lx * lx + ly * ly + lz * lz) > dist * dist)
    return ~((np.abs(lx) > dist) | (np.abs(ly) > dist) | (np.abs(lz) > dist))


def query_neighbors(support, xyz_cnt, new_xyz, new_cnt, dist, nsample, neighbor_type):
    """-> list (M) of i64 arrays of GLOBAL rows"""
    support, new_xyz, dist = support.astype(F), new_xyz.astype(F), F(dist)
    out = []
    for m in range(len(new_xyz)):
        bs = frame_of(m, new_cnt)
        start, n = int(np.sum(xyz_cnt[:bs])), int(xyz_cnt[bs])
        keep = np.nonzero(_in_range(support[start:start + n] - new_xyz[m], dist, neighbor_type))[0]
        keep = keep[:MAX_CANDIDATES]
        if nsample > 0:
            keep = keep[:nsample]
        out.append(keep + start)
    return out


def three_nn(support, xyz_cnt, new_xyz, new_cnt, centers, dist, nsample, neighbor_type):
    """-> idx (M, G, 3) i32, dist (M, G, 3) f32 (square roots), the lists' lengths (M)"""
    lists = query_neighbors(support, xyz_cnt, new_xyz, new_cnt, dist, nsample, neighbor_type)
    idx, d2 = three_nn_over_lists(support, centers, lists)
    return idx, np.sqrt(d2), np.array([len(v) for v in lists])


def three_nn_over_lists(support, centers, lists):
    """query_three_nn_by_stacked_local_idxs_kernel: lists (M) of global rows -> idx (M, G, 3) i32, squared distances (M, G, 3) f32"""
    support, centers = support.astype(F), centers.astype(F)
    M, G = centers.shape[:2]
    idx = np.full((M, G, 3), -1, np.int32)
    d2 = np.zeros((M, G, 3), F)
    for m in range(M):
        best = np.full((3, G), 1e40, np.float64)
        besti = np.full((3, G), -1, np.int64)
        cx, cy, cz = centers[m, :, 0], centers[m, :, 1], centers[m, :, 2]
        for row in lists[m]:
            x, y, z = support[row]
            d = (cx - x) * (cx - x) + (cy - y) * (cy - y) + (cz - z) * (cz - z)          # f32, left to right
            a = d < best[0]
            b = ~a & (d < best[1])
            c = ~a & ~b & (d < best[2])
            s = a | b
            best[2], besti[2] = np.where(s, best[1], np.where(c, d, best[2])), np.where(s, besti[1], np.where(c, row, besti[2]))
            best[1], besti[1] = np.where(a, best[0], np.where(b, d, best[1])), np.where(a, besti[0], np.where(b, row, besti[1]))
            best[0], besti[0] = np.where(a, d, best[0]), np.where(a, row, besti[0])
        for j in (1, 2):
            miss = besti[j] == -1
            besti[j], best[j] = np.where(miss, besti[0], besti[j]), np.where(miss, best[0], best[j])
        idx[m] = besti.T
        with np.errstate(over='ignore'):
            d2[m] = best.T.astype(F)                                                     # (1e40 -> +inf)
    return idx, d2


def grid_sizes(R, num_grid):
    return [F(R) * F(2) / F(n) for n in num_grid]


def voxel_pool(support, xyz_cnt, feats, new_xyz, new_cnt, num_grid, R, nsample, neighbor_type):
    """-> new_features (M, G C), new_local_xyz (M, 3 G), point_cnt (M, G) i32, pick (M, G) i32"""
    support, new_xyz, feats, R = support.astype(F), new_xyz.astype(F), feats.astype(F), F(R)
    gx, gy, gz = num_grid
    G, C, M = gx * gy * gz, feats.shape[1], len(new_xyz)
    sx, sy, sz = grid_sizes(R, num_grid)
    out_f, out_l = np.zeros((M, G, C), F), np.zeros((M, G, 3), F)
    cnt, pick = np.zeros((M, G), np.int32), np.full((M, G), -1, np.int32)
    for m in range(M):
        bs = frame_of(m, new_cnt)
        start, n = int(np.sum(xyz_cnt[:bs])), int(xyz_cnt[bs])
        local = support[start:start + n] - new_xyz[m]
        keep = _in_range(local, R, neighbor_type)
        ix = np.floor((local[:, 0] + R) / sx).astype(np.int64)
        iy = np.floor((local[:, 1] + R) / sy).astype(np.int64)
        iz = np.floor((local[:, 2] + R) / sz).astype(np.int64)
        cell = np.clip(ix * gy * gz + iy * gz + iz, 0, G - 1)
        sample_cnt = 0
        for k in np.nonzero(keep)[0]:
            g = cell[k]
            if cnt[m, g] == 0:
                cnt[m, g] = 1
                out_f[m, g], out_l[m, g], pick[m, g] = feats[start + k], local[k], start + k
                sample_cnt += 1
                if (nsample > 0 and sample_cnt >= nsample) or sample_cnt >= G:
                    break
    return out_f.reshape(M, G * C), out_l.reshape(M, 3 * G), cnt, pick


def voxel_pool_grad(grad_new_features, pick, N):
    """-> grad_support_features (N, C) f32, row sums in ascending (new point, cell) order"""
    M, G = pick.shape
    g = grad_new_features.astype(F).reshape(M, G, -1)
    out = np.zeros((N, g.shape[2]), F)
    for m in range(M):
        for c in range(G):
            if pick[m, c] >= 0:
                out[pick[m, c]] += g[m, c]
    return out


# ---- the f64 definition of the interpolation (VectorPoolLocalInterpolateModule.forward, pointnet2_modules.py:220-238) ----
def interp_weights_f64(dist):
    r = 1.0 / (dist.astype(np.float64) + 1e-8)
    return r / np.maximum(r.sum(-1, keepdims=True), 1e-8)


def interp_f64(idx, dist, centers, support, feats):
    """-> (M, G, C + 9) f64: interpolated channels, then centre - xyz[idx_j]; empty cells (idx < 0) are zeros"""
    M, G = idx.shape[:2]
    C = feats.shape[1]
    out = np.zeros((M, G, C + 9))
    ok = idx[:, :, 0] >= 0
    if not ok.any():
        return out
    i = np.where(idx < 0, 0, idx)
    w = np.where(ok[:, :, None], interp_weights_f64(np.where(ok[:, :, None], dist, 1.0)), 0.0)
    f, p = feats.astype(np.float64), support.astype(np.float64)
    out[:, :, :C] = (w[..., None] * f[i]).sum(2)
    out[:, :, C:] = (centers.astype(np.float64)[:, :, None, :] - p[i]).reshape(M, G, 9)
    return out * ok[:, :, None]


def interp_grad_f64(idx, dist, grad_out, N):
    """grad_out (M, G, C + 9) -> d loss / d feats (N, C) f64"""
    C = grad_out.shape[2] - 9
    ok = idx[:, :, 0] >= 0
    out = np.zeros((N, C))
    if not ok.any():
        return out
    w = np.where(ok[:, :, None], interp_weights_f64(np.where(ok[:, :, None], dist, 1.0)), 0.0)
    contrib = w[..., None] * grad_out.astype(np.float64)[:, :, None, :C]                # (M, G, 3, C)
    np.add.at(out, np.where(idx < 0, 0, idx)[ok], contrib[ok])
    return out


# ---- cases ----
def grid_centers(new_xyz, R, num_grid):
    """cell centres (M, G, 3) f32, z fastest (VectorPoolAggregationModule.get_dense_voxels_by_center's layout)"""
    axes = [(np.arange(n) * (2.0 * R / n) + (-R + R / n)).astype(F) for n in num_grid]
    off = np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3)
    return (new_xyz.astype(F)[:, None, :] + off[None, :, :]).astype(F)


def _case(name, support, xyz_cnt, new_xyz, new_cnt, grid, R=0.5, mult=2.0, nsample=-1, ntype=0):
    support, new_xyz = np.asarray(support, F).reshape(-1, 3), np.asarray(new_xyz, F).reshape(-1, 3)
    assert sum(xyz_cnt) == len(support) and sum(new_cnt) == len(new_xyz)
    return {'name': name, 'support': support, 'xyz_cnt': np.array(xyz_cnt, np.int32), 'new_xyz': new_xyz,
            'new_cnt': np.array(new_cnt, np.int32), 'grid': tuple(grid), 'R': R, 'mult': mult, 'nsample': nsample, 'ntype': ntype,
            'centers': grid_centers(new_xyz, R, grid)}


def _shell(rng, k, lo, hi):
    """k points with max-norm in [lo, hi] around the origin"""
    p = rng.uniform(-1, 1, (k, 3))
    p /= np.abs(p).max(1, keepdims=True)
    return p * rng.uniform(lo, hi, (k, 1))


def three_nn_cases():
    """name -> case. Every case has M that is no multiple of 4 (the workgroup's rows) unless it is a single new point."""
    rng = np.random.default_rng(2024)
    cases = []
    # three frames: 0, 1 and ~300 support points; one frame without new points
    for grid in ((2, 2, 2), (3, 3, 3), (1, 2, 3)):
        for tag, new_cnt in (('a', (3, 0, 10)), ('b', (0, 2, 9))):
            sup = np.concatenate([[[0.1, -0.2, 0.3]], rng.uniform(-2, 2, (301, 3))])
            new = rng.uniform(-1.8, 1.8, (sum(new_cnt), 3))
            if new_cnt[1]:
                new[new_cnt[0]] = [0.2, 0.0, 0.1]                    # next to frame 1's only point
            cases.append(_case('frames_%d%d%d_%s' % (grid + (tag,)), sup, (0, 1, 301), new, new_cnt, grid, ntype=len(cases) % 2))
    # the only neighbours of frame 0's new point lie in frame 1
    sup = np.concatenate([rng.uniform(50, 60, (20, 3)), rng.uniform(-0.5, 0.5, (30, 3))])
    cases.append(_case('other_frame', sup, (20, 30), [[0, 0, 0], [0.1, 0.1, 0.1], [55, 55, 55]], (1, 2), (3, 3, 3)))
    # k in-range neighbours around one new point, out-of-range points in between
    for k in (1, 2, 3, 63, 64, 65, 129):
        near, far = _shell(rng, k, 0.05, 0.95), _shell(rng, 40, 1.2, 3.0)
        sup = np.concatenate([near, far])[rng.permutation(k + 40)]
        cases.append(_case('count_%d' % k, sup + 5.0, (k + 40,), [[5, 5, 5]], (1,), (3, 3, 3)))
    # 1100 in range, the three nearest at rows >= 1000: they are not seen
    cen = grid_centers(np.zeros((1, 3), F), 0.5, (3, 3, 3))[0]
    sup = np.concatenate([_shell(rng, 1019, 0.5, 0.95), np.repeat(cen, 3, 0) + rng.uniform(-0.01, 0.01, (81, 3))])
    cases.append(_case('past_1000', sup, (1100,), [[0, 0, 0]], (1,), (3, 3, 3)))
    # nsample 5: nearer points after the fifth
    sup = np.concatenate([_shell(rng, 5, 0.7, 0.9), _shell(rng, 30, 0.01, 0.3)])
    cases.append(_case('nsample_5', sup, (35,), [[0, 0, 0], [0.2, 0, 0], [0, 0.1, 0.1]], (3,), (2, 2, 2), nsample=5))
    # lattice: multiples of 1/8, duplicates, exact ties, points exactly on the cube face (|local| = 1.0) / the sphere (0.75)
    lat = rng.integers(-10, 11, (160, 3)) / 8.0
    lat[10:20] = lat[0:10]                                            # duplicates
    face = np.array([[1.0, 0.25, -0.5], [-1.0, 0, 0], [0.5, 1.0, 1.0], [0.125, -1.0, 0.75], [1.125, 0, 0], [0, 0, -1.125]])
    sphere = np.array([[0.75, 0, 0], [0, -0.75, 0], [0.5, 0.5, 0.25], [-0.5, 0.25, 0.5], [0.5, 0.5, 0.375], [0.75, 0.125, 0]])
    new = np.array([[0, 0, 0], [0.25, -0.125, 0.5], [-0.5, 0.5, 0], [0, 0, 0], [1, 1, 1]])
    cases.append(_case('lattice_cube', np.concatenate([face, lat]), (166,), new, (5,), (3, 3, 3), R=0.5, mult=2.0, ntype=0))
    cases.append(_case('lattice_ball', np.concatenate([sphere, lat]), (166,), new, (5,), (2, 2, 2), R=0.5, mult=1.5, ntype=1))
    # no support points at all
    cases.append(_case('n_zero', np.zeros((0, 3)), (0,), rng.uniform(-1, 1, (5, 3)), (5,), (3, 3, 3)))
    return {c['name']: c for c in cases}


def voxel_cases():
    """R = 0.75, (3, 3, 3): the f32 grid size is 0.5 exactly. Coordinates are multiples of 1/8: points at local = +-R, on the cell
    boundaries (local = +-0.25), several points per cell, other frames, a frame without support points, one without new points."""
    rng = np.random.default_rng(77)
    R, grid, C = 0.75, (3, 3, 3), 4
    assert [float(g) for g in grid_sizes(R, grid)] == [0.5] * 3
    edge = np.array([[0.75, 0.75, 0.75], [-0.75, -0.75, -0.75], [0.75, -0.75, 0.25], [-0.25, 0.25, -0.25], [0.25, 0.25, 0.25],
                     [0.25, 0.25, 0.25], [0.0, 0.0, 0.0], [0.125, -0.125, 0.0], [0.875, 0, 0], [-0.75, 0.25, 0.75], [0.75, 0.0, -0.25]])
    lat = rng.integers(-8, 9, (120, 3)) / 8.0
    sup0 = np.concatenate([edge, lat])
    sup2 = rng.integers(-8, 9, (70, 3)) / 8.0 + 4.0
    sup = np.concatenate([sup0, sup2])
    new0 = np.array([[0, 0, 0], [0.125, 0, -0.125], [0.5, 0.5, 0.5], [-0.25, 0.25, 0], [3, 3, 3]])
    new1 = np.array([[0, 0, 0], [4, 4, 4]])
    new2 = np.array([[4, 4, 4], [4.25, 3.75, 4.125], [0, 0, 0], [3.5, 4.5, 4]])
    new = np.concatenate([new0, new1, new2])
    out = {}
    for ntype in (0, 1):
        for nsample in (-1, 5):
            c = _case('voxel_t%d_n%d' % (ntype, nsample), sup, (len(sup0), 0, len(sup2)), new, (5, 2, 4), grid, R=R, nsample=nsample, ntype=ntype)
            c['feats'] = rng.normal(0, 1, (len(sup), C)).astype(F)
            out[c['name']] = c
    c = _case('voxel_no_new_frame', sup, (len(sup0), len(sup2)), new0, (5, 0), grid, R=R)
    c['feats'] = rng.normal(0, 1, (len(sup), C)).astype(F)
    out[c['name']] = c
    c = _case('voxel_n_zero', np.zeros((0, 3)), (0,), new0, (5,), grid, R=R)
    c['feats'] = np.zeros((0, C), F)
    out[c['name']] = c
    return out


def module_case(seed=5, C_in=8):
    """two ragged frames for the module goldens: clustered support points with C_in features, new points on and off the clusters"""
    rng = np.random.default_rng(seed)
    cnt, new_cnt = (180, 140), (21, 16)
    sup = np.concatenate([rng.normal(0, 0.5, (n, 3)) + rng.uniform(-1, 1, (1, 3)) for n in cnt]).astype(F)
    new = np.concatenate([rng.normal(0, 0.6, (n, 3)) for n in new_cnt]).astype(F)
    new[3] = [9, 9, 9]                                                # nothing near: every cell empty
    return {'xyz': sup, 'xyz_cnt': np.array(cnt, np.int32), 'new_xyz': new, 'new_cnt': np.array(new_cnt, np.int32),
            'features': rng.normal(0, 1, (sum(cnt), C_in)).astype(F)}


def module_cfgs():
    """name -> (input channels, config dict): the two aggregation types, 2 groups with different grids"""
    def cfg(kind, reduced, nsample):
        return {'NAME': 'VectorPoolAggregationModuleMSG', 'NUM_GROUPS': 2, 'LOCAL_AGGREGATION_TYPE': kind, 'NUM_REDUCED_CHANNELS': reduced,
                'NUM_CHANNELS_OF_LOCAL_AGGREGATION': 32, 'MSG_POST_MLPS': [32],
                'GROUP_CFG_0': {'NUM_LOCAL_VOXEL': [2, 2, 2], 'MAX_NEIGHBOR_DISTANCE': 0.4, 'NEIGHBOR_NSAMPLE': nsample, 'POST_MLPS': [16, 16]},
                'GROUP_CFG_1': {'NUM_LOCAL_VOXEL': [3, 3, 3], 'MAX_NEIGHBOR_DISTANCE': 0.8, 'NEIGHBOR_NSAMPLE': nsample, 'POST_MLPS': [16, 16]}}
    return {'interp': (8, cfg('local_interpolation', 4, -1)), 'voxel': (8, cfg('voxel_random_choice', 4, 8))}


# named gradients of the detector golden (ref_pvrcnn_plusplus_vp.npz): the non-aggregation ones of tests/golden/_constants.PV_GRADS and
# one separate_local_aggregation_layer, one post_mlps and one msg_post_mlps weight for the PFE and for the RoI head
VP_GRADS = {'backbone_3d.conv_input.0.weight': np.s_[:], 'backbone_3d.conv3.1.0.weight': np.s_[:16],
            'backbone_2d.blocks.0.1.weight': np.s_[:24], 'roi_head.shared_fc_layer.0.weight': np.s_[:, :128],
            'point_head.cls_layers.0.weight': np.s_[:64], 'dense_head.conv_box.weight': np.s_[:],
            'pfe.SA_layers.1.layer_0.separate_local_aggregation_layer.0.weight': np.s_[:216], 'pfe.SA_layers.0.layer_1.post_mlps.0.weight': np.s_[:, :256],
            'pfe.SA_rawpoints.msg_post_mlps.0.weight': np.s_[:],
            'roi_head.roi_grid_pool_layer.layer_0.separate_local_aggregation_layer.0.weight': np.s_[:216],
            'roi_head.roi_grid_pool_layer.layer_1.post_mlps.3.weight': np.s_[:], 'roi_head.roi_grid_pool_layer.msg_post_mlps.0.weight': np.s_[:]}


# ---- the module step of ref_vector_pool.npz on the port (imports the port lazily: the golden generator never calls these) ----
def run_module(name, gold, dev):
    """a training step and an eval pass of the port's VectorPoolAggregationModuleMSG -> dict of arrays named as in the golden"""
    import torch
    from golden._constants import seeded_state
    from pcdet.config import EasyDict
    from pcdet.ops.pointnet2.pointnet2_stack import pointnet2_modules as pm
    t = torch.from_numpy
    c_in, cfg = module_cfgs()[name]
    torch.manual_seed(0)
    mod, c_out = pm.build_local_aggregation_module(c_in, EasyDict(cfg))
    assert c_out == cfg['MSG_POST_MLPS'][-1] and isinstance(mod, pm.VectorPoolAggregationModuleMSG)
    state = seeded_state(mod, 91)
    mc, pre = module_case(), 'module/%s/' % name
    res = {'keys': sorted(mod.state_dict().keys())}
    mod.load_state_dict(state)
    mod.to(dev).train()
    kw = lambda f: dict(xyz=t(mc['xyz']).to(dev), xyz_batch_cnt=t(mc['xyz_cnt']).to(dev), new_xyz=t(mc['new_xyz']).to(dev),
                        new_xyz_batch_cnt=t(mc['new_cnt']).to(dev), features=f, query_group=8)      # (an unknown keyword: ignored)
    feats = t(mc['features']).to(dev).requires_grad_(True)
    _, y = mod(**kw(feats))
    (y * t(gold[pre + 'probe']).to(dev)).sum().backward()
    res.update(out_train=y.detach().cpu().numpy(), grad_features=feats.grad.cpu().numpy(),
               running_mean=mod.msg_post_mlps[1].running_mean.cpu().numpy().copy())
    for k, p in mod.named_parameters():
        res['grad/' + k] = p.grad.cpu().numpy()
    mod.load_state_dict({k: v.to(dev) for k, v in state.items()})
    mod.eval()
    with torch.no_grad():
        _, y = mod(**kw(t(mc['features']).to(dev)))
    res['out_eval'] = y.cpu().numpy()
    return res


def check_module(name, gold, res, out_tol, grad_tol):
    """every array of run_module against the golden, relative to the golden's largest entry; prints each figure before asserting"""
    pre = 'module/%s/' % name
    assert res['keys'] == list(gold[pre + 'keys'])
    worst = {}
    for k, v in res.items():
        if k == 'keys':
            continue
        want = gold[pre + k]
        assert v.shape == want.shape, k
        worst[k] = float(np.abs(v - want).max() / max(np.abs(want).max(), 1e-12))
        print('%-60s %.2e' % (k, worst[k]))
    bad = {k: e for k, e in worst.items() if not e <= (grad_tol if k.startswith('grad') else out_tol)}
    assert not bad, bad
