"""VectorPool aggregation of PV-RCNN++ (csrc/vector_pool.hip): what three_nn_for_vector_pool_by_two_step, the body of
VectorPoolLocalInterpolateModule.forward and vector_pool_with_voxel_query_op (voxel_random_choice) of the reference compute, without
its neighbour lists, cursors, retries and read-backs.

three_nn         support_xyz (N, 3), counts, new_xyz (M, 3), grid centres (M, G, 3) -> idx (M, G, 3) i32, dist (M, G, 3) f32
interpolate      idx, dist, centres, support_xyz, features (N, C) -> (G, M, C + 9): interpolated channels + centre - xyz[idx_j];
                 differentiable in the features (inverse lists by a stable sort, fixed summation order)
voxel_pool       -> new_features (M, G C), new_local_xyz (M, 3 G), point_cnt (M, G) i32, pick (M, G) i32; differentiable likewise

Row counts per frame are (B) integer tensors on the device. G <= 64."""
import torch
from torch.autograd import Function

from ._lib import lib, check, ptr, cur_stream, require_cuda, CrbHipError

MAX_CELLS = 64


def _f32(t, shape, what):
    if t.dtype != torch.float32 or t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise CrbHipError('crb_vector_pool: %s f32 of shape %s expected, got %s %s' % (what, shape, t.dtype, tuple(t.shape)))
    return t.contiguous()


def _cnt(t, dev):
    return torch.as_tensor(t).to(device=dev, dtype=torch.int32).contiguous().view(-1)


@torch.no_grad()
def three_nn(support_xyz, xyz_batch_cnt, new_xyz, grid_centers, new_xyz_batch_cnt, query_dist, nsample, neighbor_type):
    require_cuda(support_xyz, new_xyz, grid_centers)
    support_xyz, new_xyz = _f32(support_xyz, (None, 3), 'support_xyz'), _f32(new_xyz, (None, 3), 'new_xyz')
    M = int(new_xyz.shape[0])
    grid_centers = _f32(grid_centers, (M, None, 3), 'new_xyz_grid_centers')
    G, dev = int(grid_centers.shape[1]), new_xyz.device
    if not 0 < G <= MAX_CELLS:
        raise CrbHipError('crb_vector_pool_three_nn: 1 .. %d cells per new point, got %d' % (MAX_CELLS, G))
    a, b = _cnt(xyz_batch_cnt, dev), _cnt(new_xyz_batch_cnt, dev)
    if a.shape != b.shape:
        raise CrbHipError('crb_vector_pool_three_nn: xyz_batch_cnt and new_xyz_batch_cnt differ in length')
    idx = torch.empty((M, G, 3), dtype=torch.int32, device=dev)
    dist = torch.empty((M, G, 3), dtype=torch.float32, device=dev)
    check(lib.crb_vector_pool_three_nn(ptr(support_xyz), int(support_xyz.shape[0]), ptr(a), ptr(new_xyz), M, ptr(b), int(a.shape[0]),
                                       ptr(grid_centers), G, float(query_dist), int(nsample), int(neighbor_type), ptr(idx), ptr(dist),
                                       cur_stream(dev)), 'crb_vector_pool_three_nn')
    return idx, dist


def inverse_lists(rows):
    """rows (...) i32 -> (sorted rows (E) i32 ascending, order (E) i64): the stable sort that fixes the summation order"""
    srt, order = torch.sort(rows.reshape(-1), stable=True)
    return srt.contiguous(), order.contiguous()


class _Interpolate(Function):
    @staticmethod
    def forward(ctx, features, idx, dist, grid_centers, support_xyz):
        require_cuda(features, idx, dist, grid_centers, support_xyz)
        M, G = int(idx.shape[0]), int(idx.shape[1])
        features = _f32(features, (None, None), 'features')
        N, C = int(features.shape[0]), int(features.shape[1])
        support_xyz, dist = _f32(support_xyz, (N, 3), 'support_xyz'), _f32(dist, (M, G, 3), 'dist')
        grid_centers = _f32(grid_centers, (M, G, 3), 'new_xyz_grid_centers')
        if idx.dtype != torch.int32 or idx.shape != (M, G, 3):
            raise CrbHipError('crb_vector_pool_interp_forward: idx (M, G, 3) i32 expected')
        idx = idx.contiguous()
        out = torch.empty((G, M, C + 9), dtype=torch.float32, device=features.device)
        check(lib.crb_vector_pool_interp_forward(ptr(idx), ptr(dist), ptr(grid_centers), ptr(support_xyz), ptr(features), N, M, G, C,
                                                 ptr(out), cur_stream(out.device)), 'crb_vector_pool_interp_forward')
        ctx.save_for_backward(idx, dist)
        ctx.dims = (N, M, G, C)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx, dist = ctx.saved_tensors
        N, M, G, C = ctx.dims
        grad = torch.empty((N, C), dtype=torch.float32, device=grad_out.device)
        srt, order = inverse_lists(idx)
        g = grad_out.contiguous().float()
        check(lib.crb_vector_pool_interp_backward(ptr(g), ptr(dist), ptr(srt), ptr(order), N, M, G, C, ptr(grad), cur_stream(g.device)),
              'crb_vector_pool_interp_backward')
        return grad, None, None, None, None


def interpolate(features, idx, dist, grid_centers, support_xyz):
    return _Interpolate.apply(features, idx, dist, grid_centers, support_xyz)


class _VoxelPool(Function):
    @staticmethod
    def forward(ctx, features, support_xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, num_grid, max_distance, nsample, neighbor_type):
        require_cuda(features, support_xyz, new_xyz)
        features = _f32(features, (None, None), 'support_features')
        N, C = int(features.shape[0]), int(features.shape[1])
        support_xyz, new_xyz = _f32(support_xyz, (N, 3), 'support_xyz'), _f32(new_xyz, (None, 3), 'new_xyz')
        M, dev = int(new_xyz.shape[0]), new_xyz.device
        gx, gy, gz = (int(v) for v in num_grid)
        G = gx * gy * gz
        if not 0 < G <= MAX_CELLS:
            raise CrbHipError('crb_vector_pool_voxel_forward: 1 .. %d cells per new point, got %d' % (MAX_CELLS, G))
        a, b = _cnt(xyz_batch_cnt, dev), _cnt(new_xyz_batch_cnt, dev)
        if a.shape != b.shape:
            raise CrbHipError('crb_vector_pool_voxel_forward: xyz_batch_cnt and new_xyz_batch_cnt differ in length')
        R = torch.tensor(float(max_distance), dtype=torch.float32)
        gs = [float(R * 2 / n) for n in (gx, gy, gz)]            # f32 on the host, as the reference's launcher
        new_features = torch.empty((M, G * C), dtype=torch.float32, device=dev)
        new_local_xyz = torch.empty((M, 3 * G), dtype=torch.float32, device=dev)
        point_cnt = torch.empty((M, G), dtype=torch.int32, device=dev)
        pick = torch.empty((M, G), dtype=torch.int32, device=dev)
        check(lib.crb_vector_pool_voxel_forward(ptr(support_xyz), ptr(features), N, ptr(a), ptr(new_xyz), M, ptr(b), int(a.shape[0]),
                                                gx, gy, gz, float(R), gs[0], gs[1], gs[2], C, int(nsample), int(neighbor_type),
                                                ptr(new_features), ptr(new_local_xyz), ptr(point_cnt), ptr(pick), cur_stream(dev)),
              'crb_vector_pool_voxel_forward')
        ctx.save_for_backward(pick)
        ctx.dims = (N, M, G, C)
        ctx.mark_non_differentiable(new_local_xyz, point_cnt, pick)
        return new_features, new_local_xyz, point_cnt, pick

    @staticmethod
    def backward(ctx, grad_new_features, *unused):
        pick, = ctx.saved_tensors
        N, M, G, C = ctx.dims
        grad = torch.empty((N, C), dtype=torch.float32, device=grad_new_features.device)
        srt, order = inverse_lists(pick)
        g = grad_new_features.contiguous().float()
        check(lib.crb_vector_pool_voxel_backward(ptr(g), ptr(srt), ptr(order), N, M, G, C, ptr(grad), cur_stream(g.device)),
              'crb_vector_pool_voxel_backward')
        return grad, None, None, None, None, None, None, None, None


def voxel_pool(features, support_xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, num_grid, max_distance, nsample, neighbor_type):
    return _VoxelPool.apply(features, support_xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, num_grid, max_distance, nsample,
                            neighbor_type)
