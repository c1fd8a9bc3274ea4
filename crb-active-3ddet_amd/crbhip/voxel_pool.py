"""Voxel query and the fused pooling body of one NeighborVoxelSAModuleMSG scale (csrc/voxel_pool.hip).

Host mirror of voxel_query_gpu.cu + voxel_query_utils.py + voxel_pool_modules.py:96-120 of the reference. The site lookup is the
x-grouped hash of crbhip.sparse.build_hash: no dense (B, Z, Y, X) index, no (M, C, nsample) / (M, 3, nsample) grouped tensor."""
import torch

from ._lib import lib, check, ptr, cur_stream, require_cuda, host_i32x3, CrbHipError

POOLS = {'max_pool': 0, 'avg_pool': 1}


def query_supported(nsample, ranges):
    """the shapes crb_voxel_query takes: 1 <= nsample <= 32, every range in 0 .. 4"""
    return 1 <= int(nsample) <= 32 and all(0 <= int(r) <= 4 for r in ranges)


def supported(C, nsample):
    """the shapes crb_voxel_pool_forward / _backward take (crb_voxel_pool_supported): C in {32, 64}, 1 <= nsample <= 32"""
    return bool(lib.crb_voxel_pool_supported(int(C), int(nsample)))


@torch.no_grad()
def voxel_query(xyz, new_xyz, new_coords, batch_size, shape, ranges, radius, nsample, hkeys, hvals, cap):
    """xyz (N,3) voxel centres, new_xyz (M,3), new_coords (M,4) i32 [b,z,y,x] at the level, shape (D,H,W), ranges (rz,ry,rx),
    site hash of the level's coordinates -> idx (M,nsample) i32 global rows, cnt (M) i32 hits kept (0 = empty ball)"""
    require_cuda(xyz, new_xyz, new_coords, hkeys, hvals)
    if new_coords.dtype != torch.int32 or new_coords.dim() != 2 or new_coords.shape[1] != 4 or new_xyz.shape[0] != new_coords.shape[0]:
        raise CrbHipError('crb_voxel_query: new_coords (M,4) int32 [b,z,y,x] and new_xyz (M,3) expected')
    xyz, new_xyz, new_coords = xyz.detach().float().contiguous(), new_xyz.detach().float().contiguous(), new_coords.contiguous()
    M = int(new_xyz.shape[0])
    idx = torch.empty((M, int(nsample)), dtype=torch.int32, device=xyz.device)
    cnt = torch.empty((M,), dtype=torch.int32, device=xyz.device)
    check(lib.crb_voxel_query(ptr(xyz), int(xyz.shape[0]), ptr(new_xyz), ptr(new_coords), M, int(batch_size), host_i32x3(shape),
                              host_i32x3(ranges), float(radius), int(nsample), ptr(hkeys), ptr(hvals), int(cap), ptr(idx), ptr(cnt),
                              cur_stream(xyz.device)), 'crb_voxel_query')
    return idx, cnt


@torch.no_grad()
def moments(xyz, new_xyz, idx, cnt):
    """-> (mu (3), Sigma (3,3)) f64: mean and (biased) covariance of d = xyz[idx] - new_xyz over all M * nsample slots"""
    require_cuda(xyz, new_xyz, idx, cnt)
    M, ns = int(idx.shape[0]), int(idx.shape[1])
    sums = torch.empty((9,), dtype=torch.float64, device=xyz.device)
    nbytes = int(lib.crb_voxel_pool_moments_workspace_bytes(M))
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=xyz.device)
    check(lib.crb_voxel_pool_moments(ptr(xyz), ptr(new_xyz), ptr(idx), ptr(cnt), M, ns, ptr(sums), ptr(ws), nbytes,
                                     cur_stream(xyz.device)), 'crb_voxel_pool_moments')
    n = float(M * ns)
    mu = sums[:3] / n
    s2 = sums[3:] / n
    second = torch.stack((s2[0], s2[1], s2[2], s2[1], s2[3], s2[4], s2[2], s2[4], s2[5])).view(3, 3)
    return mu, second - mu[:, None] * mu[None, :]


class _VoxelPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features_in, A, b, xyz, new_xyz, idx, cnt, pool):
        f, A, b = features_in.contiguous(), A.contiguous(), b.contiguous()
        N, C = (int(v) for v in f.shape)
        M, ns = int(idx.shape[0]), int(idx.shape[1])
        out = torch.empty((M, C), dtype=torch.float32, device=f.device)
        check(lib.crb_voxel_pool_forward(ptr(f), N, C, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(cnt), M, ns, pool, ptr(A), ptr(b), ptr(out),
                                         cur_stream(f.device)), 'crb_voxel_pool_forward')
        ctx.save_for_backward(f, A, b, xyz, new_xyz, idx, cnt)
        ctx.pool = pool
        return out

    @staticmethod
    def backward(ctx, grad_out):
        f, A, b, xyz, new_xyz, idx, cnt = ctx.saved_tensors
        N, C = (int(v) for v in f.shape)
        M, ns = int(idx.shape[0]), int(idx.shape[1])
        g = grad_out.contiguous().float()
        dev = f.device
        d_ab = torch.empty((C, 4), dtype=torch.float32, device=dev)
        nbytes = int(lib.crb_voxel_pool_backward_workspace_bytes(M, C))
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
        need_f = ctx.needs_input_grad[0]
        deterministic = torch.are_deterministic_algorithms_enabled() and need_f
        if deterministic and ctx.pool == POOLS['avg_pool']:
            raise CrbHipError('crb_voxel_pool_backward: avg pooling has no reproducible scatter (no single selected row per output); '
                              'switch torch.use_deterministic_algorithms on before the forward pass, which then takes the torch route')
        if deterministic:
            # reproducible route (max pooling): the compact gradient and the row it belongs to go through torch's deterministic
            # index_add_; the atomics of the default route sum in an order that varies from call to call
            g_sel = torch.empty((M, C), dtype=torch.float32, device=dev)
            a_row = torch.empty((M, C), dtype=torch.int32, device=dev)
            d_f = None
        else:
            g_sel = a_row = None
            d_f = torch.zeros((N, C), dtype=torch.float32, device=dev)
        check(lib.crb_voxel_pool_backward(ptr(g), ptr(f), N, C, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(cnt), M, ns, ctx.pool, ptr(A), ptr(b),
                                          ptr(d_f), ptr(g_sel), ptr(a_row), ptr(d_ab), ptr(ws), nbytes, cur_stream(dev)),
              'crb_voxel_pool_backward')
        if deterministic:
            flat = a_row.clamp_(min=0).long().mul_(C).add_(torch.arange(C, device=dev))        # g_sel is 0 where no row is selected
            d_f = torch.zeros((N * C,), dtype=torch.float32, device=dev).index_add_(0, flat.view(-1), g_sel.view(-1)).view(N, C)
        return (d_f if need_f else None), d_ab[:, :3], d_ab[:, 3], None, None, None, None, None


def voxel_pool(features_in, A, b, xyz, new_xyz, idx, cnt, pool_method):
    """features_in (N,C), A (C,3), b (C) (differentiable), xyz (N,3), new_xyz (M,3), idx (M,nsample) i32, cnt (M) i32 -> (M,C)"""
    require_cuda(features_in, A, b, xyz, new_xyz, idx, cnt)
    if pool_method not in POOLS:
        raise NotImplementedError(pool_method)
    if features_in.dim() != 2 or features_in.dtype != torch.float32 or idx.dtype != torch.int32 or cnt.dtype != torch.int32:
        raise CrbHipError('crb_voxel_pool: features_in (N,C) f32, idx / cnt int32 expected')
    return _VoxelPool.apply(features_in, A.float(), b.float(), xyz.detach().float().contiguous(), new_xyz.detach().float().contiguous(),
                            idx.contiguous(), cnt.contiguous(), POOLS[pool_method])
