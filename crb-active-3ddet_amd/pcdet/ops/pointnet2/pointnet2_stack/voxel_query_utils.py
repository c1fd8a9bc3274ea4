"""voxel_query / VoxelQueryAndGrouping (pcdet/ops/pointnet2/pointnet2_stack/voxel_query_utils.py:10-100).

Two routes with the reference's semantics (scan dz, dy, dx ascending over [-range, +range]; skip sites outside the volume, empty
sites and neighbours with dist2 > radius^2; keep the first nsample hits; fill the other slots with the first hit; an empty ball reads
row 0 and is flagged):
  * torch route (`voxel_query_torch`): the reference's dense (B, Z, Y, X) index, any device. The definition, the CPU path and the
    fallback for shapes the kernel does not take.
  * HIP route: handed the level's SparseConvTensor instead of a dense index, device tensors go to crb_voxel_query, which looks
    sites up in the site hash of the tensor's coordinates; no dense index is built."""
import torch
import torch.nn as nn


def _is_sparse_tensor(x):
    return hasattr(x, 'indices') and hasattr(x, 'spatial_shape')


def voxel_query_torch(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices, chunk=4096):
    """xyz (N,3), new_xyz (M,3), new_coords (M,4) int [b,z,y,x], point_indices (B,Z,Y,X) int32 -> idx (M,nsample) int32 global rows,
    empty_ball_mask (M) bool"""
    B, Z, Y, X = point_indices.shape
    rz, ry, rx = (int(r) for r in max_range)
    dev = xyz.device
    dz, dy, dx = torch.meshgrid(torch.arange(-rz, rz + 1, device=dev), torch.arange(-ry, ry + 1, device=dev),
                                torch.arange(-rx, rx + 1, device=dev), indexing='ij')
    dz, dy, dx = dz.reshape(1, -1), dy.reshape(1, -1), dx.reshape(1, -1)               # scan order: dz slowest, dx fastest
    K = dz.shape[1]
    r2 = torch.tensor(float(radius), dtype=torch.float32, device=dev) ** 2
    flat = point_indices.reshape(-1)
    pos_k = torch.arange(K, device=dev).view(1, K)
    take = min(int(nsample), K)
    out_idx, out_empty = [], []
    for s in range(0, new_coords.shape[0], chunk):
        c = new_coords[s:s + chunk].long()
        n = new_xyz[s:s + chunk].float()
        b, z, y, x = c[:, 0:1], c[:, 1:2] + dz, c[:, 2:3] + dy, c[:, 3:4] + dx
        ok = (b >= 0) & (b < B) & (z >= 0) & (z < Z) & (y >= 0) & (y < Y) & (x >= 0) & (x < X)
        lin = ((b * Z + z) * Y + y) * X + x
        row = torch.where(ok, flat[torch.where(ok, lin, torch.zeros_like(lin))].long(), torch.full_like(lin, -1))
        hit = row >= 0
        p = xyz[row.clamp(min=0)].float()                                                  # (m, K, 3)
        d = p - n.unsqueeze(1)
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        hit = hit & ~(d2 > r2)
        key = torch.where(hit, pos_k.expand_as(row), torch.full_like(row, K))
        first_pos = torch.topk(key, take, dim=1, largest=False, sorted=True).values        # the first hits in scan order
        valid = first_pos < K
        rows = torch.gather(row, 1, first_pos.clamp(max=K - 1))
        if take < nsample:
            valid = torch.cat([valid, valid.new_zeros(valid.shape[0], nsample - take)], dim=1)
            rows = torch.cat([rows, rows.new_zeros(rows.shape[0], nsample - take)], dim=1)
        idx = torch.where(valid, rows, rows[:, 0:1].expand_as(rows))
        empty = ~valid[:, 0]
        idx = torch.where(empty.unsqueeze(1), torch.zeros_like(idx), idx)
        out_idx.append(idx.to(torch.int32))
        out_empty.append(empty)
    if not out_idx:
        return torch.zeros((0, nsample), dtype=torch.int32, device=dev), torch.zeros((0,), dtype=torch.bool, device=dev)
    return torch.cat(out_idx, 0), torch.cat(out_empty, 0)


def site_hash_of(sparse_tensor):
    """(hkeys, hvals, capacity) of the tensor's coordinates, built once per tensor and kept on it"""
    cached = getattr(sparse_tensor, '_crb_site_hash', None)
    if cached is None or cached[0] is not sparse_tensor.indices:
        from crbhip import sparse
        cached = (sparse_tensor.indices, sparse.build_hash(sparse_tensor.indices, sparse_tensor.spatial_shape))
        sparse_tensor._crb_site_hash = cached
    return cached[1]


def voxel_query_hip(max_range, radius, nsample, xyz, new_xyz, new_coords, sparse_tensor):
    """the HIP route -> idx (M,nsample) int32, cnt (M) int32 hits kept (0 = empty ball)"""
    from crbhip import voxel_pool
    hkeys, hvals, cap = site_hash_of(sparse_tensor)
    return voxel_pool.voxel_query(xyz, new_xyz, new_coords.int(), sparse_tensor.batch_size, sparse_tensor.spatial_shape, max_range,
                                  radius, nsample, hkeys, hvals, cap)


@torch.no_grad()
def voxel_query(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices):
    """the reference's signature; point_indices is its dense (B, Z, Y, X) tensor (torch route, any device) or the level's
    SparseConvTensor (device tensors: the HIP route; host tensors: the dense index is built here) -> (idx, empty_ball_mask)"""
    if _is_sparse_tensor(point_indices):
        if xyz.is_cuda:
            from crbhip import voxel_pool
            if voxel_pool.query_supported(nsample, max_range):
                idx, cnt = voxel_query_hip(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices)
                return idx, cnt == 0
        from ....utils import common_utils
        point_indices = common_utils.generate_voxel2pinds(point_indices)
    return voxel_query_torch(max_range, radius, nsample, xyz, new_xyz, new_coords, point_indices)


class VoxelQueryAndGrouping(nn.Module):
    def __init__(self, max_range, radius, nsample):
        super().__init__()
        self.max_range, self.radius, self.nsample = max_range, radius, nsample

    def forward(self, new_coords, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, voxel2point_indices):
        """new_coords (M,4) [b,z,y,x], xyz (N,3), new_xyz (M,3), features (N,C) -> grouped_features (M,C,nsample), grouped_xyz
        (M,3,nsample), empty_ball_mask (M). The query returns global rows: the reference's per-frame re-basing of idx and the
        stacked grouping_operation that undoes it are one gather."""
        assert xyz.shape[0] == int(xyz_batch_cnt.sum()) and new_coords.shape[0] == int(new_xyz_batch_cnt.sum())
        idx, empty_ball_mask = voxel_query(self.max_range, self.radius, self.nsample, xyz, new_xyz, new_coords, voxel2point_indices)
        rows = idx.long()
        grouped_xyz = xyz[rows].permute(0, 2, 1).contiguous()
        grouped_features = features[rows].permute(0, 2, 1).contiguous()
        return grouped_features, grouped_xyz, empty_ball_mask
