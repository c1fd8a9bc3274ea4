"""Golden vectors of dynamic voxelization (tests/golden/ref_dyn_voxel.npz) from the reference's own DynamicMeanVFE and
DynamicPillarVFE.

Runs ONLY in the authoring container (needs the reference tree); the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_dyn_voxel.py
Nothing from the reference is copied: the script imports its modules through the stub recipe of make_goldens.py, feeds the seeded
points of tests/dyn_voxel_cases.py and stores outputs. The reference's modules need torch_scatter, which is not available; a small
stand-in of our own (scatter_mean / scatter_max on index_add_ / scatter_reduce) is installed under that name.

Per case: DynamicMeanVFE's voxel_features and voxel_coords from its f32 run, and e_ref = max|f32 features - the f64 means of the very
same voxels| (tests/dyn_voxel_cases.definition, whose grouping is asserted to equal the reference's), the reference's own f32 error.
An f64 run of the reference is no yardstick here: it forms the cells in f64 and puts the points that sit on a cell face in f32 into
other voxels. Also recorded: DynamicPillarVFE's voxel_coords (its grouping in pillar mode; its features: make_goldens_dyn_pillar.py). The two NaN rows of case a are
taken out before the reference sees them: its floor(NaN).int() is undefined, and dropping them is this project's stated rule. The
empty case is not run: the reference's modules are not defined on an empty input."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg                      # noqa: E402
import dyn_voxel_cases as cases                # noqa: E402
from _constants import EasyDict                # noqa: E402


def install_torch_scatter():
    def scatter_mean(src, index, dim=0):
        assert dim == 0
        n = int(index.max()) + 1 if index.numel() else 0
        s = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
        cnt = torch.zeros(n, dtype=src.dtype).index_add_(0, index, torch.ones(len(index), dtype=src.dtype))
        return s / cnt.clamp(min=1).reshape((n,) + (1,) * (src.dim() - 1))

    def scatter_max(src, index, dim=0):
        assert dim == 0
        n = int(index.max()) + 1 if index.numel() else 0
        out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype)
        out = out.scatter_reduce(0, index[:, None].expand_as(src), src, 'amax', include_self=False)
        return out, None

    m = types.ModuleType('torch_scatter')
    m.scatter_mean, m.scatter_max = scatter_mean, scatter_max
    sys.modules['torch_scatter'] = m


def main():
    mg.import_reference()
    install_torch_scatter()
    from pcdet.models.backbones_3d.vfe.dynamic_mean_vfe import DynamicMeanVFE
    from pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe import DynamicPillarVFE
    out = {}
    for name, p in cases.CASES.items():
        if name == 'empty':
            continue
        pts = cases.make_case(name)['points']
        pts = pts[~np.isnan(pts).any(1)]
        mean = DynamicMeanVFE(model_cfg=EasyDict({'NAME': 'DynMeanVFE'}), num_point_features=p['C'], voxel_size=cases.VOXEL['voxel'],
                              grid_size=cases.GRID['voxel'], point_cloud_range=cases.PCR)
        bd = mean({'points': torch.from_numpy(pts), 'batch_size': p['B']})
        feats, coords = mg._np(bd['voxel_features']), mg._np(bd['voxel_coords']).astype(np.int32)
        d = cases.definition(pts, p['B'], 'voxel')
        assert coords.shape == d['coords'].shape and (coords == d['coords']).all()
        out['mean_%s_features' % name] = feats
        out['mean_%s_e_ref' % name] = np.array([np.abs(feats.astype(np.float64) - d['mean64']).max()])
        out['mean_%s_coords' % name] = coords
        cfg = EasyDict({'NAME': 'DynPillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [64, 64]})
        pil = DynamicPillarVFE(model_cfg=cfg, num_point_features=p['C'], voxel_size=cases.VOXEL['pillar'], grid_size=cases.GRID['pillar'],
                               point_cloud_range=cases.PCR).eval()
        with torch.no_grad():
            bd = pil({'points': torch.from_numpy(pts), 'batch_size': p['B']})
        out['pillar_%s_coords' % name] = mg._np(bd['voxel_coords']).astype(np.int32)
        print('  case %s: N %d, %d voxels (e_ref of the mean %.3g), %d pillars' % (
            name, len(pts), len(out['mean_%s_coords' % name]), out['mean_%s_e_ref' % name][0], len(out['pillar_%s_coords' % name])))
    path = os.path.join(HERE, 'ref_dyn_voxel.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
