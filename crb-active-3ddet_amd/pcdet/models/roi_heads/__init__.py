__all__ = {}
try:
    from .roi_head_template import RoIHeadTemplate
    from .pvrcnn_head import PVRCNNHead
    from .partA2_head import PartA2FCHead
    from .second_head import SECONDHead
    from .voxelrcnn_head import VoxelRCNNHead
    __all__.update({'RoIHeadTemplate': RoIHeadTemplate, 'PVRCNNHead': PVRCNNHead, 'PartA2FCHead': PartA2FCHead,
                    'SECONDHead': SECONDHead, 'VoxelRCNNHead': VoxelRCNNHead})
except ImportError:
    pass
