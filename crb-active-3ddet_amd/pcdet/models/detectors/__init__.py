from .detector3d_template import Detector3DTemplate
from .second_net import SECONDNet

__all__ = {
    'Detector3DTemplate': Detector3DTemplate,
    'SECONDNet': SECONDNet,
}

try:
    from .pv_rcnn import PVRCNN
    __all__['PVRCNN'] = PVRCNN
except ImportError:   # PV-RCNN pieces land after SECOND
    pass

try:
    from .second_net_iou import SECONDNetIoU
    __all__['SECONDNetIoU'] = SECONDNetIoU
except ImportError:
    pass

try:
    from .voxel_rcnn import VoxelRCNN
    __all__['VoxelRCNN'] = VoxelRCNN
except ImportError:
    pass

from .pv_rcnn_plusplus import PVRCNNPlusPlus
__all__['PVRCNNPlusPlus'] = PVRCNNPlusPlus

from .pointpillar import PointPillar
__all__['PointPillar'] = PointPillar

from .centerpoint import CenterPoint
__all__['CenterPoint'] = CenterPoint

from .part_a2_net import PartA2Net
__all__['PartA2Net'] = PartA2Net

from .point_rcnn import PointRCNN
__all__['PointRCNN'] = PointRCNN


def build_detector(model_cfg, num_class, dataset):
    return __all__[model_cfg.NAME](model_cfg=model_cfg, num_class=num_class, dataset=dataset)
