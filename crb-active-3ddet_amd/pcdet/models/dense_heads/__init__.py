"""dense / point heads on the SECOND, PV-RCNN and Part-A2 paths, looked up by the NAME field of the model config"""
from . import anchor_head_single, anchor_head_template, center_head, point_head_box, point_head_simple, point_head_template, \
    point_intra_part_head
from .anchor_head_multi import AnchorHeadMulti, SingleHead
from .anchor_head_single import AnchorHeadSingle
from .anchor_head_template import AnchorHeadTemplate
from .center_head import CenterHead
from .point_head_box import PointHeadBox
from .point_head_simple import PointHeadSimple
from .point_head_template import PointHeadTemplate
from .point_intra_part_head import PointIntraPartOffsetHead

__all__ = {cls.__name__: cls for cls in (AnchorHeadTemplate, AnchorHeadSingle, AnchorHeadMulti, PointHeadTemplate, PointHeadSimple,
                                         CenterHead, PointIntraPartOffsetHead, PointHeadBox)}
