"""PVRCNNPlusPlus (pcdet/models/detectors/pv_rcnn_plusplus.py:4-53): PV-RCNN whose keypoints are sampled around the first stage's
proposals (PFE.SAMPLE_METHOD SPC, crbhip/spc.py). The proposal layer therefore runs BEFORE the PFE, and in training the RoI sampler
too: the PFE sees the sampled rois. RoIHeadTemplate.proposal_layer returns early when `rois` exist and PVRCNNHead.forward takes
batch_dict['roi_targets_dict'], so the RoI head itself is PV-RCNN's.
The set-abstraction layers and the RoI grid pool are StackSAModuleMSG by default (pcdet.model_cfgs.pv_rcnn_plusplus_cfg);
aggregation='vector_pool' there installs the reference yaml's VectorPoolAggregationModuleMSG sections (csrc/vector_pool.hip).
Not supported on this detector: the LLAL loss net (its per-frame point loss reshapes by NUM_KEYPOINTS, which SPC does not keep)."""
from .pv_rcnn import PVRCNN


class PVRCNNPlusPlus(PVRCNN):
    def __init__(self, model_cfg, num_class, dataset):
        if model_cfg.get('ROI_HEAD', {}).get('LOSS_NET', None) is not None:
            raise NotImplementedError('PVRCNNPlusPlus with ROI_HEAD.LOSS_NET (LLAL): the per-frame point loss reshapes by NUM_KEYPOINTS, '
                                      'and SPC sampling gives every frame its own keypoint count')
        super().__init__(model_cfg=model_cfg, num_class=num_class, dataset=dataset)

    def scheduled_modules(self):
        """vfe -> backbone_3d -> map_to_bev -> backbone_2d -> dense_head -> (proposals, RoI sampling) -> pfe -> point_head -> roi_head"""
        order = ('vfe', 'backbone_3d', 'map_to_bev_module', 'backbone_2d', 'dense_head', 'pfe', 'point_head', 'roi_head')
        return [m for m in (getattr(self, n, None) for n in order) if m is not None]

    def propose(self, batch_dict):
        """the first stage's proposals, and in training the sampled rois the PFE and the RoI head work on"""
        head = self.roi_head
        batch_dict = head.proposal_layer(batch_dict, nms_config=head.model_cfg.NMS_CONFIG['TRAIN' if self.training else 'TEST'])
        if self.training:
            targets_dict = batch_dict.get('roi_targets_dict', None)        # injected RoI sample (tests / measurements)
            if targets_dict is None:
                targets_dict = head.assign_targets(batch_dict)
            batch_dict['rois'] = targets_dict['rois']
            batch_dict['roi_labels'] = targets_dict['roi_labels']
            batch_dict['roi_targets_dict'] = targets_dict
            if 'roi_valid_num' in batch_dict:
                batch_dict['roi_valid_num'] = [targets_dict['rois'].shape[1] for _ in range(batch_dict['batch_size'])]
        return batch_dict

    def run_modules(self, batch_dict, before_pfe=None):
        if getattr(getattr(self, 'backbone_3d', None), 'ACCEPTS_LAZY_VOXELS', False) and 'voxels' not in batch_dict:
            batch_dict['_lazy_voxel_count'] = True
        vfe_done = batch_dict.pop('_vfe_done', False)
        for stage in self.scheduled_modules():
            if vfe_done and stage is getattr(self, 'vfe', None):
                continue
            if stage is self.pfe:
                if before_pfe is not None:
                    before_pfe()
                    before_pfe = None
                batch_dict = self.propose(batch_dict)
            batch_dict = stage(batch_dict)
        return batch_dict

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_point, tb_dict = self.point_head.get_loss(tb_dict)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_point + loss_rcnn, tb_dict, {}
