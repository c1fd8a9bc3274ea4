"""LLALSampling (pcdet/query_strategies/llal_sampling.py:8-63): the loss the LossNet of the LLAL detector predicts for a frame,
dropout OFF; the SELECT_NUMS frames with the largest prediction, in ascending order of value. Needs a PV-RCNN with
ROI_HEAD.LOSS_NET (pcdet.model_cfgs.pv_rcnn_llal_cfg)."""
from .pool_eval import _ScalarScoreSampling


class LLALSampling(_ScalarScoreSampling):
    MC_DROPOUT = False

    def frame_value(self, batch, pred_dicts, b):
        # the reference indexes the batch's (B, 1) prediction tensor by the frame's position in the batch
        preds = pred_dicts[b]['loss_predictions']
        if preds is None:
            raise KeyError('llal: the detector returned no loss_predictions (ROI_HEAD.LOSS_NET is not set)')
        return preds[b]
