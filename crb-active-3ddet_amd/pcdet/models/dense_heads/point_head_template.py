"""PointHeadTemplate (pcdet/models/dense_heads/point_head_template.py:8-215), the parts PointHeadSimple uses.
Target assignment runs ONE batched points-in-boxes launch per box set instead of a per-frame loop (:78-92)."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...ops.roiaware_pool3d import roiaware_pool3d_utils
from ...utils import loss_utils


# point labels and the focal classification loss (+ gradient) as HIP launches (csrc/point_head.hip); CRB_POINT_HEAD_FUSED=0 = the torch
# expressions below (A/B, and what the kernels are tested against)
FUSED = __import__('os').environ.get('CRB_POINT_HEAD_FUSED', '1') == '1'


class _PointFocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, labels, alpha, gamma, weight):
        from crbhip import lib, check, ptr, cur_stream
        p = preds.contiguous().float()
        n, C = p.shape
        buf = torch.empty((3,), dtype=torch.float32, device=p.device)
        d = torch.empty_like(p)
        check(lib.crb_point_focal_loss(ptr(p), ptr(labels.contiguous()), n, C, alpha, gamma, weight, ptr(buf), ptr(d), cur_stream(p.device)),
              'crb_point_focal_loss')
        ctx.save_for_backward(d)
        ctx.pshape = preds.shape
        pos = buf[1]
        ctx.mark_non_differentiable(pos)
        ctx.set_materialize_grads(False)
        return buf[2], pos

    @staticmethod
    def backward(ctx, g, _gp):
        if g is None:
            return None, None, None, None, None
        (d,) = ctx.saved_tensors
        return (d * g).view(ctx.pshape), None, None, None, None



class _PointFocalLossPerFrame(torch.autograd.Function):
    """reduce=False form: (B,) per-frame losses with the batch-wide positive normaliser (csrc/point_head.hip)"""
    @staticmethod
    def forward(ctx, preds, labels, B, alpha, gamma, weight):
        from crbhip import lib, check, ptr, cur_stream
        p = preds.contiguous().float()
        n, C = p.shape
        buf = torch.empty((B + 1,), dtype=torch.float32, device=p.device)
        d = torch.empty_like(p)
        check(lib.crb_point_focal_loss_per_frame(ptr(p), ptr(labels.contiguous()), n, C, B, alpha, gamma, weight, ptr(buf), ptr(d),
                                                 cur_stream(p.device)), 'crb_point_focal_loss_per_frame')
        ctx.save_for_backward(d)
        ctx.pshape, ctx.B = preds.shape, B
        loss, pos = buf[:B], buf[B]
        ctx.mark_non_differentiable(pos)
        ctx.set_materialize_grads(False)
        return loss, pos

    @staticmethod
    def backward(ctx, g, _gp):
        if g is None:
            return None, None, None, None, None, None
        from crbhip.rcnn_loss import scale_rows_per_frame
        (d,) = ctx.saved_tensors
        return scale_rows_per_frame(d, g, ctx.B).view(ctx.pshape), None, None, None, None, None

class PointHeadTemplate(nn.Module):
    def __init__(self, model_cfg, num_class):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.build_losses(self.model_cfg.LOSS_CONFIG)
        self.forward_ret_dict = None

    def build_losses(self, losses_cfg):
        self.add_module('cls_loss_func', loss_utils.SigmoidFocalClassificationLoss(alpha=0.25, gamma=2.0))
        reg = losses_cfg.get('LOSS_REG', None)
        if reg == 'l1':
            self.reg_loss_func = F.l1_loss
        elif reg == 'WeightedSmoothL1Loss':
            cw = losses_cfg.LOSS_WEIGHTS.get('code_weights', None)
            self.reg_loss_func = loss_utils.WeightedSmoothL1Loss(code_weights=cw)
            # the loss's code_weights buffer moves to the device with the module; the fused losses take the eight weights as host
            # floats, kept here (rounded to f32 like the buffer) so that no training step reads the buffer back
            self.box_code_weights = (1.0,) * 8 if cw is None else tuple(float(w) for w in np.asarray(cw, np.float32))
        else:
            self.reg_loss_func = F.smooth_l1_loss

    @staticmethod
    def make_fc_layers(fc_cfg, input_channels, output_channels):
        layers, c_in = [], input_channels
        for c in fc_cfg:
            layers += [nn.Linear(c_in, c, bias=False), nn.BatchNorm1d(c), nn.ReLU()]
            c_in = c
        layers.append(nn.Linear(c_in, output_channels, bias=True))
        return nn.Sequential(*layers)

    def assign_stack_targets(self, points, gt_boxes, extend_gt_boxes=None, ret_box_labels=False, ret_part_labels=False,
                             set_ignore_flag=True, use_ball_constraint=False, central_radius=2.0, point_counts=None):
        """points (N,4) [b,x,y,z], frame-sorted, the same count per frame unless point_counts (B host ints: the frames' own counts,
        SPC keypoints) says otherwise; gt_boxes (B,M,8)
        -> point_cls_labels (N) long: class (or 1) inside a gt box, -1 in the enlarged shell only, 0 elsewhere"""
        assert points.dim() == 2 and points.shape[1] == 4 and gt_boxes.dim() == 3 and gt_boxes.shape[2] == 8
        if ret_part_labels or (ret_box_labels and getattr(self, 'box_coder', None) is not None):
            return self.assign_part_targets(points, gt_boxes, ret_box_labels, set_ignore_flag, use_ball_constraint,
                                            ret_part_labels=ret_part_labels)
        assert set_ignore_flag and not use_ball_constraint and not ret_box_labels and not ret_part_labels, \
            'only the PointHeadSimple target mode is on the hot path'
        B = gt_boxes.shape[0]
        if point_counts is not None and len(set(int(c) for c in point_counts)) > 1:
            # ragged frames: the dense (B, max, 3) form of the same points (pad rows far outside every box), labels gathered back
            cnt = [int(c) for c in point_counts]
            assert len(cnt) == B and sum(cnt) == points.shape[0], (cnt, tuple(points.shape))
            M = max(cnt)
            start = torch.tensor([sum(cnt[:b]) for b in range(B)], device=points.device)
            frame = torch.repeat_interleave(torch.arange(B, device=points.device), torch.tensor(cnt, device=points.device),
                                            output_size=points.shape[0])
            flat = frame * M + (torch.arange(points.shape[0], device=points.device) - start[frame])
            dense = points.new_full((B * M, 4), 1e6)
            dense[:, 0] = torch.arange(B, device=points.device).repeat_interleave(M)
            dense[flat] = points
            padded = self.assign_stack_targets(dense, gt_boxes, extend_gt_boxes, ret_box_labels, ret_part_labels, set_ignore_flag,
                                               use_ball_constraint, central_radius)
            return {'point_cls_labels': padded['point_cls_labels'][flat], 'point_box_labels': None, 'point_part_labels': None}
        bs = points[:, 0].long()
        M = int(points.shape[0] // B)
        if points.shape[0] != M * B:
            raise NotImplementedError('ragged keypoint counts: pad to a dense (B,M,3) tensor first')
        pts = points[:, 1:4].reshape(B, M, 3).contiguous()
        if FUSED and pts.is_cuda and gt_boxes.shape[1] > 0:
            # the label arithmetic behind the two point-in-box queries as one launch (csrc/point_head.hip)
            from crbhip import lib, check, ptr, cur_stream
            inner = roiaware_pool3d_utils.points_in_boxes_gpu(pts, gt_boxes[:, :, 0:7].contiguous())
            outer = roiaware_pool3d_utils.points_in_boxes_gpu(pts, extend_gt_boxes[:, :, 0:7].contiguous())
            labels = torch.empty((B * M,), dtype=torch.int64, device=pts.device)
            gt = gt_boxes.contiguous().float()
            check(lib.crb_point_labels(ptr(inner), ptr(outer), ptr(gt), B, M, int(gt.shape[1]), int(gt.shape[2]), int(self.num_class),
                                       ptr(labels), cur_stream(pts.device)), 'crb_point_labels')
            return {'point_cls_labels': labels, 'point_box_labels': None, 'point_part_labels': None}
        inner = roiaware_pool3d_utils.points_in_boxes_gpu(pts, gt_boxes[:, :, 0:7].contiguous()).long().view(-1)
        outer = roiaware_pool3d_utils.points_in_boxes_gpu(pts, extend_gt_boxes[:, :, 0:7].contiguous()).view(-1)
        fg = inner >= 0
        ignore = fg ^ (outer >= 0)
        labels = torch.zeros_like(inner)
        labels = torch.where(ignore, torch.full_like(labels, -1), labels)
        if self.num_class == 1:
            fg_val = torch.ones_like(labels)
        else:
            fg_val = gt_boxes[bs, inner.clamp(min=0), -1].long()
        labels = torch.where(fg, fg_val, labels)
        return {'point_cls_labels': labels, 'point_box_labels': None, 'point_part_labels': None}

    def assign_part_targets(self, points, gt_boxes, ret_box_labels=False, set_ignore_flag=True, use_ball_constraint=False,
                            ret_part_labels=True):
        """the part-label mode of assign_stack_targets (Part-A2: ret_part_labels=True, set_ignore_flag) and its box-label modes
        (ret_box_labels with or without ret_part_labels: PartA2_free.yaml, PointHeadBox; only on a head with a box coder): frames of any
        size, all in one launch on device tensors (csrc/part_head.hip, csrc/point_box.hip), the batched torch expressions on host tensors
        or with FUSED off
        -> point_cls_labels (N) long, point_part_labels (N,3): rotate_z(p - c, -rz) / dims + 0.5 inside the owning box, zeros elsewhere,
           point_box_labels (N,8): PointResidualCoder.encode_torch against the owning box, zeros elsewhere"""
        from crbhip import part_head, point_box
        assert set_ignore_flag and not use_ball_constraint, 'part / box labels: only the set_ignore_flag mode is built'
        assert not ret_box_labels or getattr(self, 'box_coder', None) is not None, 'box labels need TARGET_CONFIG.BOX_CODER'
        extra = self.model_cfg.TARGET_CONFIG.GT_EXTRA_WIDTH
        if ret_box_labels:
            route = point_box.point_box_targets if FUSED else point_box.point_box_targets_torch
            labels, _, box, part = route(points.detach(), gt_boxes.detach(), extra, self.num_class, self.box_coder,
                                         with_part=ret_part_labels)
            return {'point_cls_labels': labels, 'point_box_labels': box, 'point_part_labels': part}
        route = part_head.part_targets if FUSED else part_head.part_targets_torch
        labels, part, _ = route(points.detach(), gt_boxes.detach(), extra, self.num_class)
        return {'point_cls_labels': labels, 'point_box_labels': None, 'point_part_labels': part}

    def get_part_head_loss(self, tb_dict=None):
        """get_cls_layer_loss + get_part_layer_loss (+ get_box_layer_loss when the head predicts boxes) of the reference
        (point_head_template.py:131-195) as one pair of launches; the torch expressions on host tensors or with FUSED off
        -> point_loss_cls + point_loss_part (+ point_loss_box). A head without part predictions (PointHeadBox) has no point_loss_part"""
        from crbhip import part_head, point_box
        ret = self.forward_ret_dict
        labels = ret['point_cls_labels'].view(-1)
        cls_preds = ret['point_cls_preds'].view(-1, self.num_class)
        weights = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        tb_dict = {} if tb_dict is None else tb_dict
        alpha, gamma = float(self.cls_loss_func.alpha), float(self.cls_loss_func.gamma)
        if ret.get('point_box_preds', None) is None:
            args = (cls_preds, ret['point_part_preds'], labels, ret['point_part_labels'], alpha, gamma,
                    float(weights['point_cls_weight']), float(weights['point_part_weight']))
            loss_cls, loss_part, pos = (part_head.part_loss if FUSED else part_head.part_loss_torch)(*args)
            tb_dict.update({'point_loss_cls': loss_cls.detach(), 'point_loss_part': loss_part.detach(), 'point_pos_num': pos.detach()})
            return loss_cls + loss_part, tb_dict
        assert type(self.reg_loss_func).__name__ == 'WeightedSmoothL1Loss', 'the box branch is built for LOSS_REG: WeightedSmoothL1Loss'
        has_part = ret.get('point_part_preds', None) is not None
        args = (cls_preds, ret.get('point_part_preds', None), ret['point_box_preds'], labels, ret.get('point_part_labels', None),
                ret['point_box_labels'], alpha, gamma, self.box_code_weights,
                float(self.reg_loss_func.beta), float(weights['point_cls_weight']),
                float(weights['point_part_weight']) if has_part else 0.0, float(weights['point_box_weight']))
        loss_cls, loss_part, loss_box, pos = (point_box.point_box_loss if FUSED else point_box.point_box_loss_torch)(*args)
        tb_dict.update({'point_loss_cls': loss_cls.detach(), 'point_loss_box': loss_box.detach(), 'point_pos_num': pos.detach()})
        if not has_part:
            return loss_cls + loss_box, tb_dict
        tb_dict['point_loss_part'] = loss_part.detach()
        return loss_cls + loss_part + loss_box, tb_dict

    def get_box_layer_loss(self, tb_dict=None):
        """point_loss_box alone, with the reference's signature (point_head_template.py:175-195); the heads' get_loss takes it together
        with the other losses in get_part_head_loss"""
        from crbhip import point_box
        ret = self.forward_ret_dict
        labels = ret['point_cls_labels'].view(-1)
        route = point_box.point_box_loss if FUSED else point_box.point_box_loss_torch
        _, _, loss_box, _ = route(ret['point_cls_preds'].view(-1, self.num_class).detach(), None, ret['point_box_preds'], labels, None,
                                  ret['point_box_labels'], float(self.cls_loss_func.alpha), float(self.cls_loss_func.gamma),
                                  self.box_code_weights, float(self.reg_loss_func.beta),
                                  0.0, 0.0, float(self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_box_weight']))
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'point_loss_box': loss_box.detach()})
        return loss_box, tb_dict

    def generate_predicted_boxes(self, points, point_cls_preds, point_box_preds):
        """points (N,3), point_cls_preds (N,num_class), point_box_preds (N,8) -> the same logits, boxes (N,7) decoded against the mean
        size of the argmax class (point_head_template.py:197-211); the stacked form, in torch on any device"""
        _, pred_classes = point_cls_preds.max(dim=-1)
        return point_cls_preds, self.box_coder.decode_torch(point_box_preds, points, pred_classes + 1)

    def predicted_boxes_to_batch(self, batch_dict, point_cls_preds, point_box_preds):
        """what the reference's heads leave for RoIHeadTemplate.proposal_layer. Host route (host tensors, f64, FUSED off): the
        reference's stacked batch_cls_preds (N,C), batch_box_preds (N,7) and batch_index (N). Device route: one launch
        (crb_point_box_decode) writes the dense, frame-padded batch_cls_preds (B,Amax,C) (-inf past a frame's rows), batch_box_preds
        (B,Amax,7) and batch_counts (B) i32; batch_index is left out. Amax comes from batch_dict['point_coords_counts_host'] when the
        batch carries it, else from one read-back of the (B+1) frame offsets"""
        from crbhip import point_box
        coords = batch_dict['point_coords']
        cls_d, box_d = point_cls_preds.detach(), point_box_preds.detach()
        if FUSED and point_box._fused_ok(coords, cls_d, box_d):
            cls_b, box_b, batch_dict['batch_counts'] = point_box.point_box_decode(
                coords, cls_d, box_d, self.box_coder, batch_dict['batch_size'], counts=batch_dict.get('point_coords_counts_host', None))
            batch_dict.pop('batch_index', None)
        else:
            cls_b, box_b = self.generate_predicted_boxes(coords[:, 1:4], point_cls_preds, point_box_preds)
            batch_dict['batch_index'] = coords[:, 0]
            batch_dict.pop('batch_counts', None)
        batch_dict['batch_cls_preds'] = cls_b
        batch_dict['batch_box_preds'] = box_b
        batch_dict['cls_preds_normalized'] = False
        return batch_dict

    def get_cls_layer_loss(self, tb_dict=None, reduce=True):
        labels = self.forward_ret_dict['point_cls_labels'].view(-1)
        preds = self.forward_ret_dict['point_cls_preds'].view(-1, self.num_class)
        if FUSED and reduce and preds.is_cuda and type(self.cls_loss_func).__name__ == 'SigmoidFocalClassificationLoss' and \
                labels.dtype == torch.int64:
            # focal loss + its gradient as one launch (csrc/point_head.hip)
            loss, pos = _PointFocalLoss.apply(preds, labels, float(self.cls_loss_func.alpha), float(self.cls_loss_func.gamma),
                                              float(self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_cls_weight']))
            tb_dict = {} if tb_dict is None else tb_dict
            tb_dict.update({'point_loss_cls': loss.detach(), 'point_pos_num': pos})
            return loss, tb_dict
        if FUSED and not reduce and preds.is_cuda and type(self.cls_loss_func).__name__ == 'SigmoidFocalClassificationLoss' and \
                labels.dtype == torch.int64 and preds.shape[1] == 1 and labels.numel() % self.model_cfg.NUM_KEYPOINTS == 0:
            # (one class: view(-1, NUM_KEYPOINTS).sum(-1) is a per-frame sum; with more it mixes classes, the torch path keeps that)
            # reduce=False (LLAL loss-net phase): per-frame sums, one launch each way
            loss, pos = _PointFocalLossPerFrame.apply(preds, labels, labels.numel() // self.model_cfg.NUM_KEYPOINTS,
                                                      float(self.cls_loss_func.alpha), float(self.cls_loss_func.gamma),
                                                      float(self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_cls_weight']))
            tb_dict = {} if tb_dict is None else tb_dict
            tb_dict.update({'point_loss_cls': loss[0].detach(), 'point_pos_num': pos})
            return loss, tb_dict
        positives = labels > 0
        cls_weights = ((labels == 0) * 1.0 + 1.0 * positives).float()
        pos_normalizer = positives.sum(dim=0).float()
        cls_weights = cls_weights / torch.clamp(pos_normalizer, min=1.0)
        one_hot = preds.new_zeros(*labels.shape, self.num_class + 1)
        one_hot.scatter_(-1, (labels * (labels >= 0).long()).unsqueeze(-1).long(), 1.0)
        src = self.cls_loss_func(preds, one_hot[..., 1:], weights=cls_weights)
        loss = src.sum() if reduce else src.view(-1, self.model_cfg.NUM_KEYPOINTS).sum(-1)
        loss = loss * self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS['point_cls_weight']
        tb_dict = {} if tb_dict is None else tb_dict
        tb_dict.update({'point_loss_cls': (loss if reduce else loss[0]).detach(), 'point_pos_num': pos_normalizer.detach()})
        return loss, tb_dict

    def forward(self, **kwargs):
        raise NotImplementedError
