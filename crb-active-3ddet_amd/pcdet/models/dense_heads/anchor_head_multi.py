"""AnchorHeadMulti and SingleHead (pcdet/models/dense_heads/anchor_head_multi.py:9-373): one small head per class group on an
optional shared 3 x 3 convolution. Same constructor contract, module tree and parameter names as the reference (its state_dict
loads), the same outputs in the multi-head layout (B, a*H*W, C): every head's anchors as (anchor, y, x), the heads one after another.

Kept as the reference has them: the class column offset of a head runs over RPN_HEAD_CFGS in order (c_idx, :279-288), with
SEPARATE_MULTIHEAD off every head predicts all num_class columns, a head's convolutions take the SHARED map's channel count even when
the head has layers of its own, and the heading goes through the sine difference only with a direction classifier (:341-345).

Different, host side only (as in the other heads here): tb_dict values are detached tensors and nothing calls .item(), so a training
step of the head makes no host synchronisation. On device tensors the three losses of all heads are ONE forward and ONE backward
launch (crbhip.multihead.multihead_loss, csrc/multihead_loss.hip) when the configuration is the one the kernel implements; `loss_torch`
restates the reference's loop and is the route of every other configuration (with a warning), of host tensors and of f64."""
import os
import warnings

import numpy as np
import torch
import torch.nn as nn

from ...utils import loss_utils
from ..backbones_2d import BaseBEVBackbone
from ..backbones_2d import base_bev_backbone as _bev
from .anchor_head_template import AnchorHeadTemplate

FUSED_LOSS = True            # False: the torch restatement for device tensors too (A/B, tools/time_multihead.py)
# per-class selection of the whole batch on the device (CRB_MULTICLASS_NMS=0: the per-segment loop, A/B and test reference)
MULTICLASS_NMS = os.environ.get('CRB_MULTICLASS_NMS', '1') == '1'


def _conv_bn_relu(c_in, c_out):
    return [nn.Conv2d(c_in, c_out, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(c_out), nn.ReLU()]


class SingleHead(BaseBEVBackbone):
    def __init__(self, model_cfg, input_channels, num_class, num_anchors_per_location, code_size, rpn_head_cfg=None,
                 head_label_indices=None, separate_reg_config=None):
        super().__init__(rpn_head_cfg, input_channels)
        self.num_anchors_per_location = num_anchors_per_location
        self.num_class = num_class
        self.code_size = code_size
        self.model_cfg = model_cfg
        self.separate_reg_config = separate_reg_config
        self.register_buffer('head_label_indices', head_label_indices)
        a = num_anchors_per_location
        if separate_reg_config is not None:
            n_mid, c_mid = separate_reg_config.NUM_MIDDLE_CONV, separate_reg_config.NUM_MIDDLE_FILTER

            def tower(c_out):
                layers, c_in = [], input_channels
                for _ in range(n_mid):
                    layers += _conv_bn_relu(c_in, c_mid)
                    c_in = c_mid
                return nn.Sequential(*layers, nn.Conv2d(c_in, c_out, kernel_size=3, stride=1, padding=1))
            self.conv_cls = tower(a * num_class)
            self.conv_box = nn.ModuleDict()
            self.conv_box_names = []
            total = 0
            for entry in separate_reg_config.REG_LIST:
                name, channels = entry.split(':')
                total += int(channels)
                self.conv_box['conv_' + name] = tower(a * int(channels))
                self.conv_box_names.append('conv_' + name)
            for m in self.conv_box.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                    if m.bias is not None:
                        nn.init.constant_(m.bias, 0)
            assert total == code_size, 'Code size does not match: %d:%d' % (total, code_size)
        else:
            self.conv_cls = nn.Conv2d(input_channels, a * num_class, kernel_size=1)
            self.conv_box = nn.Conv2d(input_channels, a * code_size, kernel_size=1)
        if model_cfg.get('USE_DIRECTION_CLASSIFIER', None) is not None:
            self.conv_dir_cls = nn.Conv2d(input_channels, a * model_cfg.NUM_DIR_BINS, kernel_size=1)
        else:
            self.conv_dir_cls = None
        self.use_multihead = model_cfg.get('USE_MULTIHEAD', False)
        self.init_weights()

    def init_weights(self):
        pi = 0.01
        last = self.conv_cls if isinstance(self.conv_cls, nn.Conv2d) else self.conv_cls[-1]
        nn.init.constant_(last.bias, -np.log((1 - pi) / pi))

    def _layout(self, y, c):
        """(B, a*c, H, W) -> (B, a*H*W, c) multi-head layout, or (B, H, W, a*c) without USE_MULTIHEAD"""
        if not self.use_multihead:
            return y.permute(0, 2, 3, 1).contiguous()
        B, _, H, W = y.shape
        return y.reshape(B, self.num_anchors_per_location, c, H, W).permute(0, 1, 3, 4, 2).reshape(B, -1, c)

    def forward(self, spatial_features_2d):
        x = spatial_features_2d
        if len(self.blocks) > 0:             # an entry with only HEAD_CLS_NAME has no layers: the identity
            x = super().forward({'spatial_features': x})['spatial_features_2d']
        cls_preds = self.conv_cls(x)
        if self.separate_reg_config is None:
            box_preds = self.conv_box(x)
        else:
            box_preds = torch.cat([self.conv_box[n](x) for n in self.conv_box_names], dim=1)
        ret = {'cls_preds': self._layout(cls_preds, self.num_class), 'box_preds': self._layout(box_preds, self.code_size),
               'dir_cls_preds': None}
        if self.conv_dir_cls is not None:
            ret['dir_cls_preds'] = self._layout(self.conv_dir_cls(x), self.model_cfg.NUM_DIR_BINS)
        return ret


class AnchorHeadMulti(AnchorHeadTemplate):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__(model_cfg=model_cfg, num_class=num_class, class_names=class_names, grid_size=grid_size,
                         point_cloud_range=point_cloud_range, predict_boxes_when_training=predict_boxes_when_training)
        self.model_cfg = model_cfg
        self.separate_multihead = self.model_cfg.get('SEPARATE_MULTIHEAD', False)
        c = self.model_cfg.get('SHARED_CONV_NUM_FILTER', None)
        if c is not None:
            self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, c, 3, stride=1, padding=1, bias=False),
                                             nn.BatchNorm2d(c, eps=1e-3, momentum=0.01), nn.ReLU())
        else:
            self.shared_conv, c = None, input_channels
        self.rpn_heads = None
        self.make_multihead(c)

    def make_multihead(self, input_channels):
        cfgs = self.model_cfg.RPN_HEAD_CFGS
        names = [n for c in cfgs for n in c['HEAD_CLS_NAME']]
        heads = []
        for c in cfgs:
            per_loc = sum(self.num_anchors_per_location[names.index(n)] for n in c['HEAD_CLS_NAME'])
            labels = torch.from_numpy(np.array([self.class_names.index(n) + 1 for n in c['HEAD_CLS_NAME']]))
            heads.append(SingleHead(self.model_cfg, input_channels,
                                    len(c['HEAD_CLS_NAME']) if self.separate_multihead else self.num_class, per_loc,
                                    self.box_coder.code_size, c, head_label_indices=labels,
                                    separate_reg_config=self.model_cfg.get('SEPARATE_REG_CONFIG', None)))
        self.rpn_heads = nn.ModuleList(heads)

    def _shared(self, x):
        """the shared 3 x 3 convolution + BatchNorm + ReLU on the 2-D backbone's own layer routines (Winograd convolution, fused row
        BatchNorm) where they take the tensor, as the module otherwise"""
        if x.is_cuda and x.is_contiguous(memory_format=torch.channels_last):
            if not self.training and not torch.is_grad_enabled():
                return BaseBEVBackbone._run_folded(self.shared_conv, x)
            if self.training and _bev.ROWS_TRAIN:
                return BaseBEVBackbone._run_rows_train(self.shared_conv, x)
        return self.shared_conv(x)

    def forward(self, data_dict):
        x = data_dict['spatial_features_2d']
        if self.shared_conv is not None:
            x = self._shared(x)
        rets = [head(x) for head in self.rpn_heads]
        cat = (lambda ts: ts) if self.separate_multihead else (lambda ts: torch.cat(ts, dim=1))
        ret = {'cls_preds': cat([r['cls_preds'] for r in rets]), 'box_preds': cat([r['box_preds'] for r in rets])}
        if self.model_cfg.get('USE_DIRECTION_CLASSIFIER', False):
            ret['dir_cls_preds'] = cat([r['dir_cls_preds'] for r in rets])
        self.forward_ret_dict.pop('dir_cls_preds', None)
        self.forward_ret_dict.update(ret)
        if self.training:
            self.forward_ret_dict.update(self.assign_targets(gt_boxes=data_dict['gt_boxes']))
        if not self.training or self.predict_boxes_when_training:
            B = data_dict['batch_size']
            data_dict['cls_preds_normalized'] = False
            if isinstance(ret['cls_preds'], list):
                data_dict['multihead_label_mapping'] = [h.head_label_indices for h in self.rpn_heads]
                # post-processing's per-class selection decodes the picks of every head alone (decode_head); the full decode below is
                # what the loop route and every other reader take
                data_dict['multihead_box_decoder'] = self._head_decoder(B, ret['box_preds'], ret.get('dir_cls_preds', None))
            if isinstance(ret['cls_preds'], list) and MULTICLASS_NMS and ret['box_preds'][0].is_cuda and not self.predict_boxes_when_training:
                data_dict['batch_cls_preds'] = ret['cls_preds']
                data_dict.pop('batch_box_preds', None)
                data_dict['batch_box_decoder_full'] = lambda: self.generate_predicted_boxes(
                    batch_size=B, cls_preds=ret['cls_preds'], box_preds=ret['box_preds'], dir_cls_preds=ret.get('dir_cls_preds', None))[1]
            else:
                data_dict['batch_cls_preds'], data_dict['batch_box_preds'] = self.generate_predicted_boxes(
                    batch_size=B, cls_preds=ret['cls_preds'], box_preds=ret['box_preds'], dir_cls_preds=ret.get('dir_cls_preds', None))
        return data_dict

    def head_anchor_ranges(self):
        """[(first anchor, anchor count)] of every head in the multi-head order"""
        cfgs = self.model_cfg.RPN_HEAD_CFGS
        names = [n for c in cfgs for n in c['HEAD_CLS_NAME']]
        per_class = [a.numel() // a.shape[-1] for a in self.anchors]
        out, start = [], 0
        for c in cfgs:
            n = sum(per_class[names.index(k)] for k in c['HEAD_CLS_NAME'])
            out.append((start, n))
            start += n
        return out

    def _head_decoder(self, B, box_preds, dir_preds):
        ranges = self.head_anchor_ranges()

        def decode(h, idx):
            """(B,k) long indices into head h's anchors -> (B,k,7+C) decoded boxes of those anchors"""
            s, n = ranges[h]
            anchors = self._flat_anchors()[s:s + n]
            return self.generate_predicted_boxes(batch_size=B, cls_preds=[], box_preds=box_preds[h],
                                                 dir_cls_preds=None if dir_preds is None else dir_preds[h], anchor_idx=idx,
                                                 anchors=anchors)[1]
        return decode

    # ------------------------------------------------------------------------------------------------ losses
    def _cls_weights(self):
        lw = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        if 'pos_cls_weight' in lw:
            return float(lw['pos_cls_weight']), float(lw['neg_cls_weight'])
        return 1.0, 1.0

    def _class_starts(self):
        """first class column of every head (the reference's c_idx), None when every head predicts all classes"""
        if not self.separate_multihead:
            return None
        starts, c = [], 0
        for h in self.rpn_heads:
            starts.append(c)
            c += h.num_class
        return starts

    def fused_loss_unsupported(self):
        """None when csrc/multihead_loss.hip implements this head's losses, else the reason"""
        from crbhip import multihead as _mh
        if self.box_coder.code_size != 7:
            return 'code size %d' % self.box_coder.code_size
        if type(self.reg_loss_func) is not loss_utils.WeightedSmoothL1Loss or self.reg_loss_func.code_weights is None:
            return 'regression loss %s' % type(self.reg_loss_func).__name__
        if type(self.cls_loss_func) is not loss_utils.SigmoidFocalClassificationLoss:
            return 'classification loss %s' % type(self.cls_loss_func).__name__
        if max(h.num_class for h in self.rpn_heads) > _mh.MAX_HEAD_CLASSES:
            return 'more than %d classes in a head' % _mh.MAX_HEAD_CLASSES
        if self.model_cfg.get('NUM_DIR_BINS', 2) > 8:
            return '%d direction bins' % self.model_cfg.NUM_DIR_BINS
        if len(self.rpn_heads) > _mh.MAX_HEADS:
            return '%d heads' % len(self.rpn_heads)
        if not self.use_multihead:
            return 'USE_MULTIHEAD off'
        return None

    def _pred_lists(self):
        d = self.forward_ret_dict
        B = int(d['box_cls_labels'].shape[0])
        ranges = self.head_anchor_ranges()

        def split(t):
            if t is None or isinstance(t, list):
                return t
            t = t.view(B, sum(n for _, n in ranges), -1)
            return [t[:, s:s + n] for s, n in ranges]
        return split(d['cls_preds']), split(d['box_preds']), split(d.get('dir_cls_preds', None))

    def loss_fused(self):
        from crbhip import multihead as _mh, rpn_loss as _rl
        d = self.forward_ret_dict
        lw = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        cls, box, dirs = self._pred_lists()
        B = int(d['box_cls_labels'].shape[0])
        # the struct is cached, keyed on every value it snapshots (reading the code weights back is a host synchronisation)
        cw = self.reg_loss_func.code_weights
        key = (self.num_class, self.model_cfg.get('NUM_DIR_BINS', 2), lw['cls_weight'], lw['loc_weight'], lw.get('dir_weight', 0.0),
               self.model_cfg.get('DIR_OFFSET', 0.0), self.cls_loss_func.alpha, self.cls_loss_func.gamma, self.reg_loss_func.beta,
               cw.data_ptr(), cw._version)
        if self.__dict__.get('_crb_loss_cfg', (None, None))[0] != key:
            self.__dict__['_crb_loss_cfg'] = (key, _rl.make_cfg(
                self.num_class, self.model_cfg.get('NUM_DIR_BINS', 2), cw.tolist(), lw['cls_weight'], lw['loc_weight'],
                lw.get('dir_weight', 0.0), self.model_cfg.get('DIR_OFFSET', 0.0), alpha=self.cls_loss_func.alpha,
                gamma=self.cls_loss_func.gamma, beta=self.reg_loss_func.beta))
        cfg = self.__dict__['_crb_loss_cfg'][1]
        pos_w, neg_w = self._cls_weights()
        per_frame = _mh.multihead_loss(cls, box, dirs, d['box_cls_labels'], d['box_reg_targets'], self._flat_anchors().view(-1, 7), cfg,
                                       class_starts=self._class_starts(), pos_cls_weight=pos_w, neg_cls_weight=neg_w)      # (B,3)
        parts = per_frame.sum(0) / B
        det = parts.detach()
        tb = {'rpn_loss_cls': det[0], 'rpn_loss_loc': det[1]}
        rpn_loss = parts.sum() if dirs is not None else parts[:2].sum()
        if dirs is not None:
            tb['rpn_loss_dir'] = det[2]
        tb['rpn_loss'] = rpn_loss.detach()
        return rpn_loss, tb

    def loss_torch(self):
        """get_cls_layer_loss + get_box_reg_layer_loss of the reference (:245-373) for all heads, in the dtype of the predictions"""
        d = self.forward_ret_dict
        lw = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        cls, box, dirs = self._pred_lists()
        labels, reg_targets = d['box_cls_labels'], d['box_reg_targets'].to(box[0].dtype)
        B = int(labels.shape[0])
        pos_w, neg_w = self._cls_weights()
        positives, negatives, cared = labels > 0, labels == 0, labels >= 0
        # (the classification and regression weights are f32 whatever the predictions are, the direction weights follow the logits:
        # .float() at :263-265 and :310, type_as at :362)
        norm = torch.clamp(positives.sum(1, keepdim=True).float(), min=1.0)
        cls_weights = (neg_w * negatives + pos_w * positives).float() / norm
        reg_weights = positives.float() / norm
        dir_weights = positives.to(box[0].dtype)
        dir_weights = dir_weights / torch.clamp(dir_weights.sum(-1, keepdim=True), min=1.0)
        if self.num_class == 1:
            labels = torch.where(positives, torch.ones_like(labels), labels)
        cls_targets = (labels * cared.type_as(labels)).long()
        one_hot = torch.zeros(*cls_targets.shape, self.num_class + 1, dtype=cls[0].dtype, device=labels.device)
        one_hot.scatter_(-1, cls_targets.unsqueeze(-1), 1.0)
        one_hot = one_hot[..., 1:]
        dir_targets = None
        if dirs is not None:
            anchors = self._flat_anchors().to(box[0].dtype)
            anchors = anchors.view(1, -1, anchors.shape[-1]).expand(B, -1, -1)
            dir_targets = self.get_direction_target(anchors, reg_targets, dir_offset=self.model_cfg.DIR_OFFSET,
                                                    num_bins=self.model_cfg.NUM_DIR_BINS)
        start = c_idx = 0
        cls_loss = loc_loss = dir_loss = 0
        for h, head in enumerate(self.rpn_heads):
            n, nc = cls[h].shape[1], head.num_class
            sl = slice(start, start + n)
            target = one_hot[:, sl, c_idx:c_idx + nc] if self.separate_multihead else one_hot[:, sl]
            if self.separate_multihead:
                c_idx += nc
            cls_loss = cls_loss + self.cls_loss_func(cls[h].reshape(B, n, nc), target, weights=cls_weights[:, sl]).sum() / B
            p, t = box[h].reshape(B, n, -1), reg_targets[:, sl]
            if dirs is not None:
                p, t = self.add_sin_difference(p, t)
            loc_loss = loc_loss + self.reg_loss_func(p, t, weights=reg_weights[:, sl]).sum() / B
            if dirs is not None:
                logits = dirs[h].reshape(B, n, self.model_cfg.NUM_DIR_BINS)
                dir_loss = dir_loss + self.dir_loss_func(logits, dir_targets[:, sl].to(logits.dtype), weights=dir_weights[:, sl]).sum() / B
            start += n
        assert start == one_hot.shape[1]
        cls_loss, loc_loss = cls_loss * lw['cls_weight'], loc_loss * lw['loc_weight']
        tb = {'rpn_loss_cls': cls_loss.detach(), 'rpn_loss_loc': loc_loss.detach()}
        rpn_loss = cls_loss + loc_loss
        if dirs is not None:
            dir_loss = dir_loss * lw['dir_weight']
            tb['rpn_loss_dir'] = dir_loss.detach()
            rpn_loss = rpn_loss + dir_loss
        tb['rpn_loss'] = rpn_loss.detach()
        return rpn_loss, tb

    def get_loss(self):
        cls0 = self.forward_ret_dict['cls_preds']
        cls0 = cls0[0] if isinstance(cls0, list) else cls0
        if FUSED_LOSS and cls0.is_cuda and cls0.dtype == torch.float32:
            why = self.fused_loss_unsupported()
            if why is None:
                return self.loss_fused()
            warnings.warn('AnchorHeadMulti.get_loss: torch route (%s)' % why)
        return self.loss_torch()
