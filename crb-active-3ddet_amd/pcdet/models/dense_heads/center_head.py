"""CenterHead / SeparateHead (pcdet/models/dense_heads/center_head.py:11-355): the anchor-free head of CenterPoint. Same module tree
=> same state_dict keys and shapes; the reference's initialisation.

What differs from the reference:
  * assign_targets is one launch sequence on the device for all frames and heads (crbhip.center_head.assign_targets) instead of three
    nested Python loops on the host; it does NOT write the head-local class id back into the batch's gt_boxes (the reference does,
    through a view: center_head.py:194-195). Every object goes to the head that names its class, with id = index in that head + 1.
  * get_loss is one forward and one backward launch pair per head (crbhip.center_head.center_loss); pred_dict['hm'] keeps the logits
    (the reference overwrites it with the clamped sigmoid); tb_dict holds detached tensors, not .item() values.
  * the first 3x3 + BN + ReLU layers of all branches of a head read the same map and run as ONE convolution over the concatenated
    filters (FUSED_HEAD_CONVS); shared_conv and that convolution go through the Winograd / fused BatchNorm routes of the BEV
    backbone where they qualify. The final 3x3 convolutions (1-3 output channels) stay on F.conv2d.
  * generate_predicted_boxes decodes the K picked cells of every head in one launch and leaves the per-head tensors in
    data_dict['center_preds'] for CenterPoint.post_processing (one batched NMS per head); it also gathers the heatmap logits of all
    heads at every box's cell (pred_logits, the detector's class order).
Kept quirks: slot = rank among the frame's boxes of the head in input order, NUM_MAX_OBJS truncation, num_pos over the whole batch,
no gradient outside the sigmoid clamp."""
import copy

import torch
import torch.nn as nn
from torch.nn.init import kaiming_normal_

from crbhip import center_head as _ch

from ..backbones_2d import base_bev_backbone as _bev

FUSED_HEAD_CONVS = True     # the branches' first 3x3 convolutions as one convolution over the concatenated filters


def _run(seq, x):
    """a [Conv2d, BatchNorm2d, ReLU] sequence on the routes of the BEV backbone (Winograd 3x3, fused BatchNorm + ReLU rows)"""
    if not x.is_cuda or not x.is_contiguous(memory_format=torch.channels_last):
        return seq(x)
    if not seq.training and not torch.is_grad_enabled():
        return _bev.BaseBEVBackbone._run_folded(seq, x)
    return _bev.BaseBEVBackbone._run_rows_train(seq, x) if _bev.ROWS_TRAIN else seq(x)


def _conv3x3(x, weight, bias):
    if _bev.WINOGRAD and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last):
        from crbhip import winograd
        if winograd.supported2(weight.shape[1], weight.shape[0], x.shape[2], x.shape[3]):
            return winograd.conv3x3(x, weight, bias)
    return torch.nn.functional.conv2d(x, weight, bias, padding=1)


def _bn_relu(bn, relu, x):
    """BatchNorm2d + ReLU of a channel slice of the fused convolution's output. The slice is a strided rows view (row stride = all
    branches' channels); bnrelu.bn_relu makes it contiguous, one copy of the slice each way (bn_relu_concat / bn_apply_into write INTO
    slices of a shared map, the opposite direction)."""
    from crbhip import bnrelu
    if _bev.ROWS_TRAIN and x.is_cuda and x.dtype == torch.float32 and x.permute(0, 2, 3, 1).stride(3) == 1 and \
            bnrelu.supported(x.new_empty((2, x.shape[1])), bn) and not bnrelu.frame_groups_active():
        n, c, h, w = x.shape
        rows = x.permute(0, 2, 3, 1).reshape(n * h * w, c)
        return bnrelu.bn_relu(rows, bn, relu=True).view(n, h, w, c).permute(0, 3, 1, 2)
    return relu(bn(x))


class SeparateHead(nn.Module):
    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for cur_name in self.sep_head_dict:
            output_channels = self.sep_head_dict[cur_name]['out_channels']
            num_conv = self.sep_head_dict[cur_name]['num_conv']
            fc_list = []
            for k in range(num_conv - 1):
                fc_list.append(nn.Sequential(
                    nn.Conv2d(input_channels, input_channels, kernel_size=3, stride=1, padding=1, bias=use_bias),
                    nn.BatchNorm2d(input_channels), nn.ReLU()))
            fc_list.append(nn.Conv2d(input_channels, output_channels, kernel_size=3, stride=1, padding=1, bias=True))
            fc = nn.Sequential(*fc_list)
            if 'hm' in cur_name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        kaiming_normal_(m.weight.data)
                        if hasattr(m, 'bias') and m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            self.__setattr__(cur_name, fc)

    def forward(self, x):
        names = list(self.sep_head_dict)
        seqs = {n: self.__getattr__(n) for n in names}
        first = {n: s[0] for n, s in seqs.items() if len(s) > 1}
        mid = {}
        convs = [f[0] for f in first.values()]
        if FUSED_HEAD_CONVS and len(first) > 1 and all(isinstance(f[1], nn.BatchNorm2d) for f in first.values()) and \
                len({c.bias is None for c in convs}) == 1:
            # the first layers read the same map: one convolution over the concatenated filters reads it once and writes its
            # gradient once (as AnchorHeadSingle.FUSED_HEAD_CONVS); the parameters stay the separate modules'
            w = torch.cat([c.weight for c in convs], 0)
            b = torch.cat([c.bias for c in convs], 0) if convs[0].bias is not None else None
            y = _conv3x3(x, w, b)
            for (n, f), part in zip(first.items(), torch.split(y, [c.out_channels for c in convs], 1)):
                mid[n] = _bn_relu(f[1], f[2], part)
        else:
            for n, f in first.items():
                mid[n] = _run(f, x)
        ret = {}
        for n, s in seqs.items():
            t = mid.get(n, x)
            for layer in list(s)[1:-1]:
                t = _run(layer, t)
            ret[n] = s[-1](t)
        return ret


class CenterHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True, **kwargs):
        super().__init__()
        if predict_boxes_when_training:
            raise NotImplementedError('CenterHead: a RoI head behind the centre head (predict_boxes_when_training) is not supported')
        if model_cfg.POST_PROCESSING.NMS_CONFIG.NMS_TYPE == 'circle_nms':
            raise NotImplementedError('CenterHead: NMS_TYPE circle_nms is not supported (the reference asserts False on it)')
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size = grid_size
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        self.voxel_size = [float(v) for v in voxel_size]
        self.feature_map_stride = self.model_cfg.TARGET_ASSIGNER_CONFIG.get('FEATURE_MAP_STRIDE', None)
        self.class_names = list(class_names)
        self.class_names_each_head = [[x for x in names if x in class_names] for names in self.model_cfg.CLASS_NAMES_EACH_HEAD]
        self.class_id_mapping_each_head = [[self.class_names.index(x) for x in names] for names in self.class_names_each_head]
        total_classes = sum(len(x) for x in self.class_names_each_head)
        assert total_classes == len(self.class_names), f'class_names_each_head={self.class_names_each_head}'
        self.class_head, self.class_local, self.head_channels = _ch.class_tables(self.class_names, self.model_cfg.CLASS_NAMES_EACH_HEAD)
        use_bias = self.model_cfg.get('USE_BIAS_BEFORE_NORM', False)
        self.shared_conv = nn.Sequential(
            nn.Conv2d(input_channels, self.model_cfg.SHARED_CONV_CHANNEL, 3, stride=1, padding=1, bias=use_bias),
            nn.BatchNorm2d(self.model_cfg.SHARED_CONV_CHANNEL), nn.ReLU())
        self.heads_list = nn.ModuleList()
        self.separate_head_cfg = self.model_cfg.SEPARATE_HEAD_CFG
        for cur_class_names in self.class_names_each_head:
            cur_head_dict = copy.deepcopy(dict(self.separate_head_cfg.HEAD_DICT))
            cur_head_dict['hm'] = dict(out_channels=len(cur_class_names), num_conv=self.model_cfg.NUM_HM_CONV)
            self.heads_list.append(SeparateHead(input_channels=self.model_cfg.SHARED_CONV_CHANNEL, sep_head_dict=cur_head_dict,
                                                init_bias=-2.19, use_bias=use_bias))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}

    def assign_targets(self, gt_boxes, feature_map_size=None, **kwargs):
        """gt_boxes (B, M, 7 + E + 1), feature_map_size (H, W) -> {'heatmaps', 'target_boxes', 'inds', 'masks'}: lists over heads.
        gt_boxes is not written."""
        cfg = self.model_cfg.TARGET_ASSIGNER_CONFIG
        H, W = int(feature_map_size[0]), int(feature_map_size[1])
        per_head = _ch.assign_targets(gt_boxes, self.class_head, self.class_local, self.head_channels, H, W, self.point_cloud_range,
                                      self.voxel_size, cfg.FEATURE_MAP_STRIDE, cfg.NUM_MAX_OBJS, cfg.GAUSSIAN_OVERLAP, cfg.MIN_RADIUS)
        return {'heatmaps': [p[0] for p in per_head], 'target_boxes': [p[1] for p in per_head], 'inds': [p[2] for p in per_head],
                'masks': [p[3] for p in per_head], 'heatmap_masks': []}

    def get_loss(self):
        pred_dicts = self.forward_ret_dict['pred_dicts']
        target_dicts = self.forward_ret_dict['target_dicts']
        w = self.model_cfg.LOSS_CONFIG.LOSS_WEIGHTS
        tb_dict = {}
        loss = 0
        for idx, pred_dict in enumerate(pred_dicts):
            parts = _ch.center_loss(pred_dict['hm'], target_dicts['heatmaps'][idx],
                                    [pred_dict[n] for n in self.separate_head_cfg.HEAD_ORDER], target_dicts['target_boxes'][idx],
                                    target_dicts['inds'][idx], target_dicts['masks'][idx], w['code_weights'], w['cls_weight'],
                                    w['loc_weight']).to(pred_dict['hm'].dtype)
            loss = loss + (parts[0] + parts[1])
            tb_dict['hm_loss_head_%d' % idx] = parts[0].detach()
            tb_dict['loc_loss_head_%d' % idx] = parts[1].detach()
        tb_dict['rpn_loss'] = loss.detach()
        return loss, tb_dict

    @torch.no_grad()
    def generate_predicted_boxes(self, batch_size, pred_dicts):
        """-> list over heads of {'boxes' (B,K,7+), 'scores' (B,K), 'labels' (B,K) 0-based in the detector's class order, 'keep' (B,K)
        bool, 'logits' (B,K,num_class)}; rows in descending score order"""
        cfg = self.model_cfg.POST_PROCESSING
        order = ['center', 'center_z', 'dim', 'rot'] + (['vel'] if 'vel' in self.separate_head_cfg.HEAD_ORDER else [])
        out = []
        for idx, pred_dict in enumerate(pred_dicts):
            hm = pred_dict['hm']
            top = _ch.top_cells(hm.detach(), cfg.MAX_OBJ_PER_SAMPLE)
            boxes, scores, labels, keep = _ch.decode(hm, [pred_dict[n] for n in order], cfg.MAX_OBJ_PER_SAMPLE, self.point_cloud_range,
                                                     self.voxel_size, self.feature_map_stride, cfg.POST_CENTER_LIMIT_RANGE,
                                                     cfg.SCORE_THRESH, top=top)
            mapping = torch.tensor(self.class_id_mapping_each_head[idx], dtype=torch.int64, device=hm.device)
            _, flat, cl = top                                          # the logits of ALL heads at the box's cell
            cell = flat // hm.shape[1] if cl else flat % (hm.shape[2] * hm.shape[3])
            logits = hm.new_zeros((hm.shape[0], cell.shape[1], self.num_class))
            for h2, p2 in enumerate(pred_dicts):
                logits[..., self.class_id_mapping_each_head[h2]] = _ch.gather_at([p2['hm'].detach()], cell)
            out.append({'boxes': boxes, 'scores': scores, 'labels': mapping[labels], 'keep': keep, 'logits': logits})
        return out

    def forward(self, data_dict):
        spatial_features_2d = data_dict['spatial_features_2d']
        x = _run(self.shared_conv, spatial_features_2d)
        pred_dicts = [head(x) for head in self.heads_list]
        if self.training:
            self.forward_ret_dict['target_dicts'] = self.assign_targets(
                data_dict['gt_boxes'], feature_map_size=spatial_features_2d.size()[2:],
                feature_map_stride=data_dict.get('spatial_features_2d_strides', None))
        self.forward_ret_dict['pred_dicts'] = pred_dicts
        if not self.training:
            data_dict['center_preds'] = self.generate_predicted_boxes(data_dict['batch_size'], pred_dicts)
        return data_dict
