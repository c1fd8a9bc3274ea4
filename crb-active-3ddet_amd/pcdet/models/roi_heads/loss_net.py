"""LossNet (pcdet/models/roi_heads/loss_net.py:4-70): the loss-prediction module of LLAL (Learning Loss for Active Learning).
Per shared-FC layer k of the RoI head: Conv1d(SHARED_FC[k] -> 1, k=1, bias=False), BatchNorm1d(1), ReLU over the RoI rows; the
(frames, ROI_PER_IMAGE) maps of all layers side by side go through one Linear(ROI_PER_IMAGE * num_layer -> 1).

Submodule names and their registration order (conv_0, bn_0, relu_0, conv_1, ..., linear) are those of the reference: its training
loop reads `list(loss_net.children())[0].weight.requires_grad`, and its checkpoints carry these state-dict keys.
Device tensors go through two HIP launches each way (crbhip.loss_net, csrc/loss_net.hip); CPU tensors run the torch expressions."""
import torch
import torch.nn as nn


class LossNet(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_layer = len(self.model_cfg.LOSS_NET.SHARED_FC)
        for k in range(self.num_layer):
            setattr(self, 'conv_%d' % k, nn.Conv1d(self.model_cfg.LOSS_NET.SHARED_FC[k], 1, kernel_size=1, bias=False))
            setattr(self, 'bn_%d' % k, nn.BatchNorm1d(1))
            setattr(self, 'relu_%d' % k, nn.ReLU())
        self.rows_per_frame = model_cfg.TARGET_CONFIG.ROI_PER_IMAGE
        self.linear = nn.Linear(self.rows_per_frame * self.num_layer, 1)
        self.init_weights(weight_init='xavier')

    def init_weights(self, weight_init='xavier'):
        init = {'kaiming': nn.init.kaiming_normal_, 'xavier': nn.init.xavier_normal_, 'normal': nn.init.normal_}[weight_init]
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Conv1d)):
                if weight_init == 'normal':
                    init(m.weight, mean=0, std=0.001)
                else:
                    init(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def forward(self, features, batch_size=None):
        """features: num_layer latents (frames * ROI_PER_IMAGE, SHARED_FC[k], 1) -> (frames, 1) loss predictions"""
        if features[0].is_cuda:
            from crbhip import loss_net
            return loss_net.loss_net(self, features, batch_size)
        out_list = []
        for k in range(self.num_layer):
            out = getattr(self, 'conv_%d' % k)(features[k])
            out = getattr(self, 'bn_%d' % k)(out)
            out = getattr(self, 'relu_%d' % k)(out)
            out_list.append(out.view(batch_size, -1))
        return self.linear(torch.cat(out_list, 1))
