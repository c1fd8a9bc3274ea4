"""Generate ref_llal.npz from the reference's own LLAL modules (companion of make_goldens.py, whose import recipe it reuses).

Runs ONLY where the reference tree is mounted; the .npz it writes is committed and is the only thing that travels.
Usage:  python tests/golden/make_goldens_llal.py [ref_llal.npz] [ref_pvrcnn_llal.npz]
ref_llal.npz records, from the reference's PVRCNNHead built with ROI_HEAD.LOSS_NET (small FC widths, ROI_PER_IMAGE 128):
  * the loss net's child names in registration order and its state-dict keys (as the head registers them)
  * LossNet on seeded latents of 4 frames: train-mode output, BatchNorm running statistics after the step, and the gradients of
    a seeded upstream vector w.r.t. every loss-net parameter and both latents; then the eval-mode output
  * RoIHeadTemplate.LossPredLoss ('mean' and 'none') on seeded predictions / per-frame losses
ref_pvrcnn_llal.npz: make_goldens.gen_pvrcnn_detector (same two frames, seeded weights, recorded RoI-sampler draws) on the
reference's PVRCNN with ROI_HEAD.LOSS_NET set (the LLAL config's SHARED_FC [256, 256]):
  * the loss-net phase (loss net trainable, lal_flag on): loss, tb_dict, second-stage outputs, the eight detector gradients
    (what ref_pvrcnn_detector.npz holds, without the intermediate features), the per-frame rpn / point / rcnn losses, the loss
    predictions, loss_loss_net, every loss-net gradient and the loss net's BatchNorm running statistics after the step; then the
    loss net in eval mode on the latents of that step (its running statistics as the step left them)
  * the frozen step (loss-net parameters requires_grad False): loss, tb_dict and the loss net's running statistics after it"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_goldens import import_reference, save, _np, EasyDict  # noqa: E402

FRAMES, ROWS, WIDTH = 4, 128, 32


def head_cfg():
    return EasyDict({
        'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [WIDTH, WIDTH], 'CLS_FC': [WIDTH, WIDTH],
        'REG_FC': [WIDTH, WIDTH], 'DP_RATIO': 0.3, 'LOSS_NET': {'SHARED_FC': [WIDTH, WIDTH]}, 'EMBEDDING_REQUIRED': False,
        'NMS_CONFIG': {'TRAIN': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,
                                 'NMS_POST_MAXSIZE': 512, 'NMS_THRESH': 0.8},
                       'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 1024,
                                'NMS_POST_MAXSIZE': ROWS, 'NMS_THRESH': 0.7}},
        'ROI_GRID_POOL': {'GRID_SIZE': 2, 'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.8, 1.6], 'NSAMPLE': [16, 16],
                          'POOL_METHOD': 'max_pool'},
        'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': ROWS, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                          'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                          'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
        'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                        'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                         'code_weights': [1.0] * 7}}})


def llal_inputs():
    """seeded loss-net state and inputs (float64), shared with tests/test_llal_cpu.py through the stored arrays"""
    rng = np.random.default_rng(2023)
    d = {}
    for k in range(2):
        d['conv_%d' % k] = rng.normal(0, 0.3, (1, WIDTH, 1))
        d['gamma_%d' % k] = rng.uniform(0.5, 1.5, (1,))
        d['beta_%d' % k] = rng.uniform(-0.2, 0.2, (1,))
        d['rmean_%d' % k] = rng.uniform(-0.1, 0.1, (1,))
        d['rvar_%d' % k] = rng.uniform(0.8, 1.2, (1,))
        d['latent_%d' % k] = np.maximum(rng.normal(0, 1, (FRAMES * ROWS, WIDTH, 1)), 0.0)
    d['lin_w'] = rng.normal(0, 0.05, (1, 2 * ROWS))
    d['lin_b'] = rng.normal(0, 0.05, (1,))
    d['upstream'] = rng.normal(0, 1, (FRAMES, 1))
    d['lpl_input'] = rng.normal(0, 1, (FRAMES, 1))
    d['lpl_target'] = rng.normal(0, 1, (FRAMES,))
    return d


def gen_llal(out):
    from pcdet.config import cfg as ref_cfg
    ref_cfg.CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist']
    from pcdet.models.roi_heads.pvrcnn_head import PVRCNNHead
    torch.manual_seed(0)
    head = PVRCNNHead(input_channels=12, model_cfg=head_cfg(), num_class=1).double()
    ln = head.loss_net
    out['children'] = np.array([n for n, _ in ln.named_children()])
    out['head_keys'] = np.array([k for k in head.state_dict().keys() if k.startswith('loss_net.')])
    inp = llal_inputs()
    out.update({'in/' + k: v for k, v in inp.items()})
    with torch.no_grad():
        for k in range(2):
            getattr(ln, 'conv_%d' % k).weight.copy_(torch.from_numpy(inp['conv_%d' % k]))
            bn = getattr(ln, 'bn_%d' % k)
            bn.weight.copy_(torch.from_numpy(inp['gamma_%d' % k]))
            bn.bias.copy_(torch.from_numpy(inp['beta_%d' % k]))
            bn.running_mean.copy_(torch.from_numpy(inp['rmean_%d' % k]))
            bn.running_var.copy_(torch.from_numpy(inp['rvar_%d' % k]))
        ln.linear.weight.copy_(torch.from_numpy(inp['lin_w']))
        ln.linear.bias.copy_(torch.from_numpy(inp['lin_b']))
    lat = [torch.from_numpy(inp['latent_%d' % k]).requires_grad_(True) for k in range(2)]
    ln.train()
    pred = ln(lat, batch_size=FRAMES)
    pred.backward(torch.from_numpy(inp['upstream']))
    out['train_out'] = _np(pred)
    for n, p in ln.named_parameters():
        out['grad/' + n] = _np(p.grad)
    for k in range(2):
        out['grad/latent_%d' % k] = _np(lat[k].grad)
        bn = getattr(ln, 'bn_%d' % k)
        out['after/running_mean_%d' % k] = _np(bn.running_mean)
        out['after/running_var_%d' % k] = _np(bn.running_var)
        out['after/num_batches_tracked_%d' % k] = _np(bn.num_batches_tracked)
    ln.eval()
    with torch.no_grad():
        out['eval_out'] = _np(ln([t.detach() for t in lat], batch_size=FRAMES))
    x, t = torch.from_numpy(inp['lpl_input']), torch.from_numpy(inp['lpl_target'])
    out['lpl_mean'] = _np(head.LossPredLoss(x, t))
    out['lpl_none'] = _np(head.LossPredLoss(x, t, reduction='none'))
    print('  children', list(out['children']), 'train_out', out['train_out'].ravel(), 'lpl', out['lpl_mean'])


def gen_pvrcnn_llal(out):
    import make_goldens as mg
    import pcdet.models as ref_models
    from pcdet.models.roi_heads.roi_head_template import RoIHeadTemplate
    orig_cfg, orig_build, orig_lln = mg.pvrcnn_model_cfg, ref_models.build_network, RoIHeadTemplate.get_loss_loss_net

    def llal_cfg(kind='kitti'):
        m, names = orig_cfg(kind)
        m.ROI_HEAD.LOSS_NET = EasyDict({'SHARED_FC': [256, 256]})
        m.POINT_HEAD.NUM_KEYPOINTS = m.PFE.NUM_KEYPOINTS          # pv_rcnn_active_llal.yaml sets it (reduce=False reads it)
        m.ROI_HEAD.pop('SAMPLING_ROUND', None)
        m.ROI_HEAD.EMBEDDING_REQUIRED = False
        return m, names
    rec = {}
    built = []

    def recorded(obj, name, key):
        fn = getattr(obj, name)

        def wrapper(*a, **k):
            r = fn(*a, **k)
            rec[key] = (r[0] if isinstance(r, tuple) else r).detach().clone()
            return r
        setattr(obj, name, wrapper)

    def build(frozen):
        def fn(**kw):
            model = orig_build(**kw)
            for head, key in ((model.dense_head, 'rpn'), (model.point_head, 'point'), (model.roi_head, 'rcnn')):
                recorded(head, 'get_loss', key)
            ln = model.roi_head.loss_net
            ln_forward = ln.forward

            def ln_capture(features, batch_size=None):
                rec['latents'] = [f.detach().clone() for f in features]
                return ln_forward(features, batch_size=batch_size)
            ln.forward = ln_capture
            if frozen:
                for p in ln.parameters():
                    p.requires_grad_(False)
            built.append(model)
            return model
        return fn

    def lln(self, tb_dict=None, loss=None):
        r = orig_lln(self, tb_dict, loss)
        rec['target'], rec['pred'], rec['lln'] = loss.detach().clone(), self.forward_ret_dict['loss_predictions'].detach().clone(), r.detach()
        return r
    drop = ('pv_point_features', 'pv_pooled', 'pv_point_coords', 'pv_point_cls_scores')
    mg.pvrcnn_model_cfg, RoIHeadTemplate.get_loss_loss_net = llal_cfg, lln
    try:
        ref_models.build_network = build(False)
        step = {}
        mg.gen_pvrcnn_detector(step)
        out.update({k: v for k, v in step.items() if k not in drop})
        model = built[-1]
        ln = model.roi_head.loss_net
        for key in ('rpn', 'point', 'rcnn'):
            out['llal/loss_' + key] = _np(rec[key])
            assert out['llal/loss_' + key].shape == (2,), (key, out['llal/loss_' + key].shape)
        out['llal/target'], out['llal/pred'], out['llal/loss_loss_net'] = _np(rec['target']), _np(rec['pred']), np.array([float(rec['lln'])])
        for n, p in ln.named_parameters():
            out['llal/grad/' + n] = _np(p.grad)
        for k in range(2):
            bn = getattr(ln, 'bn_%d' % k)
            out['llal/after/running_mean_%d' % k], out['llal/after/running_var_%d' % k] = _np(bn.running_mean), _np(bn.running_var)
        ln.eval()
        with torch.no_grad():
            out['llal/eval_pred'] = _np(ln(rec['latents'], batch_size=2))
        ref_models.build_network = build(True)
        frozen = {}
        mg.gen_pvrcnn_detector(frozen)
        out['frozen/loss'] = frozen['pv_loss']
        out['frozen/tb_keys'], out['frozen/tb_vals'] = frozen['pv_tb_keys'], frozen['pv_tb_vals']
        ln = built[-1].roi_head.loss_net
        for k in range(2):
            bn = getattr(ln, 'bn_%d' % k)
            out['frozen/running_mean_%d' % k], out['frozen/running_var_%d' % k] = _np(bn.running_mean), _np(bn.running_var)
    finally:
        mg.pvrcnn_model_cfg, ref_models.build_network, RoIHeadTemplate.get_loss_loss_net = orig_cfg, orig_build, orig_lln
    print('  llal loss %.5f, per frame rpn %s point %s rcnn %s, pred %s, loss_loss_net %.5f, eval pred %s; frozen loss %.5f' % (
        float(out['pv_loss'][0]), out['llal/loss_rpn'], out['llal/loss_point'], out['llal/loss_rcnn'], out['llal/pred'].ravel(),
        float(out['llal/loss_loss_net'][0]), out['llal/eval_pred'].ravel(), float(out['frozen/loss'][0])))


if __name__ == '__main__':
    import_reference()
    only = sys.argv[1:]
    for name, fn in (('ref_llal.npz', gen_llal), ('ref_pvrcnn_llal.npz', gen_pvrcnn_llal)):
        if only and name not in only:
            continue
        d = {}
        fn(d)
        save(name, d)
