"""CPU: the LLAL pieces (loss-prediction module, ranking loss, strategy registration, config) against ref_llal.npz, which
tests/golden/make_goldens_llal.py records from the reference's own PVRCNNHead with ROI_HEAD.LOSS_NET."""
import copy
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_llal.npz')
FRAMES, ROWS, WIDTH = 4, 128, 32


def _t(a):
    return torch.from_numpy(np.array(a))


def make_head(width=WIDTH, rows=ROWS):
    """the generator's small PVRCNNHead: FC widths `width`, ROI_PER_IMAGE = NMS_POST_MAXSIZE (TEST) = `rows`, LOSS_NET set"""
    from pcdet.config import EasyDict
    from pcdet.model_cfgs import pv_rcnn_llal_cfg
    from pcdet.models.roi_heads import PVRCNNHead
    cfg = copy.deepcopy(pv_rcnn_llal_cfg().MODEL.ROI_HEAD)
    cfg.SHARED_FC, cfg.CLS_FC, cfg.REG_FC = [width, width], [width, width], [width, width]
    cfg.LOSS_NET.SHARED_FC = [width, width]
    cfg.TARGET_CONFIG.ROI_PER_IMAGE = rows
    cfg.NMS_CONFIG.TEST.NMS_POST_MAXSIZE = rows
    cfg.ROI_GRID_POOL = EasyDict({'GRID_SIZE': 2, 'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.8, 1.6],
                                  'NSAMPLE': [16, 16], 'POOL_METHOD': 'max_pool'})
    torch.manual_seed(0)
    return PVRCNNHead(input_channels=12, model_cfg=cfg, num_class=1)


def load_golden_state(ln, g):
    with torch.no_grad():
        for k in range(2):
            getattr(ln, 'conv_%d' % k).weight.copy_(_t(g['in/conv_%d' % k]))
            bn = getattr(ln, 'bn_%d' % k)
            bn.weight.copy_(_t(g['in/gamma_%d' % k]))
            bn.bias.copy_(_t(g['in/beta_%d' % k]))
            bn.running_mean.copy_(_t(g['in/rmean_%d' % k]))
            bn.running_var.copy_(_t(g['in/rvar_%d' % k]))
            bn.num_batches_tracked.zero_()
        ln.linear.weight.copy_(_t(g['in/lin_w']))
        ln.linear.bias.copy_(_t(g['in/lin_b']))


def test_llal_is_registered():
    from pcdet.query_strategies import names, build_strategy, LLALSampling  # noqa: F401
    assert 'llal' in names()
    with pytest.raises(KeyError):
        build_strategy('no-such-strategy', None, None, None, 0, '/tmp', None)


def test_llal_config_variant():
    from pcdet.model_cfgs import pv_rcnn_llal_cfg, pv_rcnn_cfg
    c, base = pv_rcnn_llal_cfg(), pv_rcnn_cfg()
    h = c.MODEL.ROI_HEAD
    assert h.LOSS_NET.SHARED_FC == [256, 256] and h.EMBEDDING_REQUIRED is False and 'SAMPLING_ROUND' not in h
    assert h.TARGET_CONFIG.ROI_PER_IMAGE == h.NMS_CONFIG.TEST.NMS_POST_MAXSIZE == 128
    assert c.OPTIMIZATION.LOSS_NET_SKIP is True and c.ACTIVE_TRAIN.METHOD == 'llal' and c.ACTIVE_TRAIN.LOSS_NET_TRAIN_EPOCH == 10
    assert 'LOSS_NET' not in base.MODEL.ROI_HEAD and base.MODEL.ROI_HEAD.SAMPLING_ROUND == 5     # the CRB config is untouched


def test_loss_net_module_order_and_state_dict_keys_match_the_reference():
    g = np.load(G)
    head = make_head()
    assert [n for n, _ in head.loss_net.named_children()] == list(g['children'])
    assert list(head.loss_net.children())[0] is head.loss_net.conv_0
    assert [k for k in head.state_dict().keys() if k.startswith('loss_net.')] == list(g['head_keys'])
    assert head.loss_net.conv_0.weight.shape == (1, WIDTH, 1) and head.loss_net.linear.weight.shape == (1, 2 * ROWS)


def test_loss_net_torch_path_matches_the_reference():
    """float64 CPU LossNet: train-mode output, running statistics, num_batches_tracked, every gradient, then eval output"""
    g = np.load(G)
    ln = make_head().loss_net.double()
    load_golden_state(ln, g)
    lat = [_t(g['in/latent_%d' % k]).requires_grad_(True) for k in range(2)]
    ln.train()
    pred = ln(lat, batch_size=FRAMES)
    pred.backward(_t(g['in/upstream']))
    np.testing.assert_allclose(pred.detach().numpy(), g['train_out'], rtol=1e-12, atol=1e-14)
    for n, p in ln.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), g['grad/' + n], rtol=1e-10, atol=1e-13, err_msg=n)
    for k in range(2):
        np.testing.assert_allclose(lat[k].grad.numpy(), g['grad/latent_%d' % k], rtol=1e-10, atol=1e-14)
        bn = getattr(ln, 'bn_%d' % k)
        np.testing.assert_allclose(bn.running_mean.numpy(), g['after/running_mean_%d' % k], rtol=1e-12)
        np.testing.assert_allclose(bn.running_var.numpy(), g['after/running_var_%d' % k], rtol=1e-12)
        assert int(bn.num_batches_tracked) == int(g['after/num_batches_tracked_%d' % k]) == 1
    ln.eval()
    with torch.no_grad():
        np.testing.assert_allclose(ln([t.detach() for t in lat], batch_size=FRAMES).numpy(), g['eval_out'], rtol=1e-12, atol=1e-14)


def test_loss_pred_loss_matches_the_reference_and_needs_an_even_batch():
    from pcdet.models.roi_heads import RoIHeadTemplate
    g = np.load(G)
    x, t = _t(g['in/lpl_input']), _t(g['in/lpl_target'])
    np.testing.assert_allclose(RoIHeadTemplate.LossPredLoss(x, t).numpy(), g['lpl_mean'], rtol=1e-14)
    np.testing.assert_allclose(RoIHeadTemplate.LossPredLoss(x, t, reduction='none').numpy(), g['lpl_none'], rtol=1e-14)
    xg = x.clone().requires_grad_(True)
    tg = t.clone().requires_grad_(True)
    RoIHeadTemplate.LossPredLoss(xg, tg).backward()
    assert tg.grad is None and xg.grad is not None                   # the target is detached
    with pytest.raises(AssertionError):
        RoIHeadTemplate.LossPredLoss(x[:3], t[:3])


def test_loss_net_bookkeeping_of_the_head():
    """get_loss_loss_net reads forward_ret_dict['loss_predictions'] and leaves a detached tensor in tb_dict"""
    head = make_head()
    preds = torch.randn(4, 1, requires_grad=True)
    head.forward_ret_dict = {'loss_predictions': preds}
    tb = {}
    loss = head.get_loss_loss_net(tb, torch.randn(4))
    assert torch.is_tensor(tb['loss_loss_net']) and not tb['loss_loss_net'].requires_grad
    assert float(tb['loss_loss_net']) == float(loss.detach())


def test_head_runs_on_cpu_tensors_train_and_eval():
    """the shared-FC paths of the head hand the post-ReLU latents to the loss net (CPU tensors: torch LossNet): training path,
    eval fast path (folded conv-BN, no extra FC pass) and the plain eval path agree; a RoI count other than ROI_PER_IMAGE per
    frame is refused"""
    head = make_head()
    g3, c = 8, 8 * 2                                                    # GRID_SIZE 2, two 8-channel MLP outputs
    torch.manual_seed(1)
    pooled = torch.rand(2 * ROWS, g3, c)
    head.train()
    taps = []
    head._heads_pooled(pooled, taps)
    assert len(taps) == 2 and all(t.shape == (2 * ROWS, WIDTH, 1) for t in taps)
    pred_train = head.predict_loss(taps, 2)
    assert pred_train.shape == (2, 1) and pred_train.requires_grad
    assert int(head.loss_net.bn_0.num_batches_tracked) == 1
    head.eval()
    with torch.no_grad():
        fast = []
        head._heads_eval(pooled, 1, fast)
        plain = []
        head._heads(pooled.permute(0, 2, 1).contiguous().view(2 * ROWS, -1, 1), plain)
        assert len(fast) == len(plain) == 2
        for a, b in zip(fast, plain):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(head.predict_loss(fast, 2), head.predict_loss(plain, 2), rtol=1e-5, atol=1e-6)
        with pytest.raises(ValueError, match='ROI_PER_IMAGE'):
            head.predict_loss([t[:ROWS + 1] for t in fast], 2)
