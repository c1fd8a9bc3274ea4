"""GPU: LLAL (loss-prediction module of PV-RCNN and the `llal` query strategy) through the HIP path — the loss-net kernels against a
float64 torch LossNet, the detector step in the loss-net phase and with the loss net frozen, determinism, and the strategy's pick."""
import copy
import pickle

import numpy as np
import pytest
import torch

from synth import kitti_batch

pytestmark = pytest.mark.gpu

C, P = 256, 128


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _lossnet(seed=0):
    from pcdet.config import EasyDict
    from pcdet.models.roi_heads.loss_net import LossNet
    torch.manual_seed(seed)
    ln = LossNet(EasyDict({'LOSS_NET': {'SHARED_FC': [C, C]}, 'TARGET_CONFIG': {'ROI_PER_IMAGE': P}}))
    with torch.no_grad():
        for k in range(2):
            bn = getattr(ln, 'bn_%d' % k)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.2, 0.2)
            bn.running_mean.uniform_(-0.1, 0.1)
            bn.running_var.uniform_(0.8, 1.2)
    return ln


@pytest.mark.parametrize('train', [True, False])
@pytest.mark.parametrize('B', [2, 4, 16])
def test_loss_net_kernels_match_float64_torch(dev, B, train):
    ref = _lossnet().double()
    gpu = _lossnet().to(dev)
    ref.train(train)
    gpu.train(train)
    torch.manual_seed(B)
    lat = [torch.relu(torch.randn(B * P, C, 1)) for _ in range(2)]
    up = torch.randn(B, 1)
    xs = [t.to(dev).requires_grad_(True) for t in lat]
    out = gpu(xs, batch_size=B)
    out.backward(up.to(dev))
    xr = [t.double().requires_grad_(True) for t in lat]
    out_ref = ref(xr, batch_size=B)
    out_ref.backward(up.double())
    assert out.shape == (B, 1) and _rel(out, out_ref) <= 1e-6
    for (n, p), (_, pr) in zip(gpu.named_parameters(), ref.named_parameters()):
        assert _rel(p.grad, pr.grad) <= 1e-6, (n, _rel(p.grad, pr.grad))
    for k in range(2):
        assert _rel(xs[k].grad, xr[k].grad) <= 1e-6, k
        bn, bnr = getattr(gpu, 'bn_%d' % k), getattr(ref, 'bn_%d' % k)
        assert _rel(bn.running_mean, bnr.running_mean) <= 1e-6 and _rel(bn.running_var, bnr.running_var) <= 1e-6
        assert int(bn.num_batches_tracked) == int(bnr.num_batches_tracked) == (1 if train else 0)


def test_loss_net_kernels_are_bit_reproducible(dev):
    torch.manual_seed(3)
    lat = [torch.relu(torch.randn(16 * P, C, 1, device=dev)) for _ in range(2)]
    up = torch.randn(16, 1, device=dev)
    runs = []
    for _ in range(2):
        ln = _lossnet().to(dev).train()
        xs = [t.clone().requires_grad_(True) for t in lat]
        out = ln(xs, batch_size=16)
        out.backward(up)
        runs.append([out] + [x.grad for x in xs] + [p.grad for p in ln.parameters()] + list(ln.buffers()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _model(dev, loss_net=True):
    from pcdet.datasets import SyntheticDataset
    from pcdet.model_cfgs import pv_rcnn_llal_cfg
    from pcdet.models import build_network
    cfg = pv_rcnn_llal_cfg()
    if not loss_net:
        cfg.MODEL.ROI_HEAD.pop('LOSS_NET')
    torch.manual_seed(0)
    return build_network(cfg.MODEL, 3, SyntheticDataset(num_frames=2)).to(dev)


def _batch(dev, first=0, B=2, n=20000):
    pts, off, gt = kitti_batch(first, B, n)
    bidx = np.repeat(np.arange(B, dtype=np.float32), np.diff(off))
    return {'points': torch.from_numpy(np.concatenate([bidx[:, None], pts], 1)).to(dev),
            'point_frame_offsets': torch.from_numpy(off).to(dev), 'gt_boxes': torch.from_numpy(gt).to(dev),
            'batch_size': B, 'point_frame_counts_host': np.diff(off).tolist(),
            'frame_id': np.array(['%06d' % (first + i) for i in range(B)])}


def _step(model, dev, seed=5):
    model.train()
    np.random.seed(seed)
    torch.manual_seed(seed)
    ret, tb, _ = model(_batch(dev))
    model.zero_grad(set_to_none=True)
    ret['loss'].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return ret['loss'].detach().clone(), tb, grads


def _set_loss_net_trainable(model, flag):
    for p in model.roi_head.loss_net.parameters():
        p.requires_grad_(flag)


def test_loss_net_phase_step_and_frozen_step(dev):
    """loss-net phase (lal_flag on): per-frame losses, ranking loss and gradients into the loss net and, through the latents,
    into the shared FC layers. Frozen (LOSS_NET_SKIP): loss and every gradient bit-equal to the same weights without a loss net,
    while the loss net's BatchNorm running statistics still advance."""
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        model = _model(dev)
        state = copy.deepcopy(model.state_dict())
        loss, tb, grads = _step(model, dev)
        assert torch.isfinite(loss) and 'loss_loss_net' in tb and torch.is_tensor(tb['loss_loss_net'])
        preds = model.roi_head.forward_ret_dict['loss_predictions']
        assert preds.shape == (2, 1)
        for n in ('roi_head.loss_net.conv_0.weight', 'roi_head.loss_net.conv_1.weight', 'roi_head.loss_net.bn_0.weight',
                  'roi_head.loss_net.linear.weight', 'roi_head.shared_fc_layer.0.weight'):
            assert n in grads and torch.isfinite(grads[n]).all() and float(grads[n].abs().sum()) > 0, n
        # the ranking loss sees prediction differences of frame pairs: the linear bias cancels, its gradient is exactly 0
        assert float(grads['roi_head.loss_net.linear.bias'].abs().sum()) == 0.0
        assert int(model.roi_head.loss_net.bn_0.num_batches_tracked) == 1

        # frozen: the ordinary step, bit for bit
        model.load_state_dict(state)
        _set_loss_net_trainable(model, False)
        loss_f, tb_f, grads_f = _step(model, dev)
        assert 'loss_loss_net' not in tb_f
        assert not any('loss_net' in n for n in grads_f)
        assert int(model.roi_head.loss_net.bn_0.num_batches_tracked) == 1
        assert not torch.equal(model.roi_head.loss_net.bn_0.running_mean, state['roi_head.loss_net.bn_0.running_mean'])
        plain = _model(dev, loss_net=False)
        plain.load_state_dict({k: v for k, v in state.items() if '.loss_net.' not in k})
        loss_p, _, grads_p = _step(plain, dev)
        assert torch.equal(loss_f, loss_p), (float(loss_f), float(loss_p))
        assert grads_f.keys() == grads_p.keys()
        for n in grads_p:
            assert torch.equal(grads_f[n], grads_p[n]), n
    finally:
        torch.use_deterministic_algorithms(was)


def test_loss_net_phase_step_is_deterministic(dev):
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        model = _model(dev)
        state = copy.deepcopy(model.state_dict())
        runs = []
        for _ in range(2):
            model.load_state_dict(state)
            loss, tb, grads = _step(model, dev)
            ln = model.roi_head.loss_net
            runs.append((loss, tb['loss_loss_net'], {n: g for n, g in grads.items() if 'loss_net' in n},
                         [b.clone() for b in ln.buffers()]))
        (l0, r0, g0, b0), (l1, r1, g1, b1) = runs
        assert torch.equal(l0, l1) and torch.equal(r0, r1)
        assert g0.keys() == g1.keys() and len(g0) == 8
        for n in g0:
            assert torch.equal(g0[n], g1[n]), n
        for a, b in zip(b0, b1):
            assert torch.equal(a, b)
    finally:
        torch.use_deterministic_algorithms(was)


def test_llal_query_small_pool(dev, tmp_path):
    """build_strategy('llal').query() picks the SELECT_NUMS frames with the highest loss prediction — recomputed here by the torch
    LossNet (float64, CPU) from the latents the head handed to the kernels — and writes the reference's pickle"""
    from pcdet.datasets import SyntheticDataset, build_synthetic_dataloader
    from pcdet.model_cfgs import pv_rcnn_llal_cfg
    from pcdet.models import build_network
    from pcdet.query_strategies import build_strategy
    cfg = pv_rcnn_llal_cfg()
    cfg.ACTIVE_TRAIN.SELECT_NUMS = 3
    pool = SyntheticDataset(num_frames=10, first_frame=300)
    lab = SyntheticDataset(num_frames=4, first_frame=0)
    torch.manual_seed(0)
    model = build_network(cfg.MODEL, 3, pool).to(dev)
    head = model.roi_head
    with torch.no_grad():
        head.loss_net.linear.weight.normal_(0, 0.5)       # spread the predictions of the random-init detector
    # a random-init RPN puts its proposals far from any point (every frame would pool the same empty balls): jittered GT boxes
    orig_proposal_layer, orig_predict = head.proposal_layer, head.predict_loss

    def gt_proposals(batch_dict, nms_config):
        batch_dict = orig_proposal_layer(batch_dict, nms_config=nms_config)
        gt = batch_dict['gt_boxes'][..., :7]
        reps = -(-batch_dict['rois'].shape[1] // gt.shape[1])
        rois = gt.repeat(1, reps, 1)[:, :batch_dict['rois'].shape[1]].clone()
        rois[..., :3] += 0.2 * torch.randn_like(rois[..., :3])
        batch_dict['rois'] = rois
        return batch_dict
    seen = []

    def recording(latents, batch_size):
        seen.append(([t.detach().double().cpu() for t in latents], batch_size))
        return orig_predict(latents, batch_size)
    head.proposal_layer, head.predict_loss = gt_proposals, recording
    strat = build_strategy('llal', model, build_synthetic_dataloader(lab, 2), build_synthetic_dataloader(pool, 4), 0,
                           str(tmp_path), cfg)
    picked = strat.query(cur_epoch=0)
    ref_ln = copy.deepcopy(head.loss_net).double().cpu().eval()
    with torch.no_grad():
        ref = torch.cat([ref_ln(lat, batch_size=b).view(-1) for lat, b in seen])
    assert ref.numel() == len(pool.sample_id_list)
    assert _rel(strat.last_values, ref) <= 1e-5
    assert len(set(ref.tolist())) == ref.numel()
    order = torch.argsort(ref, stable=True)[-3:].tolist()
    assert picked == [pool.sample_id_list[i] for i in order]
    strat.save_active_labels(selected_frames=picked, cur_epoch=3)
    with open(str(tmp_path / 'selected_frames_epoch_3_rank_0.pkl'), 'rb') as f:
        d = pickle.load(f)
    assert list(d.keys()) == ['frame_id', 'selected_mean_points', 'selected_bbox', 'selected_median_points',
                              'selected_variance_points']
    assert d['frame_id'] == picked and len(d['selected_bbox']) == 3
