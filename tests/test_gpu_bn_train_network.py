"""Train-mode BatchNorm of the depth networks on the native kernels (csrc/bn_train.hip behind e2ehip.nn_ops.batch_norm_train): no
call of torch.nn.functional.batch_norm on that path, agreement with the oracle's train-mode evaluation, the version bump that makes
a later eval() fold the UPDATED statistics, and the module fallback for a BatchNorm the kernels do not cover."""
import pytest
import torch
import torch.nn.functional as F

import disp_head_ref as DR
from oracle import depthnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 64, 96


def _inputs():
    g = torch.Generator().manual_seed(11)
    return torch.rand(2, H, W, 3, generator=g), torch.randn(2, 1, H, W, generator=g) / (H * W)


def _indoor(sd):
    from depth_estimation.networks import DispResNet_Indoor
    m = DispResNet_Indoor(18, False)
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _oracle_train(sd, x, wgt=None):
    """The functional restatement with BatchNorm in training mode; running buffers of sd_o are updated in place."""
    keys = [k for k in sd if sd[k].dtype.is_floating_point and "running" not in k]
    sd_o = {k: (v.clone().requires_grad_(True) if k in keys else v.clone()) for k, v in sd.items()}
    depthnet.BN_TRAINING[0] = True
    try:
        d = depthnet.disp_forward(sd_o, x)
        if wgt is not None:
            (d * wgt).sum().backward()
    finally:
        depthnet.BN_TRAINING[0] = False
    return d.detach(), sd_o


def _bn_grads_finite(model):
    """The number of BatchNorm modules of `model`, every one with a finite gradient on its weight and bias."""
    bns = [b for b in model.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    for b in bns:
        assert b.weight.grad is not None and b.bias.grad is not None
        assert torch.isfinite(b.weight.grad).all() and torch.isfinite(b.bias.grad).all()
    return len(bns)


def test_no_functional_batch_norm_on_the_native_path(monkeypatch):
    """Both networks, train mode, forward and backward on 2 x 64 x 96 with torch.nn.functional.batch_norm replaced by a function that
    raises: every BatchNorm runs on the kernels, and every BatchNorm parameter and the stem's weight get a gradient."""
    from depth_estimation.networks import DepthDecoder, ResnetEncoder

    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.batch_norm was called on the native train-mode path")
    monkeypatch.setattr(F, "batch_norm", refuse)
    monkeypatch.delenv("E2E_BN_NATIVE", raising=False)
    x, wgt = _inputs()
    sd = depthnet.random_state_dict(0)
    m = _indoor(sd)
    disp = m(x.to(DEV), 0)[("disp", 0, 0)]
    (disp * wgt.to(DEV)).sum().backward()
    assert _bn_grads_finite(m) == 20 and torch.isfinite(m.encoder.encoder.conv1.weight.grad).all()
    counts = {int(b) for n, b in m.named_buffers() if n.endswith("num_batches_tracked")}
    assert counts == {int(sd["encoder.encoder.bn1.num_batches_tracked"]) + 1}
    part = DR.split_state_dict(sd, range(4))
    enc = ResnetEncoder(18, False)
    dec = DepthDecoder(enc.num_ch_enc, range(4))
    enc.load_state_dict(part["depth_encoder"])
    dec.load_state_dict(part["depth_decoder"])
    enc.to(DEV).train()
    dec.to(DEV).train()
    out = dec(enc(x.to(DEV)), 0)
    sum(out[("disp", 0, s)].mean() for s in range(4)).backward()
    assert _bn_grads_finite(enc) == 20 and torch.isfinite(enc.encoder.conv1.weight.grad).all()
    assert len([n for n, b in enc.named_buffers() if n.endswith("num_batches_tracked")]) == 20


def test_indoor_network_agrees_with_the_oracle(monkeypatch):
    """Disparity, four named gradients and three BatchNorms' buffers against oracle.depthnet under BN_TRAINING, with the tolerances of
    tests/test_gpu_network.py::test_train_mode_batchnorm_compatibility_path."""
    monkeypatch.delenv("E2E_BN_NATIVE", raising=False)
    x, wgt = _inputs()
    sd = depthnet.random_state_dict(0)
    m = _indoor(sd)
    disp = m(x.to(DEV), 0)[("disp", 0, 0)]
    (disp * wgt.to(DEV)).sum().backward()
    d_ref, sd_o = _oracle_train(sd, x, wgt)
    torch.testing.assert_close(disp.detach().cpu(), d_ref, rtol=1e-4, atol=1e-5)
    pm = dict(m.named_parameters())
    for k in ("encoder.encoder.conv1.weight", "encoder.encoder.bn1.weight", "encoder.encoder.layer2.0.downsample.1.bias", "decoder.decoder.0.conv.conv.weight"):
        a, b = pm[k].grad.cpu(), sd_o[k].grad
        assert float((a - b).abs().max()) <= 2e-4 * float(b.abs().max()) + 1e-9, k
    bufs = dict(m.named_buffers())
    for k in ("encoder.encoder.bn1", "encoder.encoder.layer3.0.downsample.1", "encoder.encoder.layer4.1.bn2"):
        torch.testing.assert_close(bufs[k + ".running_mean"].cpu(), sd_o[k + ".running_mean"], rtol=1e-4, atol=1e-6)
        torch.testing.assert_close(bufs[k + ".running_var"].cpu(), sd_o[k + ".running_var"], rtol=1e-4, atol=1e-6)
        assert int(bufs[k + ".num_batches_tracked"]) == int(sd[k + ".num_batches_tracked"]) + 1


def test_eval_after_train_folds_the_updated_statistics(monkeypatch):
    """The kernels write running_mean / running_var behind torch's back; nn_ops._fold_bn keys its cache on their version counters.
    With the BatchNorm parameters frozen as the refinement mode freezes them (only then is the fold cached): an eval forward (fills the
    cache), one train forward (moves the statistics), eval again -- the last one must equal the oracle's eval forward on the UPDATED
    statistics."""
    monkeypatch.delenv("E2E_BN_NATIVE", raising=False)
    x, _ = _inputs()
    sd = depthnet.random_state_dict(0)
    m = _indoor(sd)
    for name, p in m.named_parameters():
        if "bn" in name:
            p.requires_grad = False
    with torch.no_grad():
        m.eval()
        before = m(x.to(DEV), 0)[("disp", 0, 0)].cpu()
        v0 = m.encoder.encoder.bn1.running_mean._version
        m.train()
        m(x.to(DEV), 0)
        assert m.encoder.encoder.bn1.running_mean._version > v0 and m.encoder.encoder.bn1.running_var._version > v0
        m.eval()
        after = m(x.to(DEV), 0)[("disp", 0, 0)].cpu()
    _, sd_o = _oracle_train(sd, x)
    with torch.no_grad():
        want = depthnet.disp_forward({k: v.detach() for k, v in sd_o.items()}, x)
    torch.testing.assert_close(after, want, rtol=1e-4, atol=1e-5)
    assert not torch.allclose(before, want, rtol=1e-4, atol=1e-5), "the train forward did not move the statistics: the test shows nothing"


def test_module_without_running_statistics_stays_on_the_module(monkeypatch):
    """track_running_stats=False is one of the three fallbacks: _ConvBN.run keeps such a module on nn.BatchNorm2d, and the result
    agrees with torch's own convolution + BatchNorm."""
    from depth_estimation.networks import _ConvBN
    from e2ehip import nn_ops
    monkeypatch.delenv("E2E_BN_NATIVE", raising=False)
    g = torch.Generator().manual_seed(3)
    conv = torch.nn.Conv2d(16, 32, 3, 1, 1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(32, track_running_stats=False).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(32, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(32, generator=g))
    assert not nn_ops.bn_train_native(bn) and nn_ops.bn_train_native(torch.nn.BatchNorm2d(32))
    assert not nn_ops.bn_train_native(torch.nn.BatchNorm2d(32, affine=False)) and not nn_ops.bn_train_native(torch.nn.BatchNorm2d(30))
    with pytest.raises(NotImplementedError):
        nn_ops.batch_norm_train(torch.zeros(2, 32, 4, 4, device=DEV), bn)
    x = torch.randn(2, 16, 12, 20, generator=g).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    res = torch.randn(2, 32, 12, 20, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    calls = []
    real = F.batch_norm
    monkeypatch.setattr(F, "batch_norm", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    y = _ConvBN.run(conv, bn, x, True, residual=res)
    y.square().sum().backward()
    assert calls, "the module did not normalise"
    gx, gw = x.grad.clone(), bn.weight.grad.clone()
    x.grad = bn.weight.grad = conv.weight.grad = None
    want = torch.relu(bn(F.conv2d(x, conv.weight, None, 1, 1)) + res)
    want.square().sum().backward()
    torch.testing.assert_close(y, want, rtol=1e-4, atol=1e-5)
    assert float((gx - x.grad).abs().max()) <= 2e-4 * float(x.grad.abs().max())
    assert float((gw - bn.weight.grad).abs().max()) <= 2e-4 * float(bn.weight.grad.abs().max())
    # one value per channel: torch's own refusal on the native path
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        nn_ops.batch_norm_train(torch.zeros(1, 32, 1, 1, device=DEV), torch.nn.BatchNorm2d(32).to(DEV).train())


def test_conv2d_bn_train_is_the_convolution_followed_by_the_operator(monkeypatch):
    """e2ehip.conv.conv2d_bn_train(x, weight, bn_module, ...) = nn_ops.conv2d + nn_ops.batch_norm_train, bit for bit, momentum=None included
    (the count of batches is read on the device: two calls give 1 / 1 and 1 / 2)."""
    from e2ehip import conv as C
    from e2ehip import nn_ops
    monkeypatch.delenv("E2E_BN_NATIVE", raising=False)
    g = torch.Generator().manual_seed(4)
    w = (torch.randn(32, 16, 3, 3, generator=g) / 12).to(DEV)
    x = torch.randn(2, 16, 9, 14, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    res = torch.randn(2, 32, 9, 14, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    a, b = (torch.nn.BatchNorm2d(32, momentum=None).to(DEV).train() for _ in range(2))
    for _ in range(2):
        ya = C.conv2d_bn_train(x, w, a, 1, 1, "zeros", res, True)
        yb = nn_ops.batch_norm_train(nn_ops.conv2d(x, w, None, 1, 1), b, True, res)
        assert torch.equal(ya, yb)
    assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 2
    assert torch.equal(a.running_mean, b.running_mean) and torch.equal(a.running_var, b.running_var)
    z = F.conv2d(x, w, None, 1, 1)
    torch.testing.assert_close(a.running_mean, z.mean((0, 2, 3)), rtol=1e-4, atol=1e-5)          # the cumulative average of two equal batches
    torch.testing.assert_close(a.running_var, z.var((0, 2, 3), unbiased=True), rtol=1e-4, atol=1e-5)
