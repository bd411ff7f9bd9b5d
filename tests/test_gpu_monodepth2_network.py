"""The monodepth2 depth network (ResnetEncoder + DepthDecoder with a sigmoid head at every scale) on the GPU against the vectors
recorded from the reference's own classes (tests/golden/g10_monodepth2.npz), under the tolerances tests/test_gpu_network.py holds the
indoor network to against g7_net; and ops.depth_from_disp_range against the reference's convert_disp_to_depth."""
import pytest
import torch

import disp_head_ref as R
from oracle import depthnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _models(scales=range(4)):
    from depth_estimation.networks import DepthDecoder, ResnetEncoder
    part = R.split_state_dict(depthnet.random_state_dict(0), scales)
    enc = ResnetEncoder(18, False)
    dec = DepthDecoder(enc.num_ch_enc, scales)
    enc.load_state_dict(part["depth_encoder"])
    dec.load_state_dict(part["depth_decoder"])
    return enc.to(DEV).eval(), dec.to(DEV).eval()


def test_forward_backward_vs_golden(golden):
    g = golden("g10_monodepth2")
    enc, dec = _models()
    out = dec(enc(g["img"].to(DEV)), 0)
    assert list(out.keys()) == [("disp", 0, s) for s in (3, 2, 1, 0)]
    for s in range(4):
        assert out[("disp", 0, s)].shape == g[f"disp{s}"].shape
        torch.testing.assert_close(out[("disp", 0, s)].cpu(), g[f"disp{s}"], rtol=1e-4, atol=1e-5)
    sum((out[("disp", 0, s)] * g[f"wgt{s}"].to(DEV)).sum() for s in range(4)).backward()
    names = list(g["grad_names"])
    params = {"encoder." + n: p for n, p in enc.named_parameters()}
    params.update({"decoder." + n: p for n, p in dec.named_parameters()})
    assert sorted(params) == sorted(names)
    for n, ref in zip(names, g["grad_norms"]):
        if ref < 0:
            assert params[n].grad is None
        else:
            torch.testing.assert_close(params[n].grad.norm().cpu(), ref, rtol=1e-3, atol=1e-7)
    for k in [k for k in g if k.startswith("gs_")]:
        name = [n for n in names if "gs_" + n.replace(".", "_") == k][0]
        ref = g[k]
        got = params[name].grad.flatten()[:16].cpu()
        assert (got - ref).abs().max() <= 2e-3 * ref.abs().max() + 1e-7, name


def test_batch_of_two_equals_two_calls(golden):
    colors = golden("g8_refine")["colors"].to(DEV)
    enc, dec = _models()
    with torch.no_grad():
        a = dict(dec(enc(colors[:, 0]), 0))
        b = dict(dec(enc(colors[:, 1]), 0))
        both = dict(dec(enc(colors[0]), 0))
    for s in range(4):
        k = ("disp", 0, s)
        torch.testing.assert_close(both[k], torch.cat([a[k], b[k]], 0), rtol=1e-5, atol=1e-6)


def test_single_scale_decoder_evaluates_one_head(golden):
    """DATA.scales: [0] -- the reference's 11-module decoder; its one output is scale 0 of the four-scale network"""
    g = golden("g10_monodepth2")
    enc, dec = _models([0])
    assert len(dec.decoder) == 11 and list(dec.convs.keys())[-1] == ("dispconv", 0)
    assert list(dec.state_dict().keys()) == ["decoder.%d.%s" % (i, s) for i in range(11) for s in (("conv.conv.weight", "conv.conv.bias") if i < 10 else ("conv.weight", "conv.bias"))]
    with torch.no_grad():
        out = dec(enc(g["img"].to(DEV)), 2)
    assert list(out.keys()) == [("disp", 2, 0)]
    torch.testing.assert_close(out[("disp", 2, 0)].cpu(), g["disp0"], rtol=1e-4, atol=1e-5)


def test_depth_from_disp_range_vs_golden_and_float64(golden):
    from e2ehip import ops
    g = golden("g10_monodepth2")
    disp = g["disp0"].to(DEV).requires_grad_(True)
    depth = ops.depth_from_disp_range(disp, 0.1, 80.0, 1.0)
    assert R.rel(depth.detach().cpu(), g["depth0"]) < R.BOUND                  # the reference's convert_disp_to_depth
    wgt = torch.randn(g["disp0"].shape, generator=torch.Generator().manual_seed(4))
    for scale in (1.0, 6.9):
        disp.grad = None
        depth = ops.depth_from_disp_range(disp, 0.1, 80.0, scale)
        assert R.rel(depth.detach().cpu(), R.range_depth(g["disp0"], 0.1, 80.0, scale)) < R.BOUND
        (depth * wgt.to(DEV)).sum().backward()
        assert R.rel(disp.grad.cpu(), R.range_depth_bwd(wgt, g["disp0"], 0.1, 80.0, scale)) < R.GRAD_BOUND
