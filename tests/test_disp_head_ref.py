"""Host checks of tests/disp_head_ref.py: the float64 references of the multi-scale disparity heads against explicit index arithmetic and
against autograd through the activation, the qualification of every input the GPU contract module uses (the float32 CPU evaluation stays
within a quarter of the bound of the float64 one), the depth-range formula, and the plain-torch restatement of the monodepth2 network
against the vectors recorded from the reference (tests/golden/g10_monodepth2.npz).  Also the host-visible part of the feature: the
layer shapes e2ehip.conv accepts and the decoder's module list."""
import pytest
import torch

import disp_head_ref as R
from oracle import depthnet


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


@pytest.mark.parametrize("Cin,shape", [(16, (1, 2, 2)), (32, (1, 3, 3)), (16, (2, 5, 7))])
def test_head_forward_reference_against_index_arithmetic(Cin, shape):
    B, H, W = shape
    t = R.head_inputs(Cin, B, H, W)
    x, w = t["x"].double(), t["w"].double()
    want = torch.zeros(B, H, W, dtype=torch.float64)
    for h in range(H):
        for ww in range(W):
            for kh in range(3):
                for kw in range(3):
                    want[:, h, ww] += (x[:, _reflect(h + kh - 1, H), _reflect(ww + kw - 1, W), :] * w[0, :, kh, kw]).sum(-1)
    torch.testing.assert_close(R.head_fwd(t["x"], t["w"], None, R.ACT_NONE), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.head_fwd(t["x"], t["w"], t["bias"], R.ACT_SIGMOID), torch.sigmoid(want + t["bias"].double()), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.head_fwd(t["x"], t["w"], t["bias"], R.ACT_DISP), 10 * torch.sigmoid(want + t["bias"].double()) + 0.01,
                               rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("Cin,shape", [(16, (1, 2, 2)), (64, (1, 3, 3)), (32, (2, 5, 7)), (128, (2, 5, 7))])
def test_backward_contract_equals_autograd_through_the_activation(Cin, shape, act):
    """dz = dy * act'(y) from the OUTPUT, then the convolution's adjoints: the same numbers as autograd through act itself"""
    t = R.head_inputs(Cin, *shape)
    y, dx, dw, db = R.head_grads_autograd(t["x"], t["w"], t["bias"], t["dy"], act)
    gx, gw, gb = R.head_bwd(t["dy"], y, t["x"], t["w"], act)
    for a, b in ((gx, dx), (gw, dw), (gb, db)):
        assert R.rel(a, b) < 1e-12


@pytest.mark.parametrize("Cin", R.CINS)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_contract_inputs_qualify(Cin, shape):
    """every case of tests/test_gpu_disp_head_contracts.py: float32 on the CPU within a quarter of the GPU's bound"""
    t = R.head_inputs(Cin, *shape)
    for act in R.ACTS:
        for bias in (t["bias"], None):
            r64 = R.head_fwd(t["x"], t["w"], bias, act)
            e = R.rel(R.head_fwd(t["x"], t["w"], bias, act, torch.float32), r64)
            assert e < R.QUALIFY, ("forward", act, e)
        y = R.head_fwd(t["x"], t["w"], t["bias"], act).float()
        want = R.head_bwd(t["dy"], y, t["x"], t["w"], act)
        got = R.head_bwd(t["dy"], y, t["x"], t["w"], act, torch.float32)
        for name, a, b in zip(("dx", "dw", "dbias"), got, want):
            e = R.rel(a, b)
            assert e < R.GRAD_QUALIFY, (name, act, e)


@pytest.mark.parametrize("n,limits,scale", R.RANGE_CASES)
def test_depth_range_reference_and_its_inputs(n, limits, scale):
    t = R.range_inputs(n, limits, scale)
    assert float(t["disp"].min()) > 0 and float(t["disp"].max()) < 1
    d64 = R.range_depth(t["disp"], *limits, scale)
    lo, hi = 1 / limits[1], 1 / limits[0]
    torch.testing.assert_close(d64, scale / (lo + (hi - lo) * t["disp"].double()), rtol=1e-14, atol=0)
    g64 = R.range_depth_bwd(t["g"], t["disp"], *limits, scale)
    assert R.rel(g64, R.range_depth_grad_autograd(t["g"], t["disp"], *limits, scale)) < 1e-12
    assert R.rel(R.range_depth(t["disp"], *limits, scale, torch.float32), d64) < R.QUALIFY
    assert R.rel(R.range_depth_bwd(t["g"], t["disp"], *limits, scale, torch.float32), g64) < R.GRAD_QUALIFY


def test_restatement_reproduces_the_recorded_monodepth2_network(golden):
    """the tolerances tests/test_oracle_golden.py holds the indoor restatement to against g7_net"""
    g = golden("g10_monodepth2")
    sd = depthnet.random_state_dict(0)
    names = list(g["grad_names"])
    live = [n for n, r in zip(names, g["grad_norms"]) if r >= 0]
    assert len(names) == 90 and len(live) == 88 and set(names) - set(live) == {"encoder.encoder.fc.weight", "encoder.encoder.fc.bias"}
    for n in live:
        sd[n].requires_grad_(True)
    disp = R.monodepth2_forward(sd, g["img"])
    assert list(disp) == [3, 2, 1, 0]
    for s in range(4):
        torch.testing.assert_close(disp[s], g[f"disp{s}"], rtol=1e-4, atol=1e-5)
    sum((disp[s] * g[f"wgt{s}"]).sum() for s in range(4)).backward()
    for n, ref in zip(names, g["grad_norms"]):
        if ref >= 0:
            torch.testing.assert_close(sd[n].grad.norm(), ref, rtol=2e-4, atol=1e-7)
    sampled = [k for k in g if k.startswith("gs_")]
    assert sum("decoder_decoder_1%d_conv_weight" % s in k for k in sampled for s in range(4)) == 4          # the four head weights
    for k in sampled:
        name = [n for n in names if "gs_" + n.replace(".", "_") == k][0]
        torch.testing.assert_close(sd[name].grad.flatten()[:16], g[k], rtol=2e-3, atol=1e-6)
    # convert_disp_to_depth of the reference at (0.1, 80)
    assert R.rel(R.range_depth(g["disp0"], 0.1, 80.0, 1.0), g["depth0"]) < 1e-6


def test_conv_module_accepts_the_four_heads():
    from e2ehip import conv
    assert conv.ACT == {None: 0, "relu": 1, "elu": 2, "disp": 3, "sigmoid": 4}
    for c in R.CINS:
        assert conv.supports(torch.empty(1, c, 3, 3))
    for shape in ((1, 8, 3, 3), (1, 48, 3, 3), (1, 32, 1, 1), (2, 32, 3, 3)):
        assert not conv.supports(torch.empty(*shape))
    assert conv.supports(torch.empty(1, 1, 1, 1)) and conv.supports(torch.empty(32, 5, 3, 3))


def test_decoder_module_list_and_keys_follow_the_scales():
    """DepthDecoder(num_ch_enc, scales=[0]): the reference's 11-module list (ten trunk convolutions + one head); range(4): 14"""
    from depth_estimation.networks import DepthDecoder, ResnetEncoder
    sd = depthnet.random_state_dict(0)
    enc = ResnetEncoder(18, False)
    for scales, n in (([0], 11), (range(4), 14)):
        dec = DepthDecoder(enc.num_ch_enc, scales)
        part = R.split_state_dict(sd, scales)
        assert len(dec.decoder) == n and list(dec.state_dict().keys()) == list(part["depth_decoder"].keys())
        assert [tuple(v.shape) for v in dec.state_dict().values()] == [tuple(v.shape) for v in part["depth_decoder"].values()]
        dec.load_state_dict(part["depth_decoder"])
        assert isinstance(dec.sigmoid, torch.nn.Sigmoid)
    enc.load_state_dict(R.split_state_dict(sd)["depth_encoder"])
