"""One tiny convolution step through e2ehip._lib.call positionally and by the header's parameter names: the two argument vectors must
launch the same work (bit-identical outputs, equal to the module path e2ehip.conv.conv2d on the same data), and KernelTimer must
account the keyword call by name."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# apart from KH = KW every value is distinct, so a transposed pair shows
GEOM = dict(B=2, Hs=12, Ws=20, Cin=8, Cout=16, Ho=6, Wo=10, KH=3, KW=3, stride=2, pad=1, pad_mode=0, C1=8, up=1, in_sub=0.0, in_mul=1.0)


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(5)
    q = GEOM
    return dict(x=torch.randn(q["B"], q["Hs"], q["Ws"], q["Cin"], generator=g).to(DEV), w=torch.randn(q["Cout"], q["Cin"], q["KH"], q["KW"], generator=g).to(DEV),
                bias=torch.randn(q["Cout"], generator=g).to(DEV), da=torch.randn(q["B"], q["Ho"], q["Wo"], q["Cout"], generator=g).to(DEV))


def _step(d, by_name):
    """weight layouts -> forward -> backward-data -> backward-weight; by_name: keywords + the geometry mapping, else the positional lists."""
    from e2ehip import _lib as L
    from e2ehip.conv import _gemm_workspace, _ld
    q = GEOM
    B, Hs, Ws, Cin, Cout, Ho, Wo, KH, KW, stride, pad, pm, C1, up, isub, imul = q.values()
    ldf, ldb = _ld(Cout), _ld(Cin)
    wf, wb = torch.zeros(KH * KW * Cin, ldf, device=DEV), torch.zeros(KH * KW * Cout, ldb, device=DEV)
    out, dx = torch.full((B, Ho, Wo, Cout), float("nan"), device=DEV), torch.full((B, Hs, Ws, Cin), float("nan"), device=DEV)
    dw, db = torch.full((Cout, Cin, KH, KW), float("nan"), device=DEV), torch.full((Cout,), float("nan"), device=DEV)
    ws_f = _gemm_workspace(L.query("e2e_conv2d_splitk_workspace_floats", B * Ho * Wo, Cout, KH * KW * Cin), DEV)
    ws_w = torch.empty(L.query("e2e_conv2d_wgrad_workspace_floats", B, Ho, Wo, Cin, Cout, KH, KW, 1), device=DEV)
    st = L.stream()
    if by_name:
        ws_b = _gemm_workspace(L.query("e2e_conv2d_bwd_data_workspace_floats", geom=q, Hd=Hs, Wd=Ws, cols=Cin, K=KH * KW * Cout), DEV)
        L.call("e2e_conv_weight_layouts", geom=q, w=L.ptr(d["w"]), w_fwd=L.ptr(wf), ld_fwd=ldf, w_bwd=L.ptr(wb), ld_bwd=ldb, stream=st)
        L.call("e2e_conv2d_fwd", geom=q, src0=L.ptr(d["x"]), src1=None, w_fwd=L.ptr(wf), ld_fwd=ldf, scale=None, shift=L.ptr(d["bias"]), residual=None,
               out=L.ptr(out), act=0, workspace=L.ptr(ws_f), stream=st)
        L.call("e2e_conv2d_bwd_data", geom=q, dz=L.ptr(d["da"]), w_bwd=L.ptr(wb), ld_bwd=ldb, dxp=L.ptr(dx), workspace=L.ptr(ws_b), stream=st)
        L.call("e2e_conv2d_bwd_weight_scaled", geom=q, da=L.ptr(d["da"]), out_scale=None, src0=L.ptr(d["x"]), src1=None, dw=L.ptr(dw), dbias=L.ptr(db),
               workspace=L.ptr(ws_w), accumulate=0, stream=st)
    else:
        ws_b = _gemm_workspace(L.query("e2e_conv2d_bwd_data_workspace_floats", B, Hs, Ws, Cin, KH * KW * Cout, stride), DEV)
        L.call("e2e_conv_weight_layouts", L.ptr(d["w"]), Cout, Cin, KH, KW, L.ptr(wf), ldf, L.ptr(wb), ldb, st)
        L.call("e2e_conv2d_fwd", L.ptr(d["x"]), None, C1, up, L.ptr(wf), ldf, None, L.ptr(d["bias"]), None, L.ptr(out), B, Hs, Ws, Cin, Cout, KH, KW,
               stride, pad, pm, 0, isub, imul, L.ptr(ws_f), st)
        L.call("e2e_conv2d_bwd_data", L.ptr(d["da"]), L.ptr(wb), ldb, L.ptr(dx), B, Hs, Ws, Cin, Cout, Ho, Wo, KH, KW, stride, pad, pm, L.ptr(ws_b), st)
        L.call("e2e_conv2d_bwd_weight_scaled", L.ptr(d["da"]), None, L.ptr(d["x"]), None, C1, up, L.ptr(dw), L.ptr(db), L.ptr(ws_w), B, Hs, Ws, Cin, Cout,
               Ho, Wo, KH, KW, stride, pad, pm, 0, isub, imul, st)
    torch.cuda.synchronize()
    return dict(wf=wf, wb=wb, out=out, dx=dx, dw=dw, db=db)


def test_conv_step_positional_and_by_name_are_bit_identical(data):
    from e2ehip.conv import conv2d
    pos, named = _step(data, False), _step(data, True)
    x = data["x"].permute(0, 3, 1, 2).requires_grad_(True)                       # the module path: NCHW view of the same NHWC memory
    w, bias = data["w"].clone().requires_grad_(True), data["bias"].clone().requires_grad_(True)
    y = conv2d(x, w, bias, stride=GEOM["stride"], padding=GEOM["pad"])
    y.backward(data["da"].permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    module = dict(wf=w._e2e_layouts["wf"], wb=w._e2e_layouts["wb"], out=y.detach().permute(0, 2, 3, 1), dx=x.grad.permute(0, 2, 3, 1), dw=w.grad, db=bias.grad)
    for k, v in pos.items():
        assert not torch.isnan(v).any(), k
        assert torch.equal(v, named[k]), f"{k}: the keyword call differs from the positional call"
        assert torch.equal(v, module[k]), f"{k}: differs from e2ehip.conv.conv2d"


def test_kernel_timer_accounts_the_keyword_call_by_name(data):
    from e2ehip import _lib as L
    from e2ehip.conv import _gemm_workspace
    from e2ehip.profile import KernelTimer
    q = GEOM
    wf = _step(data, True)["wf"]
    out = torch.empty(q["B"], q["Ho"], q["Wo"], q["Cout"], device=DEV)
    ws = _gemm_workspace(L.query("e2e_conv2d_splitk_workspace_floats", q["B"] * q["Ho"] * q["Wo"], q["Cout"], q["KH"] * q["KW"] * q["Cin"]), DEV)
    with KernelTimer() as kt:
        L.call("e2e_conv2d_fwd", geom=q, src0=L.ptr(data["x"]), src1=None, w_fwd=L.ptr(wf), ld_fwd=wf.shape[1], scale=None, shift=L.ptr(data["bias"]),
               residual=None, out=L.ptr(out), act=0, workspace=L.ptr(ws), stream=L.stream())
    row = kt.summary()["e2e_conv2d_fwd"]
    assert (row["calls"], row["flops"], row["bytes"]) == (1, 276480, 27648) and row["ms"] > 0
