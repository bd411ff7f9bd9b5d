"""e2e_head_bwd_act with both gradients asked for runs ONE pass over the activation (k_head_bwd_fused) instead of k_head_bwd_data + k_head_bwd_weight;
E2E_HEAD_BWD_FUSED=0 (read by every call) restores the two kernels.  The fused pass keeps the partition, the lane mapping and every summation
order of the kernels it replaces, so dx, dw and dbias must be equal BIT FOR BIT between the two settings in the same build; both are also
compared with float64 autograd on the CPU under the gradient bound of tests/test_gpu_conv.py::test_disparity_head (5e-5 of max |reference|)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
HC = 16

SHAPES = [(1, 3, 3),       # every pixel is a border or border-adjacent pixel
          (1, 7, 5),
          (2, 24, 40),
          (2, 33, 17),     # pixel count no multiple of 64, ragged per-workgroup ranges
          (2, 256, 320)]   # 80 pixels per workgroup: a second, ragged pass of the 64 pixel slots


def _inputs(shape, in_act, seed):
    B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, H, W, HC, generator=g)
    x = {0: u, 1: F.relu(u), 2: F.elu(u)}[in_act]
    return dict(x=x, dz=torch.randn(B, H, W, generator=g), w=torch.randn(1, HC, 3, 3, generator=g) * 0.1)


def _run(t, shape, in_act, with_bias, fused, monkeypatch):
    from e2ehip import _lib as L
    B, H, W = shape
    monkeypatch.setenv("E2E_HEAD_BWD_FUSED", "1" if fused else "0")
    x, dz, w = (t[k].to(DEV) for k in ("x", "dz", "w"))
    n = B * H * W * HC
    dx = torch.full((n + SENTINEL,), float("nan"), device=DEV)
    dw = torch.full((9 * HC + SENTINEL,), float("nan"), device=DEV)
    db = torch.full((1 + SENTINEL,), float("nan"), device=DEV)
    ws = torch.full((L.load().e2e_head_workspace_floats() + SENTINEL,), float("nan"), device=DEV)
    L.call("e2e_head_bwd_act", dz=L.ptr(dz), x=L.ptr(x), w=L.ptr(w), dx=L.ptr(dx), dw=L.ptr(dw), dbias=L.ptr(db) if with_bias else None, workspace=L.ptr(ws),
           B=B, H=H, W=W, Cin=HC, in_act=in_act, stream=L.stream())
    torch.cuda.synchronize()
    for name, buf in (("dx", dx), ("dw", dw), ("dbias", db), ("workspace", ws)):
        assert torch.isnan(buf[-SENTINEL:]).all(), f"{name}: written past its end"
    assert torch.isnan(db[0]).item() == (not with_bias)
    return dx[:n], dw[:9 * HC], db[:1]


def _ref64(t, in_act):
    x = t["x"].double().permute(0, 3, 1, 2).requires_grad_(True)
    w = t["w"].double().requires_grad_(True)
    b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], t["dz"].double().unsqueeze(1))
    xd = x.detach()
    if in_act == 1:
        gx = gx * (xd > 0)
    elif in_act == 2:
        gx = gx * torch.where(xd > 0, torch.ones_like(xd), xd + 1)
    return gx.permute(0, 2, 3, 1).contiguous().flatten(), gw.flatten(), gb


@pytest.mark.parametrize("with_bias", [True, False], ids=["dbias", "nodbias"])
@pytest.mark.parametrize("in_act", [0, 2], ids=["none", "elu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_pass_equals_the_two_kernels(shape, in_act, with_bias, monkeypatch):
    t = _inputs(shape, in_act, seed=shape[1] * 100 + shape[2])
    two = _run(t, shape, in_act, with_bias, False, monkeypatch)
    one = _run(t, shape, in_act, with_bias, True, monkeypatch)
    names = ("dx", "dw", "dbias") if with_bias else ("dx", "dw")
    for name, a, b in zip(names, one, two):
        assert not torch.isnan(b).any() and torch.equal(a, b), f"{shape} in_act {in_act}: {name} differs between the fused pass and the two kernels"
    for name, a, r in zip(names, one, _ref64(t, in_act)):
        err = ((a.double().cpu() - r).abs().max() / (r.abs().max() + 1e-30)).item()
        print(f"{shape} in_act {in_act} {name}: {err:.2e} of max |reference|")
        assert err < 5e-5, f"{shape} in_act {in_act}: {name} against float64: {err:.2e}"


def test_relu_input_and_single_gradient_forms(monkeypatch):
    """ReLU as the producer's activation; and a call that asks for one gradient only takes the kernel it always took, under either setting."""
    from e2ehip import _lib as L
    shape = (2, 33, 17)
    t = _inputs(shape, 1, seed=9)
    two, one = _run(t, shape, 1, True, False, monkeypatch), _run(t, shape, 1, True, True, monkeypatch)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    B, H, W = shape
    x, dz, w = (t[k].to(DEV) for k in ("x", "dz", "w"))
    ws = torch.empty(L.load().e2e_head_workspace_floats(), device=DEV)
    for fused in ("0", "1"):
        monkeypatch.setenv("E2E_HEAD_BWD_FUSED", fused)
        dx, dw, db = torch.full_like(one[0], float("nan")), torch.full_like(one[1], float("nan")), torch.full_like(one[2], float("nan"))
        L.call("e2e_head_bwd_act", L.ptr(dz), L.ptr(x), L.ptr(w), L.ptr(dx), None, None, L.ptr(ws), B, H, W, HC, 1, L.stream())
        L.call("e2e_head_bwd_act", L.ptr(dz), L.ptr(x), L.ptr(w), None, L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, HC, 1, L.stream())
        torch.cuda.synchronize()
        assert torch.equal(dx, one[0]) and torch.equal(dw, one[1]) and torch.equal(db, one[2])
