"""k_wgrad3x3_thin_regs (dZ operand from global memory to registers, the next tile's loads under the MFMAs, the bias column only in
the workgroups that store it) against k_wgrad3x3_thin (dZ staged in LDS; E2E_THIN_WGRAD_REGS=0), through the product's entry point:
every accumulator receives the same MFMAs in the same order, so dW and dbias are the same bits.  Plus the float64 reference at the
bound tests/test_gpu_conv.py uses for backward-weight."""
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
# B, C(x), C(skip), up, H, W, Cout, bias -- and what wgrad_plan makes of it: tiles_x, nxg
CASES = {
    # total = 2 * 120 * 7 = 1680 tiles: two per workgroup, the fourth workgroup of a row walks ONE tile whose last 8 columns are cut off
    "16to16_up2_480x392": ((2, 16, 0, 2, 480, 392, 16, True), (2, 4)),
    # total = 2 * 61 * 3 * 6 = 2196: two tiles + one per row; the last two rows of the last row tile lie below the image; six groups
    # of 16 input channels (two behind the upsample, four of the skip), only the first stores the bias column
    "32+64to32_up2_242x136": ((2, 32, 64, 2, 242, 136, 32, True), (2, 2)),
    # one tile per workgroup, two channel groups, ragged in both axes
    "32to16_10x72": ((1, 32, 0, 1, 10, 72, 16, True), (1, 2)),
    # dbias not requested: no workgroup computes the bias column
    "32to16_10x72_nobias": ((1, 32, 0, 1, 10, 72, 16, False), (1, 2)),
}


def _plan(B, Cin, H, W):
    """wgrad_plan's arithmetic for the thin path (csrc/conv.hip): 4 x 64 tiles, workgroups of tiles_x consecutive ones, at most ~1400"""
    txt, ny = (W + 63) // 64, (H + 3) // 4
    total = B * ny * txt * (Cin // 16)
    tiles_x = 1
    while total // tiles_x > 1400 and tiles_x < txt:
        tiles_x += 1
    nxg = (txt + tiles_x - 1) // tiles_x
    return tiles_x, nxg, B * ny * nxg


@pytest.mark.parametrize("name", list(CASES))
def test_shapes_take_the_stated_partition(name):
    (B, Cx, Cs, up, H, W, Cout, bias), (tiles_x, nxg) = CASES[name]
    assert _plan(B, Cx + Cs, H, W)[:2] == (tiles_x, nxg)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_same_bits_as_the_lds_kernel_and_float64(name, monkeypatch):
    from e2ehip import conv, _lib as L
    (B, Cx, Cs, up, H, W, Cout, use_bias), _ = CASES[name]
    Cin = Cx + Cs
    g = torch.Generator().manual_seed(H * W + Cin)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    x = rnd(B, Cx, H // up, W // up).to(DEV).contiguous(memory_format=torch.channels_last)
    skip = rnd(B, Cs, H, W).to(DEV).contiguous(memory_format=torch.channels_last) if Cs else None
    w = (rnd(Cout, Cin, 3, 3) / (Cin * 9) ** 0.5).to(DEV).requires_grad_(True)
    bias = rnd(Cout).to(DEV).requires_grad_(True) if use_bias else None
    gy = rnd(B, Cout, H, W).to(DEV).contiguous(memory_format=torch.channels_last)
    # the workspace covers one slab [Cout][npad] per workgroup position of the thin path
    S = _plan(B, Cin, H, W)[2]
    npad = (9 * Cin + (1 if use_bias else 0) + 3) // 4 * 4
    ws = L.load().e2e_conv2d_wgrad_workspace_floats(B, H, W, Cin, Cout, 3, 3, 1 if use_bias else 0)
    assert ws >= S * Cout * npad
    leaves = [w] + ([bias] if use_bias else [])
    got = {}
    for regs in ("1", "0"):
        monkeypatch.setenv("E2E_THIN_WGRAD_REGS", regs)
        y = conv.conv2d(x, w, bias, 1, 1, "reflect", None, None, None, skip, up)
        got[regs] = torch.autograd.grad(y, leaves, gy)
    for a, b in zip(got["1"], got["0"]):
        assert torch.equal(a, b)
    xr = x.double()
    if up != 1:
        xr = F.interpolate(xr, scale_factor=up, mode="nearest")
    if skip is not None:
        xr = torch.cat([xr, skip.double()], 1)
    wr = w.detach().double().requires_grad_(True)
    yr = F.conv2d(F.pad(xr, (1, 1, 1, 1), mode="reflect"), wr)
    ref = [torch.autograd.grad(yr, [wr], gy.double())[0]] + ([gy.double().sum((0, 2, 3))] if use_bias else [])
    for a, r, what in zip(got["1"], ref, ("dW", "dbias")):
        e = ((a.double() - r).abs().max() / (r.abs().max() + 1e-30)).item()
        assert e < 5e-5, f"{what}: {e:.2e}"
