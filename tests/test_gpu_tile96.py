"""The 96-column workgroup tiles (32 x 96 and 64 x 96: one column tile of three 32-column wave blocks) of the convolution GEMM.
A tile's shape decides which wave computes an element, not the K order of its sum: with the same slice count every output is the
bits the 64 x 64 tiling gives."""
import pytest
import torch

from test_gpu_conv import _mask_kinks, _ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILES = [(32, 96), (64, 96)]
# Cin, Cout, H, W, stride: 96 columns in both directions; Cout = 80 masks columns 80 .. 95 of the forward; rows (2 x 22 x 36, 2 x 21 x 27,
# the stride-2 parity classes of 21 x 27) are no multiple of 32 or 64
LAYERS = ((96, 96, 22, 36, 1), (96, 80, 21, 27, 1), (96, 80, 21, 27, 2))


def _layer(Cin, Cout, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    x = rnd(2, Cin, H, W).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (rnd(Cout, Cin, 3, 3) / (Cin * 9) ** 0.5).to(DEV).requires_grad_(True)
    return x, w, (rnd(Cout).abs() + 0.5).to(DEV), rnd(Cout).to(DEV), rnd


@pytest.fixture(scope="module")
def tiled64():
    """y, dx and the upstream gradient of every layer under tuning (64, 64, 1): computed once, never modified"""
    from e2ehip import conv
    out = []
    for i, (Cin, Cout, H, W, s) in enumerate(LAYERS):
        x, w, scale, shift, rnd = _layer(Cin, Cout, H, W, 960 + i)
        y = conv.conv2d(x, w, None, s, 1, "zeros", "relu", (scale, shift), tuning=(64, 64, 1))
        gy = rnd(*y.shape).to(DEV)
        gx, = torch.autograd.grad(y, [x], gy)
        out.append((y.detach(), gx, gy))
    return out


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_bit_identical_to_64x64(tile, tiled64):
    from e2ehip import conv
    for i, (Cin, Cout, H, W, s) in enumerate(LAYERS):
        x, w, scale, shift, _ = _layer(Cin, Cout, H, W, 960 + i)
        y0, gx0, gy = tiled64[i]
        y = conv.conv2d(x, w, None, s, 1, "zeros", "relu", (scale, shift), tuning=(tile[0], tile[1], 1))
        gx, = torch.autograd.grad(y, [x], gy)
        assert torch.equal(y, y0), f"y {Cin}->{Cout} stride {s}"
        assert torch.equal(gx, gx0), f"dx {Cin}->{Cout} stride {s}"


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_split_in_three_against_float64(tile):
    """ksplit = 3 (the stride-2 class form slices by tap instead) at the bound of test_every_gemm_decomposition"""
    from e2ehip import conv
    for i, (Cin, Cout, H, W, s) in enumerate(LAYERS):
        x, w, scale, shift, rnd = _layer(Cin, Cout, H, W, 970 + i)
        y = conv.conv2d(x, w, None, s, 1, "zeros", "relu", (scale, shift), tuning=(tile[0], tile[1], 3))
        yr = _ref(x, None, w, None, scale, shift, None, 1, s, 1, "zeros", "relu", None)
        gy = _mask_kinks(rnd(*y.shape).to(DEV), yr, "relu")
        gx, gw = torch.autograd.grad(y, [x, w], gy)
        gxr, gwr = torch.autograd.grad(yr, [x, w], gy.double())
        for a, b, name in ((y, yr, "y"), (gx, gxr, "dx"), (gw, gwr, "dw")):
            e = ((a.double() - b).abs().max() / (b.abs().max() + 1e-30)).item()
            assert e < 5e-5, f"{name} {Cin}->{Cout} stride {s}: {e:.2e}"


def test_library_choice_on_a_miniature_of_upconv11():
    """32 upsampled + 64 skip channels -> 32, reflection, ELU, 16 x 24, batch 2: the library's own choice for the 96-column backward-data
    GEMM (a 96-wide tile, asserted through the host-side query) gives the input gradients of tuning (64, 64, 1) bit for bit"""
    from e2ehip import conv, _lib as L
    import ctypes
    out3 = (ctypes.c_int * 3)()
    L.call("e2e_conv_gemm_choice", 2 * 18 * 26, 96, 9 * 32, 32, 1, out3)
    assert out3[1] == 96 and out3[2] == 1, list(out3)
    g = torch.Generator().manual_seed(1196)
    rnd = lambda *shape: torch.randn(*shape, generator=g)
    x = rnd(2, 32, 8, 12).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    skip = rnd(2, 64, 16, 24).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (rnd(32, 96, 3, 3) / (96 * 9) ** 0.5).to(DEV)
    bias = rnd(32).to(DEV)
    gy = rnd(2, 32, 16, 24).to(DEV)
    res = []
    for tuning in (None, (64, 64, 1)):
        y = conv.conv2d(x, w, bias, 1, 1, "reflect", "elu", None, None, skip, 2, tuning=tuning)
        res.append(torch.autograd.grad(y, [x, skip], gy))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
