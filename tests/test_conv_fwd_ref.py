"""Host only: the float64 reference of the forward convolution contract (tests/conv_fwd_ref.py) against a second, independent formulation --
an explicit loop over output pixels and taps in numpy float64 that indexes the two sources itself (no torch.nn.functional, no padding
tensor, no interpolate) -- on tiny shapes; the weight layouts and the head against loops over their indices; and, for every case of
tests/test_gpu_conv_fwd_contracts.py, the input qualification: the same reference in float32 stays within a quarter of the bound the GPU
module asserts, so that bound is not spent on the comparison's own rounding."""
import numpy as np
import pytest
import torch

import conv_fwd_ref as R
import test_gpu_conv_fwd_contracts as G
from conv_fwd_ref import layer


def _reflect(i, n):
    return -i if i < 0 else (2 * (n - 1) - i if i >= n else i)


def _act(v, act):
    if act == R.ACT_RELU:
        return np.maximum(v, 0.0)
    if act == R.ACT_ELU:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    if act == R.ACT_DISP:
        return 10.0 / (1.0 + np.exp(-v)) + 0.01
    return v


def loop_conv(s, t, epi):
    """the header's sentence, literally: output pixel by output pixel, tap by tap"""
    sc, sh, rs, act = epi
    src0, w = t["src0"].double().numpy(), t["w"].double().numpy()
    src1 = t["src1"].double().numpy() if t["src1"] is not None else None
    sub, mul = R.norm_of(s)
    Ho, Wo = R.out_size(s)
    out = np.zeros((s.B, Ho, Wo, s.Cout))
    for b in range(s.B):
        for yo in range(Ho):
            for xo in range(Wo):
                acc = np.zeros(s.Cout)
                for kh in range(s.KH):
                    for kw in range(s.KW):
                        ys, xs = yo * s.stride + kh - s.pad, xo * s.stride + kw - s.pad
                        if s.pad_mode == 1:
                            ys, xs = _reflect(ys, s.Hs), _reflect(xs, s.Ws)
                        elif not (0 <= ys < s.Hs and 0 <= xs < s.Ws):
                            continue                                       # a zero of the (normalised) padded image
                        v = src0[b, ys // s.up, xs // s.up, :]
                        v = (v - sub) * mul
                        if src1 is not None:
                            v = np.concatenate([v, src1[b, ys, xs, :]])
                        acc += w[:, :, kh, kw] @ v
                if sc:
                    acc = acc * t["scale"].double().numpy()
                if sh:
                    acc = acc + t["shift"].double().numpy()
                if rs:
                    acc = acc + t["res"].double().numpy()[b, yo, xo]
                out[b, yo, xo] = _act(acc, act)
    return out


TINY = {
    "up2_cat_reflect": layer(2, 5, 4, 6, 3, pad_mode=1, C1=2, up=2),              # upsample + concat indexing, reflection at all four borders
    "up2_reflect": layer(1, 3, 2, 4, 2, pad_mode=1, up=2),                         # the smallest reflected image: 2 rows
    "cat_up1_zero": layer(1, 4, 3, 5, 3, C1=1),
    "s2_odd_zero": layer(2, 3, 7, 5, 4, stride=2),                                 # stride 2, odd sizes: the last output's window ends on the border
    "s2_odd_reflect": layer(1, 2, 5, 7, 3, stride=2, pad_mode=1),                  # ... and reflects there
    "s2_even_reflect": layer(1, 2, 4, 6, 3, stride=2, pad_mode=1),
    "pad0": layer(1, 3, 4, 5, 2, pad=0),
    "1x3_pad0": layer(1, 2, 3, 6, 3, k=1, kw=3, pad=0),
    "3x1_pad0": layer(1, 2, 6, 3, 3, k=3, kw=1, pad=0),
    "1x3_pad1": layer(1, 2, 3, 5, 3, k=1, kw=3, pad=1),                            # two output rows that read padding only
    "3x1_reflect": layer(1, 2, 4, 3, 3, k=3, kw=1, pad=1, pad_mode=1),
    "1x1_s2": layer(2, 3, 5, 4, 4, k=1, stride=2, pad=0),
    "7x7_s2_norm": layer(1, 3, 9, 11, 4, k=7, stride=2, pad=3, norm=True),         # the stem's form: zero padding of the NORMALISED image
    "3x3_norm": layer(1, 3, 4, 4, 2, norm=True),
}


@pytest.mark.parametrize("name", list(TINY))
def test_reference_against_explicit_loops(name):
    s = TINY[name]
    t = R.make_inputs(s)
    z = R.layer_raw(s, t)
    assert tuple(z.shape) == (s.B, *R.out_size(s), s.Cout) and z.dtype == torch.float64
    for epi in G.MATRIX:
        a = R.layer_out(t, z, epi).numpy()
        b = loop_conv(s, t, epi)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (name, epi)
    sub, mul = R.norm_of(s)
    direct = R.conv_fwd(t["src0"], t["src1"], s.up, t["w"], t["scale"], t["shift"], t["res"], s.stride, s.pad, s.pad_mode, R.ACT_ELU, sub, mul)
    assert torch.equal(direct, R.layer_out(t, z, (1, 1, 1, R.ACT_ELU)))


def test_inputs_draw_scales_of_both_signs_and_exercise_every_activation_branch():
    for s in TINY.values():
        t = R.make_inputs(s)
        assert (t["scale"] > 0).any() and (t["scale"] < 0).any() and (t["scale"].abs() >= 0.5).all()
        z = R.layer_raw(s, t)
        assert (z > 0).any() and (z < 0).any()                 # both sides of the ReLU / ELU kink


def test_float32_mode_is_float32():
    s = TINY["up2_cat_reflect"]
    t = R.make_inputs(s)
    z32 = R.layer_raw(s, t, torch.float32)
    assert z32.dtype == torch.float32 and R.layer_out(t, z32, (1, 1, 1, 2)).dtype == torch.float32
    assert 0 < R.rel(z32, R.layer_raw(s, t)) < 1e-5


LAYOUTS = [(1, 16, 3, 3), (5, 3, 2, 3), (4, 6, 1, 3), (3, 2, 7, 7), (33, 31, 1, 1)]


@pytest.mark.parametrize("shape", LAYOUTS, ids=["x".join(map(str, s)) for s in LAYOUTS])
def test_weight_layouts_against_index_loops(shape):
    Cout, Cin, KH, KW = shape
    w = torch.randn(*shape, generator=torch.Generator().manual_seed(Cout))
    f = torch.rand(Cout, generator=torch.Generator().manual_seed(Cin)) - 0.5
    for extra in (0, 8):
        ldf, ldb = R.ceil4(Cout) + extra, R.ceil4(Cin) + extra
        ef, eb, ebf = (np.full((KH * KW * Cin, ldf), -3.0, np.float32), np.full((KH * KW * Cout, ldb), -3.0, np.float32),
                       np.full((KH * KW * Cout, ldb), -3.0, np.float32))
        for co in range(Cout):
            for ci in range(Cin):
                for kh in range(KH):
                    for kw in range(KW):
                        ef[(kh * KW + kw) * Cin + ci, co] = w[co, ci, kh, kw]
                        eb[(kh * KW + kw) * Cout + co, ci] = w[co, ci, kh, kw]
                        ebf[(kh * KW + kw) * Cout + co, ci] = np.float32(w[co, ci, kh, kw].item()) * np.float32(f[co].item())
        assert np.array_equal(R.w_fwd(w, ldf, -3.0).numpy(), ef)
        assert np.array_equal(R.w_bwd(w, ldb, None, -3.0).numpy(), eb)
        assert np.array_equal(R.w_bwd(w, ldb, f, -3.0).numpy(), ebf)
        # through float64 and rounded once: the same bits as the float32 product (the product of two float32 values is exact in float64)
        assert np.array_equal(R.w_bwd(w.double(), ldb, f.double(), -3.0).float().numpy(), ebf)
    assert (R.w_fwd(w, R.ceil4(Cout) + 4)[:, Cout:] == 0).all()


@pytest.mark.parametrize("size", [(2, 2), (3, 5)])
def test_head_against_explicit_loops(size):
    H, W = size
    t = R.head_inputs(2, H, W)
    x, w = t["x"].double().numpy(), t["w"].double().numpy()
    for act in (R.ACT_NONE, R.ACT_DISP):
        for bias in (None, t["bias"]):
            e = np.zeros((2, H, W))
            for b in range(2):
                for y in range(H):
                    for xx in range(W):
                        acc = 0.0 if bias is None else float(bias[0])
                        for kh in range(3):
                            for kw in range(3):
                                acc += w[0, :, kh, kw] @ x[b, _reflect(y + kh - 1, H), _reflect(xx + kw - 1, W), :]
                        e[b, y, xx] = _act(acc, act)
            a = R.head_fwd(t["x"], t["w"], bias, act).numpy()
            assert a.shape == e.shape and np.abs(a - e).max() <= 1e-12 * np.abs(e).max()


# ---- input qualification of the GPU module's cases -------------------------------------------------------------------------------------
CASES = list(G.all_cases())


def test_case_tables_are_what_the_module_says():
    assert len({(sec, name) for sec, name, _, _ in CASES}) == len(CASES)
    for sec, name, s, epis in CASES:
        Ho, Wo = R.out_size(s)
        assert Ho > 0 and Wo > 0 and s.Hs % s.up == 0 and s.Ws % s.up == 0 and epis, (sec, name)
        assert s.B * Ho * Wo <= 4000 or name == "16to24_600_tiles", (sec, name)           # small: the one large case is 1x1 on 16 channels
        scalar = s.Cin % 16 != 0
        assert (scalar or not s.norm) and (not scalar or (s.C1 == s.Cin and s.up == 1)), (sec, name)
        assert all(len(e) == 4 and e[3] in (0, 1, 2, 3) for e in epis)
    assert {s.Cout for _, _, s, _ in CASES} >= {6, 20, 50, 66, 130, 16, 32, 64, 96, 128, 256}
    assert len(G.MATRIX) == 32 == len(set(G.MATRIX))
    assert len(G.TILES) == 10 == len(set(G.TILES))


@pytest.mark.parametrize("sec,name,s,epis", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_inputs_qualify(sec, name, s, epis):
    """max |r32 - r64| / max |r64| <= bound / 4 for every output the GPU module compares (whole output, no element exempt)"""
    t = R.make_inputs(s)
    z64, z32 = R.layer_raw(s, t), R.layer_raw(s, t, torch.float32)
    for epi in epis:
        r64, r32 = R.layer_out(t, z64, epi), R.layer_out(t, z32, epi)
        assert r32.dtype == torch.float32 and torch.isfinite(r64).all() and r64.abs().max() > 0.1
        e = R.rel(r32, r64)
        assert e <= R.QUALIFY, f"{sec} {name} {epi}: float32 reference {e:.2e} from float64"


@pytest.mark.parametrize("size", G.HEAD_SIZES, ids=[f"{h}x{w}" for h, w in G.HEAD_SIZES])
def test_head_inputs_qualify(size):
    for B in (1, 3):
        t = R.head_inputs(B, *size)
        for act in (R.ACT_NONE, R.ACT_DISP):
            for bias in (None, t["bias"]):
                e = R.rel(R.head_fwd(t["x"], t["w"], bias, act, torch.float32), R.head_fwd(t["x"], t["w"], bias, act))
                assert e <= R.QUALIFY, f"head {B} {size} act {act}: {e:.2e}"
