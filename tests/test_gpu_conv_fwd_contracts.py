"""The forward entry points of csrc/conv.hip, called straight through the C ABI, against the float64 reference of the contract
include/e2eslam.h states (tests/conv_fwd_ref.py) -- not through e2ehip.conv.conv2d, and not only at the network's own layer shapes:

  A. e2e_conv_weight_layouts / _batched: bit-equal to the permutes, padding columns untouched, skipped addresses, the slot-9 factor, a
     table longer than one launch takes;
  B. e2e_conv2d_fwd, one table per launch path of conv_fwd_impl / plan_gemm: the scalar-gather GEMM, the stem and thin patch kernels,
     every tile family the cost model picks with the direct epilogue, both split-K tails, the source layouts, and the whole
     scale x shift x residual x activation matrix on each of them;
  C. e2e_conv2d_fwd_tuned: all ten tile shapes x K slices, stream-K, tile_m == 0, and the triple e2e_conv_gemm_choice reports;
  D. the host-side queries;  E. e2e_head_fwd;  F. the argument combinations the header rules out: E2EError, nothing written.

Every output is NaN-filled and followed by a NaN sentinel; every workspace is allocated at exactly the size its query returns, flag head
zeroed, sentinel behind.  After each call: everything meant to be written was written, nothing past any end was, the stream-K flags and
the error word are zero.  Every forward call is made twice and must give the same bits (the forward has no atomics).
Error measure and bound: max |gpu - r64| / max |r64| < 2e-5 over the whole output (no element exempt); tests/test_conv_fwd_ref.py checks
on the host that the float32 reference of every case here stays within a quarter of that.  Every comparison prints its figure."""
import ctypes
import functools

import pytest
import torch

import conv_fwd_ref as R
from conv_fwd_ref import layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
FILL = 12345.0                    # what the caller put into a weight layout's buffer

# epi = (scale given, shift given, residual given, act)
PLAIN, BN, BN_RES, BIAS_ELU, BIAS_DISP, SCALE_ONLY = (0, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 1), (0, 1, 0, 2), (0, 1, 0, 3), (1, 0, 0, 0)
MATRIX = [(sc, sh, rs, act) for sc in (0, 1) for sh in (0, 1) for rs in (0, 1) for act in (0, 1, 2, 3)]

# name -> (layer, the path the default entry takes with its workspace given, epilogues).  Paths: "scalar" (GK_SCALAR), "stem"
# (k_conv7x7_stem), "thin" (k_conv3x3_thin), "tile:BMxBN" (k_conv_gemm, direct epilogue), "splitk4:BMxBN" / "splitk:BMxBN" (slabs +
# k_conv_splitk_epilogue4 / k_conv_splitk_epilogue); _path() derives them from the library's own choice and every test asserts them.
SCALAR = {
    "3to32_norm": (layer(2, 3, 9, 13, 32, norm=True), "scalar", [PLAIN, BN, BIAS_ELU]),               # 234 rows, 32 columns
    "6to48_1x1": (layer(1, 6, 11, 13, 48, k=1, pad=0), "scalar", [PLAIN, BN_RES]),
    "20to64_s2_odd": (layer(3, 20, 13, 17, 64, stride=2), "scalar", [BN, BIAS_DISP]),                  # 3 x 7 x 9 = 189 rows
    "stem_with_residual": (layer(1, 3, 19, 27, 64, k=7, stride=2, pad=3, norm=True), "scalar", [BN_RES, (0, 0, 1, 0)]),
    "stem_to32": (layer(1, 3, 19, 27, 32, k=7, stride=2, pad=3, norm=True), "scalar", [PLAIN, BN]),
    "7to70_reflect_s2": (layer(3, 7, 12, 15, 70, stride=2, pad_mode=1), "scalar", [PLAIN, BN_RES, BIAS_ELU]),   # 144 rows, two column tiles
    "5to6_reflect": (layer(2, 5, 10, 9, 6, pad_mode=1), "scalar", [SCALE_ONLY, BIAS_ELU]),
}
STEM_SHAPES = [(1, 33, 47), (3, 33, 47), (1, 64, 96)]
STEM = {f"stem_b{b}_{h}x{w}": (layer(b, 3, h, w, 64, k=7, stride=2, pad=3, norm=True), "stem", [PLAIN, BN, (1, 0, 0, 1), (0, 1, 0, 0)])
        for b, h, w in STEM_SHAPES}
THIN = {
    "thin16_up2": (layer(2, 16, 10, 70, 16, pad_mode=1, up=2), "thin", [PLAIN, BIAS_ELU, (0, 0, 0, 2), (0, 1, 0, 0)]),   # 64 x 8 patches overhang
    "thin32": (layer(2, 32, 6, 66, 16, pad_mode=1), "thin", [PLAIN, BIAS_ELU, (0, 0, 0, 2), (0, 1, 0, 0)]),              # 64 x 4 patches overhang
    # their nearest neighbours, which the condition sends to the GEMM
    "thin16_up2_scale": (layer(2, 16, 10, 70, 16, pad_mode=1, up=2), "tile:64x32", [SCALE_ONLY, BN]),
    "thin32_residual": (layer(2, 32, 6, 66, 16, pad_mode=1), "tile:64x32", [(0, 1, 1, 2), (0, 0, 1, 0)]),
    "48to16": (layer(1, 48, 6, 66, 16, pad_mode=1), "tile:64x32", [PLAIN, BIAS_ELU]),
}
# one layer per column band of choose_cfg, rows (2 x 9 x 11 = 198) ragged against every tile height, and ragged columns next to them
_BAND = {6: "64x32", 16: "64x32", 20: "64x32", 32: "64x32", 50: "64x64", 64: "64x64", 66: "32x96", 96: "32x96", 100: "64x64", 128: "32x128",
         130: "32x128"}
TILE = {f"32to{c}": (layer(2, 32, 9, 11, c), "tile:" + t, [PLAIN, BN_RES, BIAS_ELU]) for c, t in _BAND.items()}
# the other side of the 600-tile rule of the <= 32-column band: ceil(277 * 277 / 128) = 600 row tiles of 128
TILE["16to24_600_tiles"] = (layer(1, 16, 277, 277, 24, k=1, pad=0), "tile:128x32", [BN_RES])
SPLITK = {
    "512to256": (layer(2, 512, 2, 3, 256, pad_mode=1), "splitk4:32x128", [PLAIN, BIAS_ELU, BN_RES]),     # upconv(4,0) at the smallest size
    "512to256_two_row_tiles": (layer(3, 512, 3, 5, 256), "splitk4:32x128", [BN_RES]),                    # 45 rows
    "256to66": (layer(2, 256, 2, 3, 66), "splitk:32x96", [PLAIN, BIAS_ELU, BN_RES]),                     # Cout % 4 != 0: the scalar tail
    "128to64": (layer(1, 128, 5, 7, 64), "splitk4:64x64", [BN]),
    "128to50": (layer(1, 128, 5, 7, 50), "splitk:64x64", [BN]),
}
SOURCES = {
    "up2": (layer(2, 32, 8, 12, 32, pad_mode=1, up=2), "tile:64x32", [PLAIN, BIAS_ELU]),
    "up2_cat_32_96": (layer(1, 96, 8, 12, 32, pad_mode=1, C1=32, up=2), "tile:64x32", [PLAIN, BIAS_ELU]),
    "cat_up1": (layer(2, 64, 7, 9, 48, C1=32), "splitk4:64x64", [PLAIN, BN_RES]),                            # 2 tiles, 18 chunks: two K slices
    "cat_16_48_up2": (layer(1, 48, 6, 10, 32, pad_mode=1, C1=16, up=2), "tile:64x32", [PLAIN, BIAS_ELU]),      # chunk depth 16
    "cat_16_48_up1": (layer(2, 48, 5, 7, 20, C1=16), "tile:64x32", [PLAIN, BN_RES]),
    "cat_32_48": (layer(1, 48, 5, 7, 32, C1=32), "tile:64x32", [PLAIN, BN]),
    "s2_reflect_odd": (layer(2, 32, 9, 11, 48, stride=2, pad_mode=1), "tile:64x64", [PLAIN, BIAS_ELU]),        # the last tap reflects
    "s2_reflect_even": (layer(1, 32, 8, 10, 48, stride=2, pad_mode=1), "tile:64x64", [PLAIN]),
    "pad0": (layer(2, 32, 7, 9, 32, pad=0), "tile:64x32", [PLAIN, BN_RES]),
    "1x3": (layer(2, 32, 6, 9, 32, k=1, kw=3, pad=0), "tile:64x32", [PLAIN, BN]),
    "3x1": (layer(2, 32, 6, 9, 32, k=3, kw=1, pad=0), "tile:64x32", [PLAIN, BN]),
    "1x3_pad1": (layer(1, 32, 6, 9, 32, k=1, kw=3, pad=1), "tile:64x32", [PLAIN]),
    "3x1_reflect": (layer(1, 32, 6, 9, 48, k=3, kw=1, pad=1, pad_mode=1), "tile:64x64", [PLAIN, BIAS_ELU]),
}
# the epilogue matrix: one small layer per epilogue implementation; `paths`: what its 32 operand choices may reach
EPILOGUE = {
    "direct": (layer(2, 32, 9, 11, 50), {"tile:64x64"}),
    "splitk4": (layer(1, 128, 5, 7, 64), {"splitk4:64x64"}),
    "splitk": (layer(1, 128, 5, 7, 50), {"splitk:64x64"}),
    "scalar": (layer(2, 3, 9, 13, 32, norm=True), {"scalar"}),
    "thin16": (layer(1, 16, 10, 70, 16, pad_mode=1, up=2), {"thin", "tile:64x32"}),           # thin without scale and residual
    "thin32": (layer(1, 32, 6, 66, 16, pad_mode=1), {"thin", "tile:64x32"}),
    "stem": (layer(1, 3, 33, 47, 64, k=7, stride=2, pad=3, norm=True), {"stem", "scalar"}),   # stem without residual
}
# e2e_conv2d_fwd_tuned, full epilogue: chunk depth 32 (128 x 128 gives way to 128 x 64) and 16 (Cin = 48: 128 x 128 stays, two blocks per
# wave in each direction); 100 and 66 columns leave every tile width ragged, 66 takes the scalar tail when split
TUNED = {"64to100": layer(2, 64, 9, 11, 100), "48to66": layer(2, 48, 9, 11, 66)}
TUNED_EPIS = [BN_RES, BIAS_DISP, PLAIN]            # stream-K runs all three, the tile shapes the first
TILES = [(64, 64), (128, 64), (128, 128), (128, 32), (32, 128), (32, 64), (64, 32), (32, 32), (32, 96), (64, 96)]     # the header's ten

FWD_TABLES = {"scalar": SCALAR, "stem": STEM, "thin": THIN, "tile": TILE, "splitk": SPLITK, "sources": SOURCES}
HEAD_SIZES = [(2, 2), (5, 7), (3, 130), (20, 28)]


def all_cases():
    """every (section, name, layer, epilogues) whose output this module compares with the reference: what the host-side input
    qualification of tests/test_conv_fwd_ref.py walks"""
    for sec, table in FWD_TABLES.items():
        for name, (s, _, epis) in table.items():
            yield sec, name, s, epis
    for name, (s, _) in EPILOGUE.items():
        yield "epilogue", name, s, MATRIX
    for name, s in TUNED.items():
        yield "tuned", name, s, TUNED_EPIS


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _out(n):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV)


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _workspace(n):
    """exactly n floats of NaN + sentinel, the stream-K flag head zeroed (its owner's duty); None for n == 0"""
    if n == 0:
        return None
    buf = torch.full((n + SENTINEL,), float("nan"), device=DEV)
    buf[:min(n, _L().load().e2e_conv_workspace_flag_floats())] = 0
    return buf


def _workspace_ok(ws, n):
    if ws is None:
        return
    assert torch.isnan(ws[n:]).all(), "workspace: written past the size its query returned"
    f = min(n, _L().load().e2e_conv_workspace_flag_floats())
    assert (ws[:f].view(torch.int32) == 0).all(), "workspace: stream-K flags left raised, or the error word set"


def _geom(s):
    Ho, Wo = R.out_size(s)
    return Ho, Wo, s.B * Ho * Wo, s.KH * s.KW * s.Cin


def _depth(s):
    return 32 if s.Cin % 32 == 0 and (s.C1 == s.Cin or s.C1 % 32 == 0) else 16


def _choice(rows, cols, K, depth, allow_split):
    out3 = (ctypes.c_int * 3)()
    _L().call("e2e_conv_gemm_choice", rows, cols, K, depth, int(allow_split), out3)
    return tuple(out3)


def _path(s, epi, has_ws):
    """what conv_fwd_impl launches for this call (mirrors its conditions; the GEMM's decomposition is the library's own report)"""
    sc, sh, rs, act = epi
    Ho, Wo, rows, K = _geom(s)
    one = s.C1 == s.Cin
    if (s.KH, s.KW, s.stride, s.pad, s.pad_mode, s.Cin, s.Cout) == (7, 7, 2, 3, 0, 3, 64) and one and s.up == 1 and not rs:
        return "stem"
    if (s.KH, s.KW, s.stride, s.pad, s.pad_mode, s.Cout) == (3, 3, 1, 1, 1, 16) and one and not sc and not rs and (s.Cin, s.up) in ((16, 2), (32, 1)):
        return "thin"
    if s.Cin % 16 or (not one and s.C1 % 16):
        return "scalar"
    bm, bn, S = _choice(rows, s.Cout, K, _depth(s), has_ws)
    if S > 1:
        nchunks = -(-K // _depth(s))
        cps = -(-nchunks // S)
        if -(-nchunks // cps) > 1:
            return f"{'splitk4' if s.Cout % 4 == 0 else 'splitk'}:{bm}x{bn}"
    return f"tile:{bm}x{bn}"


@functools.lru_cache(maxsize=None)
def _case(s):
    """a layer's operands on the device and conv(x) in float64, computed once and shared by every epilogue and decomposition"""
    t = R.make_inputs(s)
    t["spec"] = s
    t["z"] = R.layer_raw(s, t)
    t["dev"] = {k: (v.to(DEV) if v is not None else None) for k, v in t.items() if k in ("src0", "src1", "scale", "shift", "res")}
    t["wf"] = {}
    return t


def _wf(t, ld_extra):
    """w_fwd by the reference's permute (section A holds the library's own layouts to the same permute), padding columns zeroed"""
    if ld_extra not in t["wf"]:
        ld = R.ceil4(t["spec"].Cout) + ld_extra
        t["wf"][ld_extra] = (ld, R.w_fwd(t["w"], ld).to(DEV))
    return t["wf"][ld_extra]


def _run(t, epi, ws, nws, ld_extra=0, tuned=None):
    """one forward call into a fresh NaN-filled output; `ws`: a workspace of exactly nws floats from _workspace(), or None"""
    L = _L()
    s, d = t["spec"], t["dev"]
    sc, sh, rs, act = epi
    Ho, Wo, rows, K = _geom(s)
    n = rows * s.Cout
    out = _out(n)
    ld, wf = _wf(t, ld_extra)
    sub, mul = R.norm_of(s)
    args = [L.ptr(d["src0"]), L.ptr(d["src1"]), s.C1, s.up, L.ptr(wf), ld, L.ptr(d["scale"] if sc else None), L.ptr(d["shift"] if sh else None),
            L.ptr(d["res"] if rs else None), L.ptr(out), s.B, s.Hs, s.Ws, s.Cin, s.Cout, s.KH, s.KW, s.stride, s.pad, s.pad_mode, act,
            ctypes.c_float(sub), ctypes.c_float(mul), L.ptr(ws)]
    if tuned is None:
        L.call("e2e_conv2d_fwd", *args, L.stream())
    else:
        L.call("e2e_conv2d_fwd_tuned", *args, *tuned, L.stream())
    torch.cuda.synchronize()
    _written(out, n, f"out ({epi}, {tuned})")
    _workspace_ok(ws, nws)
    return out[:n].reshape(s.B, Ho, Wo, s.Cout)


def _default_ws(s):
    Ho, Wo, rows, K = _geom(s)
    return _L().load().e2e_conv2d_splitk_workspace_floats(rows, s.Cout, K)


def _tuned_ws(s):
    Ho, Wo, rows, K = _geom(s)
    return _L().load().e2e_conv_tuned_workspace_floats(rows, s.Cout)


def _compare(section, label, a, ref):
    e = R.rel(a.cpu(), ref)
    print(f"ratio {section} {label}: {e / R.BOUND:.3f} ({e:.2e})")
    assert e < R.BOUND, f"{section} {label}: {e:.2e}"


def _check_default(section, name, s, epi, paths, ld_extra=0):
    """e2e_conv2d_fwd with a workspace of exactly the queried size and with workspace == NULL: each twice (same bits), each against
    float64; `paths`: the launch paths the call with its workspace may take"""
    t = _case(s)
    ref = R.layer_out(t, t["z"], epi)
    nws = _default_ws(s)
    assert _path(s, epi, nws > 0) in paths, (name, epi, _path(s, epi, nws > 0))
    for n in {nws, 0}:
        a = _run(t, epi, _workspace(n), n, ld_extra)
        b = _run(t, epi, _workspace(n), n, ld_extra)
        assert torch.equal(a, b), f"{name} {epi}: two calls differ"
        _compare(section, f"{name} {epi} ld+{ld_extra} {'ws' if n else 'nows'}", a, ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. weight layouts
# ---------------------------------------------------------------------------------------------------------------------------------------
# Cout, Cin, KH, KW: the 32-element tile edges of the batched kernel in both directions, its 3x3 / 1x1 tile form and its element-wise form
WL_SHAPES = [(1, 16, 3, 3), (64, 3, 7, 7), (48, 6, 3, 3), (33, 31, 1, 1), (16, 32, 1, 3), (128, 64, 3, 3)]


def _weight(shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape) + seed))


def _filled(n):
    """n floats of FILL + a FILL sentinel: a layout's buffer as the caller left it"""
    return torch.full((n + SENTINEL,), FILL, device=DEV)


def _same(buf, expect, what):
    n = expect.numel()
    assert (buf[n:] == FILL).all(), f"{what}: written past the end"
    assert torch.equal(buf[:n].cpu().view(expect.shape), expect), f"{what}: differs from the permute (or a padding column was written)"


def _layouts(w_d, shape, ldf, ldb, fwd, bwd):
    L = _L()
    Cout, Cin, KH, KW = shape
    wf = _filled(KH * KW * Cin * ldf)
    wb = _filled(KH * KW * Cout * ldb)
    L.call("e2e_conv_weight_layouts", L.ptr(w_d), Cout, Cin, KH, KW, L.ptr(wf if fwd else None), ldf, L.ptr(wb if bwd else None), ldb, L.stream())
    torch.cuda.synchronize()
    return wf, wb


@pytest.mark.parametrize("extra", [0, 4, 12])
@pytest.mark.parametrize("shape", WL_SHAPES, ids=["x".join(map(str, s)) for s in WL_SHAPES])
def test_weight_layouts(shape, extra):
    Cout, Cin, KH, KW = shape
    w = _weight(shape)
    w_d = w.to(DEV)
    ldf, ldb = R.ceil4(Cout) + extra, R.ceil4(Cin) + extra
    untouched_f, untouched_b = torch.full((KH * KW * Cin, ldf), FILL), torch.full((KH * KW * Cout, ldb), FILL)
    for fwd, bwd in ((1, 0), (0, 1), (1, 1)):
        wf, wb = _layouts(w_d, shape, ldf, ldb, fwd, bwd)
        _same(wf, R.w_fwd(w, ldf, FILL) if fwd else untouched_f, f"w_fwd (fwd={fwd}, bwd={bwd})")
        _same(wb, R.w_bwd(w, ldb, None, FILL) if bwd else untouched_b, f"w_bwd (fwd={fwd}, bwd={bwd})")


def _batched(rows):
    """rows: (shape, ldf, ldb, fwd, bwd, factor given, w tensor on the device or None) -> per row (w, factor, wf, wb) after ONE
    e2e_conv_weight_layouts_batched call over the table"""
    L = _L()
    held, table = [], []
    for i, (shape, ldf, ldb, fwd, bwd, fac, w_d) in enumerate(rows):
        Cout, Cin, KH, KW = shape
        w = _weight(shape, i) if w_d is None else w_d.cpu().view(shape)
        w_d = w.to(DEV) if w_d is None else w_d
        f = (torch.rand(Cout, generator=torch.Generator().manual_seed(i)) + 0.5) * (-1) ** i if fac else None
        f_d = f.to(DEV) if fac else None
        wf, wb = _filled(KH * KW * Cin * ldf), _filled(KH * KW * Cout * ldb)
        held.append((w, f, wf, wb, w_d, f_d))
        table.append([w_d.data_ptr(), wf.data_ptr() if fwd else 0, wb.data_ptr() if bwd else 0, Cout, Cin, KH, KW, ldf, ldb, f_d.data_ptr() if fac else 0])
    desc = torch.tensor(table, dtype=torch.int64).to(DEV)
    L.call("e2e_conv_weight_layouts_batched", L.ptr(desc), len(rows), L.stream())
    torch.cuda.synchronize()
    return held


def _batched_check(rows, held, against_single):
    for i, ((shape, ldf, ldb, fwd, bwd, fac, _), (w, f, wf, wb, w_d, f_d)) in enumerate(zip(rows, held)):
        Cout, Cin, KH, KW = shape
        # the float64 product of two float32 values is exact: .float() rounds it once, as a float32 multiply does
        eb = R.w_bwd(w.double(), ldb, f.double() if fac else None, FILL).float() if bwd else torch.full((KH * KW * Cout, ldb), FILL)
        ef = R.w_fwd(w, ldf, FILL) if fwd else torch.full((KH * KW * Cin, ldf), FILL)
        _same(wf, ef, f"row {i} {shape}: w_fwd")
        _same(wb, eb, f"row {i} {shape}: w_bwd")
        if against_single and not fac:
            sf, sb = _layouts(w_d, shape, ldf, ldb, fwd or not bwd, bwd)
            if fwd:
                assert torch.equal(sf, wf), f"row {i} {shape}: w_fwd differs from the per-layer call"
            if bwd:
                assert torch.equal(sb, wb), f"row {i} {shape}: w_bwd differs from the per-layer call"


def test_weight_layouts_batched_mixed_table():
    rows = []
    for i, shape in enumerate(WL_SHAPES * 3):
        Cout, Cin, KH, KW = shape
        rnd = i // len(WL_SHAPES)
        extra = (0, 4, 8)[(i + rnd) % 3]
        fwd, bwd = ((1, 1), (1, 0), (0, 1))[(i + 2 * rnd) % 3]
        rows.append((shape, R.ceil4(Cout) + extra, R.ceil4(Cin) + extra, fwd, bwd, bool(bwd and (rnd == 1 or i % 2 == 1)), None))
    assert any(r[5] for r in rows) and any(not r[3] for r in rows) and any(not r[4] for r in rows)
    assert {r[0] for r in rows if r[5]} >= {(64, 3, 7, 7), (128, 64, 3, 3), (33, 31, 1, 1)}        # the factor in every form of the kernel
    _batched_check(rows, _batched(rows), True)


def test_weight_layouts_batched_longer_than_one_launch():
    """WL_MAXL + 3 = 259 tiny layers: the second launch takes the last three.  The weights are carved out of ONE buffer back to back, so
    most of them start off a 16-byte boundary (the kernel's scalar staging loop)."""
    shapes = [(1, 16, 3, 3), (5, 3, 1, 1), (4, 4, 3, 3), (3, 2, 2, 2), (2, 5, 1, 3), (7, 8, 3, 3), (34, 4, 1, 1)]
    n = 256 + 3
    flat = torch.randn(sum(s[0] * s[1] * s[2] * s[3] for s in (shapes[i % len(shapes)] for i in range(n))) + 3,
                       generator=torch.Generator().manual_seed(259)).to(DEV)
    rows, o = [], 3
    for i in range(n):
        shape = shapes[i % len(shapes)]
        Cout, Cin, KH, KW = shape
        m = Cout * Cin * KH * KW
        rows.append((shape, R.ceil4(Cout) + 4 * (i % 2), R.ceil4(Cin), i % 5 != 1, i % 5 != 3, i % 3 == 0 and i % 5 != 3, flat[o:o + m]))
        o += m
    assert any(r[6].data_ptr() % 16 for r in rows) and not all(r[6].data_ptr() % 16 for r in rows)
    _batched_check(rows, _batched(rows), False)


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. e2e_conv2d_fwd, one table per launch path
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ids(table):
    return [(name, i) for name, (_, _, epis) in table.items() for i in range(len(epis))]


def _table_test(section, table, name, i, ld_extras=(0,)):
    s, path, epis = table[name]
    for ld_extra in ld_extras:
        _check_default(section, name, s, epis[i], {path}, ld_extra)


@pytest.mark.parametrize("name,i", _ids(SCALAR), ids=lambda v: str(v))
def test_fwd_scalar_gather(name, i):
    """Cin % 16 != 0: k_conv_gemm<4, 1, 1, 2, 1, false, 16> -- also the 7x7 / 2 stems that fall off k_conv7x7_stem's condition"""
    _table_test("scalar", SCALAR, name, i, (0, 8))


@pytest.mark.parametrize("ld_extra", [0, 4])
@pytest.mark.parametrize("name,i", _ids(STEM), ids=lambda v: str(v))
def test_fwd_stem_patch_kernel(name, i, ld_extra):
    _table_test("stem", STEM, name, i, (ld_extra,))


@pytest.mark.parametrize("name,i", _ids(THIN), ids=lambda v: str(v))
def test_fwd_thin_kernels_and_their_neighbours(name, i):
    _table_test("thin", THIN, name, i, (0, 4))


@pytest.mark.parametrize("name,i", _ids(TILE), ids=lambda v: str(v))
def test_fwd_tile_kernels_direct_epilogue(name, i):
    _table_test("tile", TILE, name, i, (0, 4) if i == 0 else (0,))


@pytest.mark.parametrize("name,i", _ids(SPLITK), ids=lambda v: str(v))
def test_fwd_splitk_tails(name, i):
    s, path, epis = SPLITK[name]
    assert _default_ws(s) > 0 and _path(s, epis[i], False).startswith("tile:")
    _table_test("splitk", SPLITK, name, i)


@pytest.mark.parametrize("name,i", _ids(SOURCES), ids=lambda v: str(v))
def test_fwd_source_layouts(name, i):
    _table_test("sources", SOURCES, name, i)


@pytest.mark.parametrize("lo", [0, 8, 16, 24])
@pytest.mark.parametrize("name", list(EPILOGUE))
def test_fwd_epilogue_matrix(name, lo):
    """scale {NULL, given} x shift {NULL, given} x residual {NULL, given} x act {none, ReLU, ELU, disparity}, eight at a time"""
    s, paths = EPILOGUE[name]
    seen = set()
    for epi in MATRIX[lo:lo + 8]:
        _check_default("epilogue", name, s, epi, paths)
        seen.add(_path(s, epi, _default_ws(s) > 0))
    assert seen <= paths


def test_fwd_epilogue_matrix_reaches_every_path_it_names():
    for name, (s, paths) in EPILOGUE.items():
        assert {_path(s, epi, _default_ws(s) > 0) for epi in MATRIX} == paths, name


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. e2e_conv2d_fwd_tuned
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tuned_twice(t, epi, tuned, ws_given=True):
    n = _tuned_ws(t["spec"]) if ws_given else 0
    a = _run(t, epi, _workspace(n), n, 0, tuned)
    b = _run(t, epi, _workspace(n), n, 0, tuned)
    assert torch.equal(a, b), f"{tuned}: two calls differ"
    return a


@pytest.mark.parametrize("tile", TILES, ids=[f"{m}x{n}" for m, n in TILES])
@pytest.mark.parametrize("name", list(TUNED))
def test_fwd_tuned_every_tile_shape(name, tile):
    t = _case(TUNED[name])
    ref = R.layer_out(t, t["z"], BN_RES)
    for ksplit in (1, 3, 16):
        _compare("tuned", f"{name} {tile} / {ksplit}", _tuned_twice(t, BN_RES, (*tile, ksplit)), ref)
    _compare("tuned", f"{name} {tile} / 3 nows", _tuned_twice(t, BN_RES, (*tile, 3), ws_given=False), ref)      # no workspace: unsplit


@pytest.mark.parametrize("G", [1, 7, 768])
@pytest.mark.parametrize("name", list(TUNED))
def test_fwd_tuned_streamk(name, G):
    t = _case(TUNED[name])
    for epi in TUNED_EPIS:
        _compare("tuned", f"{name} stream-K G={G} {epi}", _tuned_twice(t, epi, (64, 64, -G)), R.layer_out(t, t["z"], epi))


def _tile_cases():
    for sec in ("tile", "splitk", "sources", "thin"):
        for name, (s, path, epis) in FWD_TABLES[sec].items():
            if path != "thin":
                yield pytest.param(s, epis[-1], id=f"{sec}-{name}")
    for name, s in TUNED.items():
        yield pytest.param(s, BN_RES, id=f"tuned-{name}")


@pytest.mark.parametrize("s,epi", list(_tile_cases()))
def test_fwd_tuned_with_the_reported_choice_is_the_default_entry(s, epi):
    """e2e_conv_gemm_choice tied to what e2e_conv2d_fwd runs: the tuned entry with the reported triple (the layer's rows, columns, K and
    chunk depth; allow_split as a workspace is given or not) gives the default entry's bits, and so does tile_m == 0"""
    t = _case(s)
    Ho, Wo, rows, K = _geom(s)
    for given in (True, False):
        nws = _default_ws(s) if given else 0
        if given and nws == 0:
            continue
        base = _run(t, epi, _workspace(nws), nws)
        triple = _choice(rows, s.Cout, K, _depth(s), given)
        assert (triple[0], triple[1]) in TILES and (triple[2] == 1 or given)
        assert torch.equal(_tuned_twice(t, epi, triple, given), base), f"reported choice {triple} (workspace {given})"
        nt = _tuned_ws(s) if given else 0
        assert torch.equal(_run(t, epi, _workspace(nt), nt, 0, (0, 0, 0)), base), f"tile_m == 0 (workspace {given})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. queries
# ---------------------------------------------------------------------------------------------------------------------------------------
Q_ROWS = [1, 12, 198, 4800, 38400, 76729, 614400]
Q_COLS = [1, 6, 16, 32, 33, 64, 66, 96, 100, 128, 256, 512]
Q_K = [16, 144, 288, 576, 1152, 2304, 4608]


def test_gemm_choice_and_workspace_queries():
    lib = _L().load()
    flags = lib.e2e_conv_workspace_flag_floats()
    split_seen = 0
    for rows in Q_ROWS:
        for cols in Q_COLS:
            for K in Q_K:
                smax = 1
                for depth in (16, 32):
                    bm, bn, S = _choice(rows, cols, K, depth, 1)
                    assert (bm, bn) in TILES and 1 <= S <= 12, (rows, cols, K, depth, bm, bn, S)
                    assert (bm, bn) != (128, 128)                                   # the depth-16-only shape is never the built-in choice
                    assert _choice(rows, cols, K, depth, 0) == (bm, bn, 1), (rows, cols, K, depth)
                    smax = max(smax, S)
                n = lib.e2e_conv2d_splitk_workspace_floats(rows, cols, K)
                # a layer that no depth splits needs no workspace; one that is split needs the flag head and S slabs of rows x cols
                assert n == 0 if smax == 1 else n >= flags + smax * rows * cols, (rows, cols, K, smax, n)
                split_seen += smax > 1
                assert lib.e2e_conv_tuned_workspace_floats(rows, cols) >= flags + 16 * rows * cols
    assert split_seen > 20
    for K in (27, 147, 8, 40):
        assert lib.e2e_conv2d_splitk_workspace_floats(198, 64, K) == 0


def test_flag_region_holds_the_error_word():
    lib = _L().load()
    assert 0 < lib.e2e_conv_streamk_error_index() < lib.e2e_conv_workspace_flag_floats()
    # the stream-K launches of this module use up to 768 flags below the error word
    assert lib.e2e_conv_streamk_error_index() >= 768


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. the disparity head
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("size", HEAD_SIZES, ids=[f"{h}x{w}" for h, w in HEAD_SIZES])
def test_head_fwd(size, B):
    L = _L()
    H, W = size
    t = R.head_inputs(B, H, W)
    x, w, bias = (t[k].to(DEV) for k in ("x", "w", "bias"))
    for act in (R.ACT_NONE, R.ACT_DISP):
        for with_bias in (0, 1):
            runs = []
            for _ in range(2):
                y = _out(B * H * W)
                L.call("e2e_head_fwd", L.ptr(x), L.ptr(w), L.ptr(bias if with_bias else None), L.ptr(y), B, H, W, 16, act, L.stream())
                torch.cuda.synchronize()
                _written(y, B * H * W, "y")
                runs.append(y[:B * H * W].reshape(B, H, W))
            assert torch.equal(*runs)
            _compare("head", f"B{B} {H}x{W} act {act} bias {with_bias}", runs[0], R.head_fwd(t["x"], t["w"], t["bias"] if with_bias else None, act))


# ---------------------------------------------------------------------------------------------------------------------------------------
# F. refusals.  Every buffer holds 2^20 floats (the workspace 2^22): far more than the largest reading of any argument list below, so a
# call the library wrongly accepted would still stay inside them.  The 1 GB / 2 GB limits are left out for the same reason.
# ---------------------------------------------------------------------------------------------------------------------------------------
BIG = 1 << 20


@functools.lru_cache(maxsize=None)
def _big():
    g = torch.Generator().manual_seed(3)
    return {k: torch.randn(BIG, generator=g).to(DEV) for k in ("src0", "src1", "w", "vec", "res")}


def _fwd_args(out_buf, ws_buf, **over):
    """a valid 32 -> 32 3x3 call on a 6 x 8 image (by the header's parameter names), with `over` replacing what a case breaks"""
    L, b = _L(), _big()
    d = dict(src0=L.ptr(b["src0"]), src1=None, C1=32, up=1, w_fwd=L.ptr(b["w"]), ld_fwd=32, scale=None, shift=None, residual=None, out=L.ptr(out_buf),
             B=1, Hs=6, Ws=8, Cin=32, Cout=32, KH=3, KW=3, stride=1, pad=1, pad_mode=0, act=0, in_sub=ctypes.c_float(0.0),
             in_mul=ctypes.c_float(1.0), workspace=L.ptr(ws_buf), stream=L.stream())
    d.update(over)
    return d


def _refused(name, **kw):
    from e2ehip import E2EError
    with pytest.raises(E2EError):
        _L().call(name, **kw)
    torch.cuda.synchronize()


def _refusal_buffers():
    out = _out(BIG)
    ws = _workspace(4 * BIG)
    return out, ws


def _untouched(out, ws):
    assert torch.isnan(out).all(), "a refused call wrote its output"
    f = _L().load().e2e_conv_workspace_flag_floats()
    assert (ws[:f].view(torch.int32) == 0).all() and torch.isnan(ws[f:]).all(), "a refused call wrote its workspace"


def test_the_refusal_base_call_is_accepted():
    """what the refusal cases break one argument of: accepted as it stands, by both entries"""
    L = _L()
    out, ws = _refusal_buffers()
    L.call("e2e_conv2d_fwd", **_fwd_args(out, ws))
    L.call("e2e_conv2d_fwd_tuned", **_fwd_args(out, ws), tile_m=64, tile_n=64, ksplit=-768)
    torch.cuda.synchronize()
    _written(out, 6 * 8 * 32, "out")


FWD_REFUSALS = {
    "src0 NULL": dict(src0=None), "w_fwd NULL": dict(w_fwd=None), "out NULL": dict(out=None),
    "B 0": dict(B=0), "B -1": dict(B=-1), "Hs 0": dict(Hs=0), "Ws 0": dict(Ws=0), "Ws -8": dict(Ws=-8), "Cin 0": dict(Cin=0, C1=0),
    "Cout 0": dict(Cout=0), "Cout -32": dict(Cout=-32), "KH 0": dict(KH=0), "KW 0": dict(KW=0), "KW -3": dict(KW=-3),
    "up 3": dict(up=3, Hs=6, Ws=9), "up 0": dict(up=0), "up 4": dict(up=4, Hs=8, Ws=8),
    "C1 0": dict(C1=0, src1="src1"), "C1 > Cin": dict(C1=64, src1="src1"), "C1 < Cin, src1 NULL": dict(C1=16),
    "reflection, pad 0": dict(pad_mode=1, pad=0), "reflection, pad 2": dict(pad_mode=1, pad=2), "reflection, Hs 1": dict(pad_mode=1, Hs=1),
    "reflection, Ws 1": dict(pad_mode=1, Ws=1), "pad_mode 2": dict(pad_mode=2), "pad_mode -1": dict(pad_mode=-1),
    "stride 3": dict(stride=3), "stride 0": dict(stride=0),
    "Hs % up": dict(up=2, Hs=7), "Ws % up": dict(up=2, Ws=9),
    "ld_fwd % 4": dict(ld_fwd=34), "ld_fwd < Cout": dict(ld_fwd=28),
    "kernel larger than the padded input": dict(pad=0, Hs=2), "pad -1": dict(pad=-1),
    "scalar path, up 2": dict(Cin=6, C1=6, up=2), "scalar path, second source": dict(Cin=6, C1=3, src1="src1"),
    "scalar path, C1 % 16 with a second source": dict(Cin=32, C1=8, src1="src1"),
    "quad path, 5x5": dict(KH=5, KW=5, pad=2), "quad path, 1x5": dict(KH=1, KW=5, pad=2),
}
TUNED_REFUSALS = [(48, 48, 1), (64, 64, 17), (64, 64, 0), (128, 64, -4), (64, 64, -769), (64, 16, 1), (96, 32, 1), (-64, 64, 1)]


def _resolve(over):
    return {k: (_L().ptr(_big()[v]) if isinstance(v, str) else v) for k, v in over.items()}


@pytest.mark.parametrize("what", list(FWD_REFUSALS))
def test_fwd_refusals(what):
    out, ws = _refusal_buffers()
    over = _resolve(FWD_REFUSALS[what])
    _refused("e2e_conv2d_fwd", **_fwd_args(out, ws, **over))
    _refused("e2e_conv2d_fwd", **_fwd_args(out, None, **over))
    _refused("e2e_conv2d_fwd_tuned", **_fwd_args(out, ws, **over), tile_m=64, tile_n=64, ksplit=1)
    _refused("e2e_conv2d_fwd_tuned", **_fwd_args(out, ws, **over), tile_m=0, tile_n=0, ksplit=0)
    _untouched(out, ws)


def test_fwd_tuned_refusals():
    out, ws = _refusal_buffers()
    for tm, tn, ks in TUNED_REFUSALS:
        _refused("e2e_conv2d_fwd_tuned", **_fwd_args(out, ws), tile_m=tm, tile_n=tn, ksplit=ks)
    _untouched(out, ws)


def test_weight_layout_refusals():
    L, b = _L(), _big()
    wf, wb = _out(BIG), _out(BIG)
    ok = dict(w=L.ptr(b["w"]), Cout=20, Cin=6, KH=3, KW=3, w_fwd=L.ptr(wf), ld_fwd=20, w_bwd=L.ptr(wb), ld_bwd=8, stream=L.stream())
    for over in (dict(w=None), dict(Cout=0), dict(Cin=0), dict(KH=0), dict(KW=-1), dict(w_fwd=None, w_bwd=None), dict(ld_fwd=16), dict(ld_fwd=22),
                 dict(ld_bwd=4), dict(ld_bwd=10), dict(ld_fwd=18, w_bwd=None), dict(ld_bwd=7, w_fwd=None)):
        _refused("e2e_conv_weight_layouts", **{**ok, **over})
    desc = torch.tensor([[b["w"].data_ptr(), wf.data_ptr(), wb.data_ptr(), 20, 6, 3, 3, 20, 8, 0]], dtype=torch.int64).to(DEV)
    _refused("e2e_conv_weight_layouts_batched", desc=None, nlayers=1, stream=L.stream())
    _refused("e2e_conv_weight_layouts_batched", desc=L.ptr(desc), nlayers=0, stream=L.stream())
    _refused("e2e_conv_weight_layouts_batched", desc=L.ptr(desc), nlayers=-1, stream=L.stream())
    assert torch.isnan(wf).all() and torch.isnan(wb).all(), "a refused call wrote a layout"
    L.call("e2e_conv_weight_layouts", **ok)                    # the base call itself is accepted
    L.call("e2e_conv_weight_layouts_batched", desc=L.ptr(desc), nlayers=1, stream=L.stream())
    torch.cuda.synchronize()


def test_head_refusals():
    L, b = _L(), _big()
    y = _out(BIG)
    ok = dict(x=L.ptr(b["src0"]), w=L.ptr(b["w"]), bias=L.ptr(b["vec"]), y=L.ptr(y), B=2, H=4, W=6, Cin=16, act=0, stream=L.stream())
    for over in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(B=-2), dict(H=1), dict(W=1), dict(H=0), dict(W=-6), dict(Cin=8), dict(Cin=32),
                 dict(Cin=0)):
        _refused("e2e_head_fwd", **{**ok, **over})
    assert torch.isnan(y).all(), "a refused call wrote its output"
    L.call("e2e_head_fwd", **ok)
    torch.cuda.synchronize()
    _written(y, 2 * 4 * 6, "y")


def test_gemm_choice_refusals():
    out3 = (ctypes.c_int * 3)(-7, -7, -7)
    ok = dict(rows=198, cols=64, K=288, chunk_depth=32, allow_split=1, out3_host=out3)
    for over in (dict(out3_host=None), dict(rows=0), dict(rows=-5), dict(cols=0), dict(K=0), dict(K=-16), dict(chunk_depth=8), dict(chunk_depth=64),
                 dict(chunk_depth=0), dict(chunk_depth=24)):
        _refused("e2e_conv_gemm_choice", **{**ok, **over})
    assert tuple(out3) == (-7, -7, -7), "a refused query wrote its result"
    _L().call("e2e_conv_gemm_choice", **ok)
    assert tuple(out3) == (64, 64, 1)
