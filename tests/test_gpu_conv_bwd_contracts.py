"""The backward entry points the launch plan (e2ehip.netplan) calls, against float64 torch references of the contracts include/e2eslam.h
states -- not against each other:

  A. e2e_conv2d_bwd_data_fused / _fused_tuned:  dxp (+)= (dA * W^T + pre_add) * act'(x_in), over every epilogue of conv.hip
     (direct block epilogue of k_conv_gemm and k_conv_gemm_sk, class-form scatter, k_conv_splitk_epilogue4 / _epilogue / _epilogue_cls);
  B. e2e_conv2d_bwd_weight_scaled / _scaled_tuned / _scaled_deferred + e2e_wgrad_reduce_batched:  dW = out_scale (.) d/dW, d bias = sum dA,
     over every WgradKernel of wgrad_setup, the patch kernels, and slab counts on both sides of the reduction's unrolled / ragged loops;
  C. e2e_conv2d_gather_adjoint_act and e2e_conv2d_act_bwd_acc;
  D. e2e_conv2d_bwd_pair_deferred (both orders) against the same references;
  E. the argument combinations the header rules out: E2EError, outputs untouched.

Every output buffer is NaN-filled (except where an accumulate flag reads it) and followed by a NaN sentinel; workspaces are allocated at
exactly the size their *_workspace_floats query returns, also followed by a sentinel.  So each case also checks that every element meant
to be written was written and that nothing past any buffer's end was.  Error measure (tests/test_gpu_conv.py): max |err| / max |ref|."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
GRAD_BOUND = 5e-5


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _rel(a, ref):
    return ((a.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def _out(n, init=None):
    """n floats + NaN sentinel; NaN-filled unless `init` (the accumulate input) is given"""
    buf = torch.full((n + SENTINEL,), float("nan"), device=DEV)
    if init is not None:
        buf[:n] = init.flatten().to(DEV)
    return buf


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _workspace(n, flags=True):
    """exactly n floats of NaN + sentinel; the stream-K flag head of a convolution GEMM workspace zeroed (its owner's duty)"""
    if n == 0:
        return None
    buf = torch.full((n + SENTINEL,), float("nan"), device=DEV)
    if flags:
        buf[:min(n, _L().load().e2e_conv_workspace_flag_floats())] = 0
    return buf


def _workspace_ok(ws, n, flags=True):
    if ws is None:
        return
    assert torch.isnan(ws[n:]).all(), "workspace: written past the size its query returned"
    if flags:
        f = min(n, _L().load().e2e_conv_workspace_flag_floats())
        assert (ws[:f] == 0).all(), "workspace: stream-K flags left raised (or the time-out word set)"


def _w_bwd(w):
    """w_bwd [(kh,kw,co)][ld] from a torch weight (Cout,Cin,KH,KW) through e2e_conv_weight_layouts, padding columns zeroed"""
    L = _L()
    Cout, Cin, KH, KW = w.shape
    ld = (Cin + 3) // 4 * 4
    wb = torch.zeros(KH * KW * Cout, ld, device=DEV)
    L.call("e2e_conv_weight_layouts", L.ptr(w), Cout, Cin, KH, KW, None, 0, L.ptr(wb), ld, L.stream())
    return wb, ld


def _act_deriv(y, act):
    """act'(u) from the activation's OUTPUT y (float64): 1 ReLU, 2 ELU, 3 disparity sigmoid"""
    y = y.double()
    if act == 1:
        return (y > 0).double()
    if act == 2:
        return torch.where(y > 0, torch.ones_like(y), y + 1)
    if act == 3:
        s = (y - 0.01) * 0.1
        return 10 * s * (1 - s)
    return torch.ones_like(y)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. backward-data, fused forms (pad mode 0: dxp is (B, Hs, Ws, Cin))
# ---------------------------------------------------------------------------------------------------------------------------------------
# B, Cin, Hs, Ws, Cout, k, stride, pad -- and what each reaches (default entry, workspace given, unless said otherwise)
DATA = {
    # split-K (2 slices, 18 chunks of 32) -> k_conv_splitk_epilogue4; NULL workspace and tuned ksplit 1 -> epilogue_block of k_conv_gemm;
    # tuned stream-K -> epilogue_block of k_conv_gemm_sk
    "s1": (2, 64, 12, 20, 64, 3, 1, 1),
    # Cin % 4 != 0: tuned ksplit 3 -> the scalar k_conv_splitk_epilogue; otherwise the direct epilogue with a partial column quad
    "s1_cin6": (1, 6, 10, 14, 32, 3, 1, 1),
    # Cout % 32 != 0: 16-deep K chunks, the only depth at which tuned 128 x 128 tiles stay 128 x 128 (k_conv_gemm<2, 2, 2, 2, 4, true, 16>)
    "s1_cout48": (1, 32, 10, 14, 48, 3, 1, 1),
    # stride 2, class form split by tap (8 class workgroups < 500) -> k_conv_splitk_epilogue_cls; NULL workspace -> class scatter
    "s2_even": (2, 64, 12, 20, 128, 3, 2, 1),
    "s2_odd": (1, 64, 17, 23, 128, 3, 2, 1),                # unequal parity classes (9 x 12, 9 x 11, 8 x 12, 8 x 11)
    # class form with >= 500 class workgroups under tuned 32 x 32 tiles (4 x 68 x 2 = 544) -> class scatter with a workspace given
    "s2_large": (2, 64, 62, 70, 32, 3, 2, 1),
    # 1x1 stride 2: one class carries the tap, three have none (memset + class scatter) -- odd sizes make the empty classes unequal
    "1x1_even": (2, 64, 16, 24, 128, 1, 2, 0),
    "1x1_odd": (1, 64, 13, 9, 128, 1, 2, 0),
}
# mode -> (accumulate, pre_add, in_act)
MODES = {"plain": (0, 0, 0), "acc": (1, 0, 0), "pre": (0, 1, 0), "relu": (0, 0, 1), "elu": (0, 0, 2), "acc+pre+relu": (1, 1, 1),
         "acc+pre+elu": (1, 1, 2)}
TILES = [(64, 64), (128, 64), (128, 128), (128, 32), (32, 128), (32, 64), (64, 32), (32, 32)]


@functools.lru_cache(maxsize=None)
def _data_case(name):
    B, Cin, Hs, Ws, Cout, k, s, p = DATA[name]
    g = torch.Generator().manual_seed(sum(DATA[name]))
    Ho, Wo = (Hs + 2 * p - k) // s + 1, (Ws + 2 * p - k) // s + 1
    t = dict(spec=DATA[name], Ho=Ho, Wo=Wo)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    da = torch.randn(B, Ho, Wo, Cout, generator=g)
    t["dx0"] = torch.randn(B, Hs, Ws, Cin, generator=g)
    t["pre"] = torch.randn(B, Hs, Ws, Cin, generator=g)
    t["x1"] = F.relu(torch.randn(B, Hs, Ws, Cin, generator=g))         # exact zeros: act' taken from the same values on both sides
    t["x2"] = F.elu(torch.randn(B, Hs, Ws, Cin, generator=g))
    x = torch.zeros(B, Cin, Hs, Ws, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w.double(), None, s, p)
    t["gx"] = _nhwc(torch.autograd.grad(y, x, da.double().permute(0, 3, 1, 2))[0])
    for key in ("dx0", "pre", "x1", "x2"):
        t[key + "_d"] = t[key].to(DEV)
    t["da_d"] = da.to(DEV)
    t["wb"], t["ld"] = _w_bwd(w.to(DEV))
    return t


def _data_ref(t, mode):
    acc, pre, act = MODES[mode]
    r = t["gx"] + (t["pre"].double() if pre else 0)
    if act:
        r = r * _act_deriv(t["x%d" % act], act)
    return r + (t["dx0"].double() if acc else 0)


def _data_run(t, mode, dec, entry="e2e_conv2d_bwd_data_fused"):
    """dec: 'default' (workspace from e2e_conv2d_bwd_data_workspace_floats), 'nows' (NULL workspace) or (tile_m, tile_n, ksplit) (tuned entry,
    workspace from e2e_conv_tuned_workspace_floats)"""
    L = _L()
    lib = L.load()
    B, Cin, Hs, Ws, Cout, k, s, p = t["spec"]
    acc, pre, act = MODES[mode]
    n = B * Hs * Ws * Cin
    out = _out(n, t["dx0"] if acc else None)
    if dec == "default":
        nws = lib.e2e_conv2d_bwd_data_workspace_floats(B, Hs, Ws, Cin, k * k * Cout, s)
    elif dec == "nows":
        nws = 0
    else:
        nws = lib.e2e_conv_tuned_workspace_floats(B * Hs * Ws, Cin)
    ws = _workspace(nws)
    args = [L.ptr(t["da_d"]), L.ptr(t["wb"]), t["ld"], L.ptr(out), B, Hs, Ws, Cin, Cout, t["Ho"], t["Wo"], k, k, s, p, 0, acc,
            L.ptr(t["x%d_d" % act] if act else None), act, L.ptr(t["pre_d"] if pre else None), L.ptr(ws)]
    if isinstance(dec, tuple):
        L.call("e2e_conv2d_bwd_data_fused_tuned", *args, *dec, L.stream())
    else:
        L.call(entry, *args, L.stream())
    torch.cuda.synchronize()
    _written(out, n, f"dxp ({mode}, {dec})")
    _workspace_ok(ws, nws)
    return out[:n].reshape(B, Hs, Ws, Cin)


@pytest.mark.parametrize("dec", ["default", "nows"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(DATA))
def test_bwd_data_fused(name, mode, dec):
    t = _data_case(name)
    e = _rel(_data_run(t, mode, dec), _data_ref(t, mode))
    assert e < GRAD_BOUND, f"{name} {mode} {dec}: {e:.2e}"


@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize("tile", TILES, ids=[f"{m}x{n}" for m, n in TILES])
@pytest.mark.parametrize("name", list(DATA))
def test_bwd_data_fused_tuned(name, tile, ksplit):
    """every tile family at 1 and 3 K slices (the class form ignores the slice count: it splits by tap when it has few workgroups)"""
    t = _data_case(name)
    for mode in ("pre", "acc+pre+relu", "acc+pre+elu"):
        e = _rel(_data_run(t, mode, (*tile, ksplit)), _data_ref(t, mode))
        assert e < GRAD_BOUND, f"{name} {mode} {tile} / {ksplit}: {e:.2e}"


@pytest.mark.parametrize("G", [1, 7, 512])
def test_bwd_data_fused_streamk(G):
    """stream-K on G persistent workgroups (k_conv_gemm_sk: partial tiles handed over through the workspace, fused epilogue by the finisher)"""
    t = _data_case("s1")
    for mode in MODES:
        e = _rel(_data_run(t, mode, (64, 64, -G)), _data_ref(t, mode))
        assert e < GRAD_BOUND, f"stream-K G={G} {mode}: {e:.2e}"


def test_bwd_data_unfused_entries_match_contract():
    """e2e_conv2d_bwd_data / _acc are the fused entry with accumulate = 0 / 1 and no pre-add / act' (the autograd path's forms)"""
    L = _L()
    lib = L.load()
    for name in ("s1", "s2_odd", "1x1_odd"):
        t = _data_case(name)
        B, Cin, Hs, Ws, Cout, k, s, p = t["spec"]
        n = B * Hs * Ws * Cin
        for acc in (0, 1):
            out = _out(n, t["dx0"] if acc else None)
            nws = lib.e2e_conv2d_bwd_data_workspace_floats(B, Hs, Ws, Cin, k * k * Cout, s)
            ws = _workspace(nws)
            L.call("e2e_conv2d_bwd_data_acc", L.ptr(t["da_d"]), L.ptr(t["wb"]), t["ld"], L.ptr(out), B, Hs, Ws, Cin, Cout, t["Ho"], t["Wo"],
                   k, k, s, p, 0, acc, L.ptr(ws), L.stream())
            torch.cuda.synchronize()
            _written(out, n, f"{name} acc={acc}")
            _workspace_ok(ws, nws)
            e = _rel(out[:n].reshape(B, Hs, Ws, Cin), _data_ref(t, "acc" if acc else "plain"))
            assert e < GRAD_BOUND, f"{name} acc={acc}: {e:.2e}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. backward-weight
# ---------------------------------------------------------------------------------------------------------------------------------------
# B, Cx, Cs, up, H, W (full resolution), Cout, k, stride, pad, pad_mode -- the kernel each reaches through the untuned entries (the tuned
# entry runs the implicit-GEMM kernels only: the same WgradKernel, except where noted)
WGRAD = {
    "gemm16": (1, 64, 0, 1, 20, 36, 16, 3, 1, 1, 0),          # WK_GEMM16 (k_wgrad_gemm16)
    "gemm4_32": (2, 64, 0, 1, 14, 20, 32, 3, 1, 1, 0),        # WK_GEMM4_32, one source
    "gemm4_64": (2, 64, 0, 1, 12, 20, 64, 3, 1, 1, 0),        # WK_GEMM4_64, one source
    "gemm4_64_s2": (2, 64, 0, 1, 30, 44, 128, 3, 2, 1, 0),    # WK_GEMM4_64, stride 2, two row tiles
    "gemm4_64_two": (1, 64, 64, 2, 12, 16, 64, 3, 1, 1, 1),   # WK_GEMM4_64, two sources (x2 upsample + skip), reflection padding
    "gemm_32_v4": (2, 64, 0, 1, 6, 6, 32, 3, 1, 1, 0),        # Wo < 8: WK_GEMM_32 (k_wgrad_gemm<1, 4, 4>)
    "gemm_64_v4": (2, 64, 0, 1, 5, 7, 64, 3, 1, 1, 0),        # Wo < 8: WK_GEMM_64 (k_wgrad_gemm<2, 2, 4>)
    "1x1_s2": (1, 64, 0, 1, 13, 9, 128, 1, 2, 0, 0),          # 1x1 / 2, Wo = 5: WK_GEMM_64 vec 4
    "gemm_32_v1": (1, 6, 0, 1, 12, 20, 32, 3, 1, 1, 0),       # Cin % 4 != 0: WK_GEMM_32 (k_wgrad_gemm<1, 4, 1>, scalar gather)
    "gemm_64_v1": (1, 6, 0, 1, 12, 20, 64, 3, 1, 1, 0),       # WK_GEMM_64 (k_wgrad_gemm<2, 2, 1>)
    # the RGB stem with (v - in_sub) * in_mul: k_wgrad7x7_stem without bias, WK_GEMM_64 vec 1 with bias and through the tuned entry
    "stem": (2, 3, 0, 1, 32, 48, 64, 7, 2, 3, 0),
    # thin patch kernels (untuned, reflection padding): k_wgrad3x3_thin<1> (16 -> 16); k_wgrad3x3_thin<2> (64 up + 32 skip -> 32), whose
    # tuned form is WK_GEMM4_32 with two sources
    "thin16": (1, 16, 0, 1, 24, 40, 16, 3, 1, 1, 1),
    "thin32_two": (1, 64, 32, 2, 16, 24, 32, 3, 1, 1, 1),
    # P = 10240 pixels: the tuned sweep reaches 8, 9, 13 and 40 slabs (zl = 8, ragged and unrolled reduction loops)
    "sweep": (2, 64, 0, 1, 64, 80, 64, 3, 1, 1, 0),
}
STEM_NORM = (0.45, 1 / 0.225)
# (scale, bias) combinations
SB = [(0, 0), (1, 0), (0, 1), (1, 1)]


@functools.lru_cache(maxsize=None)
def _wgrad_case(name):
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = WGRAD[name]
    g = torch.Generator().manual_seed(sum(WGRAD[name]) + 7)
    Cin = Cx + Cs
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    t = dict(spec=WGRAD[name], Cin=Cin, Ho=Ho, Wo=Wo)
    src0 = torch.rand(B, H // up, W // up, Cx, generator=g) if Cx == 3 else torch.randn(B, H // up, W // up, Cx, generator=g)
    src1 = torch.randn(B, H, W, Cs, generator=g) if Cs else None
    da = torch.randn(B, Ho, Wo, Cout, generator=g)
    t["scale"] = torch.rand(Cout, generator=g) + 0.5
    t["dw0"] = torch.randn(Cout, Cin, k, k, generator=g)
    t["db0"] = torch.randn(Cout, generator=g)
    x = src0.double().permute(0, 3, 1, 2)
    if Cx == 3:
        x = (x - STEM_NORM[0]) * STEM_NORM[1]
    if up > 1:
        x = F.interpolate(x, scale_factor=up, mode="nearest")
    if Cs:
        x = torch.cat([x, src1.double().permute(0, 3, 1, 2)], 1)
    if pm:
        x = F.pad(x, (p,) * 4, mode="reflect")
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, s, 0 if pm else p)
    t["gw"] = torch.autograd.grad(y, w, da.double().permute(0, 3, 1, 2))[0]
    t["gb"] = da.double().sum((0, 1, 2))
    t["src0"], t["src1"], t["da"] = src0.to(DEV), src1.to(DEV) if Cs else None, da.to(DEV)
    t["scale_d"] = t["scale"].to(DEV)
    return t


def _wgrad_refs(t, sc, bias, acc):
    dw = t["gw"] * (t["scale"].double().view(-1, 1, 1, 1) if sc else 1) + (t["dw0"].double() if acc else 0)
    db = (t["gb"] + (t["db0"].double() if acc else 0)) if bias else None
    return dw, db


def _wgrad_run(t, sc, bias, acc, how, target=0):
    """how: 'scaled' (e2e_conv2d_bwd_weight_scaled), 'deferred' (+ e2e_wgrad_reduce_batched) or 'tuned' (target_workgroups); returns
    dW, dbias and, for 'deferred', the reduction descriptor"""
    L = _L()
    lib = L.load()
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = t["spec"]
    Cin, Ho, Wo = t["Cin"], t["Ho"], t["Wo"]
    nw = Cout * Cin * k * k
    dw = _out(nw, t["dw0"] if acc else None)
    db = _out(Cout, t["db0"] if acc else None) if bias else None
    if how == "tuned":
        nws = lib.e2e_conv2d_wgrad_tuned_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, bias, target)
    else:
        nws = lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, bias)
    ws = _workspace(nws, flags=False)
    sub, mul = STEM_NORM if Cx == 3 else (0.0, 1.0)
    args = [L.ptr(t["da"]), L.ptr(t["scale_d"] if sc else None), L.ptr(t["src0"]), L.ptr(t["src1"]), Cx, up, L.ptr(dw), L.ptr(db), L.ptr(ws),
            B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, acc, ctypes.c_float(sub), ctypes.c_float(mul)]
    desc = None
    if how == "scaled":
        L.call("e2e_conv2d_bwd_weight_scaled", *args, L.stream())
    elif how == "tuned":
        L.call("e2e_conv2d_bwd_weight_scaled_tuned", *args, target, L.stream())
    else:
        desc = L.WgradReduceDesc()
        L.call("e2e_conv2d_bwd_weight_scaled_deferred", *args, ctypes.byref(desc), L.stream())
        _reduce_batched([desc])
    torch.cuda.synchronize()
    _written(dw, nw, f"dW ({how})")
    if bias:
        _written(db, Cout, f"dbias ({how})")
    _workspace_ok(ws, nws, flags=False)
    return dw[:nw].reshape(Cout, Cin, k, k), db[:Cout] if bias else None, desc


def _reduce_batched(descs):
    L = _L()
    arr = (L.WgradReduceDesc * len(descs))(*descs)
    total = L.load().e2e_wgrad_reduce_batch_prepare(arr, len(descs))
    assert total > 0
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.call("e2e_wgrad_reduce_batched", L.ptr(table), len(descs), total, L.stream())
    torch.cuda.synchronize()


def _wgrad_check(t, sc, bias, acc, how, target=0):
    dw, db, desc = _wgrad_run(t, sc, bias, acc, how, target)
    rdw, rdb = _wgrad_refs(t, sc, bias, acc)
    e = _rel(dw, rdw)
    assert e < GRAD_BOUND, f"dW ({how}, scale={sc}, bias={bias}, acc={acc}, target={target}): {e:.2e}"
    if bias:
        e = _rel(db, rdb)
        assert e < GRAD_BOUND, f"dbias ({how}, scale={sc}, bias={bias}, acc={acc}, target={target}): {e:.2e}"
    return desc


@pytest.mark.parametrize("how", ["scaled", "deferred"])
@pytest.mark.parametrize("name", list(WGRAD))
def test_bwd_weight_scaled(name, how):
    t = _wgrad_case(name)
    for sc, bias in SB:
        for acc in (0, 1):
            _wgrad_check(t, sc, bias, acc, how)


def _wgrad_slices(t, bias, target):
    """the slab count wgrad_plan + wgrad_setup give an implicit-GEMM backward-weight call (mirrors conv.hip; checked against the library's
    own descriptors by test_slab_count_mirror)"""
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = t["spec"]
    Cin, P = t["Cin"], B * t["Ho"] * t["Wo"]
    lean = Cin % 4 == 0 and Cx % 4 == 0 and Cout % 4 == 0 and t["Wo"] >= 8
    use16 = lean and Cout == 16
    tm, tn = (16, 160) if use16 else ((32, 128) if Cout <= 32 else (64, 64))
    tiles = -(-Cout // tm) * -(-(k * k * Cin + bias) // tn)
    S = max(1, min(-(-(target * 3 // 4 if use16 else target) // tiles), -(-P // 256)))
    cbp = 32 if lean else 16
    pps = -(-(-(-P // S)) // cbp) * cbp
    return -(-P // pps)


# (shape, bias, target_workgroups): slab counts 1, 2 - 7 (reduced by 2 waves), 8, and ragged counts past the 4 x 8 unrolled loop
SWEEP = [("1x1_s2", 1, 64), ("gemm4_64", 0, 64), ("gemm16", 1, 1024), ("gemm4_64_s2", 0, 96), ("gemm4_32", 1, 256), ("sweep", 1, 64),
         ("sweep", 0, 64), ("sweep", 0, 81), ("sweep", 0, 117), ("sweep", 0, 360), ("sweep", 1, 8192), ("gemm_64_v1", 1, 64),
         ("gemm_32_v4", 0, 2048), ("thin32_two", 1, 512), ("stem", 0, 256), ("stem", 1, 4096)]


def test_slab_sweep_covers_the_reduction_loops():
    S = {_wgrad_slices(_wgrad_case(n), b, tg) for n, b, tg in SWEEP}
    assert 1 in S and 8 in S and any(2 <= v <= 7 for v in S), sorted(S)
    assert any(v > 8 and v % 32 for v in S) and any(v > 32 for v in S), sorted(S)


@pytest.mark.parametrize("case", SWEEP, ids=[f"{n}-b{b}-t{tg}" for n, b, tg in SWEEP])
def test_bwd_weight_scaled_tuned(case):
    name, bias, target = case
    t = _wgrad_case(name)
    for sc in (0, 1):
        for acc in (0, 1):
            _wgrad_check(t, sc, bias, acc, "tuned", target)


@pytest.mark.parametrize("name", [n for n in WGRAD if n not in ("stem", "thin16", "thin32_two")])
def test_slab_count_mirror(name):
    """_wgrad_slices agrees with the slab count of the library's own reduction descriptor (default target: 1024 workgroups)"""
    t = _wgrad_case(name)
    for bias in (0, 1):
        desc = _wgrad_check(t, 1, bias, 0, "deferred")
        assert desc.S == _wgrad_slices(t, bias, 1024) and desc.zl == (8 if desc.S >= 8 else 2), (desc.S, desc.zl)


def test_batched_reduction_of_several_layers():
    """one e2e_wgrad_reduce_batched launch over descriptors with different slab counts, zl and accumulate flags"""
    L = _L()
    lib = L.load()
    runs = []
    for name, sc, bias, acc in (("sweep", 1, 1, 1), ("gemm16", 1, 0, 0), ("gemm4_64_two", 1, 1, 0), ("1x1_s2", 0, 1, 1)):
        t = _wgrad_case(name)
        B, Cx, Cs, up, H, W, Cout, k, s, p, pm = t["spec"]
        Cin, nw = t["Cin"], Cout * t["Cin"] * k * k
        dw = _out(nw, t["dw0"] if acc else None)
        db = _out(Cout, t["db0"] if acc else None) if bias else None
        nws = lib.e2e_conv2d_wgrad_workspace_floats(B, t["Ho"], t["Wo"], Cin, Cout, k, k, bias)
        ws = _workspace(nws, flags=False)
        desc = L.WgradReduceDesc()
        L.call("e2e_conv2d_bwd_weight_scaled_deferred", L.ptr(t["da"]), L.ptr(t["scale_d"] if sc else None), L.ptr(t["src0"]),
               L.ptr(t["src1"]), Cx, up, L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, Cin, Cout, t["Ho"], t["Wo"], k, k, s, p, pm, acc,
               ctypes.c_float(0.0), ctypes.c_float(1.0), ctypes.byref(desc), L.stream())
        runs.append((t, sc, bias, acc, dw, db, ws, nws, desc))
    assert len({(r[8].S, r[8].zl) for r in runs}) >= 3
    _reduce_batched([r[8] for r in runs])
    for t, sc, bias, acc, dw, db, ws, nws, desc in runs:
        Cout, k = t["spec"][6], t["spec"][7]
        nw = Cout * t["Cin"] * k * k
        _written(dw, nw, "dW (batched)")
        _workspace_ok(ws, nws, flags=False)
        rdw, rdb = _wgrad_refs(t, sc, bias, acc)
        assert _rel(dw[:nw].reshape(rdw.shape), rdw) < GRAD_BOUND
        if bias:
            _written(db, Cout, "dbias (batched)")
            assert _rel(db[:Cout], rdb) < GRAD_BOUND


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. gather adjoint with act', activation backward
# ---------------------------------------------------------------------------------------------------------------------------------------
# B, C1, C2, up, Hs, Ws (full resolution), padded -- C1 and C2 multiples of 4: k_gather_adjoint4, otherwise k_gather_adjoint
GATHER = [
    (2, 8, 12, 2, 6, 8, 1),       # upsample + skip, reflection: quads
    (1, 6, 5, 2, 4, 6, 1),        # scalar loader
    (1, 8, 0, 1, 2, 2, 1),        # 2 x 2 image: every pixel has reflected copies on both sides
    (1, 3, 2, 1, 2, 2, 1),        # the same, scalar
    (1, 4, 4, 2, 2, 2, 1),        # 2 x 2 full resolution over a 1 x 1 upsampled source
    (2, 16, 16, 1, 5, 7, 0),      # no padding: the identity fold
    (1, 5, 0, 2, 6, 4, 0),        # upsample only, scalar, no padding
]


@pytest.mark.parametrize("case", GATHER, ids=[f"g{i}" for i in range(len(GATHER))])
def test_gather_adjoint_act(case):
    L = _L()
    B, C1, C2, up, Hs, Ws, pad = case
    g = torch.Generator().manual_seed(sum(case))
    Cin, Hp, Wp = C1 + C2, Hs + 2 * pad, Ws + 2 * pad
    dxp = torch.randn(B, Hp, Wp, Cin, generator=g)
    s0 = torch.zeros(B, C1, Hs // up, Ws // up, dtype=torch.float64, requires_grad=True)
    s1 = torch.zeros(B, C2, Hs, Ws, dtype=torch.float64, requires_grad=True)
    x = F.interpolate(s0, scale_factor=up, mode="nearest") if up > 1 else s0
    x = torch.cat([x, s1], 1) if C2 else x
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect") if pad else x
    gr = torch.autograd.grad(xp, [s0, s1] if C2 else [s0], dxp.double().permute(0, 3, 1, 2))
    ref = [_nhwc(r) for r in gr]
    shapes = [(B, Hs // up, Ws // up, C1)] + ([(B, Hs, Ws, C2)] if C2 else [])
    acts = {a: [F.relu(torch.randn(*sh, generator=g)) if a == 1 else F.elu(torch.randn(*sh, generator=g)) for sh in shapes] for a in (1, 2)}
    old = [torch.randn(*sh, generator=g) for sh in shapes]
    dxp_d = dxp.to(DEV)
    for a0 in (0, 1, 2):
        for a1 in ((0, 1, 2) if C2 else (0,)):
            for acc0, acc1 in ((0, 0), (1, 1), (1, 0), (0, 1)):
                accs, act = (acc0, acc1), (a0, a1)
                outs = [_out(old[i].numel(), old[i] if accs[i] else None) for i in range(len(shapes))]
                srcs = [acts[act[i]][i].to(DEV) if act[i] else None for i in range(len(shapes))]
                L.call("e2e_conv2d_gather_adjoint_act", L.ptr(dxp_d), B, Hs, Ws, Cin, C1, up, pad, L.ptr(outs[0]),
                       L.ptr(outs[1] if C2 else None), acc0, acc1, L.ptr(srcs[0]), a0, L.ptr(srcs[1] if C2 else None), a1, L.stream())
                torch.cuda.synchronize()
                for i in range(len(shapes)):
                    n = old[i].numel()
                    _written(outs[i], n, f"d_src{i}")
                    r = ref[i] * (_act_deriv(acts[act[i]][i], act[i]) if act[i] else 1) + (old[i].double() if accs[i] else 0)
                    e = _rel(outs[i][:n].reshape(shapes[i]), r)
                    assert e < GRAD_BOUND, f"d_src{i} act={act} acc={accs}: {e:.2e}"


@pytest.mark.parametrize("C", [16, 7])
def test_act_bwd_acc(C):
    """dz (+)= dy * act'(y) * scale[c], act' from the activation's output"""
    L = _L()
    g = torch.Generator().manual_seed(C)
    n = 3 * 11 * 13 * C
    u = torch.randn(n, generator=g)
    ys = {0: u, 1: F.relu(u), 2: F.elu(u), 3: 10 * torch.sigmoid(u) + 0.01}
    dy, dz0, scale = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.rand(C, generator=g) + 0.5
    dy_d, scale_d = dy.to(DEV), scale.to(DEV)          # device copies held for the duration of the launches
    for act in (0, 1, 2, 3):
        y_d = ys[act].to(DEV)
        for sc in (0, 1):
            for acc in (0, 1):
                out = _out(n, dz0 if acc else None)
                L.call("e2e_conv2d_act_bwd_acc", L.ptr(dy_d), L.ptr(y_d), L.ptr(scale_d if sc else None), L.ptr(out), n, C, act, acc, L.stream())
                torch.cuda.synchronize()
                _written(out, n, "dz")
                r = dy.double() * _act_deriv(ys[act], act) * (scale.double().repeat(n // C) if sc else 1) + (dz0.double() if acc else 0)
                e = _rel(out[:n], r)
                assert e < 1e-6, f"act={act} scale={sc} acc={acc}: {e:.2e}"


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. the paired launch (e2e_conv2d_bwd_pair_deferred) against the same references
# ---------------------------------------------------------------------------------------------------------------------------------------
# (data shape, mode) for the zero-padded layers: the weight gradient of the same layer reads x = x1 (the ReLU input of A)
PAIR = [("s1", "plain"), ("s1", "acc+pre+relu"), ("s2_even", "acc+pre+elu"), ("s2_odd", "relu"), ("1x1_even", "pre"), ("1x1_odd", "acc+pre+relu")]


@functools.lru_cache(maxsize=None)
def _pair_wgrad_ref(name):
    t = _data_case(name)
    B, Cin, Hs, Ws, Cout, k, s, p = t["spec"]
    x = t["x1"].double().permute(0, 3, 1, 2)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, s, p)
    return torch.autograd.grad(y, w, t["da_d"].cpu().double().permute(0, 3, 1, 2))[0]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", PAIR, ids=[f"{n}-{m}" for n, m in PAIR])
def test_bwd_pair_against_reference(case, order):
    L = _L()
    lib = L.load()
    name, mode = case
    t = _data_case(name)
    B, Cin, Hs, Ws, Cout, k, s, p = t["spec"]
    acc, pre, act = MODES[mode]
    n = B * Hs * Ws * Cin
    dx = _out(n, t["dx0"] if acc else None)
    nwsb = lib.e2e_conv2d_bwd_data_workspace_floats(B, Hs, Ws, Cin, k * k * Cout, s)
    wsb = _workspace(nwsb)
    nwsw = lib.e2e_conv2d_wgrad_workspace_floats(B, t["Ho"], t["Wo"], Cin, Cout, k, k, 0)
    wsw = _workspace(nwsw, flags=False)
    nw = Cout * Cin * k * k
    dw = _out(nw)
    scale = (torch.arange(Cout, dtype=torch.float32) % 5 * 0.25 + 0.5)
    scale_d = scale.to(DEV)                              # read by the deferred reduction: held until it ran
    desc = L.WgradReduceDesc()
    L.call("e2e_conv2d_bwd_pair_deferred", L.ptr(t["da_d"]), L.ptr(t["wb"]), t["ld"], L.ptr(dx), B, Hs, Ws, Cin, Cout, t["Ho"], t["Wo"], k, k,
           s, p, 0, acc, L.ptr(t["x%d_d" % act] if act else None), act, L.ptr(t["pre_d"] if pre else None), L.ptr(wsb), L.ptr(scale_d),
           L.ptr(t["x1_d"]), None, Cin, 1, L.ptr(dw), None, L.ptr(wsw), 0, ctypes.c_float(0.0), ctypes.c_float(1.0), ctypes.byref(desc), order,
           L.stream())
    _reduce_batched([desc])
    _written(dx, n, "dxp (pair)")
    _written(dw, nw, "dW (pair)")
    _workspace_ok(wsb, nwsb)
    _workspace_ok(wsw, nwsw, flags=False)
    e = _rel(dx[:n].reshape(B, Hs, Ws, Cin), _data_ref(t, mode))
    assert e < GRAD_BOUND, f"dxp: {e:.2e}"
    e = _rel(dw[:nw].reshape(Cout, Cin, k, k), _pair_wgrad_ref(name) * scale.double().view(-1, 1, 1, 1))
    assert e < GRAD_BOUND, f"dW: {e:.2e}"


@pytest.mark.parametrize("order", [0, 1])
def test_bwd_pair_reflect_concat_against_reference(order):
    """a decoder layer: reflection padding (dxp over the padded domain), x2 upsample + skip concat, bias column"""
    L = _L()
    lib = L.load()
    t = _wgrad_case("gemm4_64_two")
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = t["spec"]
    Cin, Ho, Wo = t["Cin"], t["Ho"], t["Wo"]
    g = torch.Generator().manual_seed(11)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    wb, ld = _w_bwd(w.to(DEV))
    xp = torch.zeros(B, Cin, H + 2, W + 2, dtype=torch.float64, requires_grad=True)
    rdx = _nhwc(torch.autograd.grad(F.conv2d(xp, w.double(), None, 1, 0), xp, t["da"].cpu().double().permute(0, 3, 1, 2))[0])
    n = B * (H + 2) * (W + 2) * Cin
    dx = _out(n)
    nwsb = lib.e2e_conv2d_bwd_data_workspace_floats(B, H + 2, W + 2, Cin, k * k * Cout, s)
    wsb = _workspace(nwsb)
    nwsw = lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, 1)
    wsw = _workspace(nwsw, flags=False)
    nw = Cout * Cin * k * k
    dw, db = _out(nw), _out(Cout)
    desc = L.WgradReduceDesc()
    L.call("e2e_conv2d_bwd_pair_deferred", L.ptr(t["da"]), L.ptr(wb), ld, L.ptr(dx), B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, 0, None, 0,
           None, L.ptr(wsb), None, L.ptr(t["src0"]), L.ptr(t["src1"]), Cx, up, L.ptr(dw), L.ptr(db), L.ptr(wsw), 0, ctypes.c_float(0.0),
           ctypes.c_float(1.0), ctypes.byref(desc), order, L.stream())
    _reduce_batched([desc])
    for buf, m, what in ((dx, n, "dxp"), (dw, nw, "dW"), (db, Cout, "dbias")):
        _written(buf, m, what)
    _workspace_ok(wsb, nwsb)
    _workspace_ok(wsw, nwsw, flags=False)
    rdw, rdb = _wgrad_refs(t, 0, 1, 0)
    assert _rel(dx[:n].reshape(rdx.shape), rdx) < GRAD_BOUND
    assert _rel(dw[:nw].reshape(rdw.shape), rdw) < GRAD_BOUND
    assert _rel(db[:Cout], rdb) < GRAD_BOUND


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def _refused(name, *args):
    from e2ehip import E2EError
    L = _L()
    with pytest.raises(E2EError):
        L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def test_bwd_data_refusals():
    L = _L()
    lib = L.load()
    B, Cin, Hs, Ws, Cout = 1, 16, 6, 8, 16
    g = torch.Generator().manual_seed(5)
    da = torch.randn(B, Hs, Ws, 32, generator=g).to(DEV)
    wb = torch.randn(9 * 32, Cin, generator=g).to(DEV)
    x_in = F.relu(torch.randn(B, Hs + 2, Ws + 2, Cin, generator=g)).to(DEV)
    pre = torch.randn(B, Hs + 2, Ws + 2, Cin, generator=g).to(DEV)
    n = B * (Hs + 2) * (Ws + 2) * Cin
    nws = lib.e2e_conv_tuned_workspace_floats(n // Cin, Cin)
    ws = _workspace(nws)
    out = _out(n)
    base = lambda cout, pm: [L.ptr(da), L.ptr(wb), Cin, L.ptr(out), B, Hs, Ws, Cin, cout, Hs, Ws, 3, 3, 1, 1, pm]
    # pre_add / act' on a reflection-padded layer (the header: pad_mode 0 only)
    _refused("e2e_conv2d_bwd_data_fused", *base(Cout, 1), 0, None, 0, L.ptr(pre), L.ptr(ws))
    _refused("e2e_conv2d_bwd_data_fused", *base(Cout, 1), 0, L.ptr(x_in), 1, None, L.ptr(ws))
    _refused("e2e_conv2d_bwd_data_fused", *base(Cout, 0), 0, None, 3, None, L.ptr(ws))          # act' of the disparity sigmoid
    _refused("e2e_conv2d_bwd_data_fused", *base(Cout, 0), 0, None, 1, None, L.ptr(ws))          # act' without x_in
    # Cout % 16 != 0
    _refused("e2e_conv2d_bwd_data_fused", *base(24, 0), 0, None, 0, None, L.ptr(ws))
    _refused("e2e_conv2d_bwd_data_fused_tuned", *base(24, 0), 0, None, 0, None, L.ptr(ws), 64, 64, 1)
    # unsupported decompositions
    for tm, tn, ks in ((48, 48, 1), (64, 64, 0), (64, 64, 17), (128, 64, -4), (64, 64, -769), (64, 16, 1)):
        _refused("e2e_conv2d_bwd_data_fused_tuned", *base(Cout, 0), 0, None, 0, None, L.ptr(ws), tm, tn, ks)
    # the paired entry shares the checks
    d = L.WgradReduceDesc()
    wsw = torch.zeros(lib.e2e_conv2d_wgrad_workspace_floats(B, Hs, Ws, Cin, Cout, 3, 3, 0) + 1, device=DEV)
    dw = _out(Cout * Cin * 9)
    _refused("e2e_conv2d_bwd_pair_deferred", *base(Cout, 1), 0, None, 0, L.ptr(pre), L.ptr(ws), None, L.ptr(x_in), None, Cin, 1, L.ptr(dw),
             None, L.ptr(wsw), 0, ctypes.c_float(0.0), ctypes.c_float(1.0), ctypes.byref(d), 0)
    assert torch.isnan(out).all(), "a refused call wrote its output"
    assert torch.isnan(dw).all(), "a refused call wrote its output"
    _workspace_ok(ws, nws)


def test_bwd_weight_refusals():
    L = _L()
    lib = L.load()
    t = _wgrad_case("gemm4_64")
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = t["spec"]
    Cin, Ho, Wo = t["Cin"], t["Ho"], t["Wo"]
    nw = Cout * Cin * k * k
    dw, db = _out(nw), _out(Cout)
    ws = torch.zeros(lib.e2e_conv2d_wgrad_tuned_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, 1, 8192), device=DEV)
    args = [L.ptr(t["da"]), None, L.ptr(t["src0"]), None, Cx, up, L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, 0,
            ctypes.c_float(0.0), ctypes.c_float(1.0)]
    for target in (0, 63, 8193, -64):
        _refused("e2e_conv2d_bwd_weight_scaled_tuned", *args, target)
    _refused("e2e_conv2d_bwd_weight_scaled_deferred", *args, None)
    # the scalar gather takes one full-resolution zero-padded source
    t6 = _wgrad_case("gemm_32_v1")
    _refused("e2e_conv2d_bwd_weight_scaled", L.ptr(t6["da"]), None, L.ptr(t6["src0"]), None, 6, 1, L.ptr(dw), None, L.ptr(ws), 1, 12, 20, 6, 32,
             12, 20, 3, 3, 1, 1, 1, 0, ctypes.c_float(0.0), ctypes.c_float(1.0))
    assert torch.isnan(dw).all() and torch.isnan(db).all(), "a refused call wrote its output"


def test_gather_adjoint_refusals():
    L = _L()
    dxp = torch.zeros(1, 4, 4, 8, device=DEV)
    d0 = _out(1 * 2 * 2 * 8)
    _refused("e2e_conv2d_gather_adjoint_act", L.ptr(dxp), 1, 2, 2, 8, 8, 1, 1, L.ptr(d0), None, 0, 0, None, 1, None, 0)   # act0 without src0
    _refused("e2e_conv2d_gather_adjoint_act", L.ptr(dxp), 1, 2, 2, 8, 8, 1, 1, L.ptr(d0), None, 0, 0, L.ptr(dxp), 3, None, 0)
    _refused("e2e_conv2d_gather_adjoint_act", L.ptr(dxp), 1, 2, 2, 8, 4, 1, 1, L.ptr(d0), None, 0, 0, None, 0, None, 0)  # split, no d_src1
    _refused("e2e_conv2d_gather_adjoint_act", L.ptr(dxp), 1, 2, 2, 8, 8, 3, 1, L.ptr(d0), None, 0, 0, None, 0, None, 0)  # up = 3
    assert torch.isnan(d0).all()
