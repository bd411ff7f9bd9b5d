"""e2e_warp_photo_geo_fwd / _bwd (csrc/warp_photo_window.hip) and what is built on them: the fused warp-photometric pair over a window of one or
two source frames WITH the geometric-consistency term of LOSS.geometric (train_depth.py:558-576, losses.py:84-95), against float64.

  1. the entry points at geo_min_valid = 0: loss, G_s, geo_count, pmap, select, synth / valid per source, g_depth_tgt, g_depth_src, and g_T on
     the admitted cases, for every shape, mode, padding, mask setting and both memory layouts; two runs bit-identical on every output;
     every output and workspace written exactly to its size; g_T = NULL gives the same g_depth_tgt and g_depth_src bits;
  2. the gate: strict, per source, decided on the device; a closed gate leaves the bits of the photometric part;
  3. two crafted scenes: projections behind the camera (no gradient through the clamped wd, the one through the sampling position stays) and
     a pile-up of every pixel on a few source pixels (a heavy many-to-one g_depth_src);
  4. the size queries and every refused call;
  5. ops.warp_photometric_window(geometric=True): depth_tgt, depth_src and T gradients against float64 and against the operator chain inside
     the same bounds, an expanded (4,4) pose, the detached route, K refused, depth_srcs missing; geometric=False launches the window as before;
  6. Depth_Estimation at 96x128, where the reference's gate (more than 10000 valid projections) is OPEN: LOSS.geometric runs on the geo entry
     points (this fails on the parent commit), agrees with oracle.train_depth and with fused_losses=False; with estimated poses both poses
     receive a gradient; the default two-frame configuration still launches e2e_warp_photo_fwd.

Bounds come from the references alone (tests/warp_geo_ref.py); tests/test_warp_geo_inputs.py proves the cases without a GPU."""
import contextlib
import io

import numpy as np
import pytest
import torch

import warp_contract_ref as R
import warp_geo_ref as G
from warp_contract_ref import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
INT_SENTINEL = -123456789
WORST = {}
f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for name in sorted(WORST):
        ratio, e, bnd, what = WORST[name]
        print(f"warp geo {name}: largest error / bound = {ratio:.3f} ({e:.2e} of {bnd:.2e} at {what})")
    print(f"warp geo: {sum(G.admitted(G.geo_case(*c)) for c in G.CASES)} of {len(G.CASES)} cases admitted for g_T and G_s on this machine")


def _nan(n, dtype=f32):
    if dtype in (i32, i64):
        return torch.full((n + SENTINEL,), INT_SENTINEL, device=DEV, dtype=dtype)
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _untouched(buf):
    return bool((buf == INT_SENTINEL).all()) if buf.dtype in (i32, i64) else bool(torch.isnan(buf).all())


def _written(buf, n, what):
    assert _untouched(buf[n:]), f"{what}: written past the end"
    bad = (buf[:n] == INT_SENTINEL) if buf.dtype in (i32, i64) else torch.isnan(buf[:n])
    assert not bad.any(), f"{what}: {int(bad.sum())} of {n} elements not written"


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(i32), b.contiguous().view(i32))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _check(name, what, got, r64, bnd, keep=None):
    err = (got.double().cpu().reshape(r64.shape) - r64).abs()
    if keep is not None:
        err = err[keep]
    e = float(err.max()) if err.numel() else 0.0
    ratio = e / bnd if bnd > 0 else (0.0 if e == 0 else float("inf"))
    if ratio >= WORST.get(name, (-1.0,))[0]:
        WORST[name] = (ratio, e, bnd, what)
    assert e <= bnd, f"{name} {what}: max|gpu - r64| = {e:.3e} > bound {bnd:.3e} ({ratio:.2f} x)"


class _Recorder:
    """the names of the entry points that go through L.call while it is active"""

    def __init__(self, L):
        self.L, self.names = L, []

    def __enter__(self):
        self.real = self.L.call
        self.L.call = lambda name, *a, **k: (self.names.append(name), self.real(name, *a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.L.call = self.real


def _run2(launch, sizes, part=None):
    """launch(bufs) twice on fresh sentinel-filled buffers {name: (n, dtype)} (n None: NULL is passed); every buffer fully written (`part`:
    {name: m} -- only the first m elements are, the rest stays untouched), nothing behind it, the two runs bit-identical -> the buffers of
    the first run, cut to size"""
    runs, part = [], part or {}
    for _ in range(2):
        bufs = {k: None if n is None else _nan(n, dt) for k, (n, dt) in sizes.items()}
        launch(bufs)
        torch.cuda.synchronize()
        for k, (n, _dt) in sizes.items():
            if n is not None:
                _written(bufs[k], part.get(k, n), k)
        runs.append(bufs)
    for k, (n, _dt) in sizes.items():
        if n is not None:
            assert torch.equal(runs[0][k].view(i32), runs[1][k].view(i32)), f"{k}: two identical calls differ"
    return {k: None if n is None else runs[0][k][:n] for k, (n, _dt) in sizes.items()}


def _device(s, S, layout="nchw"):
    B = s["B"]
    t = {k: s[k].contiguous().to(DEV) for k in ("depth", "K", "invK")}
    t["T"] = torch.stack([(T.expand(B, 4, 4) if T.dim() == 2 else T) for T in s["T"][:S]]).contiguous().to(DEV)
    t["src"] = [x.contiguous().to(DEV) if layout == "nchw" else _nhwc(x.to(DEV)) for x in s["src"][:S]] + [None] * (2 - S)
    t["tgt"] = _nhwc(s["tgt"].to(DEV)) if layout == "nchw" else s["tgt"].contiguous().to(DEV)      # the target the other way round
    t["dsrc"] = [x.contiguous().to(DEV) for x in s["dsrc"][:S]] + [None] * (2 - S)
    t["noise"] = s["noise"][:, :S].contiguous().to(DEV)
    return t


def _fwd_args(L, t, b, use_mask, pad, terms, gmin, S, B, H, W):
    return (L.ptr(t["depth"]), L.ptr(t["dsrc"][0]), L.ptr(t["dsrc"][1]), L.ptr(t["src"][0]), L.ptr(t["src"][1]), L.strides4(t["src"][0]), L.ptr(t["tgt"]),
            L.strides4(t["tgt"]), L.ptr(t["K"]), L.ptr(t["invK"]), L.ptr(t["T"]), L.ptr(t["noise"]), L.ptr(b["synth"]), L.ptr(b["valid"]), L.ptr(b["select"]),
            L.ptr(b["pmap"]), L.ptr(b["count"]), use_mask, pad, terms, gmin, L.ptr(b["loss"]), L.ptr(b["ws"]), S, B, H, W, L.stream())


def _bwd_args(L, t, fwd, gl, b, use_mask, pad, terms, gmin, S, B, H, W, pose=True):
    return (L.ptr(t["depth"]), L.ptr(t["dsrc"][0]), L.ptr(t["dsrc"][1]), L.ptr(t["src"][0]), L.ptr(t["src"][1]), L.strides4(t["src"][0]), L.ptr(t["tgt"]),
            L.strides4(t["tgt"]), L.ptr(t["K"]), L.ptr(t["invK"]), L.ptr(t["T"]), L.ptr(fwd["synth"]), L.ptr(fwd["valid"]), L.ptr(fwd["select"]),
            L.ptr(fwd["count"]), use_mask, pad, terms, gmin, L.ptr(gl), L.ptr(b["g_dt"]), L.ptr(b["g_ds"]), L.ptr(b["g_T"]) if pose else None, L.ptr(b["ws"]),
            S, B, H, W, L.stream())


def _fwd_sizes(L, S, B, H, W, with_pmap=True):
    N = B * H * W
    return dict(synth=(3 * S * N, f32), valid=(S * N, f32), select=(N, i32), pmap=(N if with_pmap else None, f32), count=(S, i32), loss=(1 + S, f32),
                ws=(L.query("e2e_warp_photo_geo_workspace_floats", S, B, H, W), f32))


def _bwd_sizes(L, S, B, H, W, pose=True):
    N = B * H * W
    nws = L.query("e2e_warp_photo_geo_bwd_workspace_bytes", S, B, H, W)
    return dict(g_dt=(N, f32), g_ds=(S * N, f32), g_T=(S * B * 16 if pose else None, f32), ws=(nws // 8, i64))


def _forward(L, t, use_mask, pad, terms, gmin, S, B, H, W, with_pmap=True):
    return _run2(lambda b: L.call("e2e_warp_photo_geo_fwd", *_fwd_args(L, t, b, use_mask, pad, terms, gmin, S, B, H, W)), _fwd_sizes(L, S, B, H, W, with_pmap))


def _backward(L, t, fwd, gl, use_mask, pad, terms, gmin, S, B, H, W, pose=True):
    fixed_words = S * B * H * W + S
    return _run2(lambda b: L.call("e2e_warp_photo_geo_bwd", *_bwd_args(L, t, fwd, gl, b, use_mask, pad, terms, gmin, S, B, H, W, pose)),
                 _bwd_sizes(L, S, B, H, W, pose), None if pose else {"ws": fixed_words})


def _compare_forward(tag, c, fwd, S, B, H, W, with_pmap, values):
    r64, r32, b64, b32 = c[F64], c[F32], c["base"][F64], c["base"][F32]
    synth, valid = fwd["synth"].view(S, B, 3, H, W).cpu(), fwd["valid"].view(S, B, H, W).cpu()
    count = fwd["count"].cpu()
    for k in range(S):
        band = c["geo"][k]["vband"]
        if not band.any():
            assert torch.equal(valid[k], b64["valid"][k]), f"{tag}: valid of source {k}"
            assert int(count[k]) == c["n"][k], f"{tag}: geo_count[{k}] = {int(count[k])}, the reference counts {c['n'][k]}"
        else:
            assert abs(int(count[k]) - c["n"][k]) <= int(band.sum()), f"{tag}: geo_count[{k}] is off by more than the validity band holds"
        assert int(count[k]) == int(valid[k].sum()), f"{tag}: geo_count[{k}] is not the number of valid projections"
        _check("synth", tag, synth[k], b64["synth"][k], R.bound(b32["synth"][k], b64["synth"][k]))
    select = fwd["select"].view(B, H, W).cpu().long()
    off = select[~c["near"]] != r64["select"][~c["near"]]
    assert not off.any(), f"{tag}: {int(off.sum())} selections differ outside the near-ties"
    if with_pmap:
        keep = ~c["pmap_excluded"]
        _check("pmap", tag, fwd["pmap"], r64["pmap"], R.bound(r32["pmap"], r64["pmap"], keep), keep)
    _check("loss", tag, fwd["loss"][0], r64["loss"], R.bound(r32["loss"], r64["loss"]))
    if values:
        for k in range(S):
            _check("G_s", f"{tag} source {k}", fwd["loss"][1 + k], r64["G"][k], R.bound(r32["G"][k], r64["G"][k]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the entry points against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, 1), ids=lambda p: R.PAD_NAME[p])
@pytest.mark.parametrize("shape", G.SHAPES, ids=str)
def test_entry_points(shape, pad):
    L = _L()
    B, H, W = shape
    s = G.scene(*shape)
    for use_mask in (0, 1):
        for mode in G.MODES:
            S, terms = mode[0], G.Wr.terms_of(mode)
            c = G.geo_case(shape, pad, use_mask, mode)
            adm = G.admitted(c)
            gl = torch.tensor(G.G_LOSS[:1 + S], device=DEV, dtype=f32)
            first = None
            for layout in ("nchw", "nhwc"):
                with_pmap = layout == "nchw"
                tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} mode={mode} src {layout}"
                t = _device(s, S, layout=layout)
                fwd = _forward(L, t, use_mask, pad, terms, 0, S, B, H, W, with_pmap)
                if first is None:
                    first = fwd
                else:
                    assert all(_same_bits(fwd[k], first[k]) for k in ("synth", "valid", "select", "loss", "count")), f"{tag}: outputs depend on the layout or on pmap"
                _compare_forward(tag, c, fwd, S, B, H, W, with_pmap, adm)
                bwd = _backward(L, t, fwd, gl, use_mask, pad, terms, 0, S, B, H, W)
                plain = _backward(L, t, fwd, gl, use_mask, pad, terms, 0, S, B, H, W, pose=False)
                assert _same_bits(bwd["g_dt"], plain["g_dt"]) and _same_bits(bwd["g_ds"], plain["g_ds"]), f"{tag}: a gradient changes with g_T = NULL"
                bnd, keep = G.grad_bound(c, "g_depth")
                _check("g_depth_tgt", tag, bwd["g_dt"], c[F64]["g_depth"], bnd, keep)
                g_ds = bwd["g_ds"].view(S, B, H, W)
                for k in range(S):
                    bnd, keep = G.grad_bound(c, "g_ds", k)
                    _check("g_depth_src", f"{tag} source {k}", g_ds[k], c[F64]["g_ds"][k], bnd, keep)
                if adm:
                    g_T = bwd["g_T"].view(S, B, 4, 4)
                    for k in range(S):
                        _check("g_T", f"{tag} source {k}", g_T[k], c[F64]["g_T"][k], G.grad_bound(c, "g_T", k)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the gate
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, 1), ids=lambda p: R.PAD_NAME[p])
def test_the_gate_is_strict_per_source_and_leaves_the_photometric_bits(pad):
    L = _L()
    shape, use_mask, mode = G.GATE_SHAPE, 1, (2, 1, 1)
    (B, H, W), S, terms = shape, mode[0], G.Wr.terms_of(mode)
    n0, n1 = G.N_VALID[shape]
    s = G.scene(*shape)
    t = _device(s, S)
    gl = torch.tensor(G.G_LOSS, device=DEV, dtype=f32)
    gl_no0 = torch.tensor((G.G_LOSS[0], 0.0, G.G_LOSS[2]), device=DEV, dtype=f32)
    gl_none = torch.tensor((G.G_LOSS[0], 0.0, 0.0), device=DEV, dtype=f32)
    # geo_min_valid = n_0: n_0 > n_0 is false, so source 0's gate is closed and source 1's is open
    c = G.geo_case(shape, pad, use_mask, mode, None, False, n0)
    tag = f"gate {R.PAD_NAME[pad]} geo_min_valid = n_0 = {n0}"
    fwd = _forward(L, t, use_mask, pad, terms, n0, S, B, H, W)
    assert fwd["count"].tolist() == [n0, n1]
    assert float(fwd["loss"][1]) == 0.0, "n_0 > n_0 opened the gate: the comparison is not strict"
    _compare_forward(tag, c, fwd, S, B, H, W, True, G.admitted(c))
    bwd = _backward(L, t, fwd, gl, use_mask, pad, terms, n0, S, B, H, W)
    g_ds = bwd["g_ds"].view(S, B, H, W)
    assert not g_ds[0].any(), "the closed source received a depth gradient"
    for kind, got in (("g_depth", bwd["g_dt"]), ("g_ds", g_ds[1])):
        bnd, keep = G.grad_bound(c, kind, 1)
        _check(f"gate {kind}", tag, got, c[F64][kind] if kind == "g_depth" else c[F64]["g_ds"][1], bnd, keep)
    g_T = bwd["g_T"].view(S, B, 4, 4)
    for k in range(S if G.admitted(c) else 0):
        _check("gate g_T", f"{tag} source {k}", g_T[k], c[F64]["g_T"][k], G.grad_bound(c, "g_T", k)[0])
    ref = _backward(L, t, fwd, gl_no0, use_mask, pad, terms, n0, S, B, H, W)              # source 0 carries its photometric part only
    assert _same_bits(bwd["g_dt"], ref["g_dt"]) and _same_bits(bwd["g_T"], ref["g_T"]) and _same_bits(bwd["g_ds"], ref["g_ds"])
    # the reference's 10000: both gates closed, the gradients are those of the photometric part alone
    shut = _forward(L, t, use_mask, pad, terms, 10000, S, B, H, W)
    assert shut["count"].tolist() == [n0, n1] and float(shut["loss"][1]) == 0.0 and float(shut["loss"][2]) == 0.0
    assert _same_bits(shut["loss"][:1], fwd["loss"][:1]) and _same_bits(shut["synth"], fwd["synth"]) and _same_bits(shut["select"], fwd["select"])
    a = _backward(L, t, shut, gl, use_mask, pad, terms, 10000, S, B, H, W)
    b = _backward(L, t, shut, gl_none, use_mask, pad, terms, 0, S, B, H, W)               # gates open, nothing upstream of the terms
    assert not a["g_ds"].any() and not b["g_ds"].any()
    assert _same_bits(a["g_dt"], b["g_dt"]) and _same_bits(a["g_T"], b["g_T"])
    shut_case = G.geo_case(shape, pad, use_mask, mode, None, False, 10000)
    bnd, keep = G.grad_bound(shut_case, "g_depth")
    _check("gate shut g_depth", tag, a["g_dt"], shut_case[F64]["g_depth"], bnd, keep)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the crafted scenes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, 1), ids=lambda p: R.PAD_NAME[p])
@pytest.mark.parametrize("shape", G.CRAFTED_SHAPES, ids=str)
@pytest.mark.parametrize("kind", ("behind", "pileup"))
def test_crafted_scenes(kind, shape, pad):
    L = _L()
    c = G.crafted(kind, shape, pad)
    (B, H, W), S, terms = shape, G.CRAFTED_MODE[0], G.Wr.terms_of(G.CRAFTED_MODE)
    t = _device(c["scene"], S)
    tag = f"{kind} {shape} {R.PAD_NAME[pad]}"
    fwd = _forward(L, t, 1, pad, terms, 0, S, B, H, W)
    _compare_forward(tag, c, fwd, S, B, H, W, True, G.admitted(c))
    gl = torch.tensor(G.CRAFTED_G_LOSS, device=DEV, dtype=f32)
    bwd = _backward(L, t, fwd, gl, 1, pad, terms, 0, S, B, H, W)                          # two runs, bit for bit, g_depth_src included
    bnd, keep = G.crafted_bound(c, "g_depth")
    _check(f"{kind} g_depth_tgt", tag, bwd["g_dt"], c[F64]["g_depth"], bnd, keep)
    g_ds = bwd["g_ds"].view(S, B, H, W)
    for k in range(S):
        bnd, keep = G.crafted_bound(c, "g_ds", k)
        _check(f"{kind} g_depth_src", f"{tag} source {k}", g_ds[k], c[F64]["g_ds"][k], bnd, keep)
    if kind == "behind":
        b64 = c["base"][F64]
        below = (b64["valid"][0] > 0) & (b64["c2"][0] < G.ZCLAMP) & ~c["grad_excluded"]
        assert int((bwd["g_dt"].view(B, H, W).cpu()[below] != 0).sum()) >= 100, "no gradient through the sampling position under the clamp"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the size queries and what the header rules out
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _L()
    for B, H, W in G.SHAPES + [(3, 8, 32), (1, 480, 640)]:
        tiles = -(-H // 8) * -(-W // 32)
        for S in (1, 2):
            assert L.query("e2e_warp_photo_geo_workspace_floats", S, B, H, W) == (1 + 2 * S) * B * tiles > 0
            assert L.query("e2e_warp_photo_geo_bwd_workspace_bytes", S, B, H, W) == 8 * (S * B * H * W + S) + 96 * S * B * tiles
    for bad in ((0, 1, 4, 4), (3, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (2, -1, 4, 4)):
        assert L.query("e2e_warp_photo_geo_workspace_floats", *bad) == 0
        assert L.query("e2e_warp_photo_geo_bwd_workspace_bytes", *bad) == 0


def test_refused_calls_leave_outputs_alone():
    L = _L()
    S, B, H, W = 2, 2, 4, 6
    N = B * H * W
    st = L.stream()
    img = torch.rand(B, 3, H, W, device=DEV)
    s4, i_ = L.strides4(img), L.ptr(img)
    mats = torch.eye(4, device=DEV).repeat(S * B, 1, 1).contiguous()
    m_ = L.ptr(mats)
    big = torch.rand(S * B * 4 * N, device=DEV) + 1
    r_ = L.ptr(big)
    sel = torch.zeros(N, device=DEV, dtype=i32)
    cnt = torch.full((S,), N, device=DEV, dtype=i32)
    f = dict(synth=_nan(3 * S * N), valid=_nan(S * N), select=_nan(N, i32), pmap=_nan(N), count=_nan(S, i32), loss=_nan(1 + S),
             ws=_nan(L.query("e2e_warp_photo_geo_workspace_floats", S, B, H, W)))
    g = dict(g_dt=_nan(N), g_ds=_nan(S * N), g_T=_nan(S * B * 16), ws=_nan(L.query("e2e_warp_photo_geo_bwd_workspace_bytes", S, B, H, W) // 8, i64))
    count = [0]

    def refused(name, outs, args):
        with pytest.raises(L.E2EError, match=name):
            L.call(name, *args)
        torch.cuda.synchronize()
        assert all(_untouched(o) for o in outs.values()), f"{name}: an output changed although the call was refused"
        count[0] += 1

    def sweep(name, outs, a, nulls, values):
        for k in nulls:
            refused(name, outs, [None if j == k else v for j, v in enumerate(a)])
        for k, vs in values.items():
            for v in vs:
                refused(name, outs, [v if j == k else x for j, x in enumerate(a)])

    #     0   1   2   3   4   5   6   7   8   9   10  11  12                 13                 14                  15                16                 17 18 19 20 21                22              23 24 25 26 27
    a = [r_, r_, r_, i_, i_, s4, i_, s4, m_, m_, m_, r_, L.ptr(f["synth"]), L.ptr(f["valid"]), L.ptr(f["select"]), L.ptr(f["pmap"]), L.ptr(f["count"]), 1, 1, 6, 0, L.ptr(f["loss"]), L.ptr(f["ws"]), S, B, H, W, st]
    dims = {18: (2, -1), 19: (1, 7, 8, -1), 20: (-1,), 23: (0, 3, -1), 24: (0, -1, 65536), 25: (0, 1), 26: (0, 1)}
    sweep("e2e_warp_photo_geo_fwd", f, a, (0, 1, 2, 3, 4, 6, 8, 9, 10, 12, 13, 14, 16, 21, 22), dims)
    #     0   1   2   3   4   5   6   7   8   9   10  11  12  13           14           15 16 17 18 19  20                 21                 22                23              24 25 26 27 28
    b = [r_, r_, r_, i_, i_, s4, i_, s4, m_, m_, m_, r_, r_, L.ptr(sel), L.ptr(cnt), 1, 1, 6, 0, r_, L.ptr(g["g_dt"]), L.ptr(g["g_ds"]), L.ptr(g["g_T"]), L.ptr(g["ws"]), S, B, H, W, st]
    dims = {16: (2, -1), 17: (1, 7, 8, -1), 18: (-1,), 24: (0, 3, -1), 25: (0, -1, 65536), 26: (0, 1), 27: (0, 1)}
    sweep("e2e_warp_photo_geo_bwd", g, b, (0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12, 13, 14, 19, 20, 21, 23), dims)
    assert count[0] == (15 + 17) + (17 + 17)
    L.call("e2e_warp_photo_geo_fwd", *a)                                           # the vectors themselves are good calls, and so are the
    L.call("e2e_warp_photo_geo_bwd", *b)                                           # optional pointers left out
    L.call("e2e_warp_photo_geo_fwd", *[None if j in (11, 15) else v for j, v in enumerate(a)])
    L.call("e2e_warp_photo_geo_bwd", *[None if j == 22 else v for j, v in enumerate(b)])
    L.call("e2e_warp_photo_geo_fwd", *[None if j in (2, 4) else (1 if j == 23 else v) for j, v in enumerate(a)])      # S = 1 needs no second source
    torch.cuda.synchronize()
    _written(f["loss"], 1 + S, "loss")
    _written(g["g_T"], S * B * 16, "g_T")
    _written(g["g_ds"], S * N, "g_depth_src")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. ops.warp_photometric_window(geometric=True)
# ---------------------------------------------------------------------------------------------------------------------------------------
ADMITTED = []
OPS_CASES = [((2, 9, 33), 1, 1, (2, 0, 0)), ((2, 9, 33), 0, 1, (2, 1, 1)), ((2, 9, 33), 1, 0, (2, 0, 1)), ((2, 9, 33), 0, 0, (1, 1, 1)),
             ((2, 9, 33), 1, 1, (2, 1, 0)), G.EXPANDED_CASE]


def _chain(ops, d, dsrcs, srcs, tgt, K, invK, Ts, pad, use_mask, mode, noise, g_loss):
    """the operator chain of train_depth.compute_losses (fused_losses=False) with LOSS.geometric on the same inputs; the operator's own
    geometric term has the reference's 10000 built in, so the last elementwise step of the term is written out here on its operands"""
    S, minrep, auto = mode
    B, _, H, W = d.shape
    maps, autos, geos = [], [], []
    for src, ds, T in zip(srcs[:S], dsrcs[:S], Ts[:S]):
        pts = ops.backproject(d, invK)
        grid, wd, valid = ops.project3d(pts, K, T, H, W, geometric=True)
        synth = ops.grid_sample(src, grid, padding_mode=R.PAD_NAME[pad], align_corners=True)
        idp = ops.grid_sample(ds, grid, padding_mode=R.PAD_NAME[pad], align_corners=False)
        x, y = (ops.mask_mul(synth, valid), ops.mask_mul(tgt, valid)) if use_mask else (synth, tgt)
        maps.append(ops.photometric(x, y))
        if auto:
            x = ops.mask_mul(src, valid) if use_mask else src
            autos.append(ops.photometric(x, y))
        geos.append((((wd - idp).abs() / (wd + idp)).clamp(0, 1) * valid).sum() / valid.sum())
    photo = torch.cat(maps, 1) if S > 1 else maps[0]
    if auto:
        a = torch.cat(autos, 1) if S > 1 else autos[0]
        if minrep:
            a = a + noise
        else:
            a, photo = ops.channel_mean(a), ops.channel_mean(photo)
        photo = torch.cat((a, photo), 1)
    elif not minrep:
        photo = ops.channel_mean(photo)
    return g_loss[0] * ops.min_reprojection(photo) + sum(g_loss[1 + k] * geos[k] for k in range(S))


@pytest.mark.parametrize("case", OPS_CASES, ids=str)
def test_ops_warp_photometric_window_geometric(case):
    from e2ehip import ops
    L = _L()
    shape, pad, use_mask, mode = case[:4]
    expanded = len(case) > 4 and case[5]
    B, H, W = shape
    S, minrep, auto = mode
    c = G.geo_case(*case)
    adm = G.admitted(c)                  # decided by the references on the machine that runs the test; T.grad, the loss and G_s need it
    ADMITTED.append(adm)
    keep_d, keep_s = ~c["grad_excluded"], [~x for x in c["src_excluded"]]
    s, r64 = c["scene"], c[F64]
    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} mode={mode}{' poses expanded' if expanded else ''}"
    depth, K, invK = (s[k].contiguous().to(DEV) for k in ("depth", "K", "invK"))
    srcs, tgt = [_nhwc(x.to(DEV)) for x in s["src"][:S]], _nhwc(s["tgt"].to(DEV))
    ds0 = [x.view(B, 1, H, W).contiguous().to(DEV) for x in s["dsrc"][:S]]
    noise = s["noise"][:, :S].contiguous().to(DEV)
    kw = dict(padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask), min_reprojection=bool(minrep), auto_masking=bool(auto), tie_noise=noise)
    T0 = [T.contiguous().to(DEV) for T in c["base"]["T"][:S]]
    gl = G.G_LOSS

    def fused(leaves, **more):
        d = depth.view(B, 1, H, W).clone().requires_grad_()
        dss = [x.clone().requires_grad_() for x in ds0]
        Ts = [T.expand(B, 4, 4) if expanded else T for T in leaves]
        with _Recorder(L) as rec:
            out = ops.warp_photometric_window(d, srcs, tgt, K, invK, Ts, geometric=True, depth_srcs=dss, geo_min_valid=0, **kw, **more)
            (gl[0] * out["photometric"] + sum(gl[1 + k] * out["geometric"][k] for k in range(S))).backward()
        return d.grad, [x.grad for x in dss], rec.names, out

    leaves = [T.clone().requires_grad_() for T in T0]
    gd, gds, names, out = fused(leaves, want_pmap=True)
    assert names == ["e2e_warp_photo_geo_fwd", "e2e_warp_photo_geo_bwd"], names
    assert out["synth"].shape == (S, B, 3, H, W) and out["valid"].shape == (S, B, 1, H, W) and out["select"].shape == (B, 1, H, W)
    assert out["geometric"].shape == (S,) and out["geo_count"].shape == (S,) and out["geo_count"].dtype == i32 and out["pmap"].shape == (B, 1, H, W)
    assert out["geo_count"].tolist() == list(c["n"])
    if adm:
        _check("ops loss", tag, out["photometric"].detach(), r64["loss"], R.bound(c[F32]["loss"], r64["loss"]))
        for k in range(S):
            _check("ops G_s", f"{tag} source {k}", out["geometric"][k].detach(), r64["G"][k], R.bound(c[F32]["G"][k], r64["G"][k]))
    _check("ops depth.grad", tag, gd, r64["g_depth"], G.grad_bound(c, "g_depth")[0], keep_d)
    for k, T in enumerate(leaves):
        assert T.grad.shape == T0[k].shape and gds[k].shape == (B, 1, H, W)
        if adm:
            _check("ops T.grad", f"{tag} source {k}", T.grad, r64["g_T"][k], G.grad_bound(c, "g_T", k)[0])
        _check("ops depth_src.grad", f"{tag} source {k}", gds[k], r64["g_ds"][k], G.grad_bound(c, "g_ds", k)[0], keep_s[k])
    gd_detached, gds_detached, names, out = fused([T.clone() for T in T0])
    assert names == ["e2e_warp_photo_geo_fwd", "e2e_warp_photo_geo_bwd"] and out["pmap"] is None
    assert torch.equal(gd, gd_detached) and all(torch.equal(a, b) for a, b in zip(gds, gds_detached)), f"{tag}: a gradient changes with the pose gradient"
    Tb = [T.expand(B, 4, 4) for T in T0]
    d0 = depth.view(B, 1, H, W)
    with torch.no_grad(), _Recorder(L) as rec:
        ops.warp_photometric_window(d0, srcs, tgt, K, invK, Tb, geometric=True, depth_srcs=ds0, **kw)
    assert rec.names == ["e2e_warp_photo_geo_fwd"]
    with pytest.raises(NotImplementedError, match="K"):
        ops.warp_photometric_window(d0, srcs, tgt, K.clone().requires_grad_(), invK, Tb, geometric=True, depth_srcs=ds0, **kw)
    with pytest.raises(NotImplementedError, match="inv_K"):
        ops.warp_photometric_window(d0, srcs, tgt, K, invK.clone().requires_grad_(), Tb, geometric=True, depth_srcs=ds0, **kw)
    with pytest.raises(ValueError, match="depth_srcs"):
        ops.warp_photometric_window(d0, srcs, tgt, K, invK, Tb, geometric=True, **kw)
    with pytest.raises(ValueError, match="depth_srcs"):
        ops.warp_photometric_window(d0, srcs, tgt, K, invK, Tb, geometric=True, depth_srcs=[x[:, 0] for x in ds0], **kw)
    with _Recorder(L) as rec:                                         # geometric=False: the window's entry points and outputs, nothing moved
        plain = ops.warp_photometric_window(d0.clone().requires_grad_(), srcs, tgt, K, invK, Tb, **kw)
        plain["photometric"].backward()
    assert rec.names == ["e2e_warp_photo_window_fwd", "e2e_warp_photo_window_bwd"] and sorted(plain) == ["photometric", "pmap", "select", "synth", "valid"]
    # the operator chain on the same inputs, inside the same bounds
    d = d0.clone().requires_grad_()
    dss = [x.clone().requires_grad_() for x in ds0]
    leaves = [T.clone().requires_grad_() for T in T0]
    _chain(ops, d, dss, srcs, tgt, K, invK, [T.expand(B, 4, 4) if expanded else T for T in leaves], pad, use_mask, mode, noise, gl).backward()
    _check("chain depth.grad", tag, d.grad, r64["g_depth"], G.grad_bound(c, "g_depth")[0], keep_d)
    for k, T in enumerate(leaves):
        if adm:
            _check("chain T.grad", f"{tag} source {k}", T.grad, r64["g_T"][k], G.grad_bound(c, "g_T", k)[0])
        _check("chain depth_src.grad", f"{tag} source {k}", dss[k].grad, r64["g_ds"][k], G.grad_bound(c, "g_ds", k)[0], keep_s[k])


def test_ops_pose_comparisons_ran():
    """admission is decided per machine (the float32 reference's error moves with the CPU's math library): most of the cases above must
    have been admitted, or T.grad went unchecked"""
    assert len(ADMITTED) == len(OPS_CASES) and sum(ADMITTED) >= len(OPS_CASES) - 2, ADMITTED


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. Depth_Estimation at 96x128: the reference's gate is open
# ---------------------------------------------------------------------------------------------------------------------------------------
HT, WT = 96, 128
GEO, WINDOW = {"e2e_warp_photo_geo_fwd", "e2e_warp_photo_geo_bwd"}, {"e2e_warp_photo_window_fwd", "e2e_warp_photo_window_bwd"}
OPERATORS = {"e2e_grid_sample_fwd", "e2e_photometric_fwd", "e2e_geometric_consistency_lossgrad", "e2e_grid_sample_bwd", "e2e_grid_sample_bwd_exact",
             "e2e_mask_mul", "e2e_min_reprojection_lossgrad"}


def _tie_plane(S):
    return torch.randn(1, S, HT, WT, generator=torch.Generator().manual_seed(11))


def _train(cfg_mod, frames, fused, steps, tie=None, estimated=False):
    """the setup of tests/test_gpu_warp_photo_window.py::_train at 96x128 -> (loss log, sequence, state dict, entry-point names, hooks' record)"""
    import train_depth as td
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    from oracle import depthnet
    L = _L()
    cfg = td.default_config(HT, WT, frames, steps)
    cfg.DEBUG.print_metrics = False
    cfg.ABLATION.dual_disparity = False
    cfg_mod(cfg)
    sd = depthnet.random_state_dict(0)
    if estimated:                                                      # the setup of tests/test_gpu_warp_photo_pose.py::_train_step
        cfg.DATA.use_gt_pose = False
        cfg.MODEL.odom = "gradicp"
        seq = make_sequence(len(frames), HT, WT, seed=5, scene="corner")
        sd["decoder.decoder.10.conv.weight"] = sd["decoder.decoder.10.conv.weight"] * 40.0
    else:
        seq = make_sequence(len(frames), HT, WT, seed=5)
    de = td.Depth_Estimation(cfg, sequence=seq, state_dict=sd, fused_losses=fused)
    seen = dict(T_requires_grad=[], g_T=[], geo_count=[], geometric=[])
    real_randn, real_window = torch.randn, ops.warp_photometric_window

    def randn(*a, **k):                                               # the tie-break plane (train_depth.py:650): the fixed one, on both routes
        if tie is not None and len(a) == 1 and isinstance(a[0], (tuple, list)) and tuple(a[0]) == tuple(tie.shape):
            return tie.to(k.get("device", "cpu"))
        return real_randn(*a, **k)

    def window(depth_tgt, srcs, tgt, K, inv_K, Ts, **kw):
        Ts = [T.view(T.shape) for T in Ts]                             # nodes of their own: their gradients are the window op's alone
        seen["T_requires_grad"].append([bool(T.requires_grad) for T in Ts])
        for k, T in enumerate(Ts):
            if T.requires_grad:
                T.register_hook(lambda g, k=k: seen["g_T"].append((k, g.detach().cpu())))
        out = real_window(depth_tgt, srcs, tgt, K, inv_K, Ts, **kw)
        if "geo_count" in out:
            seen["geo_count"].append(out["geo_count"].tolist())
            seen["geometric"].append(out["geometric"].detach().cpu().tolist())
        return out

    td.torch.randn, ops.warp_photometric_window = randn, window
    try:
        with _Recorder(L) as rec, contextlib.redirect_stdout(io.StringIO()):
            log = de.train()
    finally:
        td.torch.randn, ops.warp_photometric_window = real_randn, real_window
    return np.array(log), seq, sd, rec.names, seen


def _oracle(cfg_mod, frames, steps, seq, sd):
    from oracle import train_depth as otd
    c = otd.Config()
    c.frames, c.refinement_steps, c.dual_disparity = tuple(frames), steps, False
    cfg_mod(c)
    colors, gt, K, poses = seq
    return np.array([r["loss"] for r in otd.Trainer(sd, c).train_batch(colors, gt, poses, K)])


def _flags_gpu(min_reprojection, auto_masking):
    def mod(c):
        c.LOSS.min_reprojection, c.LOSS.auto_masking, c.LOSS.geometric = min_reprojection, auto_masking, True
    return mod


def _flags_cpu(min_reprojection, auto_masking, tie):
    def mod(c):
        c.min_reprojection, c.auto_masking, c.geometric = min_reprojection, auto_masking, True
        if tie is not None:
            c.tie_break_noise = tie * 0.00001
    return mod


DRIVER_CASES = {"a: geometric alone": (False, False), "b: min-reprojection, auto-masking and geometric": (True, True)}


@pytest.mark.parametrize("name", sorted(DRIVER_CASES))
def test_driver_runs_the_geometric_term_on_the_fused_entry_points(name):
    """the route (fails on the parent commit, whose _fused_ok sends LOSS.geometric to the operators) and the values with the gate OPEN: the loss
    log against oracle.train_depth and against fused_losses=False at the tolerance the existing three-frame tests use"""
    minrep, auto = DRIVER_CASES[name]
    frames, steps = (0, -1, 1), 2
    tie = _tie_plane(2) if (minrep and auto) else None
    log_f, seq, sd, names, seen = _train(_flags_gpu(minrep, auto), frames, True, steps, tie)
    assert GEO <= set(names), f"{name}: the geo entry points were not launched"
    assert not (OPERATORS | WINDOW) & set(names), f"{name}: the step went through {sorted((OPERATORS | WINDOW) & set(names))}"
    assert names.count("e2e_warp_photo_geo_fwd") == names.count("e2e_warp_photo_geo_bwd") == len(log_f) == steps
    assert len(seen["geo_count"]) == steps and all(n > 10000 for step in seen["geo_count"] for n in step), seen["geo_count"]      # the gate is open
    assert all(g > 1e-4 for step in seen["geometric"] for g in step), seen["geometric"]
    log_u, _, _, names_u, _ = _train(_flags_gpu(minrep, auto), frames, False, steps, tie)
    assert not GEO & set(names_u) and {"e2e_grid_sample_fwd", "e2e_photometric_fwd", "e2e_geometric_consistency_lossgrad"} <= set(names_u)
    want = _oracle(_flags_cpu(minrep, auto, tie), frames, steps, seq, sd)
    print(f"\n{name}: fused {log_f}, operators {log_u}, oracle {want}, geo_count {seen['geo_count']}, G_s {seen['geometric']}")
    np.testing.assert_allclose(log_f, want, rtol=2e-4)
    np.testing.assert_allclose(log_f, log_u, rtol=2e-4)


def test_driver_with_estimated_poses_stays_fused_and_both_poses_get_a_gradient():
    log, _, _, names, seen = _train(_flags_gpu(False, False), (0, -1, 1), True, 1, estimated=True)
    assert GEO <= set(names) and not (OPERATORS | WINDOW) & set(names)
    assert seen["T_requires_grad"] == [[True, True]], seen["T_requires_grad"]
    got = dict(seen["g_T"])
    assert set(got) == {0, 1}
    for k, g in got.items():
        assert g.shape == (1, 4, 4) and torch.isfinite(g).all() and float(g.abs().max()) > 0, f"pose {k} received no gradient"
    assert np.isfinite(log).all()


def test_default_two_frame_configuration_still_launches_the_pair():
    _, _, _, names, seen = _train(lambda c: None, (0, -1), True, 1)
    assert "e2e_warp_photo_fwd" in names and "e2e_warp_photo_bwd" in names
    assert not (WINDOW | GEO) & set(names) and not OPERATORS & set(names) and seen["T_requires_grad"] == []
