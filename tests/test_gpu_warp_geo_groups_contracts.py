"""e2e_warp_photo_geo_groups_fwd / _bwd (csrc/warp_photo_window.hip): the geo pair over scale groups of the batch.

  1. slice equality, the main contract: for every case of tests/multiscale_geo_ref.py, ungated and gated, the grouped forward's synth, valid,
     select, pmap, geo_count[s G + g] and loss_out[1 + s G + g] are torch.equal to what e2e_warp_photo_geo_fwd returns on group g's slice; the
     grouped backward's g_depth_src planes are torch.equal to the slice call's (given g_loss[1 + s] = g_loss[1 + s G + g]); for G in {1, 2, 4}
     g_depth_tgt and g_T are torch.equal too with the slice call's g_loss[0] divided by G (an exact scaling); for G = 3 those two are held to
     warp_geo_ref's float64 reference under its own gradient bounds and exclusions; loss_out[0] is held to the float64 mean of the groups'
     losses under warp_contract_ref.bound;
  2. gates: a closed group's loss slot is exactly 0.0 and its g_depth_src planes exactly 0; an open group's outputs do not move with its
     neighbour's state; the group without any valid projection gives 0 and finite gradients at geo_min_valid = 0;
  3. workspace independence: two calls give equal bits, one of them after the workspaces were filled with NaN;
  4. every new refusal returns E2E_ERR_ARG and leaves poisoned outputs untouched, after the geo pair's own refusals;
  5. with groups = 1 the grouped pair equals the existing pair bit for bit, one case per (S, mode).

Bounds and cases come from the references alone; tests/test_multiscale_geo_inputs.py proves the cases without a GPU."""
import pytest
import torch

import multiscale_geo_ref as M
import warp_contract_ref as R
import warp_geo_ref as G
from warp_contract_ref import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
INT_SENTINEL = -123456789
f32, i32, i64 = torch.float32, torch.int32, torch.int64
FWD_KEYS = ("synth", "valid", "select", "pmap", "count", "loss")
BWD_KEYS = ("g_dt", "g_ds", "g_T")


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _fill(n, dtype=f32):
    if dtype in (i32, i64):
        return torch.full((n + SENTINEL,), INT_SENTINEL, device=DEV, dtype=dtype)
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _untouched(buf):
    return bool((buf == INT_SENTINEL).all()) if buf.dtype in (i32, i64) else bool(torch.isnan(buf).all())


def _cut(bufs, sizes):
    """every buffer written to its size and not past it -> the buffers cut to size"""
    for k, n in sizes.items():
        assert _untouched(bufs[k][n:]), f"{k}: written past the end"
        head = bufs[k][:n]
        bad = (head == INT_SENTINEL) if head.dtype in (i32, i64) else torch.isnan(head)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {n} elements not written"
    return {k: bufs[k][:n] for k, n in sizes.items()}


def _bits(a, b):
    return torch.equal(a.contiguous().view(i32).reshape(-1), b.contiguous().view(i32).reshape(-1))


def _device(st, S):
    """a stacked scene (multiscale_geo_ref.stacked) or a warp_geo_ref scene on the device"""
    t = {k: st[k].contiguous().to(DEV) for k in ("depth", "K", "invK", "tgt")}
    t["T"] = torch.stack(st["T"][:S]).contiguous().to(DEV)
    t["src"] = [x.contiguous().to(DEV) for x in st["src"][:S]] + [None] * (2 - S)
    t["dsrc"] = [x.contiguous().to(DEV) for x in st["dsrc"][:S]] + [None] * (2 - S)
    t["noise"] = st["noise"][:, :S].contiguous().to(DEV)
    return t


def _slice(t, lo, hi):
    """batch items lo .. hi - 1 as operands of their own"""
    cut = lambda x: None if x is None else x[lo:hi].contiguous()
    return dict(depth=cut(t["depth"]), K=cut(t["K"]), invK=cut(t["invK"]), tgt=cut(t["tgt"]), T=t["T"][:, lo:hi].contiguous(),
                src=[cut(x) for x in t["src"]], dsrc=[cut(x) for x in t["dsrc"]], noise=cut(t["noise"]))


def _forward(L, t, S, B, H, W, terms, gmin, groups=None, ws_fill=None):
    """groups None: e2e_warp_photo_geo_fwd; else the grouped entry point"""
    N, Gn = B * H * W, groups or 1
    sizes = dict(synth=3 * S * N, valid=S * N, select=N, pmap=N, count=S * Gn, loss=1 + S * Gn)
    b = {k: _fill(n, i32 if k in ("select", "count") else f32) for k, n in sizes.items()}
    ws = torch.empty(L.query("e2e_warp_photo_geo_workspace_floats", S, B, H, W), device=DEV, dtype=f32)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    more = {} if groups is None else dict(groups=groups)
    L.call("e2e_warp_photo_geo_fwd" if groups is None else "e2e_warp_photo_geo_groups_fwd", depth_tgt=L.ptr(t["depth"]), depth_src0=L.ptr(t["dsrc"][0]),
           depth_src1=L.ptr(t["dsrc"][1]), src0=L.ptr(t["src"][0]), src1=L.ptr(t["src"][1]), src_strides=L.strides4(t["src"][0]), tgt=L.ptr(t["tgt"]),
           tgt_strides=L.strides4(t["tgt"]), K=L.ptr(t["K"]), inv_K=L.ptr(t["invK"]), T=L.ptr(t["T"]), tie_noise=L.ptr(t["noise"]), synth=L.ptr(b["synth"]),
           valid=L.ptr(b["valid"]), select=L.ptr(b["select"]), pmap=L.ptr(b["pmap"]), geo_count=L.ptr(b["count"]), use_mask=M.MASK, padding_mode=M.PAD,
           terms=terms, geo_min_valid=gmin, loss_out=L.ptr(b["loss"]), workspace=L.ptr(ws), S=S, B=B, H=H, W=W, stream=L.stream(), **more)
    torch.cuda.synchronize()
    return _cut(b, sizes)


def _backward(L, t, fwd, gl, S, B, H, W, terms, gmin, groups=None, ws_fill=None):
    N = B * H * W
    sizes = dict(g_dt=N, g_ds=S * N, g_T=S * B * 16)
    b = {k: _fill(n) for k, n in sizes.items()}
    ws = torch.empty(L.query("e2e_warp_photo_geo_bwd_workspace_bytes", S, B, H, W) // 8, device=DEV, dtype=torch.float64)
    if ws_fill is not None:
        ws.fill_(ws_fill)
    more = {} if groups is None else dict(groups=groups)
    L.call("e2e_warp_photo_geo_bwd" if groups is None else "e2e_warp_photo_geo_groups_bwd", depth_tgt=L.ptr(t["depth"]), depth_src0=L.ptr(t["dsrc"][0]),
           depth_src1=L.ptr(t["dsrc"][1]), src0=L.ptr(t["src"][0]), src1=L.ptr(t["src"][1]), src_strides=L.strides4(t["src"][0]), tgt=L.ptr(t["tgt"]),
           tgt_strides=L.strides4(t["tgt"]), K=L.ptr(t["K"]), inv_K=L.ptr(t["invK"]), T=L.ptr(t["T"]), synth=L.ptr(fwd["synth"]), valid=L.ptr(fwd["valid"]),
           select=L.ptr(fwd["select"]), geo_count=L.ptr(fwd["count"]), use_mask=M.MASK, padding_mode=M.PAD, terms=terms, geo_min_valid=gmin,
           g_loss=L.ptr(gl), g_depth_tgt=L.ptr(b["g_dt"]), g_depth_src=L.ptr(b["g_ds"]), g_T=L.ptr(b["g_T"]), workspace=L.ptr(ws), S=S, B=B, H=H, W=W,
           stream=L.stream(), **more)
    torch.cuda.synchronize()
    return _cut(b, sizes)


def _close(what, got, r64, bnd, keep=None):
    err = (got.double().cpu().reshape(r64.shape) - r64).abs()
    if keep is not None:
        err = err[keep]
    e = float(err.max()) if err.numel() else 0.0
    print(f"{what}: max|gpu - r64| = {e:.3e}, bound {bnd:.3e}")
    assert e <= bnd, f"{what}: max|gpu - r64| = {e:.3e} > bound {bnd:.3e}"


def _grouped_against_slices(case, gmin, zero_group=None):
    """the grouped pair on the stacked scene against the existing pair on every group's slice -> (grouped fwd, grouped bwd, per-group slices)"""
    L = _L()
    shape, groups, S = case
    Bg, H, W = shape
    B, terms = Bg * groups, G.Wr.terms_of(M.MODE[S])
    t = _device(M.stacked(shape, groups, zero_group), S)
    fwd = _forward(L, t, S, B, H, W, terms, gmin, groups)
    gl = torch.tensor(M.G_LOSS[:1 + S * groups], device=DEV, dtype=f32)
    bwd = _backward(L, t, fwd, gl, S, B, H, W, terms, gmin, groups)
    tag = f"{case} geo_min_valid={gmin}"
    view = dict(synth=(S, B, 3 * H * W), valid=(S, B, H * W), select=(B, H * W), pmap=(B, H * W), g_dt=(B, H * W), g_ds=(S, B, H * W), g_T=(S, B, 16))
    per_item = lambda name, x, lo, hi: x.view(view[name])[lo:hi] if len(view[name]) == 2 else x.view(view[name])[:, lo:hi]
    slices = []
    for g in range(groups):
        lo, hi = g * Bg, (g + 1) * Bg
        ts = _slice(t, lo, hi)
        fs = _forward(L, ts, S, Bg, H, W, terms, gmin)
        for k in ("synth", "valid", "select", "pmap"):
            assert _bits(per_item(k, fwd[k], lo, hi), fs[k].view(-1)), f"{tag}: {k} of group {g} differs from the slice call's"
        for s in range(S):
            assert int(fwd["count"][s * groups + g]) == int(fs["count"][s]), f"{tag}: geo_count[{s} G + {g}]"
            assert _bits(fwd["loss"][1 + s * groups + g], fs["loss"][1 + s]), f"{tag}: loss_out[1 + {s} G + {g}]"
        gls = torch.cat([gl[:1] / groups, torch.stack([gl[1 + s * groups + g] for s in range(S)])]).contiguous()
        bs = _backward(L, ts, fs, gls, S, Bg, H, W, terms, gmin)
        assert _bits(per_item("g_ds", bwd["g_ds"], lo, hi), bs["g_ds"].view(-1)), f"{tag}: g_depth_src of group {g} differs from the slice call's"
        if groups in (1, 2, 4):
            assert _bits(per_item("g_dt", bwd["g_dt"], lo, hi), bs["g_dt"].view(-1)), f"{tag}: g_depth_tgt of group {g} differs from the slice call's"
            assert _bits(per_item("g_T", bwd["g_T"], lo, hi), bs["g_T"].view(-1)), f"{tag}: g_T of group {g} differs from the slice call's"
        slices.append((fs, bs))
    return fwd, bwd, slices


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. slice equality
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=str)
def test_every_group_equals_the_pair_on_its_slice(case):
    shape, groups, S = case
    Bg, H, W = shape
    n = M.counts(shape, groups, S)
    for gmin in [0] + ([M.gate_of(case)] if case in M.GATED else []):
        fwd, bwd, _ = _grouped_against_slices(case, gmin)
        tag = f"{case} geo_min_valid={gmin}"
        assert fwd["count"].tolist() == [n[s][g] for s in range(S) for g in range(groups)], f"{tag}: geo_count against the float64 references"
        refs = [M.group_case(shape, M.SALTS[shape][g], S, gmin, M.group_g_loss(groups, S, g)) for g in range(groups)]
        l64, l32 = (torch.stack([c[dt]["loss"].double() for c in refs]).mean() for dt in (F64, F32))
        _close(f"{tag} loss_out[0]", fwd["loss"][0], l64, R.bound(l32, l64))
        if groups != 3:
            continue
        g_dt, g_T = bwd["g_dt"].view(groups, Bg, H, W), bwd["g_T"].view(S, groups, Bg, 4, 4)
        for g, c in enumerate(refs):                             # no power of two: the scaling of g_loss[0] is not exact, so against float64
            bnd, keep = G.grad_bound(c, "g_depth")
            _close(f"{tag} g_depth_tgt of group {g}", g_dt[g], c[F64]["g_depth"], bnd, keep)
            for k in range(S if G.admitted(c) else 0):
                _close(f"{tag} g_T[{k}] of group {g}", g_T[k, g], c[F64]["g_T"][k], G.grad_bound(c, "g_T", k)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. gates
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.GATED, ids=str)
def test_gates_are_per_group(case):
    shape, groups, S = case
    Bg, H, W = shape
    gmin = M.gate_of(case)
    n = M.counts(shape, groups, S)
    gated_f, gated_b, _ = _grouped_against_slices(case, gmin)
    open_f, open_b, _ = _grouped_against_slices(case, 0)
    is_open = [[n[s][g] > gmin for g in range(groups)] for s in range(S)]
    assert not all(is_open[0]) and any(is_open[0]), "the gated case does not have a closed and an open group of source 0"
    g_ds = [x["g_ds"].view(S, groups, Bg * H * W) for x in (gated_b, open_b)]
    for s in range(S):
        for g in range(groups):
            slot = 1 + s * groups + g
            if is_open[s][g]:                                    # untouched by the neighbours' closed gates
                assert _bits(gated_f["loss"][slot], open_f["loss"][slot]) and float(gated_f["loss"][slot]) > 0
                assert _bits(g_ds[0][s, g], g_ds[1][s, g]) and bool(g_ds[0][s, g].any())
            else:
                assert float(gated_f["loss"][slot]) == 0.0 and not g_ds[0][s, g].any(), f"closed gate of source {s}, group {g}"
    for g in range(groups):                                      # a group all of whose gates are open: every gradient of its items keeps its bits
        if all(is_open[s][g] for s in range(S)):
            for k, per in (("g_dt", (groups, -1)), ("g_T", (S, groups, -1))):
                a, b = gated_b[k].view(per), open_b[k].view(per)
                assert _bits(a[g] if k == "g_dt" else a[:, g], b[g] if k == "g_dt" else b[:, g]), f"{k} of open group {g} moved with a neighbour's gate"


def test_a_group_without_valid_projections_gives_zero_and_finite_gradients():
    shape, groups, S = M.ZERO
    Bg, H, W = shape
    z = M.ZERO_GROUP
    fwd, bwd, _ = _grouped_against_slices(M.ZERO, 0, zero_group=z)
    n = M.counts(shape, groups, S, zero_group=z)
    assert fwd["count"].tolist() == [n[s][g] for s in range(S) for g in range(groups)] and all(n[s][z] == 0 for s in range(S))
    for s in range(S):
        assert float(fwd["loss"][1 + s * groups + z]) == 0.0
        assert not bwd["g_ds"].view(S, groups, -1)[s, z].any()
        assert all(float(fwd["loss"][1 + s * groups + g]) > 0 for g in range(groups) if g != z)
    assert all(bool(torch.isfinite(bwd[k]).all()) for k in BWD_KEYS) and bool(torch.isfinite(fwd["loss"]).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. workspace independence
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_whatever_the_workspace_held():
    L = _L()
    shape, groups, S = (2, 9, 33), 3, 2
    Bg, H, W = shape
    B, terms, gmin = Bg * groups, G.Wr.terms_of(M.MODE[S]), M.gate_of((shape, groups, S))
    t = _device(M.stacked(shape, groups), S)
    gl = torch.tensor(M.G_LOSS[:1 + S * groups], device=DEV, dtype=f32)
    runs = []
    for fill in (0.0, float("nan")):
        fwd = _forward(L, t, S, B, H, W, terms, gmin, groups, ws_fill=fill)
        runs.append({**fwd, **_backward(L, t, fwd, gl, S, B, H, W, terms, gmin, groups, ws_fill=fill)})
    for k in FWD_KEYS + BWD_KEYS:
        assert _bits(runs[0][k], runs[1][k]), f"{k} depends on what the workspace held"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_outputs_alone():
    L = _L()
    S, B, H, W = 2, 4, 4, 6
    N = B * H * W
    img = torch.rand(B, 3, H, W, device=DEV)
    mats = torch.eye(4, device=DEV).repeat(S * B, 1, 1).contiguous()
    big = torch.rand(S * B * 4 * N, device=DEV) + 1
    sel = torch.zeros(N, device=DEV, dtype=i32)
    cnt = torch.full((S * 4,), N, device=DEV, dtype=i32)
    common = dict(depth_tgt=L.ptr(big), depth_src0=L.ptr(big), depth_src1=L.ptr(big), src0=L.ptr(img), src1=L.ptr(img), src_strides=L.strides4(img),
                  tgt=L.ptr(img), tgt_strides=L.strides4(img), K=L.ptr(mats), inv_K=L.ptr(mats), T=L.ptr(mats), use_mask=1, padding_mode=1, terms=6,
                  geo_min_valid=0, S=S, B=B, H=H, W=W, stream=L.stream())
    f = dict(synth=_fill(3 * S * N), valid=_fill(S * N), select=_fill(N, i32), pmap=_fill(N), count=_fill(S * 4, i32), loss=_fill(1 + S * 4),
             ws=_fill(L.query("e2e_warp_photo_geo_workspace_floats", S, B, H, W)))
    g = dict(g_dt=_fill(N), g_ds=_fill(S * N), g_T=_fill(S * B * 16), ws=_fill(L.query("e2e_warp_photo_geo_bwd_workspace_bytes", S, B, H, W) // 8, i64))
    fwd = dict(common, tie_noise=L.ptr(big), synth=L.ptr(f["synth"]), valid=L.ptr(f["valid"]), select=L.ptr(f["select"]), pmap=L.ptr(f["pmap"]),
               geo_count=L.ptr(f["count"]), loss_out=L.ptr(f["loss"]), workspace=L.ptr(f["ws"]))
    bwd = dict(common, synth=L.ptr(big), valid=L.ptr(big), select=L.ptr(sel), geo_count=L.ptr(cnt), g_loss=L.ptr(big), g_depth_tgt=L.ptr(g["g_dt"]),
               g_depth_src=L.ptr(g["g_ds"]), g_T=L.ptr(g["g_T"]), workspace=L.ptr(g["ws"]))
    refused = 0
    for name, args, outs in (("e2e_warp_photo_geo_groups_fwd", fwd, f), ("e2e_warp_photo_geo_groups_bwd", bwd, g)):
        for change, message in ((dict(groups=0), "groups"), (dict(groups=5), "groups"), (dict(groups=-1), "groups"), (dict(groups=3), "multiple"),
                                (dict(groups=2, B=3), "multiple"), (dict(groups=9, geo_min_valid=-1), "geo_min_valid"), (dict(groups=9, S=3), "S=3"),
                                (dict(groups=9, depth_src0=None), "null pointer"), (dict(groups=3, terms=8), "terms")):
            with pytest.raises(L.E2EError, match=rf"{name} failed \(-1\).*{message}"):          # E2E_ERR_ARG
                L.call(name, **{"groups": 2, **args, **change})
            torch.cuda.synchronize()
            assert all(_untouched(o) for o in outs.values()), f"{name} {change}: an output changed although the call was refused"
            refused += 1
    assert refused == 18
    for groups in (1, 2, 4):                                     # the vectors themselves are good calls
        L.call("e2e_warp_photo_geo_groups_fwd", groups=groups, **fwd)
        L.call("e2e_warp_photo_geo_groups_bwd", groups=groups, **bwd)
    torch.cuda.synchronize()
    assert not torch.isnan(f["loss"][:1 + S * 4]).any() and not torch.isnan(g["g_ds"][:S * N]).any()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. groups = 1 is the existing pair
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", G.MODES, ids=str)
def test_one_group_is_the_existing_pair_bit_for_bit(mode):
    L = _L()
    shape = (2, 9, 33)
    (B, H, W), S, terms = shape, mode[0], G.Wr.terms_of(mode)
    t = _device(G.scene(*shape), S)
    gl = torch.tensor(G.G_LOSS[:1 + S], device=DEV, dtype=f32)
    for gmin in (0, G.N_VALID[shape][0]):
        old_f = _forward(L, t, S, B, H, W, terms, gmin)
        new_f = _forward(L, t, S, B, H, W, terms, gmin, groups=1)
        old_b = _backward(L, t, old_f, gl, S, B, H, W, terms, gmin)
        new_b = _backward(L, t, new_f, gl, S, B, H, W, terms, gmin, groups=1)
        for k in FWD_KEYS:
            assert _bits(old_f[k], new_f[k]), f"mode {mode} geo_min_valid={gmin}: {k}"
        for k in BWD_KEYS:
            assert _bits(old_b[k], new_b[k]), f"mode {mode} geo_min_valid={gmin}: {k}"
