"""The twelve entry points of csrc/warp_photo.hip, called directly through the C ABI, against float64 references of the contracts that
include/e2eslam.h states (oracle.warp_loss and torch's grid_sample on the CPU, gradients by autograd; tests/warp_contract_ref.py):

  A. e2e_backproject_fwd / _bwd: an independent upstream gradient on all four rows, depths that are zero and negative, one block past the launch cap;
  B. e2e_project3d_fwd / _bwd: w in {1, 0.5, 2}, points behind the camera and on both sides of z_out's clamp, z_out / g_z NULL and not;
  C. e2e_grid_sample_fwd / _bwd / _bwd_exact: Hi,Wi != Ho,Wo, four memory layouts, both paddings and alignments, g_input of both backward forms,
     the second trip of the sampling loops and of the fixed-point conversion;
  D. e2e_photometric_fwd / _bwd: axes of length 2 and 3, all-zero windows, y == x, C in {1, 3, 4}, every combination of outputs and upstream gradients;
  E. e2e_warp_photo_workspace_floats, e2e_warp_photo_fwd / _bwd against the float64 composition, each half of g_depth_tgt alone;
  F. the calls the header rules out: E2EError before any launch, every output as it was.

Every float output is NaN-filled, every integer buffer poisoned, each followed by a 64-element sentinel; the workspace and g_input_fixed are
allocated at exactly their documented sizes.  After each call: all of the output written, nothing behind it touched, a second call bit-identical
(g_input of e2e_grid_sample_bwd, which uses float atomics, by value only).

Bounds and exclusions come from the references alone (tests/warp_contract_ref.py states the rule and the two places where it had to be read);
tests/test_warp_contract_inputs.py proves the excluded shares and the planted edges without a GPU.  profiles/warp_contracts.txt holds the
measured errors as fractions of their bounds."""
import pytest
import torch

import warp_contract_ref as R
from warp_contract_ref import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
POISON = -0x5A5A5A5A5A5A5A5A
WORST = {}


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print()
    for section, name in sorted(WORST):
        ratio, e, bnd, what = WORST[section, name]
        print(f"warp contracts {section} {name}: largest error / bound = {ratio:.3f} ({e:.2e} of {bnd:.2e} at {what})")


def _nan(n):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=torch.float32)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _dev(t):
    return t.contiguous().to(DEV)


def _run2(launch, sizes, atomics=()):
    """launch(bufs) twice on fresh NaN-filled buffers of the given sizes (None: the output is not requested, NULL is passed); every buffer
    fully written, its sentinel intact, the two runs bit-identical -> {name: CPU tensor of the first run}"""
    runs = []
    for _ in range(2):
        bufs = {k: None if n is None else _nan(n) for k, n in sizes.items()}
        launch(bufs)
        torch.cuda.synchronize()
        for k, n in sizes.items():
            if n is not None:
                _written(bufs[k], n, k)
        runs.append(bufs)
    for k, n in sizes.items():
        if n is not None and k not in atomics:
            assert _same_bits(runs[0][k], runs[1][k]), f"{k}: two identical calls differ"
    return {k: None if n is None else runs[0][k][:n].cpu() for k, n in sizes.items()}


def _check(section, what, dev, r64, bnd, keep=None):
    err = (dev.double().reshape(r64.shape) - r64).abs()
    if keep is not None:
        err = err[keep]
    e = float(err.max()) if err.numel() else 0.0
    ratio = e / bnd if bnd > 0 else (0.0 if e == 0 else float("inf"))
    key = (section, what.split(" | ")[-1].split(",")[0])
    if ratio >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (ratio, e, bnd, what)
    assert e <= bnd, f"{section} {what}: max|gpu - r64| = {e:.3e} > bound {bnd:.3e} ({ratio:.2f} x)"


def _cmp(section, what, dev, case, key, keep=None):
    _check(section, what, dev, case[F64][key], R.bound(case[F32][key], case[F64][key], keep), keep)


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. backproject
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.BHW_SHAPES, ids=str)
def test_backproject(shape):
    L = _L()
    B, H, W = shape
    N = H * W
    c = R.backproject_case(*shape)
    depth, invK, g_cam = _dev(c["depth"]), _dev(c["invK"]), _dev(c["g_cam"])
    out = _run2(lambda b: L.call("e2e_backproject_fwd", L.ptr(depth), L.ptr(invK), L.ptr(b["cam"]), B, H, W, L.stream()), dict(cam=B * 4 * N))
    cam = out["cam"].view(B, 4, N)
    assert (cam[:, 3] == 1).all(), "row 3 of cam_points is not exactly 1"
    _check("A", f"{shape} | cam", cam[:, :3], c[F64]["cam"][:, :3], R.bound(c[F32]["cam"][:, :3], c[F64]["cam"][:, :3]))
    out = _run2(lambda b: L.call("e2e_backproject_bwd", L.ptr(g_cam), L.ptr(invK), L.ptr(b["g"]), B, H, W, L.stream()), dict(g=B * N))
    _cmp("A", f"{shape} | g_depth", out["g"], c, "g_depth")
    g_cam3 = g_cam.clone()
    g_cam3[:, 3] = 1e6 * (1 + g_cam[:, 3].abs())                      # row 3 of the upstream gradient must not reach g_depth
    again = _run2(lambda b: L.call("e2e_backproject_bwd", L.ptr(g_cam3), L.ptr(invK), L.ptr(b["g"]), B, H, W, L.stream()), dict(g=B * N))
    assert _same_bits(again["g"], out["g"]), "g_depth depends on row 3 of g_cam"


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. project3d
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.BHW_SHAPES, ids=str)
def test_project3d(shape):
    """Divergence that is the reference's own: none found.  (NaN in max|grid| <= 1 would be one -- torch's max propagates NaN, fmaxf does not --
    but no case feeds a non-finite input.)"""
    L = _L()
    B, H, W = shape
    N = H * W
    c = R.project_case(*shape)
    r64, r32 = c[F64], c[F32]
    pts, K, T, g_grid, g_z = (_dev(c[k]) for k in ("points", "K", "T", "g_grid", "g_z"))
    groups = [("ordinary", ~c["near"])] + ([("clamp-side", c["near"])] if c["near"].any() else [])
    first = None
    for with_z in (True, False):
        out = _run2(lambda b: L.call("e2e_project3d_fwd", L.ptr(pts), L.ptr(K), L.ptr(T), L.ptr(b["grid"]), L.ptr(b["valid"]), L.ptr(b["z"]), B, H, W, L.stream()),
                    dict(grid=B * N * 2, valid=B * N, z=B * N if with_z else None))
        grid, valid = out["grid"].view(B, N, 2), out["valid"].view(B, N)
        if first is None:
            first = out
        else:
            assert _same_bits(out["grid"], first["grid"]) and _same_bits(out["valid"], first["valid"]), "grid / valid depend on z_out"
        assert ((valid == 0) | (valid == 1)).all()
        off_band = ~c["valid_band"]
        assert torch.equal(valid[off_band], r64["valid"][off_band]), f"{shape}: valid differs from the reference off the band of max|grid| = 1"
        for name, grp in groups:
            g2 = grp[..., None].expand(B, N, 2)
            _check("B", f"{shape} | grid, {name}", grid, r64["grid"].view(B, N, 2), R.bound(r32["grid"].view(B, N, 2), r64["grid"].view(B, N, 2), g2), g2)
            if with_z:
                _check("B", f"{shape} | z_out, {name}", out["z"].view(B, N), r64["z"], R.bound(r32["z"], r64["z"], grp), grp)
    for key, gz in (("g_points_z", g_z), ("g_points", None)):
        out = _run2(lambda b: L.call("e2e_project3d_bwd", L.ptr(pts), L.ptr(K), L.ptr(T), L.ptr(g_grid), L.ptr(gz), L.ptr(b["g"]), B, H, W, L.stream()), dict(g=B * 4 * N))
        g = out["g"].view(B, 4, N)
        for name, grp in groups:
            keep = (grp & ~c["gate_band"] if gz is not None else grp)[:, None].expand(B, 4, N)
            _check("B", f"{shape} | {key}, {name}", g, r64[key], R.bound(r32[key], r64[key], keep), keep)
            w_row = torch.zeros_like(keep)
            w_row[:, 3] = keep[:, 3]                                  # the w row against its own scale: its entries are the smallest
            _check("B", f"{shape} | {key} row w, {name}", g, r64[key], R.bound(r32[key], r64[key], w_row), w_row)


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. grid_sample
# ---------------------------------------------------------------------------------------------------------------------------------------
def _grid_sample(shape, layout, pad, align):
    L = _L()
    B, C, Hi, Wi, Ho, Wo = shape
    No, Ni = Ho * Wo, Hi * Wi
    c = R.grid_sample_case(shape, layout, pad, align)
    tag = f"{shape} {layout} {R.PAD_NAME[pad]} align={align}"
    inp = R.layout_view(layout, _dev(c["base"]), B)
    assert inp.stride() == R.layout_view(layout, c["base"], B).stride()
    st, grid, g_out = L.strides4(inp), _dev(c["grid"]), _dev(c["g_out"])
    dims = (B, C, Hi, Wi, Ho, Wo, pad, align, L.stream())
    out = _run2(lambda b: L.call("e2e_grid_sample_fwd", L.ptr(inp), st, L.ptr(grid), L.ptr(b["out"]), *dims), dict(out=B * C * No))
    _cmp("C", f"{tag} | out", out["out"], c, "out")                      # on the planted pixel centres and +-1 too: the function is continuous
    keep = c["keep"]
    # g_input NULL
    out = _run2(lambda b: L.call("e2e_grid_sample_bwd", L.ptr(inp), st, L.ptr(grid), L.ptr(g_out), L.ptr(b["g_grid"]), None, *dims), dict(g_grid=B * No * 2))
    _cmp("C", f"{tag} | g_grid", out["g_grid"], c, "g_grid", keep)
    g_grid0 = out["g_grid"]

    def zeroed(b):                                                     # the float-atomic form wants its g_input zeroed
        b["g_input"][:B * C * Ni] = 0
        L.call("e2e_grid_sample_bwd", L.ptr(inp), st, L.ptr(grid), L.ptr(g_out), L.ptr(b["g_grid"]), L.ptr(b["g_input"]), *dims)
    out = _run2(zeroed, dict(g_grid=B * No * 2, g_input=B * C * Ni), atomics=("g_input",))
    assert _same_bits(out["g_grid"], g_grid0), f"{tag}: g_grid depends on g_input"
    _cmp("C", f"{tag} | g_input (float atomics)", out["g_input"], c, "g_input")
    # the fixed-point form: scratch of exactly B*C*Hi*Wi + 1 words, then the sentinel
    fixed = []

    def exact(b):
        fx = torch.full((B * C * Ni + 1 + SENTINEL,), POISON, device=DEV, dtype=torch.int64)
        fixed.append(fx)
        L.call("e2e_grid_sample_bwd_exact", L.ptr(inp), st, L.ptr(grid), L.ptr(g_out), L.ptr(b["g_grid"]), L.ptr(fx), L.ptr(b["g_input"]), *dims)
    out = _run2(exact, dict(g_grid=B * No * 2, g_input=B * C * Ni))
    for fx in fixed:
        assert (fx[B * C * Ni + 1:] == POISON).all(), f"{tag}: g_input_fixed written past its B*C*Hi*Wi + 1 words"
        assert int(fx[B * C * Ni]) == 0, f"{tag}: the poison word is raised for in-range input"
    assert torch.equal(fixed[0], fixed[1])
    assert _same_bits(out["g_grid"], g_grid0), f"{tag}: g_grid of the exact form differs"
    _cmp("C", f"{tag} | g_input (fixed point)", out["g_input"], c, "g_input")


@pytest.mark.parametrize("shape,layout", R.GS_CASES, ids=str)
def test_grid_sample(shape, layout):
    for pad in (0, 1):
        for align in (0, 1):
            _grid_sample(shape, layout, pad, align)


@pytest.mark.parametrize("pad,align", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_grid_sample_second_trip_of_the_sampling_loops(pad, align):
    _grid_sample(R.GS_LOOP, "nchw", pad, align)


def test_grid_sample_second_trip_of_the_fixed_point_conversion():
    _grid_sample(R.GS_CONVERT, "nchw", 1, 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. photometric
# ---------------------------------------------------------------------------------------------------------------------------------------
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


@pytest.mark.parametrize("kind", R.PH_KINDS)
@pytest.mark.parametrize("shape", R.PH_SHAPES, ids=str)
def test_photometric(shape, kind):
    """y == x: every reference tensor is identically zero, in float32 too, and the bound is the cap at the companion case's scale
    (tests/warp_contract_ref.py says why)."""
    L = _L()
    B, C, H, W = shape
    n1, nC = B * H * W, B * C * H * W
    c = R.photometric_case(shape, kind)
    r64, bnd = c[F64], c["bound"]
    g_pmap, g_ssim = _dev(c["g_pmap"]), _dev(c["g_ssim"])
    dims = (B, C, H, W, L.stream())
    ref_bits = {}
    for lx in ("nchw", "nhwc"):
        for ly in ("nchw", "nhwc"):
            x = _dev(c["x"]) if lx == "nchw" else _nhwc(c["x"].to(DEV))
            y = _dev(c["y"]) if ly == "nchw" else _nhwc(c["y"].to(DEV))
            xs, ys = L.strides4(x), L.strides4(y)
            tag = f"{shape} {kind} x {lx} y {ly}"
            for want in ("s", "p", "sp"):
                out = _run2(lambda b: L.call("e2e_photometric_fwd", L.ptr(x), xs, L.ptr(y), ys, L.ptr(b["ssim"]), L.ptr(b["pmap"]), *dims),
                            dict(ssim=nC if "s" in want else None, pmap=n1 if "p" in want else None))
                for k in ("ssim", "pmap"):
                    if out[k] is not None:
                        _check("D", f"{tag} | {k}", out[k], r64[k], bnd[k])
                        assert _same_bits(out[k], ref_bits.setdefault(k, out[k])), f"{tag}: {k} depends on the layout or on which outputs are requested"
            for up in R.PH_UPSTREAM:
                gp, gs = g_pmap if "p" in up else None, g_ssim if "s" in up else None
                keep = ~c["excluded"][up]
                out = _run2(lambda b: L.call("e2e_photometric_bwd", L.ptr(x), xs, L.ptr(y), ys, L.ptr(gp), L.ptr(gs), L.ptr(b["g"]), *dims), dict(g=nC))
                _check("D", f"{tag} | g_x, upstream {up}", out["g"], r64["gx_" + up], bnd["gx_" + up], keep)
                assert _same_bits(out["g"], ref_bits.setdefault("gx_" + up, out["g"])), f"{tag}: g_x depends on the layout"
                out = _run2(lambda b: L.call("e2e_photometric_bwd", L.ptr(y), ys, L.ptr(x), xs, L.ptr(gp), L.ptr(gs), L.ptr(b["g"]), *dims), dict(g=nC))
                _check("D", f"{tag} | g_y (operands swapped), upstream {up}", out["g"], r64["gy_" + up], bnd["gy_" + up], keep)


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. the fused pair and its workspace query
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_query():
    L = _L()
    for B, H, W in R.FUSED_SHAPES + [(3, 8, 32), (1, 480, 640)]:
        assert L.query("e2e_warp_photo_workspace_floats", B, H, W) == 2 * B * -(-H // 8) * -(-W // 32)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert L.query("e2e_warp_photo_workspace_floats", *bad) == 0


@pytest.mark.parametrize("pad", (0, 1), ids=lambda p: R.PAD_NAME[p])
@pytest.mark.parametrize("shape", R.FUSED_SHAPES, ids=str)
def test_warp_photo_pair(shape, pad):
    L = _L()
    B, H, W = shape
    N = B * H * W
    s = R.fused_scene(*shape)
    depth, d_src, ri_t, ri_s, K, invK, T = (_dev(s[k]) for k in ("depth", "d_src", "ri_t", "ri_s", "K", "invK", "T"))
    nws = L.query("e2e_warp_photo_workspace_floats", B, H, W)
    for use_mask in (0, 1):
        for reg_kind in (0, 1, 2):
            c = R.fused_case(shape, pad, use_mask, reg_kind)
            r64, r32 = c[F64], c[F32]
            assert not c["valid_band"].any()
            reg = (L.ptr(ri_t), L.ptr(ri_s), L.ptr(d_src)) if reg_kind else (None, None, None)
            fwd_bits = None
            for with_pmap in (True, False):
                src = _dev(s["src"]) if with_pmap else _nhwc(s["src"].to(DEV))       # NCHW and NHWC memory, turn about
                tgt = _nhwc(s["tgt"].to(DEV)) if with_pmap else _dev(s["tgt"])
                ss, ts = L.strides4(src), L.strides4(tgt)
                tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} reg={reg_kind} pmap={'yes' if with_pmap else 'NULL'}"
                ws = []

                def fwd(b):
                    ws.append(_nan(nws))
                    loss = b["loss"]
                    L.call("e2e_warp_photo_fwd", L.ptr(depth), L.ptr(src), ss, L.ptr(tgt), ts, L.ptr(K), L.ptr(invK), L.ptr(T), L.ptr(b["synth"]), L.ptr(b["valid"]),
                           L.ptr(b["pmap"]), use_mask, pad, reg_kind, *reg, L.ptr(loss), L.ptr(ws[-1]), B, H, W, L.stream())
                    if not reg_kind:                                  # loss_out[1] belongs to the regulariser: the header promises nothing about it without one
                        torch.cuda.synchronize()
                        loss[1] = 0.0
                out = _run2(fwd, dict(synth=3 * N, valid=N, pmap=N if with_pmap else None, loss=2))
                for w in ws:
                    assert torch.isnan(w[nws:]).all(), f"{tag}: workspace written past the size its query returned"
                    assert not torch.isnan(w[:nws // 2 * (2 if reg_kind else 1)]).any()
                if fwd_bits is None:
                    fwd_bits = out
                else:
                    assert all(_same_bits(out[k], fwd_bits[k]) for k in ("synth", "valid", "loss")), f"{tag}: outputs depend on pmap being requested or on the layout"
                assert torch.equal(out["valid"].view(B, H, W), r64["valid"]), f"{tag}: valid"
                _cmp("E", f"{tag} | synth", out["synth"], c, "synth")
                if with_pmap:
                    _cmp("E", f"{tag} | pmap", out["pmap"], c, "pmap", ~c["pmap_excluded"])
                _cmp("E", f"{tag} | loss_out[0]", out["loss"][0], c, "loss")
                if reg_kind:
                    _cmp("E", f"{tag} | loss_out[1]", out["loss"][1], c, "reg")
            synth, valid = _dev(fwd_bits["synth"]), _dev(fwd_bits["valid"])
            src, tgt = _dev(s["src"]), _nhwc(s["tgt"].to(DEV))
            ss, ts = L.strides4(src), L.strides4(tgt)
            for g_loss in R.G_LOSS:
                tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} reg={reg_kind} g_loss={g_loss}"
                gl = torch.tensor(g_loss, device=DEV, dtype=torch.float32)
                out = _run2(lambda b: L.call("e2e_warp_photo_bwd", L.ptr(depth), L.ptr(src), ss, L.ptr(tgt), ts, L.ptr(K), L.ptr(invK), L.ptr(T), L.ptr(synth), L.ptr(valid),
                                             use_mask, pad, reg_kind, *reg, L.ptr(gl), L.ptr(b["g_dt"]), L.ptr(b["g_ds"]), B, H, W, L.stream()),
                            dict(g_dt=N, g_ds=N if reg_kind else None))
                (t64, s64), (t32, s32) = R.fused_grads(c, g_loss, F64), R.fused_grads(c, g_loss, F32)
                keep = ~(c["grad_excluded"] | (c["reg_excluded_t"] if g_loss[1] else torch.zeros_like(c["grad_excluded"])))
                _check("E", f"{tag} | g_depth_tgt", out["g_dt"], t64, R.fused_grad_bound(c, g_loss, keep), keep)
                if reg_kind:
                    _check("E", f"{tag} | g_depth_src", out["g_ds"], s64, R.bound(s32, s64, ~c["reg_excluded_s"]), ~c["reg_excluded_s"])
            if not reg_kind:                                          # g_depth_src given although there is no regulariser: it stays as it was
                g_ds, g_dt = _nan(N), _nan(N)
                L.call("e2e_warp_photo_bwd", L.ptr(depth), L.ptr(src), ss, L.ptr(tgt), ts, L.ptr(K), L.ptr(invK), L.ptr(T), L.ptr(synth), L.ptr(valid),
                       use_mask, pad, 0, None, None, None, L.ptr(gl), L.ptr(g_dt), L.ptr(g_ds), B, H, W, L.stream())
                torch.cuda.synchronize()
                assert torch.isnan(g_ds).all(), "g_depth_src written although reg_kind = 0"
                _written(g_dt, N, "g_depth_tgt")


# ---------------------------------------------------------------------------------------------------------------------------------------
# F. what the header rules out: an error before any launch, every output as it was
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_outputs_alone():
    L = _L()
    B, C, H, W = 2, 3, 4, 6
    N = B * H * W
    st = L.stream()
    img = torch.rand(B, C, H, W, device=DEV)
    s4 = L.strides4(img)
    i_ = L.ptr(img)
    mats = torch.eye(4, device=DEV).repeat(B, 1, 1).contiguous()
    m_ = L.ptr(mats)
    big = torch.rand(B * 4 * N, device=DEV)                            # any read-only (B,H,W)-sized or larger operand
    r_ = L.ptr(big)
    outs = [_nan(B * 4 * N) for _ in range(4)]
    o0, o1, o2, o3 = (L.ptr(o) for o in outs)
    fx = torch.full((B * C * H * W + 1 + SENTINEL,), POISON, device=DEV, dtype=torch.int64)
    f_ = L.ptr(fx)
    count = [0]

    def refused(name, *args):
        with pytest.raises(L.E2EError, match=name):
            L.call(name, *args)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs) and bool((fx == POISON).all()), f"{name}: an output changed although the call was refused"
        count[0] += 1

    def each_null(name, args, required):
        for k in required:
            refused(name, *[None if j == k else a for j, a in enumerate(args)])

    def each_dim(name, args, at, bad):
        for k, values in zip(at, bad):
            for v in values:
                refused(name, *[v if j == k else a for j, a in enumerate(args)])

    hw = ((0, -1), (0, 1), (0, 1))                                     # B <= 0; H, W of 0 and of 1
    a = [r_, m_, o0, B, H, W, st]
    for name in ("e2e_backproject_fwd", "e2e_backproject_bwd"):
        each_null(name, a, (0, 1, 2))
        each_dim(name, a, (3, 4, 5), hw)
    a = [r_, m_, m_, o0, o1, o2, B, H, W, st]
    each_null("e2e_project3d_fwd", a, (0, 1, 2, 3, 4))
    each_dim("e2e_project3d_fwd", a, (6, 7, 8), hw)
    a = [r_, m_, m_, r_, r_, o0, B, H, W, st]
    each_null("e2e_project3d_bwd", a, (0, 1, 2, 3, 5))
    each_dim("e2e_project3d_bwd", a, (6, 7, 8), hw)
    pos = ((0, -1),) * 6 + ((2, -1),)                                  # B, C, Hi, Wi, Ho, Wo <= 0; padding mode 2 (reflection) and -1
    a = [i_, s4, r_, o0, B, C, H, W, H, W, 1, 0, st]
    each_null("e2e_grid_sample_fwd", a, (0, 2, 3))
    each_dim("e2e_grid_sample_fwd", a, (4, 5, 6, 7, 8, 9, 10), pos)
    a = [i_, s4, r_, r_, o0, o1, B, C, H, W, H, W, 1, 0, st]
    each_null("e2e_grid_sample_bwd", a, (0, 2, 3, 4))
    each_dim("e2e_grid_sample_bwd", a, (6, 7, 8, 9, 10, 11, 12), pos)
    a = [i_, s4, r_, r_, o0, f_, o1, B, C, H, W, H, W, 1, 0, st]
    each_null("e2e_grid_sample_bwd_exact", a, (0, 2, 3, 4, 5, 6))
    each_dim("e2e_grid_sample_bwd_exact", a, (7, 8, 9, 10, 11, 12, 13), pos)
    chw = ((0, -1), (0, -1), (0, 1), (0, 1))                           # B <= 0, C <= 0, H / W of 0 and 1
    a = [i_, s4, i_, s4, o0, o1, B, C, H, W, st]
    each_null("e2e_photometric_fwd", a, (0, 2))
    refused("e2e_photometric_fwd", i_, s4, i_, s4, None, None, B, C, H, W, st)             # both outputs NULL
    each_dim("e2e_photometric_fwd", a, (6, 7, 8, 9), chw)
    a = [i_, s4, i_, s4, r_, r_, o0, B, C, H, W, st]
    each_null("e2e_photometric_bwd", a, (0, 2, 6))
    refused("e2e_photometric_bwd", i_, s4, i_, s4, None, None, o0, B, C, H, W, st)         # both upstream gradients NULL
    each_dim("e2e_photometric_bwd", a, (7, 8, 9, 10), chw)
    a = [r_, i_, s4, i_, s4, m_, m_, m_, o0, o1, o2, 1, 1, 2, r_, r_, r_, o3, L.ptr(outs[3][8:]), B, H, W, st]
    each_null("e2e_warp_photo_fwd", a, (0, 1, 3, 5, 6, 7, 8, 9, 17, 18))
    each_null("e2e_warp_photo_fwd", a, (14, 15, 16))                  # a regulariser buffer missing with reg_kind = 2
    each_dim("e2e_warp_photo_fwd", a, (12, 13, 19, 20, 21), ((2, -1), (3, -1)) + hw)
    a = [r_, i_, s4, i_, s4, m_, m_, m_, r_, r_, 1, 1, 1, r_, r_, r_, r_, o0, o1, B, H, W, st]
    each_null("e2e_warp_photo_bwd", a, (0, 1, 3, 5, 6, 7, 8, 9, 16, 17))
    each_null("e2e_warp_photo_bwd", a, (13, 14, 15, 18))              # with reg_kind = 1 g_depth_src is required as well
    each_dim("e2e_warp_photo_bwd", a, (11, 12, 19, 20, 21), ((2, -1), (3, -1)) + hw)
    print(f"\nF: {count[0]} refused calls, every output left as it was")
    assert count[0] >= 150
