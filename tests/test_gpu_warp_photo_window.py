"""e2e_warp_photo_window_fwd / _bwd (csrc/warp_photo_window.hip) and what is built on them: the fused warp-photometric pair over a window of
one or two source frames with the candidate / minimum logic of train_depth.py:621-662, against float64.

  1. the entry points: loss, pmap, select, synth / valid per source, g_depth_tgt, and g_T on the admitted cases, for every mode, padding, mask
     setting and both memory layouts; two runs bit-identical; every output and workspace written exactly to its size; g_T = NULL gives the same
     g_depth_tgt bits; a crafted case in which each source's pose gets gradient only from the pixels it won;
  2. the size queries and every refused call;
  3. ops.warp_photometric_window: depth and T.grad against float64 and the operator chain inside the same bounds, an expanded (4,4) pose, the
     detached route, K refused, S = 1 without flags against ops.warp_photometric;
  4. Depth_Estimation at 64x96: the three-frame window and the flagged terms run on the window entry points (this fails on the parent commit),
     agree with oracle.train_depth and with fused_losses=False; with estimated poses both poses receive a gradient; the default two-frame
     configuration still launches e2e_warp_photo_fwd.

Bounds come from the references alone (tests/warp_window_ref.py); tests/test_warp_window_inputs.py proves the cases without a GPU."""
import contextlib
import io

import numpy as np
import pytest
import torch

import warp_contract_ref as R
import warp_pose_ref as P
import warp_window_ref as Wr
from warp_contract_ref import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
INT_SENTINEL = -123456789
WORST = {}


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
        print(f"warp window {name}: largest error / bound = {ratio:.3f} ({e:.2e} of {bnd:.2e} at {what})")


def _nan(n, dtype=torch.float32):
    if dtype == torch.int32:
        return torch.full((n + SENTINEL,), INT_SENTINEL, device=DEV, dtype=dtype)
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _untouched(buf):
    return bool((buf == INT_SENTINEL).all()) if buf.dtype == torch.int32 else bool(torch.isnan(buf).all())


def _written(buf, n, what):
    assert _untouched(buf[n:]), f"{what}: written past the end"
    bad = (buf[:n] == INT_SENTINEL) if buf.dtype == torch.int32 else torch.isnan(buf[:n])
    assert not bad.any(), f"{what}: {int(bad.sum())} of {n} elements not written"


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


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


def _run2(launch, sizes):
    """launch(bufs) twice on fresh sentinel-filled buffers {name: (n, dtype)} (n None: NULL is passed); every buffer fully written, nothing
    behind it, the two runs bit-identical -> the buffers of the first run, cut to size"""
    runs = []
    for _ in range(2):
        bufs = {k: None if n is None else _nan(n, dt) for k, (n, dt) in sizes.items()}
        launch(bufs)
        torch.cuda.synchronize()
        for k, (n, _dt) in sizes.items():
            if n is not None:
                _written(bufs[k], n, k)
        runs.append(bufs)
    for k, (n, _dt) in sizes.items():
        if n is not None:
            a, b = runs[0][k], runs[1][k]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{k}: two identical calls differ"
    return {k: None if n is None else runs[0][k][:n] for k, (n, _dt) in sizes.items()}


def _device(s, S, Ts=None, srcs=None, layout="nchw"):
    B = s["B"]
    Ts = s["T"] if Ts is None else Ts
    t = {k: s[k].contiguous().to(DEV) for k in ("depth", "K", "invK")}
    t["T"] = torch.stack([(T.expand(B, 4, 4) if T.dim() == 2 else T) for T in Ts[:S]]).contiguous().to(DEV)
    srcs = s["src"] if srcs is None else srcs
    t["src"] = [x.contiguous().to(DEV) if layout == "nchw" else _nhwc(x.to(DEV)) for x in srcs[:S]] + [None] * (2 - S)
    t["tgt"] = _nhwc(s["tgt"].to(DEV)) if layout == "nchw" else s["tgt"].contiguous().to(DEV)      # the target the other way round
    t["noise"] = s["noise"][:, :S].contiguous().to(DEV)
    return t


def _fwd_args(L, t, b, use_mask, pad, terms, S, B, H, W):
    return (L.ptr(t["depth"]), L.ptr(t["src"][0]), L.ptr(t["src"][1]), L.strides4(t["src"][0]), L.ptr(t["tgt"]), L.strides4(t["tgt"]), L.ptr(t["K"]),
            L.ptr(t["invK"]), L.ptr(t["T"]), L.ptr(t["noise"]), L.ptr(b["synth"]), L.ptr(b["valid"]), L.ptr(b["select"]), L.ptr(b["pmap"]), use_mask, pad,
            terms, L.ptr(b["loss"]), L.ptr(b["ws"]), S, B, H, W, L.stream())


def _bwd_args(L, t, fwd, gl, b, use_mask, pad, terms, S, B, H, W, pose=True):
    return (L.ptr(t["depth"]), L.ptr(t["src"][0]), L.ptr(t["src"][1]), L.strides4(t["src"][0]), L.ptr(t["tgt"]), L.strides4(t["tgt"]), L.ptr(t["K"]),
            L.ptr(t["invK"]), L.ptr(t["T"]), L.ptr(fwd["synth"]), L.ptr(fwd["valid"]), L.ptr(fwd["select"]), use_mask, pad, terms, L.ptr(gl),
            L.ptr(b["g_dt"]), L.ptr(b["g_T"]) if pose else None, L.ptr(b["ws"]) if pose else None, S, B, H, W, L.stream())


def _fwd_sizes(L, S, B, H, W, with_pmap=True):
    N = B * H * W
    f32, i32 = torch.float32, torch.int32
    return dict(synth=(3 * S * N, f32), valid=(S * N, f32), select=(N, i32), pmap=(N if with_pmap else None, f32), loss=(1, f32),
                ws=(L.query("e2e_warp_photo_window_workspace_floats", S, B, H, W), f32))


def _bwd_sizes(L, S, B, H, W, pose=True):
    N = B * H * W
    nws = L.query("e2e_warp_photo_window_bwd_workspace_bytes", S, B, H, W)
    return dict(g_dt=(N, torch.float32), g_T=(S * B * 16 if pose else None, torch.float32), ws=(nws // 8 if pose else None, torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the entry points against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", (0, 1), ids=lambda p: R.PAD_NAME[p])
@pytest.mark.parametrize("shape", Wr.SHAPES, ids=str)
def test_entry_points(shape, pad):
    L = _L()
    B, H, W = shape
    N = B * H * W
    s = Wr.scene(*shape)
    gl = torch.tensor([Wr.G_LOSS], device=DEV, dtype=torch.float32)
    for use_mask in (0, 1):
        for mode in Wr.MODES:
            S, terms = mode[0], Wr.terms_of(mode)
            c = Wr.window_case(shape, pad, use_mask, mode)
            r64, r32, b64, b32 = c[F64], c[F32], c["base"][F64], c["base"][F32]
            first = None
            for layout in ("nchw", "nhwc"):
                with_pmap = layout == "nchw"
                tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} mode={mode} src {layout}"
                t = _device(s, S, layout=layout)
                fwd = _run2(lambda b: L.call("e2e_warp_photo_window_fwd", *_fwd_args(L, t, b, use_mask, pad, terms, S, B, H, W)),
                            _fwd_sizes(L, S, B, H, W, with_pmap))
                if first is None:
                    first = fwd
                else:
                    assert all(_same_bits(fwd[k], first[k]) for k in ("synth", "valid", "select", "loss")), f"{tag}: outputs depend on the layout or on pmap"
                synth, valid = fwd["synth"].view(S, B, 3, H, W).cpu(), fwd["valid"].view(S, B, H, W).cpu()
                for k in range(S):
                    assert torch.equal(valid[k], b64["valid"][k]), f"{tag}: valid of source {k}"
                    _check("1 synth", tag, synth[k], b64["synth"][k], R.bound(b32["synth"][k], b64["synth"][k]))
                select = fwd["select"].view(B, H, W).cpu().long()
                off = select[~c["near"]] != r64["select"][~c["near"]]
                assert not off.any(), f"{tag}: {int(off.sum())} selections differ outside the near-ties"
                if with_pmap:
                    keep = ~c["pmap_excluded"]
                    _check("1 pmap", tag, fwd["pmap"], r64["pmap"], R.bound(r32["pmap"], r64["pmap"], keep), keep)
                _check("1 loss", tag, fwd["loss"][0], r64["loss"], R.bound(r32["loss"], r64["loss"]))
                # backward on this run's own synth / valid / select: with the poses' gradient, and without
                bwd = _run2(lambda b: L.call("e2e_warp_photo_window_bwd", *_bwd_args(L, t, fwd, gl, b, use_mask, pad, terms, S, B, H, W)),
                            _bwd_sizes(L, S, B, H, W))
                plain = _run2(lambda b: L.call("e2e_warp_photo_window_bwd", *_bwd_args(L, t, fwd, gl, b, use_mask, pad, terms, S, B, H, W, pose=False)),
                              _bwd_sizes(L, S, B, H, W, pose=False))
                assert _same_bits(bwd["g_dt"], plain["g_dt"]), f"{tag}: g_depth_tgt changes with g_T = NULL"
                keep = ~c["grad_excluded"]
                _check("1 g_depth_tgt", tag, bwd["g_dt"], Wr.G_LOSS * r64["g_depth"], Wr.depth_bound(c, Wr.G_LOSS), keep)
                if (shape, pad, use_mask, mode) in Wr.POSE_CASES:
                    g_T = bwd["g_T"].view(S, B, 4, 4)
                    for k in range(S):
                        _check("1 g_T", f"{tag} source {k}", g_T[k], Wr.G_LOSS * r64["g_T"][k], Wr.pose_bound(c, k, Wr.G_LOSS))


@pytest.mark.parametrize("winner", (0, 1))
def test_each_pose_gets_gradient_only_from_the_pixels_it_won(winner):
    """the crafted case of tests/warp_window_ref.py: the other source's map loses everywhere, so its g_T is exactly zero, and the winner's is
    the float64 reference's within the bound"""
    L = _L()
    c = Wr.crafted(winner)
    shape, pad, use_mask, mode = Wr.CRAFTED
    (B, H, W), S, terms = shape, mode[0], Wr.terms_of(mode)
    t = _device(c["scene"], S, srcs=c["srcs"])
    fwd = _run2(lambda b: L.call("e2e_warp_photo_window_fwd", *_fwd_args(L, t, b, use_mask, pad, terms, S, B, H, W)), _fwd_sizes(L, S, B, H, W))
    assert (fwd["select"] == winner).all()
    gl = torch.ones(1, device=DEV)
    bwd = _run2(lambda b: L.call("e2e_warp_photo_window_bwd", *_bwd_args(L, t, fwd, gl, b, use_mask, pad, terms, S, B, H, W)), _bwd_sizes(L, S, B, H, W))
    g_T = bwd["g_T"].view(S, B, 4, 4)
    assert float(g_T[1 - winner].abs().max()) == 0.0, "the losing source's pose received a gradient"
    g64, g32 = c[F64]["g_T"][winner], c[F32]["g_T"][winner]
    top = float(g64.abs().max())
    bnd = min(max(R.bound(g32, g64), R.FACTOR * Wr.pooled_pose(pad, use_mask, mode) * top), R.CAP * top)
    _check("1 crafted g_T", f"winner {winner}", g_T[winner], g64, bnd)
    _check("1 crafted g_depth_tgt", f"winner {winner}", bwd["g_dt"], c[F64]["g_depth"], min(
        max(R.bound(c[F32]["g_depth"], c[F64]["g_depth"]), R.FACTOR * Wr.pooled_depth(pad, use_mask, mode) * float(c[F64]["g_depth"].abs().max())),
        R.CAP * float(c[F64]["g_depth"].abs().max())))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the size queries and what the header rules out
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_size_queries():
    L = _L()
    for B, H, W in Wr.SHAPES + [(3, 8, 32), (1, 480, 640)]:
        tiles = -(-H // 8) * -(-W // 32)
        for S in (1, 2):
            assert L.query("e2e_warp_photo_window_workspace_floats", S, B, H, W) == B * tiles > 0
            assert L.query("e2e_warp_photo_window_bwd_workspace_bytes", S, B, H, W) == 96 * S * B * tiles
    for bad in ((0, 1, 4, 4), (3, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (2, -1, 4, 4)):
        assert L.query("e2e_warp_photo_window_workspace_floats", *bad) == 0
        assert L.query("e2e_warp_photo_window_bwd_workspace_bytes", *bad) == 0


def test_refused_calls_leave_outputs_alone():
    L = _L()
    S, B, H, W = 2, 2, 4, 6
    N = B * H * W
    st = L.stream()
    img = torch.rand(B, 3, H, W, device=DEV)
    s4, i_ = L.strides4(img), L.ptr(img)
    mats = torch.eye(4, device=DEV).repeat(S * B, 1, 1).contiguous()
    m_ = L.ptr(mats)
    big = torch.rand(S * B * 4 * N, device=DEV)
    r_ = L.ptr(big)
    sel = torch.zeros(N, device=DEV, dtype=torch.int32)
    f32, f64, i32 = torch.float32, torch.float64, torch.int32
    f = dict(synth=_nan(3 * S * N), valid=_nan(S * N), select=_nan(N, i32), pmap=_nan(N), loss=_nan(1),
             ws=_nan(L.query("e2e_warp_photo_window_workspace_floats", S, B, H, W)))
    g = dict(g_dt=_nan(N), g_T=_nan(S * B * 16), ws=_nan(L.query("e2e_warp_photo_window_bwd_workspace_bytes", S, B, H, W) // 8, f64))
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

    #     0   1   2   3   4   5   6   7   8   9   10               11               12                13              14 15 16 17              18            19 20 21 22 23
    a = [r_, i_, i_, s4, i_, s4, m_, m_, m_, r_, L.ptr(f["synth"]), L.ptr(f["valid"]), L.ptr(f["select"]), L.ptr(f["pmap"]), 1, 1, 6, L.ptr(f["loss"]), L.ptr(f["ws"]), S, B, H, W, st]
    dims = {15: (2, -1), 16: (1, 7, 8, -1), 19: (0, 3, -1), 20: (0, -1, 65536), 21: (0, 1), 22: (0, 1)}
    sweep("e2e_warp_photo_window_fwd", f, a, (0, 1, 2, 4, 6, 7, 8, 10, 11, 12, 17, 18), dims)
    #     0   1   2   3   4   5   6   7   8   9   10  11            12 13 14 15  16                17               18             19 20 21 22 23
    b = [r_, i_, i_, s4, i_, s4, m_, m_, m_, r_, r_, L.ptr(sel), 1, 1, 6, r_, L.ptr(g["g_dt"]), L.ptr(g["g_T"]), L.ptr(g["ws"]), S, B, H, W, st]
    dims = {13: (2, -1), 14: (1, 7, 8, -1), 19: (0, 3, -1), 20: (0, -1, 65536), 21: (0, 1), 22: (0, 1)}
    sweep("e2e_warp_photo_window_bwd", g, b, (0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 15, 16, 18), dims)
    assert count[0] == (12 + 16) + (13 + 16)
    L.call("e2e_warp_photo_window_fwd", *a)                                        # the vectors themselves are good calls, and so are the
    L.call("e2e_warp_photo_window_bwd", *b)                                        # optional pointers left out
    L.call("e2e_warp_photo_window_fwd", *[None if j in (9, 13) else v for j, v in enumerate(a)])
    L.call("e2e_warp_photo_window_bwd", *[None if j in (17, 18) else v for j, v in enumerate(b)])
    L.call("e2e_warp_photo_window_fwd", *[None if j == 2 else (1 if j == 19 else v) for j, v in enumerate(a)])      # S = 1 needs no second source
    torch.cuda.synchronize()
    _written(f["loss"], 1, "loss")
    _written(g["g_T"], S * B * 16, "g_T")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. ops.warp_photometric_window
# ---------------------------------------------------------------------------------------------------------------------------------------
OPS_CASES = [((2, 9, 33), 1, 1, (2, 0, 0), False), ((2, 9, 33), 1, 1, (2, 1, 0), False), ((2, 9, 33), 1, 0, (2, 0, 1), False),
             ((2, 17, 33), 1, 1, (2, 1, 1), False), ((2, 17, 33), 0, 0, (1, 1, 1), False), ((2, 9, 33), 0, 0, (2, 1, 1), False),
             ((2, 9, 33), 0, 1, (1, 0, 1), False), Wr.EXPANDED_CASE + (True,)]
assert all(c[:4] in Wr.POSE_CASES for c in OPS_CASES)


def _chain(ops, d, srcs, tgt, K, invK, Ts, pad, use_mask, mode, noise):
    """the operator chain of train_depth.compute_losses (fused_losses=False) on the same inputs"""
    S, minrep, auto = mode
    B, _, H, W = d.shape
    maps, autos = [], []
    for src, T in zip(srcs[:S], Ts[:S]):
        pts = ops.backproject(d, invK)
        grid, valid = ops.project3d(pts, K, T, H, W)
        synth = ops.grid_sample(src, grid, padding_mode=R.PAD_NAME[pad], align_corners=False)
        x, y = (ops.mask_mul(synth, valid), ops.mask_mul(tgt, valid)) if use_mask else (synth, tgt)
        maps.append(ops.photometric(x, y))
        if auto:
            x = ops.mask_mul(src, valid) if use_mask else src
            autos.append(ops.photometric(x, y))
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
    return ops.min_reprojection(photo)


@pytest.mark.parametrize("shape,pad,use_mask,mode,expanded", OPS_CASES, ids=str)
def test_ops_warp_photometric_window(shape, pad, use_mask, mode, expanded):
    from e2ehip import ops
    L = _L()
    B, H, W = shape
    S, minrep, auto = mode
    c = Wr.window_case(shape, pad, use_mask, mode, None, expanded)
    assert not c["grad_excluded"].any()
    s, r64 = c["scene"], c[F64]
    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} mode={mode}{' poses expanded' if expanded else ''}"
    depth, K, invK = (s[k].contiguous().to(DEV) for k in ("depth", "K", "invK"))
    srcs, tgt = [_nhwc(x.to(DEV)) for x in s["src"][:S]], _nhwc(s["tgt"].to(DEV))
    noise = s["noise"][:, :S].contiguous().to(DEV)
    kw = dict(padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask), min_reprojection=bool(minrep), auto_masking=bool(auto), tie_noise=noise)
    T0 = [T.contiguous().to(DEV) for T in c["base"]["T"][:S]]

    def fused(leaves, **more):
        d = depth.view(B, 1, H, W).clone().requires_grad_()
        Ts = [T.expand(B, 4, 4) if expanded else T for T in leaves]
        with _Recorder(L) as rec:
            out = ops.warp_photometric_window(d, srcs, tgt, K, invK, Ts, **kw, **more)
            out["photometric"].backward()
        return d.grad, rec.names, out

    leaves = [T.clone().requires_grad_() for T in T0]
    gd, names, out = fused(leaves, want_pmap=True)
    assert names == ["e2e_warp_photo_window_fwd", "e2e_warp_photo_window_bwd"], names
    assert out["synth"].shape == (S, B, 3, H, W) and out["valid"].shape == (S, B, 1, H, W) and out["select"].shape == (B, 1, H, W)
    assert out["select"].dtype == torch.int32 and out["pmap"].shape == (B, 1, H, W)
    _check("3 ops loss", tag, out["photometric"].detach(), r64["loss"], R.bound(c[F32]["loss"], r64["loss"]))
    _check("3 ops depth.grad", tag, gd, r64["g_depth"], Wr.depth_bound(c))
    for k, T in enumerate(leaves):
        assert T.grad.shape == T0[k].shape
        _check("3 ops T.grad", f"{tag} source {k}", T.grad, r64["g_T"][k], Wr.pose_bound(c, k))
    gd_detached, names, out = fused([T.clone() for T in T0])
    assert names == ["e2e_warp_photo_window_fwd", "e2e_warp_photo_window_bwd"] and out["pmap"] is None
    assert torch.equal(gd, gd_detached), f"{tag}: depth.grad changes with the pose gradient"
    with torch.no_grad(), _Recorder(L) as rec:
        ops.warp_photometric_window(depth.view(B, 1, H, W), srcs, tgt, K, invK, [T.expand(B, 4, 4) for T in T0], **kw)
    assert rec.names == ["e2e_warp_photo_window_fwd"]
    Tb = [T.expand(B, 4, 4) for T in T0]
    with pytest.raises(NotImplementedError, match="K"):
        ops.warp_photometric_window(depth.view(B, 1, H, W), srcs, tgt, K.clone().requires_grad_(), invK, Tb, **kw)
    with pytest.raises(NotImplementedError, match="inv_K"):
        ops.warp_photometric_window(depth.view(B, 1, H, W), srcs, tgt, K, invK.clone().requires_grad_(), Tb, **kw)
    # the operator chain on the same inputs, inside the same bounds
    d = depth.view(B, 1, H, W).clone().requires_grad_()
    leaves = [T.clone().requires_grad_() for T in T0]
    _chain(ops, d, srcs, tgt, K, invK, [T.expand(B, 4, 4) if expanded else T for T in leaves], pad, use_mask, mode, noise).backward()
    _check("3 chain depth.grad", tag, d.grad, r64["g_depth"], Wr.depth_bound(c))
    for k, T in enumerate(leaves):
        _check("3 chain T.grad", f"{tag} source {k}", T.grad, r64["g_T"][k], Wr.pose_bound(c, k))


def test_ops_sources_with_different_strides_and_bad_arguments():
    from e2ehip import ops
    shape, pad, use_mask, mode = (2, 9, 33), 1, 1, (2, 1, 1)
    B, H, W = shape
    c = Wr.window_case(shape, pad, use_mask, mode)
    s = c["scene"]
    depth, K, invK = (s[k].contiguous().to(DEV) for k in ("depth", "K", "invK"))
    Ts = [T.contiguous().to(DEV) for T in s["T"]]
    noise = s["noise"].contiguous().to(DEV)
    kw = dict(padding_mode="border", use_mask=True, min_reprojection=True, auto_masking=True, tie_noise=noise)
    d = depth.view(B, 1, H, W)
    tgt = s["tgt"].contiguous().to(DEV)
    same = ops.warp_photometric_window(d, [_nhwc(x.to(DEV)) for x in s["src"]], tgt, K, invK, Ts, **kw)
    mixed = ops.warp_photometric_window(d, [_nhwc(s["src"][0].to(DEV)), s["src"][1].contiguous().to(DEV)], tgt, K, invK, Ts, **kw)
    for k in ("photometric", "synth", "valid", "select"):
        assert torch.equal(same[k], mixed[k]), k
    with pytest.raises(ValueError):
        ops.warp_photometric_window(d, [tgt, tgt, tgt], tgt, K, invK, Ts + Ts[:1], **kw)
    with pytest.raises(ValueError):
        ops.warp_photometric_window(d, [tgt, tgt], tgt, K, invK, Ts[:1], **kw)
    with pytest.raises(ValueError):
        ops.warp_photometric_window(d, [tgt, tgt], tgt, K, invK, Ts, **{**kw, "tie_noise": noise[:, :1]})


def test_one_source_without_flags_is_the_pair():
    """S = 1 without flags against ops.warp_photometric on a scene of tests/warp_pose_ref.py: loss, depth.grad and T.grad of both inside that
    module's bounds"""
    from e2ehip import ops
    shape, pad, use_mask = (2, 9, 33), 1, 1
    B, H, W = shape
    c = P.pose_case(shape, pad, use_mask)
    f = R.fused_case(shape, pad, use_mask, 0)
    s = c["scene"]
    depth, K, invK, T0 = (s[k].contiguous().to(DEV) for k in ("depth", "K", "invK", "T"))
    src, tgt = _nhwc(s["src"].to(DEV)), _nhwc(s["tgt"].to(DEV))
    keep = ~f["grad_excluded"]
    got = {}
    for name in ("window", "pair"):
        d, T = depth.view(B, 1, H, W).clone().requires_grad_(), T0.clone().requires_grad_()
        if name == "window":
            out = ops.warp_photometric_window(d, [src], tgt, K, invK, [T], padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask))
            assert not out["select"].any()
        else:
            out = ops.warp_photometric(d, src, tgt, K, invK, T, padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask))
        out["photometric"].backward()
        got[name] = (out["photometric"].detach(), d.grad, T.grad)
        _check("3 one source loss", name, got[name][0], f[F64]["loss"], R.bound(f[F32]["loss"], f[F64]["loss"]))
        _check("3 one source depth.grad", name, d.grad, f[F64]["g_photo"], R.fused_grad_bound(f, (1.0, 0.0), keep), keep)
        _check("3 one source T.grad", name, T.grad, c[F64]["g_T"], P.pose_bound(c))
    _check("3 window - pair depth.grad", "", got["window"][1], got["pair"][1].double().cpu().view(B, H, W), R.fused_grad_bound(f, (1.0, 0.0), keep), keep)
    _check("3 window - pair T.grad", "", got["window"][2], got["pair"][2].double().cpu(), P.pose_bound(c))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. Depth_Estimation at 64x96
# ---------------------------------------------------------------------------------------------------------------------------------------
HT, WT = 64, 96
WINDOW, OPERATORS = {"e2e_warp_photo_window_fwd", "e2e_warp_photo_window_bwd"}, {"e2e_grid_sample_fwd", "e2e_photometric_fwd"}


def _tie_plane(S):
    return torch.randn(1, S, HT, WT, generator=torch.Generator().manual_seed(11))


def _train(cfg_mod, frames, fused, steps, tie=None, estimated=False):
    """the setup of tests/test_gpu_train_depth.py::_run with a call recorder -> (loss log, sequence, state dict, entry-point names, hooks' record)"""
    import train_depth as td
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    from oracle import depthnet
    L = _L()
    cfg = td.default_config(HT, WT, frames, steps)
    cfg.DEBUG.print_metrics = False
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
    seen = dict(T_requires_grad=[], g_T=[])
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
        return real_window(depth_tgt, srcs, tgt, K, inv_K, Ts, **kw)

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
    c.frames, c.refinement_steps = tuple(frames), steps
    cfg_mod(c)
    colors, gt, K, poses = seq
    return np.array([r["loss"] for r in otd.Trainer(sd, c).train_batch(colors, gt, poses, K)])


def _flags_gpu(min_reprojection, auto_masking):
    def mod(c):
        c.LOSS.min_reprojection, c.LOSS.auto_masking = min_reprojection, auto_masking
    return mod


def _flags_cpu(min_reprojection, auto_masking, tie):
    def mod(c):
        c.min_reprojection, c.auto_masking = min_reprojection, auto_masking
        if tie is not None:
            c.tie_break_noise = tie * 0.00001
    return mod


DRIVER_CASES = {"a: three frames, default flags": ((0, -1, 1), False, False), "b: three frames, min-reprojection and auto-masking": ((0, -1, 1), True, True),
                "c: two frames, auto-masking": ((0, -1), False, True)}


@pytest.mark.parametrize("name", sorted(DRIVER_CASES))
def test_driver_runs_the_window_on_the_fused_entry_points(name):
    """the route (fails on the parent commit, whose _fused_ok sends these configurations to the operators) and the values: the loss log against
    oracle.train_depth at the tolerance tests/test_gpu_train_depth.py uses for the three-frame window, and against fused_losses=False at the same"""
    frames, minrep, auto = DRIVER_CASES[name]
    steps = 2
    tie = _tie_plane(len(frames) - 1) if (minrep and auto) else None
    log_f, seq, sd, names, _ = _train(_flags_gpu(minrep, auto), frames, True, steps, tie)
    assert WINDOW <= set(names), f"{name}: the window entry points were not launched"
    assert not OPERATORS & set(names), f"{name}: the step went through {sorted(OPERATORS & set(names))}"
    assert names.count("e2e_warp_photo_window_fwd") == names.count("e2e_warp_photo_window_bwd") == len(log_f) == steps
    log_u, _, _, names_u, _ = _train(_flags_gpu(minrep, auto), frames, False, steps, tie)
    assert not WINDOW & set(names_u) and OPERATORS <= set(names_u)
    want = _oracle(_flags_cpu(minrep, auto, tie), frames, steps, seq, sd)
    print(f"\n{name}: fused {log_f}, operators {log_u}, oracle {want}")
    np.testing.assert_allclose(log_f, want, rtol=2e-4)
    np.testing.assert_allclose(log_f, log_u, rtol=2e-4)


def test_driver_with_estimated_poses_stays_fused_and_both_poses_get_a_gradient():
    log, _, _, names, seen = _train(lambda c: None, (0, -1, 1), True, 1, estimated=True)
    assert WINDOW <= set(names) and not OPERATORS & set(names)
    assert seen["T_requires_grad"] == [[True, True]], seen["T_requires_grad"]
    got = dict(seen["g_T"])
    assert set(got) == {0, 1}
    for k, g in got.items():
        assert g.shape == (1, 4, 4) and torch.isfinite(g).all() and float(g.abs().max()) > 0, f"pose {k} received no gradient"
    assert np.isfinite(log).all()


def test_default_two_frame_configuration_still_launches_the_pair():
    _, _, _, names, seen = _train(lambda c: None, (0, -1), True, 1)
    assert "e2e_warp_photo_fwd" in names and "e2e_warp_photo_bwd" in names
    assert not WINDOW & set(names) and not OPERATORS & set(names) and seen["T_requires_grad"] == []
