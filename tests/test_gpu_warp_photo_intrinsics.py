"""The gradient of the fused warp-photometric losses with respect to the camera intrinsics K and inv_K, against float64
(csrc/warp_photo_intrinsics.hip; the kernels are the third mode of k_warp_photo_bwd / k_warp_photo_window_bwd), and what is built on it.

  1. e2e_warp_photo_bwd_intrinsics: g_K and g_inv_K within the bounds of tests/warp_intrinsics_ref.py on every admitted case; g_depth_tgt /
     g_depth_src bit-identical to e2e_warp_photo_bwd, g_T to e2e_warp_photo_bwd_pose; g_T = NULL and a second run give the same bits;
     reg_kind 1 and 2 leave both matrices unchanged; an upstream g_loss[0] != 1 scales them; the zero case gives exact zeros;
  2. e2e_warp_photo_window_bwd_intrinsics and e2e_warp_photo_geo_bwd_intrinsics: S = 1 and S = 2, flags off and min_reprojection +
     auto_masking, the same bit identities against the existing _bwd entry points;
  3. the workspace queries and the refused calls;
  4. e2e_project3d_bwd_k (with and without g_z) and e2e_backproject_bwd_invk against float64;
  5. ops.warp_photometric / warp_photometric_window(intrinsics_grad=True), the operator chain, WarpPhotoPlan.backward(intrinsics=True);
  6. tensor_refine.learn_intrinsics against torch.optim.Adam on the oracle loss, and on a photo-consistent pair.

Bounds come from the references alone; tests/test_warp_intrinsics_inputs.py proves the cases without a GPU."""
import numpy as np
import pytest
import torch

import warp_contract_ref as R
import warp_geo_ref as G
import warp_intrinsics_ref as I
import warp_window_ref as Wr
from warp_contract_ref import F32, F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
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
        print(f"warp intrinsics {name}: largest error / bound = {ratio:.3f} ({e:.2e} of {bnd:.2e} at {what})")


def _nan(n, dtype=torch.float32):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check(name, what, got, r64, bnd):
    e = float((got.double().cpu().reshape(r64.shape) - r64).abs().max())
    ratio = e / bnd if bnd > 0 else (0.0 if e == 0 else float("inf"))
    if ratio >= WORST.get(name, (-1.0,))[0]:
        WORST[name] = (ratio, e, bnd, what)
    assert e <= bnd, f"{name} {what}: max|gpu - r64| = {e:.3e} > bound {bnd:.3e} ({ratio:.2f} x)"


def _zero_rows(tag, g_K, g_iK):
    assert float(g_K[:, 3].abs().max()) == 0.0, f"{tag}: row 3 of g_K is not zero"
    assert float(g_iK[:, 3].abs().max()) == 0.0 and float(g_iK[:, :, 3].abs().max()) == 0.0, f"{tag}: row / column 3 of g_inv_K is not zero"


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


def _tiles(H, W):
    return -(-H // 8) * -(-W // 32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the pair
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pair_device(s):
    return {k: s[k].contiguous().to(DEV) for k in ("depth", "d_src", "ri_t", "ri_s", "K", "invK", "T")}


def _pair_inputs(L, t, src, tgt, pad, use_mask, B, H, W):
    return dict(depth_tgt=L.ptr(t["depth"]), src=L.ptr(src), src_strides=L.strides4(src), tgt=L.ptr(tgt), tgt_strides=L.strides4(tgt), K=L.ptr(t["K"]),
                inv_K=L.ptr(t["invK"]), T=L.ptr(t["T"]), use_mask=use_mask, padding_mode=pad, B=B, H=H, W=W, stream=L.stream())


def _pair_forward(L, inputs, B, H, W):
    N = B * H * W
    synth, valid = torch.empty(3 * N, device=DEV), torch.empty(N, device=DEV)
    loss = torch.zeros(2, device=DEV)
    ws = torch.empty(L.query("e2e_warp_photo_workspace_floats", B, H, W), device=DEV)
    L.call("e2e_warp_photo_fwd", synth=L.ptr(synth), valid=L.ptr(valid), pmap=None, reg_kind=0, reg_init_tgt=None, reg_init_src=None, depth_src=None,
           loss_out=L.ptr(loss), workspace=L.ptr(ws), **inputs)
    return synth, valid


@pytest.mark.parametrize("shape,pad,use_mask", I.PAIR_CASES + [I.ZERO_CASE], ids=str)
def test_pair_entry_point(shape, pad, use_mask):
    L = _L()
    B, H, W = shape
    N = B * H * W
    c = I.pair_case(shape, pad, use_mask)
    t = _pair_device(c["scene"])
    src, tgt = c["scene"]["src"].contiguous().to(DEV), _nhwc(c["scene"]["tgt"].to(DEV))
    inputs = _pair_inputs(L, t, src, tgt, pad, use_mask, B, H, W)
    synth, valid = _pair_forward(L, inputs, B, H, W)
    assert torch.equal(valid.view(B, H, W).cpu(), c[F64]["valid"]), "valid differs from the reference"
    nws = L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", B, H, W)
    assert nws == 8 * 21 * B * _tiles(H, W)
    nws_pose = L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W)
    bits = {}
    for reg_kind in (0, 1, 2):
        reg = dict(reg_kind=reg_kind, reg_init_tgt=L.ptr(t["ri_t"]) if reg_kind else None, reg_init_src=L.ptr(t["ri_s"]) if reg_kind else None,
                   depth_src=L.ptr(t["d_src"]) if reg_kind else None)
        for g_loss in ((1.0, 1.0), (1.3, 0.07)):
            tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} reg={reg_kind} g_loss={g_loss}"
            gl = torch.tensor(g_loss, device=DEV, dtype=torch.float32)
            common = dict(synth=L.ptr(synth), valid=L.ptr(valid), g_loss=L.ptr(gl), **reg, **inputs)
            old = dict(g_dt=_nan(N), g_ds=_nan(N), g_dt2=_nan(N), g_ds2=_nan(N), g_T=_nan(B * 16), ws=_nan(nws_pose // 8, torch.float64))
            L.call("e2e_warp_photo_bwd", g_depth_tgt=L.ptr(old["g_dt"]), g_depth_src=L.ptr(old["g_ds"]) if reg_kind else None, **common)
            L.call("e2e_warp_photo_bwd_pose", g_depth_tgt=L.ptr(old["g_dt2"]), g_depth_src=L.ptr(old["g_ds2"]) if reg_kind else None,
                   g_T=L.ptr(old["g_T"]), workspace=L.ptr(old["ws"]), **common)
            runs = []
            for with_T in (True, True, False):
                b = dict(g_dt=_nan(N), g_ds=_nan(N), g_T=_nan(B * 16), g_K=_nan(B * 16), g_iK=_nan(B * 16), ws=_nan(nws // 8, torch.float64))
                L.call("e2e_warp_photo_bwd_intrinsics", g_depth_tgt=L.ptr(b["g_dt"]), g_depth_src=L.ptr(b["g_ds"]) if reg_kind else None,
                       g_T=L.ptr(b["g_T"]) if with_T else None, g_K=L.ptr(b["g_K"]), g_inv_K=L.ptr(b["g_iK"]), workspace=L.ptr(b["ws"]), **common)
                torch.cuda.synchronize()
                for k, n in (("g_dt", N), ("g_K", B * 16), ("g_iK", B * 16), ("ws", nws // 8)) + ((("g_T", B * 16),) if with_T else ()) + \
                        ((("g_ds", N),) if reg_kind else ()):
                    _written(b[k], n, k)
                if not with_T:
                    assert torch.isnan(b["g_T"]).all(), "g_T written although NULL was passed"
                if not reg_kind:
                    assert torch.isnan(b["g_ds"]).all(), "g_depth_src written although reg_kind = 0"
                runs.append(b)
            for k in ("g_dt", "g_ds", "g_K", "g_iK", "ws"):
                assert _same(runs[0][k], runs[1][k]), f"{tag}: {k} of two identical calls differs"
                assert _same(runs[0][k], runs[2][k]), f"{tag}: {k} changes with g_T = NULL"
            assert _same(runs[0]["g_T"], runs[1]["g_T"])
            assert torch.equal(runs[0]["g_dt"][:N], old["g_dt"][:N]), f"{tag}: g_depth_tgt is not e2e_warp_photo_bwd's"
            if reg_kind:
                assert torch.equal(runs[0]["g_ds"][:N], old["g_ds"][:N]), f"{tag}: g_depth_src is not e2e_warp_photo_bwd's"
            assert torch.equal(runs[0]["g_T"][:B * 16], old["g_T"][:B * 16]), f"{tag}: g_T is not e2e_warp_photo_bwd_pose's"
            assert torch.equal(runs[0]["ws"][:B * _tiles(H, W) * 12], old["ws"][:B * _tiles(H, W) * 12]), f"{tag}: the pose sums moved"
            g_K, g_iK = runs[0]["g_K"][:B * 16].view(B, 4, 4), runs[0]["g_iK"][:B * 16].view(B, 4, 4)
            _zero_rows(tag, g_K, g_iK)
            ref = bits.setdefault(g_loss, (g_K, g_iK))
            assert torch.equal(g_K, ref[0]) and torch.equal(g_iK, ref[1]), f"{tag}: the regulariser changes the intrinsics' gradient"
            if (shape, pad, use_mask) == I.ZERO_CASE:
                assert float(g_K.abs().max()) == 0.0 and float(g_iK.abs().max()) == 0.0, f"{tag}: not exactly zero"
            else:
                _check("1 pair g_K", tag, g_K, g_loss[0] * c[F64]["g_K"], I.bound("pair", c, "g_K", g_loss[0]))
                _check("1 pair g_inv_K", tag, g_iK, g_loss[0] * c[F64]["g_invK"], I.bound("pair", c, "g_invK", g_loss[0]))
    if (shape, pad, use_mask) != I.ZERO_CASE:
        assert not torch.equal(bits[(1.0, 1.0)][0], bits[(1.3, 0.07)][0]), "g_loss[0] does not scale g_K"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the window and the geometric form
# ---------------------------------------------------------------------------------------------------------------------------------------
def _window_device(s, S, geo):
    t = {k: s[k].contiguous().to(DEV) for k in ("depth", "K", "invK")}
    t["T"] = torch.stack(list(s["T"][:S])).contiguous().to(DEV)
    t["src"] = [x.contiguous().to(DEV) for x in s["src"][:S]] + [None] * (2 - S)
    t["tgt"] = _nhwc(s["tgt"].to(DEV))
    t["noise"] = s["noise"][:, :S].contiguous().to(DEV)
    t["dsrc"] = ([x.contiguous().to(DEV) for x in s["dsrc"][:S]] + [None] * (2 - S)) if geo else [None, None]
    return t


def _window_run(L, c, geo):
    """forward, the existing backward (with g_T), the intrinsics backward with g_T twice and once without -> (old, runs)"""
    shape, pad, use_mask, mode = c["shape"], c["pad"], c["use_mask"], c["mode"]
    B, H, W = shape
    S, N, terms = mode[0], B * H * W, Wr.terms_of(mode)
    name = "e2e_warp_photo_geo" if geo else "e2e_warp_photo_window"
    t = _window_device(c["scene"], S, geo)
    inputs = dict(depth_tgt=L.ptr(t["depth"]), src0=L.ptr(t["src"][0]), src1=L.ptr(t["src"][1]), src_strides=L.strides4(t["src"][0]), tgt=L.ptr(t["tgt"]),
                  tgt_strides=L.strides4(t["tgt"]), K=L.ptr(t["K"]), inv_K=L.ptr(t["invK"]), T=L.ptr(t["T"]), use_mask=use_mask, padding_mode=pad,
                  terms=terms, S=S, B=B, H=H, W=W, stream=L.stream())
    f = dict(synth=torch.empty(3 * S * N, device=DEV), valid=torch.empty(S * N, device=DEV), select=torch.empty(N, device=DEV, dtype=torch.int32),
             loss=torch.zeros(1 + S, device=DEV), count=torch.zeros(S, device=DEV, dtype=torch.int32),
             ws=torch.empty(L.query(name + "_workspace_floats", S, B, H, W), device=DEV))
    more = dict(depth_src0=L.ptr(t["dsrc"][0]), depth_src1=L.ptr(t["dsrc"][1]), geo_min_valid=0) if geo else {}
    L.call(name + "_fwd", tie_noise=L.ptr(t["noise"]), synth=L.ptr(f["synth"]), valid=L.ptr(f["valid"]), select=L.ptr(f["select"]), pmap=None,
           loss_out=L.ptr(f["loss"]), workspace=L.ptr(f["ws"]), **(dict(geo_count=L.ptr(f["count"])) if geo else {}), **more, **inputs)
    assert torch.equal(f["select"].view(B, H, W).cpu().long(), c[F64]["select"]), "select differs from the reference"
    gl = torch.tensor(G.G_LOSS[:1 + S] if geo else (Wr.G_LOSS,), device=DEV, dtype=torch.float32)
    common = dict(synth=L.ptr(f["synth"]), valid=L.ptr(f["valid"]), select=L.ptr(f["select"]), g_loss=L.ptr(gl),
                  **(dict(geo_count=L.ptr(f["count"])) if geo else {}), **more, **inputs)
    n_old, n_new = L.query(name + "_bwd_workspace_bytes", S, B, H, W), L.query(name + "_bwd_intrinsics_workspace_bytes", S, B, H, W)
    fixed = 8 * (S * N + S) if geo else 0
    assert n_old == fixed + 96 * S * B * _tiles(H, W) and n_new == fixed + 8 * 21 * S * B * _tiles(H, W)

    def launch(entry, nws, with_T, intrinsics):
        b = dict(g_dt=_nan(N), g_ds=_nan(S * N), g_T=_nan(S * B * 16), g_K=_nan(B * 16), g_iK=_nan(B * 16), ws=_nan(nws // 8, torch.float64))
        out = dict(g_depth_tgt=L.ptr(b["g_dt"]), g_T=L.ptr(b["g_T"]) if with_T else None, workspace=L.ptr(b["ws"]))
        if geo:
            out["g_depth_src"] = L.ptr(b["g_ds"])
        if intrinsics:
            out.update(g_K=L.ptr(b["g_K"]), g_inv_K=L.ptr(b["g_iK"]))
        L.call(entry, **out, **common)
        torch.cuda.synchronize()
        for k, n in (("g_dt", N),) + ((("g_ds", S * N),) if geo else ()) + ((("g_T", S * B * 16),) if with_T else ()) + \
                ((("g_K", B * 16), ("g_iK", B * 16)) if intrinsics else ()):
            _written(b[k], n, f"{entry} {k}")
        assert torch.isnan(b["ws"][nws // 8:]).all(), f"{entry}: written past the end of the workspace"
        return b

    old = launch(name + "_bwd", n_old, True, False)
    runs = [launch(name + "_bwd_intrinsics", n_new, with_T, True) for with_T in (True, True, False)]
    return old, runs


def _window_checks(tag, c, old, runs, geo):
    B = c["shape"][0]
    for k in ("g_dt", "g_K", "g_iK") + (("g_ds",) if geo else ()):
        assert _same(runs[0][k], runs[1][k]), f"{tag}: {k} of two identical calls differs"
        assert _same(runs[0][k], runs[2][k]), f"{tag}: {k} changes with g_T = NULL"
    assert _same(runs[0]["g_T"], runs[1]["g_T"]) and torch.isnan(runs[2]["g_T"]).all()
    assert _same(runs[0]["g_dt"], old["g_dt"]), f"{tag}: g_depth_tgt is not the existing backward's"
    assert _same(runs[0]["g_T"], old["g_T"]), f"{tag}: g_T is not the existing backward's"
    if geo:
        assert _same(runs[0]["g_ds"], old["g_ds"]), f"{tag}: g_depth_src is not the existing backward's"
    g_K, g_iK = runs[0]["g_K"][:B * 16].view(B, 4, 4), runs[0]["g_iK"][:B * 16].view(B, 4, 4)
    _zero_rows(tag, g_K, g_iK)
    return g_K, g_iK


@pytest.mark.parametrize("shape,pad,use_mask,mode", I.WINDOW_CASES, ids=str)
def test_window_entry_point(shape, pad, use_mask, mode):
    L = _L()
    c = I.window_case(shape, pad, use_mask, mode)
    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} mode={mode}"
    old, runs = _window_run(L, c, False)
    g_K, g_iK = _window_checks(tag, c, old, runs, False)
    _check("2 window g_K", tag, g_K, Wr.G_LOSS * c[F64]["g_K"], I.bound("window", c, "g_K", Wr.G_LOSS))
    _check("2 window g_inv_K", tag, g_iK, Wr.G_LOSS * c[F64]["g_invK"], I.bound("window", c, "g_invK", Wr.G_LOSS))


GEO_ADMITTED = []


@pytest.mark.parametrize("shape,pad,use_mask,mode", I.GEO_CASES, ids=str)
def test_geo_entry_point(shape, pad, use_mask, mode):
    """the bit identities on every case; g_K and g_inv_K against float64 where warp_geo_ref admits the case (decided by the references on
    the machine that runs the test, as for g_T in tests/test_gpu_warp_photo_geo.py)"""
    L = _L()
    c = I.geo_case(shape, pad, use_mask, mode)
    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} mode={mode}"
    old, runs = _window_run(L, c, True)
    g_K, g_iK = _window_checks(tag, c, old, runs, True)
    GEO_ADMITTED.append(c["admitted"])
    if c["admitted"]:
        _check("2 geo g_K", tag, g_K, c[F64]["g_K"], I.bound("geo", c, "g_K"))
        _check("2 geo g_inv_K", tag, g_iK, c[F64]["g_invK"], I.bound("geo", c, "g_invK"))


def test_geo_cases_were_compared():
    assert len(GEO_ADMITTED) == len(I.GEO_CASES) and sum(GEO_ADMITTED) >= 16, "fewer geometric cases admitted than the (1,3,5) cases alone"


def test_two_sources_are_the_sum_over_the_sources():
    """flags off: the loss is the mean of the two reprojection maps, so twice the S = 2 result is the sum of the two S = 1 results, source 1
    taken as a window of its own (to a few ulps of float32: each is one rounding of a float64 sum)"""
    L = _L()
    shape, pad, use_mask = (2, 9, 33), 1, 1
    both = I.window_case(shape, pad, use_mask, (2, 0, 0))
    _, runs = _window_run(L, both, False)
    one = I.window_case(shape, pad, use_mask, (1, 0, 0))
    _, first = _window_run(L, one, False)
    s = dict(one["scene"])
    s["T"], s["src"] = [s["T"][1]], [s["src"][1]]
    swapped = dict(one, scene=s)
    swapped[F64] = dict(select=one[F64]["select"])
    _, second = _window_run(L, swapped, False)
    for k in ("g_K", "g_iK"):
        a, b = first[0][k][:32].double(), second[0][k][:32].double()
        got = 2 * runs[0][k][:32].double()
        assert float(got.abs().max()) > 0
        assert float((got - (a + b)).abs().max()) <= 4 * 2.0 ** -24 * (float(a.abs().max()) + float(b.abs().max())), k


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. workspace queries and refused calls
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_queries():
    L = _L()
    for B, H, W in [(1, 3, 5), (2, 9, 33), (1, 2, 2), (3, 8, 32), (1, 480, 640)]:
        t = B * _tiles(H, W)
        assert L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", B, H, W) == 8 * 21 * t > 0
        for S in (1, 2):
            assert L.query("e2e_warp_photo_window_bwd_intrinsics_workspace_bytes", S, B, H, W) == 8 * 21 * S * t
            assert L.query("e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes", S, B, H, W) == 8 * (S * B * H * W + S) + 8 * 21 * S * t
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", *bad) == 0
        for S in (1, 2):
            assert L.query("e2e_warp_photo_window_bwd_intrinsics_workspace_bytes", S, *bad) == 0
            assert L.query("e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes", S, *bad) == 0
    for S in (0, 3):
        assert L.query("e2e_warp_photo_window_bwd_intrinsics_workspace_bytes", S, 1, 4, 4) == 0
        assert L.query("e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes", S, 1, 4, 4) == 0
    assert L.query("e2e_project3d_bwd_k_workspace_bytes", 2) > 0 and L.query("e2e_project3d_bwd_k_workspace_bytes", 0) == 0
    assert L.query("e2e_backproject_bwd_invk_workspace_bytes", 2) > 0 and L.query("e2e_backproject_bwd_invk_workspace_bytes", -1) == 0


def _refusals(L, entry, good, outs, required, values):
    """every required pointer NULL and every bad value: E2E_ERR_ARG, the outputs keep their sentinel; the vector itself is a good call"""
    count = 0
    for kw in [{k: None} for k in required] + [{k: v} for k, vs in values for v in vs]:
        with pytest.raises(L.E2EError, match=entry):
            L.call(entry, **{**good, **kw})
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs), f"{entry}: an output changed although the call with {kw} was refused"
        count += 1
    L.call(entry, **good)
    torch.cuda.synchronize()
    assert not any(bool(torch.isnan(o[:4]).any()) for o in outs[:-1])                # the workspace may begin with fixed-point integers
    return count


def test_refused_calls_leave_outputs_alone():
    L = _L()
    B, H, W, S = 2, 4, 6, 2
    N = B * H * W
    img = torch.rand(B, 3, H, W, device=DEV)
    mats = torch.eye(4, device=DEV).repeat(S * B, 1, 1).contiguous()
    big = torch.rand(4 * S * N, device=DEV) + 1
    sel = torch.zeros(N, device=DEV, dtype=torch.int32)
    cnt = torch.full((S,), N, device=DEV, dtype=torch.int32)
    gl = torch.ones(3, device=DEV)
    i_, s4, m_, r_ = L.ptr(img), L.strides4(img), L.ptr(mats), L.ptr(big)
    # the pair
    outs = [_nan(N), _nan(N), _nan(B * 16), _nan(B * 16), _nan(B * 16), _nan(L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", B, H, W) // 8, torch.float64)]
    good = dict(depth_tgt=r_, src=i_, src_strides=s4, tgt=i_, tgt_strides=s4, K=m_, inv_K=m_, T=m_, synth=r_, valid=r_, use_mask=1, padding_mode=1,
                reg_kind=1, reg_init_tgt=r_, reg_init_src=r_, depth_src=r_, g_loss=L.ptr(gl), g_depth_tgt=L.ptr(outs[0]), g_depth_src=L.ptr(outs[1]),
                g_T=L.ptr(outs[2]), g_K=L.ptr(outs[3]), g_inv_K=L.ptr(outs[4]), workspace=L.ptr(outs[5]), B=B, H=H, W=W, stream=L.stream())
    n = _refusals(L, "e2e_warp_photo_bwd_intrinsics", good, outs,
                  ("g_K", "g_inv_K", "workspace", "depth_tgt", "src", "tgt", "K", "inv_K", "T", "synth", "valid", "g_loss", "g_depth_tgt", "reg_init_tgt",
                   "reg_init_src", "depth_src", "g_depth_src"),
                  (("padding_mode", (2, -1)), ("reg_kind", (3, -1)), ("B", (0, -1)), ("H", (0, 1)), ("W", (0, 1))))
    assert n == 27
    # the window and the geometric form
    for geo in (False, True):
        entry = "e2e_warp_photo_geo_bwd_intrinsics" if geo else "e2e_warp_photo_window_bwd_intrinsics"
        outs = [_nan(N), _nan(S * N), _nan(S * B * 16), _nan(B * 16), _nan(B * 16), _nan(L.query(entry + "_workspace_bytes", S, B, H, W) // 8, torch.float64)]
        good = dict(depth_tgt=r_, src0=i_, src1=i_, src_strides=s4, tgt=i_, tgt_strides=s4, K=m_, inv_K=m_, T=m_, synth=r_, valid=r_, select=L.ptr(sel),
                    use_mask=1, padding_mode=1, terms=6, g_loss=L.ptr(gl), g_depth_tgt=L.ptr(outs[0]), g_T=L.ptr(outs[2]), g_K=L.ptr(outs[3]),
                    g_inv_K=L.ptr(outs[4]), workspace=L.ptr(outs[5]), S=S, B=B, H=H, W=W, stream=L.stream())
        required = ["g_K", "g_inv_K", "workspace", "depth_tgt", "src0", "src1", "tgt", "K", "inv_K", "T", "synth", "valid", "select", "g_loss", "g_depth_tgt"]
        values = [("S", (3, 0)), ("padding_mode", (2, -1)), ("terms", (1, 8)), ("B", (0, 65536)), ("H", (1,)), ("W", (1,))]
        if geo:
            good.update(depth_src0=r_, depth_src1=r_, geo_count=L.ptr(cnt), geo_min_valid=0, g_depth_src=L.ptr(outs[1]))
            required += ["depth_src0", "depth_src1", "geo_count", "g_depth_src"]
            values += [("geo_min_valid", (-1,))]
        else:
            outs.pop(1)
        n = _refusals(L, entry, good, outs, required, values)
        assert n == len(required) + sum(len(v) for _, v in values)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the operators
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", I.OP_SHAPES, ids=str)
def test_operator_entry_points(shape):
    L = _L()
    B, H, W = shape
    c = I.operator_case(*shape)
    s = c["scene"]
    d = {k: c[k].contiguous().to(DEV) for k in ("pts", "g_grid", "g_z", "g_cam")}
    K, T, depth = s["K"].to(DEV), s["T"].to(DEV), s["depth"].contiguous().to(DEV)
    nk, ni = L.query("e2e_project3d_bwd_k_workspace_bytes", B), L.query("e2e_backproject_bwd_invk_workspace_bytes", B)
    for with_z in (False, True):
        runs = []
        for _ in range(2):
            g, ws = _nan(B * 16), _nan(nk // 8, torch.float64)
            L.call("e2e_project3d_bwd_k", points=L.ptr(d["pts"]), K=L.ptr(K), T=L.ptr(T), g_grid=L.ptr(d["g_grid"]), g_z=L.ptr(d["g_z"]) if with_z else None,
                   g_K=L.ptr(g), workspace=L.ptr(ws), B=B, H=H, W=W, stream=L.stream())
            torch.cuda.synchronize()
            _written(g, B * 16, "g_K")
            assert torch.isnan(ws[nk // 8:]).all()
            runs.append(g)
        assert _same(runs[0], runs[1]), "e2e_project3d_bwd_k: two identical calls differ"
        r64, r32 = (c[dt]["g_K_z" if with_z else "g_K"] for dt in (F64, F32))
        g_K = runs[0][:B * 16].view(B, 4, 4)
        assert float(g_K[:, 3].abs().max()) == 0.0
        _check("4 project3d g_K", f"{shape} g_z={with_z}", g_K, r64, R.bound(r32, r64))
    runs = []
    for _ in range(2):
        g, ws = _nan(B * 16), _nan(ni // 8, torch.float64)
        L.call("e2e_backproject_bwd_invk", g_cam=L.ptr(d["g_cam"]), depth=L.ptr(depth), g_inv_K=L.ptr(g), workspace=L.ptr(ws), B=B, H=H, W=W, stream=L.stream())
        torch.cuda.synchronize()
        _written(g, B * 16, "g_inv_K")
        assert torch.isnan(ws[ni // 8:]).all()
        runs.append(g)
    assert _same(runs[0], runs[1]), "e2e_backproject_bwd_invk: two identical calls differ"
    g_iK = runs[0][:B * 16].view(B, 4, 4)
    _zero_rows(str(shape), torch.zeros(B, 4, 4), g_iK)
    _check("4 backproject g_inv_K", str(shape), g_iK, c[F64]["g_invK"], R.bound(c[F32]["g_invK"], c[F64]["g_invK"]))
    for entry, kw in (("e2e_project3d_bwd_k", dict(points=L.ptr(d["pts"]), K=L.ptr(K), T=L.ptr(T), g_grid=L.ptr(d["g_grid"]), g_z=None, g_K=None,
                                                   workspace=L.ptr(ws))),
                      ("e2e_backproject_bwd_invk", dict(g_cam=L.ptr(d["g_cam"]), depth=None, g_inv_K=L.ptr(g), workspace=L.ptr(ws)))):
        with pytest.raises(L.E2EError, match=entry):
            L.call(entry, B=B, H=H, W=W, stream=L.stream(), **kw)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. ops and the plan
# ---------------------------------------------------------------------------------------------------------------------------------------
OPS_CASES = [((2, 9, 33), 1, 1, False), ((2, 17, 33), 0, 0, False), ((1, 37, 53), 1, 0, False), I.EXPANDED_CASE + (True,)]


@pytest.mark.parametrize("shape,pad,use_mask,expanded", OPS_CASES, ids=str)
def test_ops_warp_photometric(shape, pad, use_mask, expanded):
    from e2ehip import ops
    L = _L()
    B, H, W = shape
    c = I.pair_case(shape, pad, use_mask, expanded)
    s = c["scene"]
    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask}{' one K expanded' if expanded else ''}"
    t = _pair_device(s)
    src, tgt = _nhwc(s["src"].to(DEV)), _nhwc(s["tgt"].to(DEV))
    kw = dict(padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask))
    K0, iK0 = ((t[k][0] if expanded else t[k]).contiguous() for k in ("K", "invK"))
    bK, biK = I.bound("pair", c, "g_K"), I.bound("pair", c, "g_invK")
    view = (lambda m: m.expand(B, 4, 4)) if expanded else (lambda m: m)

    def fused(K, iK, T, **more):
        d = t["depth"].view(B, 1, H, W).clone().requires_grad_()
        with _Recorder(L) as rec:
            ops.warp_photometric(d, src, tgt, view(K), view(iK), T, **kw, **more)["photometric"].backward()
        return d.grad, rec.names

    K, iK, T = K0.clone().requires_grad_(), iK0.clone().requires_grad_(), t["T"].clone().requires_grad_()
    gd, names = fused(K, iK, T, intrinsics_grad=True)
    assert names == ["e2e_warp_photo_fwd", "e2e_warp_photo_bwd_intrinsics"], names
    assert K.grad.shape == K0.shape and iK.grad.shape == iK0.shape
    _check("5 ops K.grad", tag, K.grad, c[F64]["g_K"], bK)
    _check("5 ops inv_K.grad", tag, iK.grad, c[F64]["g_invK"], biK)
    assert float((T.grad.double().cpu() - c[F64]["g_T"]).abs().max()) <= R.CAP * float(c[F64]["g_T"].abs().max())
    # one of the two alone, the pose detached: the same entry point, the other gradient is not returned
    K1 = K0.clone().requires_grad_()
    gd1, names = fused(K1, iK0, t["T"], intrinsics_grad=True)
    assert names == ["e2e_warp_photo_fwd", "e2e_warp_photo_bwd_intrinsics"] and torch.equal(K1.grad, K.grad) and torch.equal(gd1, gd)
    # nothing requires grad but the depth: today's launches, with and without the keyword
    gd0, names = fused(K0, iK0, t["T"], intrinsics_grad=True)
    assert names == ["e2e_warp_photo_fwd", "e2e_warp_photo_bwd"], names
    assert torch.equal(gd0, gd) and torch.equal(fused(K0, iK0, t["T"])[0], gd)
    _, names = fused(K0, iK0, t["T"].clone().requires_grad_(), intrinsics_grad=True)
    assert names == ["e2e_warp_photo_fwd", "e2e_warp_photo_bwd_pose"], names
    # without the keyword the refusal stands
    with pytest.raises(NotImplementedError, match="K"):
        ops.warp_photometric(t["depth"].view(B, 1, H, W), src, tgt, view(K0.clone().requires_grad_()), view(iK0), t["T"], **kw)
    with pytest.raises(NotImplementedError, match="inv_K"):
        ops.warp_photometric(t["depth"].view(B, 1, H, W), src, tgt, view(K0), view(iK0.clone().requires_grad_()), t["T"], **kw)
    # the operator chain with K and inv_K attached: the two routes agree to twice the bound
    Kc, iKc = K0.clone().requires_grad_(), iK0.clone().requires_grad_()
    pts = ops.backproject(t["depth"].view(B, 1, H, W), view(iKc))
    grid, valid = ops.project3d(pts, view(Kc), t["T"], H, W)
    synth = ops.grid_sample(src, grid, padding_mode=R.PAD_NAME[pad], align_corners=False)
    x, y = (ops.mask_mul(synth, valid), ops.mask_mul(tgt, valid)) if use_mask else (synth, tgt)
    ops.photometric(x, y).mean().backward()
    _check("5 chain K.grad", tag, Kc.grad, c[F64]["g_K"], bK)
    _check("5 chain inv_K.grad", tag, iKc.grad, c[F64]["g_invK"], biK)
    assert float((Kc.grad - K.grad).abs().max()) <= 2 * bK and float((iKc.grad - iK.grad).abs().max()) <= 2 * biK, f"{tag}: the two routes disagree"


@pytest.mark.parametrize("geo", (False, True), ids=("window", "geo"))
def test_ops_warp_photometric_window(geo):
    from e2ehip import ops
    L = _L()
    shape, pad, use_mask, mode = (2, 9, 33), 1, 1, (2, 1, 1)
    B, H, W = shape
    c = I.geo_case(shape, pad, use_mask, mode) if geo else I.window_case(shape, pad, use_mask, mode)
    s = c["scene"]
    t = _window_device(s, 2, geo)
    srcs, tgt = [_nhwc(x) for x in t["src"]], t["tgt"]
    kw = dict(padding_mode=R.PAD_NAME[pad], use_mask=True, min_reprojection=True, auto_masking=True, tie_noise=t["noise"])
    if geo:
        kw.update(geometric=True, depth_srcs=[x.view(B, 1, H, W) for x in t["dsrc"]], geo_min_valid=0)
    name = "e2e_warp_photo_geo" if geo else "e2e_warp_photo_window"

    def run(K, iK, **more):
        d = t["depth"].view(B, 1, H, W).clone().requires_grad_()
        with _Recorder(L) as rec:
            out = ops.warp_photometric_window(d, srcs, tgt, K, iK, [t["T"][0], t["T"][1]], **kw, **more)
            total = G.G_LOSS[0] * out["photometric"] + (G.G_LOSS[1] * out["geometric"][0] + G.G_LOSS[2] * out["geometric"][1]) if geo \
                else Wr.G_LOSS * out["photometric"]
            total.backward()
        return d.grad, rec.names

    K, iK = t["K"].clone().requires_grad_(), t["invK"].clone().requires_grad_()
    gd, names = run(K, iK, intrinsics_grad=True)
    assert names == [name + "_fwd", name + "_bwd_intrinsics"], names
    a = 1.0 if geo else Wr.G_LOSS
    if not geo or c["admitted"]:
        _check("5 ops window K.grad", name, K.grad, a * c[F64]["g_K"], I.bound("geo" if geo else "window", c, "g_K", a))
        _check("5 ops window inv_K.grad", name, iK.grad, a * c[F64]["g_invK"], I.bound("geo" if geo else "window", c, "g_invK", a))
    gd0, names = run(t["K"], t["invK"], intrinsics_grad=True)
    assert names == [name + "_fwd", name + "_bwd"] and torch.equal(gd0, gd)
    with pytest.raises(NotImplementedError, match="K"):
        run(t["K"].clone().requires_grad_(), t["invK"])


def test_plan_backward_intrinsics():
    from e2ehip import ops
    from e2ehip.fused import WarpPhotoPlan
    shape, pad, use_mask = I.PLAN_CASE
    B, H, W = shape
    c = I.pair_case(shape, pad, use_mask)
    s = c["scene"]
    t = _pair_device(s)
    src, tgt = _nhwc(s["src"].to(DEV)), _nhwc(s["tgt"].to(DEV))
    v = lambda k: t[k].view(B, 1, H, W)
    plan = WarpPhotoPlan(B, H, W, DEV, padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask), reg_kind=None)
    plan.bind(v("depth"), None, None, None, src, tgt, t["K"], t["invK"], t["T"])
    assert plan.g_K is None and plan.g_inv_K is None
    plan.forward()
    out = plan.backward(pose=True, intrinsics=True)                  # the warm-up call allocates
    assert len(out) == 5 and out[3] is plan.g_K and out[4] is plan.g_inv_K and out[2] is plan.g_T
    assert len(plan.backward(intrinsics=True)) == 4 and len(plan.backward()) == 2 and len(plan.backward(pose=True)) == 3
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    plan.forward()
    plan.backward(pose=True, intrinsics=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "a later call allocated"
    got = [o.clone() for o in plan.backward(pose=True, intrinsics=True)]
    torch.cuda.synchronize()
    K, iK, T = (t[k].clone().requires_grad_() for k in ("K", "invK", "T"))
    d = v("depth").clone().requires_grad_()
    ops.warp_photometric(d, src, tgt, K, iK, T, padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask), intrinsics_grad=True)["photometric"].backward()
    for a, b, what in zip((got[0], got[2], got[3], got[4]), (d.grad, T.grad, K.grad, iK.grad), ("g_depth_tgt", "g_T", "g_K", "g_inv_K")):
        assert torch.equal(a, b), f"the plan and ops differ on {what}"
    _check("5 plan g_K", str(I.PLAN_CASE), plan.g_K, c[F64]["g_K"], I.bound("pair", c, "g_K"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. learn_intrinsics
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_learn_intrinsics_matches_cpu_adam_on_the_oracle_loss():
    """the pattern of test_scale_learning_and_grid_search_match_cpu_adam_on_the_oracle_loss: 6 steps from factors (1.05, 0.95, 1, 1), GPU
    (fused pair with the intrinsics' gradient + fused Adam) against torch autograd + torch.optim.Adam on the oracle's loss"""
    from e2ehip.tensor_refine import learn_intrinsics
    from synth import make_pair
    s = make_pair(96, 128, seed=3)
    t = {k: v.to(DEV).contiguous() for k, v in s.items()}
    steps, lr, init = 6, 1e-2, (1.05, 0.95, 1.0, 1.0)
    f, K_eff, losses = learn_intrinsics(t["depth"], t["src"].permute(0, 3, 1, 2), t["tgt"].permute(0, 3, 1, 2), t["K"], t["T"], steps, lr, init=init)
    rf, ref = I.cpu_learn_intrinsics(s["depth"], s["src"].permute(0, 3, 1, 2), s["tgt"].permute(0, 3, 1, 2), s["K"], s["T"], steps, lr, init)
    print(f"\nlearn_intrinsics: losses {losses} against {ref}; factors {f.tolist()} against {rf.tolist()}")
    np.testing.assert_allclose(losses, ref, rtol=1e-4)
    np.testing.assert_allclose(f.numpy(), rf.numpy(), rtol=0, atol=3e-4 * steps * lr)
    np.testing.assert_allclose(K_eff.cpu().numpy(), I.intrinsics_from_factors(s["K"], f)[0].numpy(), rtol=1e-6)
    bad = t["K"].clone()
    bad[:, 0, 1] = 0.3
    with pytest.raises(ValueError, match="pinhole"):
        learn_intrinsics(t["depth"], t["src"].permute(0, 3, 1, 2), t["tgt"].permute(0, 3, 1, 2), bad, t["T"], 1, lr)


def test_learn_intrinsics_recovers_a_wrong_focal_length():
    """a photo-consistent pair (the target is the source warped with the true depth and the true K): the CPU reference run reduces the loss
    and the focal error (tests/test_warp_intrinsics_inputs.py), and the GPU run ends where it does"""
    from e2ehip.tensor_refine import learn_intrinsics
    s, src, tgt = I.recovery_scene()
    steps, lr, init = I.RECOVERY["steps"], I.RECOVERY["lr"], I.RECOVERY["init"]
    rf, ref = I.cpu_learn_intrinsics(s["depth"], src, tgt, s["K"], s["T"], steps, lr, init)
    f, _, losses = learn_intrinsics(s["depth"].to(DEV), src.to(DEV), _nhwc(tgt.to(DEV)), s["K"].to(DEV), s["T"].to(DEV), steps, lr, init=init)
    print(f"\nrecovery: loss {losses[0]:.5f} -> {losses[-1]:.5f} (CPU {ref[-1]:.5f}); factors {f.tolist()} against {rf.tolist()}")
    assert ref[-1] < 0.7 * ref[0] and max(abs(float(rf[0]) - 1), abs(float(rf[1]) - 1)) < 0.7 * (init[0] - 1)
    np.testing.assert_allclose(f.numpy(), rf.numpy(), rtol=0, atol=3e-4 * steps * lr)
    assert losses[-1] < 0.7 * losses[0]
