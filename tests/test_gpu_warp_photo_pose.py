"""e2e_warp_photo_bwd_pose (csrc/warp_photo_pose.hip; the kernel is the POSE instantiation of k_warp_photo_bwd in csrc/warp_photo.hip) and
what is built on it: the gradient of the fused warp-photometric loss with respect to the relative pose T, against float64.

  1. the entry point: g_T within the bound of tests/warp_pose_ref.py for every admitted case, reg_kind 0 and 2, each g_loss of the contract
     module, both memory layouts; g_depth_tgt / g_depth_src bit-identical to e2e_warp_photo_bwd; two runs bit-identical; outputs and
     workspace written exactly to their sizes;
  2. the workspace query and the refused calls;
  3. ops.warp_photometric: T.grad for a (B,4,4) pose and for one (4,4) pose expanded over B = 2, the depth gradient unchanged, the
     detached route unchanged, K refused, and the operator chain's T.grad inside the same bound;
  4. WarpPhotoPlan.backward(pose=True): the entry point's bits, captured and replayed without allocation;
  5. Depth_Estimation with DATA.use_gt_pose: False: the step stays on the fused pair (this is the test that fails without the feature),
     agrees with the operator route, and its seam gradients agree with float64.

Bounds come from the references alone (tests/warp_pose_ref.py); tests/test_warp_pose_inputs.py proves the cases without a GPU."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import warp_contract_ref as R
import warp_pose_ref as P
from oracle import warp_loss as wl
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
        print(f"warp pose {name}: largest error / bound = {ratio:.3f} ({e:.2e} of {bnd:.2e} at {what})")


def _nan(n, dtype=torch.float32):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _check(name, what, got, r64, bnd):
    e = float((got.double().cpu().reshape(r64.shape) - r64).abs().max())
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


def _device_scene(s, T=None):
    t = {k: s[k].contiguous().to(DEV) for k in ("depth", "d_src", "ri_t", "ri_s", "K", "invK")}
    t["T"] = (s["T"] if T is None else T).contiguous().to(DEV)
    return t


def _forward(L, t, src, tgt, pad, use_mask, B, H, W):
    """e2e_warp_photo_fwd -> (synth, valid) for the backward"""
    N = B * H * W
    synth, valid = torch.empty(3 * N, device=DEV), torch.empty(N, device=DEV)
    loss = torch.zeros(2, device=DEV)
    ws = torch.empty(L.query("e2e_warp_photo_workspace_floats", B, H, W), device=DEV)
    L.call("e2e_warp_photo_fwd", L.ptr(t["depth"]), L.ptr(src), L.strides4(src), L.ptr(tgt), L.strides4(tgt), L.ptr(t["K"]), L.ptr(t["invK"]), L.ptr(t["T"]),
           L.ptr(synth), L.ptr(valid), None, use_mask, pad, 0, None, None, None, L.ptr(loss), L.ptr(ws), B, H, W, L.stream())
    return synth, valid


def _operands(L, t, src, tgt, synth, valid, pad, use_mask, reg_kind, gl):
    reg = (L.ptr(t["ri_t"]), L.ptr(t["ri_s"]), L.ptr(t["d_src"])) if reg_kind else (None, None, None)
    return (L.ptr(t["depth"]), L.ptr(src), L.strides4(src), L.ptr(tgt), L.strides4(tgt), L.ptr(t["K"]), L.ptr(t["invK"]), L.ptr(t["T"]), L.ptr(synth),
            L.ptr(valid), use_mask, pad, reg_kind, *reg, L.ptr(gl))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the entry point against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pad,use_mask", P.POSE_CASES + [P.ZERO_CASE], ids=str)
def test_entry_point(shape, pad, use_mask):
    L = _L()
    B, H, W = shape
    N = B * H * W
    c = P.pose_case(shape, pad, use_mask)
    s = c["scene"]
    g64 = c[F64]["g_T"]
    t = _device_scene(s)
    nws = L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W)
    assert nws == 96 * B * -(-H // 8) * -(-W // 32)
    bits = {}
    for layout in ("src nchw, tgt nhwc", "src nhwc, tgt nchw"):
        src = s["src"].contiguous().to(DEV) if layout.startswith("src nchw") else _nhwc(s["src"].to(DEV))
        tgt = _nhwc(s["tgt"].to(DEV)) if layout.startswith("src nchw") else s["tgt"].contiguous().to(DEV)
        synth, valid = _forward(L, t, src, tgt, pad, use_mask, B, H, W)
        assert torch.equal(valid.view(B, H, W).cpu(), c[F64]["valid"]), "valid differs from the reference"
        for reg_kind in (0, 2):
            for g_loss in R.G_LOSS:
                tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} reg={reg_kind} g_loss={g_loss} {layout}"
                gl = torch.tensor(g_loss, device=DEV, dtype=torch.float32)
                ops_ = _operands(L, t, src, tgt, synth, valid, pad, use_mask, reg_kind, gl)
                g_dt0, g_ds0 = _nan(N), _nan(N)
                L.call("e2e_warp_photo_bwd", *ops_, L.ptr(g_dt0), L.ptr(g_ds0) if reg_kind else None, B, H, W, L.stream())
                runs = []
                for _ in range(2):
                    b = dict(g_dt=_nan(N), g_ds=_nan(N), g_T=_nan(B * 16), ws=_nan(nws // 8, torch.float64))
                    L.call("e2e_warp_photo_bwd_pose", *ops_, L.ptr(b["g_dt"]), L.ptr(b["g_ds"]) if reg_kind else None, L.ptr(b["g_T"]), L.ptr(b["ws"]),
                           B, H, W, L.stream())
                    torch.cuda.synchronize()
                    _written(b["g_dt"], N, "g_depth_tgt")
                    _written(b["g_T"], B * 16, "g_T")
                    _written(b["ws"], nws // 8, "workspace")
                    if reg_kind:
                        _written(b["g_ds"], N, "g_depth_src")
                    else:
                        assert torch.isnan(b["g_ds"]).all(), "g_depth_src written although reg_kind = 0"
                    runs.append(b)
                for k in ("g_dt", "g_ds", "g_T", "ws"):
                    a, b = runs[0][k], runs[1][k]
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: {k} of two identical calls differs"
                assert torch.equal(runs[0]["g_dt"][:N], g_dt0[:N]), f"{tag}: g_depth_tgt is not e2e_warp_photo_bwd's"
                if reg_kind:
                    assert torch.equal(runs[0]["g_ds"][:N], g_ds0[:N]), f"{tag}: g_depth_src is not e2e_warp_photo_bwd's"
                g_T = runs[0]["g_T"][:B * 16].view(B, 4, 4)
                assert torch.equal(g_T, bits.setdefault(g_loss, g_T)), f"{tag}: g_T depends on the memory layout or on the regulariser"
                if g_loss[0] == 0.0 or (shape, pad, use_mask) == P.ZERO_CASE:
                    assert float(g_T.abs().max()) == 0.0, f"{tag}: g_T is not exactly zero"
                else:
                    _check("1 g_T", tag, g_T, g_loss[0] * g64, P.pose_bound(c, g_loss[0]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the workspace query and what the header rules out
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_query():
    L = _L()
    for B, H, W in sorted({c[0] for c in P.POSE_CASES}) + [(1, 2, 2), (3, 8, 32), (1, 480, 640)]:
        n = L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W)
        assert n == 12 * 8 * B * -(-H // 8) * -(-W // 32) > 0
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert L.query("e2e_warp_photo_bwd_pose_workspace_bytes", *bad) == 0


def test_refused_calls_leave_outputs_alone():
    L = _L()
    B, H, W = 2, 4, 6
    N = B * H * W
    st = L.stream()
    img = torch.rand(B, 3, H, W, device=DEV)
    s4, i_ = L.strides4(img), L.ptr(img)
    mats = torch.eye(4, device=DEV).repeat(B, 1, 1).contiguous()
    m_ = L.ptr(mats)
    big = torch.rand(B * 4 * N, device=DEV)
    r_ = L.ptr(big)
    outs = [_nan(N), _nan(N), _nan(B * 16)]
    ws = _nan(L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W) // 8, torch.float64)
    count = [0]

    def refused(*args):
        with pytest.raises(L.E2EError, match="e2e_warp_photo_bwd_pose"):
            L.call("e2e_warp_photo_bwd_pose", *args)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs + [ws]), "an output changed although the call was refused"
        count[0] += 1

    #    0   1   2   3   4   5   6   7   8   9  10 11 12  13  14  15  16  17                18                19                20          21 22 23 24
    a = [r_, i_, s4, i_, s4, m_, m_, m_, r_, r_, 1, 1, 1, r_, r_, r_, r_, L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.ptr(ws), B, H, W, st]
    for k in (19, 20) + (0, 1, 3, 5, 6, 7, 8, 9, 16, 17) + (13, 14, 15, 18):       # g_T, workspace; what e2e_warp_photo_bwd needs; the regulariser's
        refused(*[None if j == k else v for j, v in enumerate(a)])
    for k, values in zip((11, 12, 21, 22, 23), ((2, -1), (3, -1), (0, -1), (0, 1), (0, 1))):
        for v in values:
            refused(*[v if j == k else x for j, x in enumerate(a)])
    L.call("e2e_warp_photo_bwd_pose", *a)                                          # the vector itself is a good call
    torch.cuda.synchronize()
    assert not torch.isnan(outs[2][:B * 16]).any() and count[0] == 26


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. ops.warp_photometric
# ---------------------------------------------------------------------------------------------------------------------------------------
OPS_CASES = [((2, 9, 33), 1, 1, False), (P.OWN_SHAPE, 0, 1, False), (P.OWN_SHAPE, 0, 0, False), ((1, 37, 53), 1, 0, False), P.EXPANDED_CASE + (True,)]


@pytest.mark.parametrize("shape,pad,use_mask,expanded", OPS_CASES, ids=str)
def test_ops_warp_photometric(shape, pad, use_mask, expanded):
    from e2ehip import ops
    L = _L()
    B, H, W = shape
    c = P.pose_case(shape, pad, use_mask, expanded)
    s = c["scene"]
    g64, bnd = c[F64]["g_T"], P.pose_bound(c)
    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask}{' one T expanded' if expanded else ''}"
    t = _device_scene(s)
    src, tgt = _nhwc(s["src"].to(DEV)), _nhwc(s["tgt"].to(DEV))
    kw = dict(padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask))
    T0 = (s["T"][0] if expanded else s["T"]).contiguous().to(DEV)

    def fused(T_leaf):
        d = t["depth"].view(B, 1, H, W).clone().requires_grad_()
        Tb = T_leaf.expand(B, 4, 4) if expanded else T_leaf
        with _Recorder(L) as rec:
            ops.warp_photometric(d, src, tgt, t["K"], t["invK"], Tb, **kw)["photometric"].backward()
        return d.grad, rec.names

    T = T0.clone().requires_grad_()
    gd, names = fused(T)
    assert "e2e_warp_photo_bwd_pose" in names and "e2e_warp_photo_bwd" not in names
    assert T.grad.shape == T0.shape
    _check("3 ops T.grad", tag, T.grad, g64, bnd)
    gd_detached, names = fused(T0.clone())
    assert names == ["e2e_warp_photo_fwd", "e2e_warp_photo_bwd"], names              # a detached pose: today's launches, no pose gradient
    assert torch.equal(gd, gd_detached), f"{tag}: depth.grad changes with the pose gradient"
    with pytest.raises(NotImplementedError, match="K"):
        ops.warp_photometric(t["depth"].view(B, 1, H, W), src, tgt, t["K"].clone().requires_grad_(), t["invK"], T0.expand(B, 4, 4), **kw)
    with pytest.raises(NotImplementedError, match="inv_K"):
        ops.warp_photometric(t["depth"].view(B, 1, H, W), src, tgt, t["K"], t["invK"].clone().requires_grad_(), T0.expand(B, 4, 4), **kw)
    # the operator chain on the same inputs: the two routes agree with each other to twice the bound
    Tc = T0.clone().requires_grad_()
    pts = ops.backproject(t["depth"].view(B, 1, H, W), t["invK"])
    grid, valid = ops.project3d(pts, t["K"], Tc.expand(B, 4, 4) if expanded else Tc, H, W)
    synth = ops.grid_sample(src, grid, padding_mode=R.PAD_NAME[pad], align_corners=False)
    x, y = (ops.mask_mul(synth, valid), ops.mask_mul(tgt, valid)) if use_mask else (synth, tgt)
    ops.photometric(x, y).mean().backward()
    _check("3 chain T.grad", tag, Tc.grad, g64, bnd)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. WarpPhotoPlan.backward(pose=True)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_plan_backward_pose_captured():
    from e2ehip.fused import WarpPhotoPlan
    L = _L()
    shape, pad, use_mask = P.PLAN_CASE
    B, H, W = shape
    N = B * H * W
    c = P.pose_case(shape, pad, use_mask)
    s = c["scene"]
    t = _device_scene(s)
    src, tgt = _nhwc(s["src"].to(DEV)), _nhwc(s["tgt"].to(DEV))
    v = lambda k: t[k].view(B, 1, H, W)
    plan = WarpPhotoPlan(B, H, W, DEV, padding_mode=R.PAD_NAME[pad], use_mask=bool(use_mask), reg_kind="l2")
    plan.bind(v("depth"), v("d_src"), v("ri_t"), v("ri_s"), src, tgt, t["K"], t["invK"], t["T"])
    assert plan.g_T is None
    plan.forward()
    out = plan.backward(pose=True)                                    # the warm-up call: allocates g_T and its workspace
    assert len(out) == 3 and out[2] is plan.g_T and plan.g_T.shape == (B, 4, 4)
    assert len(plan.backward()) == 2                                  # the default is today's pair
    torch.cuda.synchronize()
    eager = [o.clone() for o in plan.backward(pose=True)]
    # the entry point on the plan's own synth / valid
    gl = torch.ones(2, device=DEV)
    b = dict(g_dt=_nan(N), g_ds=_nan(N), g_T=_nan(B * 16), ws=_nan(L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W) // 8, torch.float64))
    L.call("e2e_warp_photo_bwd_pose", *_operands(L, t, src, tgt, plan.synth, plan.valid, pad, use_mask, 2, gl), L.ptr(b["g_dt"]), L.ptr(b["g_ds"]),
           L.ptr(b["g_T"]), L.ptr(b["ws"]), B, H, W, L.stream())
    torch.cuda.synchronize()
    for got, want in zip(eager, (b["g_dt"][:N], b["g_ds"][:N], b["g_T"][:B * 16])):
        assert torch.equal(got.reshape(-1), want), "the plan and the entry point differ"
    _check("4 plan g_T", str(P.PLAN_CASE), eager[2], c[F64]["g_T"], P.pose_bound(c))
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.forward()
        plan.backward(pose=True)
    torch.cuda.synchronize()
    for o in (plan.g_depth_tgt, plan.g_depth_src, plan.g_T):
        o.fill_(float("nan"))
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "a replay allocated"
    for got, want in zip((plan.g_depth_tgt, plan.g_depth_src, plan.g_T), eager):
        assert torch.equal(got, want), "the replayed graph and the eager call differ"


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. Depth_Estimation, DATA.use_gt_pose: False
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _train_step(fused, pose_gradient):
    """the setup of tests/test_gpu_pose_grad.py::_train_step with the route as a parameter -> dict(loss, grads, calls, seam)"""
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    from oracle import depthnet
    from train_depth import Depth_Estimation, default_config
    cfg = default_config(64, 96, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.DATA.use_gt_pose = False
    cfg.MODEL.odom = "gradicp"
    seq = make_sequence(2, 64, 96, seed=5, scene="corner")
    sd = depthnet.random_state_dict(0)
    sd["decoder.decoder.10.conv.weight"] = sd["decoder.decoder.10.conv.weight"] * 40.0       # depth with relief: the odometry has something to hold
    de = Depth_Estimation(cfg, sequence=seq, state_dict=sd, fused_losses=fused)
    de.pose_gradient = pose_gradient
    calls, seam = dict(warp_photometric=[], grid_sample=0), {}
    real_wp, real_gs = ops.warp_photometric, ops.grid_sample

    def warp_photometric(depth_tgt, src, tgt, K, inv_K, T, **kw):
        calls["warp_photometric"].append(bool(T.requires_grad))
        d_in, T_in = depth_tgt.view(depth_tgt.shape), T.view(T.shape)            # nodes of their own: their gradients are the fused pair's alone
        seam.update(depth=depth_tgt.detach().cpu(), T=T.detach().cpu(), src=src.detach().cpu(), tgt=tgt.detach().cpu(), K=K.detach().cpu(),
                    inv_K=inv_K.detach().cpu(), kw=kw)
        if d_in.requires_grad:
            d_in.register_hook(lambda g: seam.__setitem__("g_depth", g.detach().cpu()))
        if T_in.requires_grad:
            T_in.register_hook(lambda g: seam.__setitem__("g_T", g.detach().cpu()))
        return real_wp(d_in, src, tgt, K, inv_K, T_in, **kw)

    def grid_sample(*a, **k):
        calls["grid_sample"] += 1
        return real_gs(*a, **k)

    ops.warp_photometric, ops.grid_sample = warp_photometric, grid_sample
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            log = de.train()
    finally:
        ops.warp_photometric, ops.grid_sample = real_wp, real_gs
    grads = torch.cat([p.grad.reshape(-1) for p in de.train_params if p.requires_grad and p.grad is not None]).clone()
    return dict(loss=log[0], grads=grads, calls=calls, seam=seam)


def test_driver_stays_on_the_fused_pair_with_estimated_poses():
    """the route: fails on the parent commit, whose _fused_ok sends a pose with a graph to the operators"""
    r = _train_step(True, True)
    assert r["calls"]["warp_photometric"] == [True], "ops.warp_photometric was not called with a T that requires grad"
    assert r["calls"]["grid_sample"] == 0, "the step went through ops.grid_sample"
    u = _train_step(False, True)
    assert u["calls"]["warp_photometric"] == [] and u["calls"]["grid_sample"] >= 1


# measured on the MI355X: |g_f - g_u| / |g_u| = 2.238e-04 with the pose gradient off (the yardstick), 9.416e-05 with it on (ratio 0.42;
# ten times the yardstick is admitted); both figures are printed by every run
def test_driver_values_and_agreement_of_the_two_routes():
    f_on, u_on, f_off, u_off = _train_step(True, True), _train_step(False, True), _train_step(True, False), _train_step(False, False)
    np.testing.assert_allclose(f_on["loss"], u_on["loss"], rtol=2e-5)
    assert torch.isfinite(f_on["grads"]).all()
    assert not torch.equal(f_on["grads"], f_off["grads"]), "the pose passed no gradient on"
    stat = lambda a, b: float((a["grads"] - b["grads"]).double().norm() / b["grads"].double().norm())
    yardstick, figure = stat(f_off, u_off), stat(f_on, u_on)
    print(f"\n|g_f - g_u| / |g_u|: pose gradient off (yardstick) {yardstick:.3e}, on {figure:.3e}, ratio {figure / yardstick if yardstick else float('inf'):.2f}")
    assert figure <= 10.0 * yardstick, f"|g_f - g_u| / |g_u| = {figure:.3e} with the pose gradient, {yardstick:.3e} without: more than ten times"


def test_driver_seam_gradients_against_float64():
    """the T and the target depth that entered ops.warp_photometric in the driver's step, the composition in float64 on the CPU from those
    very tensors, and the gradients the fused pair returned for them: each within CAP x max|r64|.  Measured on the MI355X: g_T 4.8e-6,
    g_depth_tgt 1.1e-5 of the largest entry."""
    seam = _train_step(True, True)["seam"]
    assert "g_T" in seam and "g_depth" in seam
    d = seam["depth"].double().requires_grad_()
    T = seam["T"].double().requires_grad_()
    B, _, H, W = d.shape
    pts = wl.backproject(d, seam["inv_K"].double())
    grid, valid = wl.project(pts, seam["K"].double(), T, H, W)
    synth = torch.nn.functional.grid_sample(seam["src"].double(), grid, mode="bilinear", padding_mode=seam["kw"]["padding_mode"], align_corners=False)
    loss, _ = wl.masked_photometric_mean(synth, seam["tgt"].double(), valid.double(), bool(seam["kw"]["use_mask"]))
    g_T, g_d = torch.autograd.grad(loss, (T, d))
    for name, got, want in (("g_T", seam["g_T"], g_T), ("g_depth_tgt", seam["g_depth"], g_d)):
        top = float(want.abs().max())
        e = float((got.double() - want).abs().max())
        print(f"seam {name}: max|gpu - r64| {e:.3e} = {e / top:.2e} of the largest entry {top:.3e} (admitted {R.CAP:.0e})")
        assert top > 0 and e <= R.CAP * top, f"seam {name}: {e:.3e} > {R.CAP * top:.3e}"
