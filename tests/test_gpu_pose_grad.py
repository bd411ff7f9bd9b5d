"""The adjoint of the odometry and the pose gradients of Project3D / transform_pointcloud (csrc/pose_grad.hip, e2ehip.icp, e2ehip.ops)
against float64 references: autograd of oracle.warp_loss.project, plain float64 sums, and tests/icp_grad_ref.py (pinned on the CPU by
tests/test_icp_grad_ref.py, which also establishes the neighbour margin that lets the float32 searches be required to agree exactly).

Every figure is the largest absolute difference relative to the largest entry of the compared float64 tensor; each bound is ten times
the figure measured on the MI355X (written next to it), and never above 1e-4, the project's figure for tensors compared with float64."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import icp_grad_ref as R
from oracle import pointfusion as opf
from oracle import warp_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _check(name, got, want, bound):
    e = _rel(got, want)
    print(f"{name}: rel {e:.3e} (bound {bound:.1e}), max|ref| {float(want.abs().max()):.3e}")
    assert bound <= 1e-4
    assert e <= bound, f"{name}: {e:.3e} > {bound:.1e}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. e2e_project3d_bwd_t
# ---------------------------------------------------------------------------------------------------------------------
def _project_inputs(B, H, W, seed=0):
    from e2ehip.synthetic import icl_intrinsics
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing="ij")
    depth = torch.stack([2.0 + 0.6 * torch.sin(3.0 * xs + b) * torch.cos(2.0 * ys) + 0.3 * ys for b in range(B)])[:, None].float()   # in [1, 3]
    K = icl_intrinsics(H, W)[None].repeat(B, 1, 1)
    pts = warp_loss.backproject(depth.double(), torch.linalg.inv(K.double())).float()
    T = torch.stack([R.se3_exp(torch.tensor([0.03, -0.02, 0.015, 0.01, -0.012, 0.008], dtype=torch.float64) * (1 + 0.5 * b)) for b in range(B)]).float()
    Wg = torch.randn(B, H, W, 2, generator=g, dtype=torch.float64)
    Wz = torch.randn(B, 1, H, W, generator=g, dtype=torch.float64)
    return pts, K, T, Wg, Wz


# measured (geometric off / on): 3x5 4.9e-8 / 4.9e-8; B=2 24x32 6.2e-8 / 5.4e-8; broadcast T 7.3e-8 / 2.4e-8  ->  bound 7.3e-7
@pytest.mark.parametrize("B,H,W,broadcast", [(1, 3, 5, False), (2, 24, 32, False), (2, 24, 32, True)])
@pytest.mark.parametrize("geometric", [False, True])
def test_project3d_gradient_wrt_T(B, H, W, broadcast, geometric):
    from e2ehip import ops
    pts, K, T, Wg, Wz = _project_inputs(B, H, W)
    if broadcast:
        T = T[0]

    def scalar(project, pts, K, T, Wg, Wz):
        Tb = T.expand(B, 4, 4) if broadcast else T
        out = project(pts, K, Tb, H, W, geometric=geometric)
        s = (out[0] * Wg).sum()
        return s + (out[1] * Wz).sum() if geometric else s

    T64 = T.double().requires_grad_(True)
    s64 = scalar(warp_loss.project, pts.double(), K.double(), T64, Wg, Wz)
    (g64,) = torch.autograd.grad(s64, T64)
    Td = T.to(DEV).requires_grad_(True)
    pd = pts.to(DEV)
    if geometric:
        grid, z, _ = ops.project3d(pd, K.to(DEV), Td.expand(B, 4, 4) if broadcast else Td, H, W, True)
        assert float(z.detach().min()) > 0.5                                   # nothing at the clamp
        s = (grid * Wg.float().to(DEV)).sum() + (z * Wz.float().to(DEV)).sum()
    else:
        grid, _ = ops.project3d(pd, K.to(DEV), Td.expand(B, 4, 4) if broadcast else Td, H, W, False)
        s = (grid * Wg.float().to(DEV)).sum()
    s.backward()
    assert Td.grad.shape == T.shape
    _check("project3d dT", Td.grad, g64, 7.3e-7)
    first = Td.grad.clone()
    Td.grad = None
    out = ops.project3d(pd, K.to(DEV), Td.expand(B, 4, 4) if broadcast else Td, H, W, geometric)
    ((out[0] * Wg.float().to(DEV)).sum() + ((out[1] * Wz.float().to(DEV)).sum() if geometric else 0.0)).backward()
    assert torch.equal(first, Td.grad)                                # no atomics: bitwise reproducible


# ---------------------------------------------------------------------------------------------------------------------
# 2. e2e_transform_points_bwd_t
# ---------------------------------------------------------------------------------------------------------------------
# measured, n = 1 / 65 / 333: the float64 sums 0 / 2.4e-16 / 5.1e-16 -> bound 5.2e-15; through autograd (float32 results) dT 1.6e-8 /
# 3.0e-8 / 3.1e-8 -> bound 3.2e-7, d/dpoints 2.6e-8 / 8.0e-8 / 7.7e-8 -> bound 8.1e-7
@pytest.mark.parametrize("n", [1, 65, 333])
def test_transform_points_gradient_wrt_T(n):
    from e2ehip import ops
    g = torch.Generator().manual_seed(n)
    gr, p = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g) + 0.5
    want = torch.cat([gr.double().T @ p.double(), gr.double().sum(0)[:, None]], 1)
    got = ops.transform_points_bwd_T(gr.to(DEV), p.to(DEV))
    assert got.dtype == torch.float64 and got.shape == (3, 4)
    _check("transform_points_bwd_T", got, want, 5.2e-15)
    assert torch.equal(got, ops.transform_points_bwd_T(gr.to(DEV), p.to(DEV)))
    # through autograd: transform_points returns a gradient for T (float32), and still the one for the points
    T = R.se3_exp(torch.tensor([0.1, -0.2, 0.3, 0.2, 0.1, -0.3], dtype=torch.float64)).float()
    Td, pd = T.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    (ops.transform_points(pd, Td) * gr.to(DEV)).sum().backward()
    full = torch.zeros(4, 4, dtype=torch.float64)
    full[:3] = want
    _check("transform_points dT", Td.grad, full, 3.2e-7)
    _check("transform_points dp", pd.grad, gr.double() @ T[:3, :3].double(), 8.1e-7)


# ---------------------------------------------------------------------------------------------------------------------
# 3. e2e_icp_normal_equations_bwd
# ---------------------------------------------------------------------------------------------------------------------
# measured (accumulate 0 / 1): n=7 1.7e-8 / 3.3e-8; n=333 4.4e-8 / 2.7e-8  ->  bound 4.5e-7
@pytest.mark.parametrize("n", [7, 333])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_normal_equations_backward(n, accumulate):
    from e2ehip import _lib as L
    g = torch.Generator().manual_seed(10 * n + accumulate)
    m = 5 if n == 7 else 40                                               # fewer targets than sources: indices repeat
    src, tgt = torch.rand(n, 3, generator=g), torch.rand(m, 3, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=1)
    idx = torch.randint(0, m, (n,), generator=g)
    assert idx.unique().numel() < n
    idx[n // 2] = m + 3                                                    # one row out of range: contributes nothing, reads nothing
    dists = torch.rand(n, generator=g) * 0.02
    thresh = 0.1                                                           # keeps dists < 0.01: about half of the rows
    keep = (dists < np.float32(thresh) * np.float32(thresh)) & (idx < m)
    assert 0 < int(keep.sum()) < n - 1
    adj = torch.randn(28, generator=g, dtype=torch.float64)
    prior = torch.randn(n, 3, generator=g)

    s64 = src.double().requires_grad_(True)
    AtA, Atb, err = R.sums(s64, tgt.double(), nrm.double(), idx.clamp(max=m - 1), keep)
    packed = torch.stack([AtA[r, c] for r in range(6) for c in range(r, 6)])
    (want,) = torch.autograd.grad((adj[:21] * packed).sum() + (adj[21:27] * Atb).sum() + adj[27] * err, s64)
    if accumulate:
        want = want + prior.double()

    sd, td, nd, idd, dd, ad = src.to(DEV), tgt.to(DEV), nrm.to(DEV), idx.to(DEV), dists.to(DEV), adj.to(DEV)
    out = prior.to(DEV).clone() if accumulate else torch.full((n, 3), float("nan"), device=DEV)

    def launch(o):
        L.call("e2e_icp_normal_equations_bwd", src=L.ptr(sd), tgt=L.ptr(td), tgt_normals=L.ptr(nd), n_tgt=m, idx=L.ptr(idd), dists=L.ptr(dd),
               dist_thresh=thresh, adj28=L.ptr(ad), n=n, g_src=L.ptr(o), accumulate=accumulate, stream=L.stream())
    launch(out)
    torch.cuda.synchronize()
    _check("normal_equations_bwd", out, want, 4.5e-7)
    skipped = out.cpu()[~keep]
    assert torch.equal(skipped, prior[~keep] if accumulate else torch.zeros_like(skipped))
    again = prior.to(DEV).clone() if accumulate else torch.empty(n, 3, device=DEV)
    launch(again)
    assert torch.equal(out, again)


# ---------------------------------------------------------------------------------------------------------------------
# 4. ICP / GradICP end to end
# ---------------------------------------------------------------------------------------------------------------------
DAMP, THRESH = 1e-3, 0.012
MODES = {"icp": dict(mode="icp"), "gradicp-nu200": dict(mode="gradicp", nu=200.0), "gradicp-nu2e4": dict(mode="gradicp", nu=2e4)}
SCENES = [(7, 8, None), (150, 12, None), (333, 12, None), (333, 12, THRESH)]


@functools.lru_cache(maxsize=None)
def _icp_reference(n, grid, thresh, mode, numiters):
    tgt, tgt_n, src = R.scene(n, grid)
    s = src.double().requires_grad_(True)
    T, recs = R.icp(s, tgt, tgt_n, numiters=numiters, damp=DAMP, dist_thresh=thresh, **MODES[mode])
    (g,) = torch.autograd.grad((R.weights((3, 4)) * T[:3]).sum(), s)
    return T.detach(), recs, g


def _same_lists(trace, recs):
    assert len(trace.iterations) == len(recs) == len(trace)
    for k, (it, r) in enumerate(zip(trace.iterations, recs)):
        assert it["cnt"] == r["cnt"] == trace[k][0], f"iteration {k}: inlier count"
        assert torch.equal(it["idx"].cpu(), r["idx"]), f"iteration {k}: neighbour list"
        if "idx2" in r:
            assert it["cnt2"] == r["cnt2"] and torch.equal(it["idx2"].cpu(), r["idx2"]), f"iteration {k}: trial neighbour list"


# measured, the largest over the four scenes and three modes, for 1 / 3 / 20 iterations: d/dsrc 5.6e-8 / 2.3e-7 / 2.6e-7 (float32 per-point
# work in every iteration), T 1.8e-11 / 1.9e-8 / 4.9e-9 (float32 clouds from the second iteration on)
ICP_BOUND = {1: 5.6e-7, 3: 2.3e-6, 20: 2.6e-6}
ICP_T_BOUND = {1: 1.8e-10, 3: 1.9e-7, 20: 4.9e-8}


@pytest.mark.parametrize("n,grid,thresh", SCENES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("numiters", [1, 3, 20])
def test_icp_gradient_wrt_source(n, grid, thresh, mode, numiters):
    from e2ehip import icp
    tgt, tgt_n, src = R.scene(n, grid)
    T64, recs, g64 = _icp_reference(n, grid, thresh, mode, numiters)
    kw = dict(numiters=numiters, damp=DAMP, dist_thresh=thresh, **MODES[mode])
    td, nd = tgt.to(DEV), tgt_n.to(DEV)
    T_plain, tr_plain = icp.point_to_plane_icp(src.to(DEV), td, nd, **kw)
    s = src.to(DEV).requires_grad_(True)
    T, trace = icp.point_to_plane_icp(s, td, nd, **kw)
    assert T.dtype == torch.float64 and T.grad_fn is not None
    assert np.array_equal(T.detach().cpu().numpy(), T_plain) and list(trace) == list(tr_plain)       # forward values bit-identical
    _same_lists(trace, recs)
    (T[:3] * R.weights((3, 4)).to(DEV)).sum().backward()
    _check(f"icp T ({numiters} it)", T.detach(), T64, ICP_T_BOUND[numiters])
    _check(f"icp d/dsrc ({numiters} it)", s.grad, g64, ICP_BOUND[numiters])
    if thresh is not None:
        assert trace[0][0] < n // 2 and all(c == n for c, _ in trace[1:])                             # the keep mask bites in the first iteration
    # reproducible run to run
    s2 = src.to(DEV).requires_grad_(True)
    T2, _ = icp.point_to_plane_icp(s2, td, nd, **kw)
    (T2[:3] * R.weights((3, 4)).to(DEV)).sum().backward()
    assert torch.equal(s.grad, s2.grad)


# ---------------------------------------------------------------------------------------------------------------------
# 5. frame_to_model: depth -> vertex maps -> ICP -> pose -> pinverse -> project3d
# ---------------------------------------------------------------------------------------------------------------------
FH, FW, DS = 24, 32, 4


@functools.lru_cache(maxsize=None)
def _frame_scene():
    from e2ehip.synthetic import make_sequence
    colors, depths, K, poses = make_sequence(2, FH, FW, seed=3, step=0.02, noise=0.0, scene="corner")
    colors, depths, K, poses = colors[0], depths[0, ..., 0], K[0, 0], poses[0]
    st, _ = opf.pointfusion_step(opf.empty_state(), colors[0], depths[0], K, poses[0])
    active = opf.find_active_map_points(st["points"], K, poses[0], FH, FW)
    sel = active[::DS, 0]
    g = torch.Generator().manual_seed(0)
    fixed = warp_loss.backproject((2.0 + 0.5 * torch.rand(1, 1, FH, FW, generator=g, dtype=torch.float64)), torch.linalg.inv(K.double())[None])
    Wg = torch.randn(1, FH, FW, 2, generator=g, dtype=torch.float64)
    return st, depths, K, poses, st["points"][sel], st["normals"][sel], fixed, Wg


@functools.lru_cache(maxsize=None)
def _frame_reference(mode, numiters):
    st, depths, K, poses, tgt, tgt_n, fixed, Wg = _frame_scene()
    d = depths[1].double().requires_grad_(True)
    K64, P0 = K.double(), poses[0].double()
    ys, xs = torch.meshgrid(torch.arange(FH, dtype=torch.float64), torch.arange(FW, dtype=torch.float64), indexing="ij")
    V = torch.stack([(xs - K64[0, 2]) / K64[0, 0] * d, (ys - K64[1, 2]) / K64[1, 1] * d, d], -1)           # vertex formula
    Vg = V @ P0[:3, :3].T + P0[:3, 3]
    sub = torch.zeros(FH, FW, dtype=torch.bool)
    sub[::DS, ::DS] = True
    src = Vg[(depths[1] != 0) & sub]
    T, recs = R.icp(src, tgt, tgt_n, numiters=numiters, damp=DAMP, **MODES[mode])
    rel = torch.linalg.pinv(P0) @ (T @ P0)
    grid, _ = warp_loss.project(fixed, K64[None], rel[None], FH, FW)
    (g,) = torch.autograd.grad((grid * Wg).sum(), d)
    return (T @ P0).detach(), recs, g, sub


# measured (icp / gradicp): d/ddepth 3 it 1.7e-7 / 1.5e-7, 20 it 1.5e-7 / 1.3e-7 -> bound 1.7e-6; pose 6.6e-8 / 1.0e-7, 2.0e-7 / 1.1e-7 -> 2.0e-6
@pytest.mark.parametrize("mode", ["icp", "gradicp-nu200"])
@pytest.mark.parametrize("numiters", [3, 20])
def test_frame_to_model_depth_gradient(mode, numiters):
    from e2ehip import icp, ops
    from e2ehip.fusionmap import FusionMap
    st, depths, K, poses, tgt, tgt_n, fixed, Wg = _frame_scene()
    pose64, recs, g64, sub = _frame_reference(mode, numiters)
    assert min(r["margin"] for r in recs) >= 1.5 and recs[0]["idx"].numel() == 48
    fm = FusionMap(3 * FH * FW, FH, FW, DEV)
    fm.load_state(st["points"].to(DEV), st["normals"].to(DEV), st["colors"].to(DEV), st["ccounts"].to(DEV))
    Kd, P0 = K.to(DEV), poses[0].to(DEV)
    kw = dict(dsratio=DS, numiters=numiters, damp=DAMP, **MODES[mode])
    pose_plain, _ = icp.frame_to_model(fm, depths[1].to(DEV), Kd, P0, **kw)
    assert not pose_plain.requires_grad
    d = depths[1].to(DEV).requires_grad_(True)
    pose, trace = icp.frame_to_model(fm, d, Kd, P0, **kw)
    assert pose.grad_fn is not None and pose.dtype == torch.float32 and torch.equal(pose.detach(), pose_plain)
    _same_lists(trace, recs)
    rel = torch.pinverse(P0) @ pose
    grid, _ = ops.project3d(fixed.float().to(DEV), Kd[None], rel[None], FH, FW)
    (grid * Wg.float().to(DEV)).sum().backward()
    assert float(d.grad[~sub.to(DEV)].abs().max()) == 0.0 and float(d.grad[sub.to(DEV)].abs().min()) > 0.0
    _check(f"frame_to_model pose ({mode}, {numiters} it)", pose.detach(), pose64, 2.0e-6)
    _check(f"frame_to_model d/ddepth ({mode}, {numiters} it)", d.grad, g64, 1.7e-6)


# ---------------------------------------------------------------------------------------------------------------------
# 6. Depth_Estimation, use_gt_pose: False
# ---------------------------------------------------------------------------------------------------------------------
def _train_step(pose_gradient, detach_in_icp=False):
    import e2ehip.icp as icp_mod
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
    de = Depth_Estimation(cfg, sequence=seq, state_dict=sd, fused_losses=False)
    de.pose_gradient = pose_gradient
    real = icp_mod.frame_to_model
    if detach_in_icp:                                                     # the parent's behaviour, whatever the switch says
        icp_mod.frame_to_model = lambda fmap, depth, *a, **k: real(fmap, depth.detach(), *a, **k)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            log = de.train()
    finally:
        icp_mod.frame_to_model = real
    grads = torch.cat([p.grad.reshape(-1) for p in de.train_params if p.requires_grad and p.grad is not None]).clone()
    its = len(de.models["SLAM"].last_trace)
    return log[0], grads, its


def test_train_depth_pose_gradient_switch():
    loss_on, g_on, its = _train_step(True)
    loss_off, g_off, _ = _train_step(False)
    loss_det, g_det, _ = _train_step(True, detach_in_icp=True)
    print(f"loss {loss_on:.6f}, ICP iterations {its}, |g| on {float(g_on.norm()):.4e} off {float(g_off.norm()):.4e}, "
          f"|g_on - g_off| / |g_off| {float((g_on - g_off).norm() / g_off.norm()):.3e}")
    assert its >= 1 and np.isfinite(loss_on) and loss_on > 0
    assert loss_on == loss_off == loss_det                                # the forward does not change
    assert torch.isfinite(g_on).all() and not torch.equal(g_on, g_off)    # the pose now passes a gradient on
    assert torch.equal(g_off, g_det)                                      # switch off == the detached call of before
