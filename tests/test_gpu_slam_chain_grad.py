"""The chain gradient (csrc/pose_grad.hip e2e_icp_normal_equations_bwd_tgt, e2ehip.icp target_gradient / map_tensors / prev_pose_gradient,
ops.vertex_normal_maps' pose gradient, FusionMap.step_differentiable(pose_gradient=True), gradslam.slam.PointFusion(chain_gradient=True),
train_depth's E2E_CHAIN_GRAD) against float64 references: autograd of tests/icp_grad_ref.py and tests/slam_chain_grad_ref.py, the
restatement of the whole chain that tests/test_slam_chain_grad_ref.py pins on the CPU.  The chain reference is GIVEN every discrete
choice of the GPU run (unique tables, target selections, neighbour lists), so every element is compared, none excluded.

Every figure is the largest absolute difference relative to the largest entry of the compared float64 tensor; each bound is ten times
the figure measured on the MI355X (written next to it), and never above 1e-4, the project's figure for tensors compared with float64
(d/d tgt_n of the end-to-end ICP cases measures 2.9e-5 from the second iteration on, so its bound is that cap: see ICP_BOUND)."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import icp_grad_ref as R
import pointfusion_grad_ref as P
import slam_chain_grad_ref as C
from oracle import pointfusion as opf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _check(name, got, want, bound):
    assert tuple(got.shape) == tuple(want.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    e = _rel(got, want)
    print(f"{name}: rel {e:.3e} (bound {bound:.1e}), max|ref| {float(want.abs().max()):.3e}")
    assert bound <= 1e-4
    assert e <= bound, f"{name}: {e:.3e} > {bound:.1e}"


def _zero_if_none(g, like):
    return torch.zeros_like(like) if g is None else g


# ---------------------------------------------------------------------------------------------------------------------
# 1. e2e_icp_normal_equations_bwd_tgt
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X (accumulate 0 / 1), g_tgt | g_tgt_normals: n=7 4.2e-8 / 3.0e-8 | 2.7e-8 / 1.7e-8; n=333 2.4e-8 / 4.6e-8 | 3.2e-8 /
# 2.4e-8; n=4099 (segments of about 680 rows: the wave path) 3.1e-8 / 3.9e-8 | 3.0e-8 / 2.0e-8 -- one float32 rounding of a float64 sum
KERNEL_BOUND = {"g_tgt": 4.6e-7, "g_tgt_normals": 3.2e-7}


@pytest.mark.parametrize("n,m", [(7, 5), (333, 40), (4099, 3)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_target_adjoint_of_the_normal_equations(n, m, accumulate):
    from e2ehip import _lib as L
    g = torch.Generator().manual_seed(10 * n + accumulate)
    src, tgt = torch.rand(n, 3, generator=g), torch.rand(m, 3, generator=g)
    nrm = torch.nn.functional.normalize(torch.randn(m, 3, generator=g), dim=1)
    idx = torch.randint(0, m - 1 if m > 3 else m, (n,), generator=g)       # indices repeat; with m > 3 the last target is never named
    assert idx.unique().numel() < n
    idx[n // 2] = m + 3                                                    # one row out of range: contributes nothing, reads nothing
    dists = torch.rand(n, generator=g) * 0.02
    thresh = 0.1                                                           # keeps dists < 0.01: about half of the rows
    keep = (dists < np.float32(thresh) * np.float32(thresh)) & (idx < m)
    assert 0 < int(keep.sum()) < n - 1
    named = torch.zeros(m, dtype=torch.bool)
    named[idx[keep]] = True
    assert bool((~named).any()) == (m > 3)
    if m == 3:
        assert int(torch.bincount(idx[keep]).min()) > 256                 # long segments: a wave sums each
    adj = torch.randn(28, generator=g, dtype=torch.float64)
    prior = [torch.randn(m, 3, generator=g), torch.randn(m, 3, generator=g)]

    t64, n64 = tgt.double().requires_grad_(True), nrm.double().requires_grad_(True)
    AtA, Atb, err = R.sums(src.double(), t64, n64, idx.clamp(max=m - 1), keep)
    packed = torch.stack([AtA[r, c] for r in range(6) for c in range(r, 6)])
    want = list(torch.autograd.grad((adj[:21] * packed).sum() + (adj[21:27] * Atb).sum() + adj[27] * err, [t64, n64]))
    closed = C.ne_bwd_tgt_closed_form(src, tgt, nrm, idx.clamp(max=m - 1), keep, adj)
    assert all(_rel(a, b) <= 1e-12 for a, b in zip(closed, want))
    if accumulate:
        want = [w + p.double() for w, p in zip(want, prior)]

    sd, td, nd, idd, dd, ad = src.to(DEV), tgt.to(DEV), nrm.to(DEV), idx.to(DEV), dists.to(DEV), adj.to(DEV)
    ws = torch.empty(L.query("e2e_icp_normal_equations_bwd_tgt_workspace_bytes", n, m), device=DEV, dtype=torch.uint8)
    assert 0 < ws.numel() <= 8 * (n + m) + 4 * (n // 64 + m // 4096) + 64 # O(n + n_tgt)
    assert L.query("e2e_icp_normal_equations_bwd_tgt_workspace_bytes", 0, m) == 0 == L.query("e2e_icp_normal_equations_bwd_tgt_workspace_bytes", n, -1)

    def launch(gt, gn):
        L.call("e2e_icp_normal_equations_bwd_tgt", src=L.ptr(sd), tgt=L.ptr(td), tgt_normals=L.ptr(nd), n_tgt=m, idx=L.ptr(idd), dists=L.ptr(dd),
               dist_thresh=thresh, adj28=L.ptr(ad), n=n, g_tgt=L.ptr(gt), g_tgt_normals=L.ptr(gn), accumulate=accumulate, workspace=L.ptr(ws),
               stream=L.stream())

    def fresh():
        return [p.to(DEV).clone() if accumulate else torch.full((m, 3), float("nan"), device=DEV) for p in prior]

    out = fresh()
    launch(*out)
    torch.cuda.synchronize()
    for name, o, w, p in zip(KERNEL_BOUND, out, want, prior):
        _check(f"{name} (n={n}, accumulate={accumulate})", o, w, KERNEL_BOUND[name])
        untouched = o.cpu()[~named]
        assert torch.equal(untouched, p[~named] if accumulate else torch.zeros_like(untouched)), name
    again = fresh()
    launch(*again)
    assert all(torch.equal(a, b) for a, b in zip(out, again))             # no float atomics: bitwise reproducible
    # each output NULL in turn: the other one is the same bits; both NULL is refused before anything is launched
    only_t, only_n = fresh(), fresh()
    launch(only_t[0], None)
    launch(None, only_n[1])
    assert torch.equal(only_t[0], out[0]) and torch.equal(only_n[1], out[1])
    with pytest.raises(L.E2EError, match=r"e2e_icp_normal_equations_bwd_tgt failed \(-1\)"):
        launch(None, None)


# ---------------------------------------------------------------------------------------------------------------------
# 2. ICP / GradICP end to end: d/d src, tgt, tgt_n, prev_pose
# ---------------------------------------------------------------------------------------------------------------------
DAMP, THRESH = 1e-3, 0.012
MODES = {"icp": dict(mode="icp"), "gradicp-nu200": dict(mode="gradicp", nu=200.0), "gradicp-nu2e4": dict(mode="gradicp", nu=2e4)}
SCENES = [(7, 8, None), (150, 12, None), (333, 12, None), (333, 12, THRESH)]
PREV = R.se3_exp(torch.tensor([0.3, -0.2, 0.1, 0.2, -0.1, 0.3], dtype=torch.float64)).float()


@functools.lru_cache(maxsize=None)
def _icp_reference(n, grid, thresh, mode, numiters):
    """float64, free searches: T, the records, d sum(w . T[:3]) / d (src, tgt, tgt_n), d sum(w . (T . PREV)[:3]) / d (src, tgt, tgt_n, PREV)."""
    tgt, tgt_n, src = R.scene(n, grid)
    s, t, tn, p = (x.double().requires_grad_(True) for x in (src, tgt, tgt_n, PREV))
    T, recs = R.icp(s, t, tn, numiters=numiters, damp=DAMP, dist_thresh=thresh, **MODES[mode])
    w = R.weights((3, 4))
    g = torch.autograd.grad((w * T[:3]).sum(), [s, t, tn], retain_graph=True)
    gp = torch.autograd.grad((w * (T @ p)[:3]).sum(), [s, t, tn, p])
    return T.detach(), recs, g, gp


# measured on the MI355X, the largest over the four scenes, the three modes and the calls without and with prev_pose, for 1 / 3 / 20
# iterations: d/d src 8.1e-8 / 2.3e-7 / 2.6e-7, d/d tgt 7.9e-8 / 2.1e-7 / 2.2e-7, d/d prev_pose 4.2e-8 / 5.6e-8 / 5.6e-8,
# d/d tgt_n 1.1e-7 / 2.9e-5 / 2.8e-5.
# d/d tgt_n from the second iteration on: its entries are sums of b_i gbar-like terms with b_i = n.(t - s_i) the millimetre residual of
# positions of order 1 (largest entry 2e-4 to 4e-4, against 0.06 to 0.17 for d/d tgt), and the moved cloud s is float32 in the forward
# (kept so: the values are bit-identical to the plain call), so b carries a relative error of 6e-8 / 2e-3.  The float64 reference itself
# moves by 7e-6 to 1e-5 of the largest entry when its moved clouds are rounded to float32 (icp(..., round32=True), measured on the
# CPU; exactly 0 for one iteration, whose cloud is src itself).  Ten times the measured figure would pass the project's cap of 1e-4,
# which holds whatever is measured: the bound is the cap.
ICP_BOUND = {"src": {1: 8.1e-7, 3: 2.3e-6, 20: 2.6e-6}, "tgt": {1: 7.9e-7, 3: 2.1e-6, 20: 2.2e-6}, "tgt_n": {1: 1.1e-6, 3: 1e-4, 20: 1e-4},
             "prev_pose": {1: 4.2e-7, 3: 5.6e-7, 20: 5.6e-7}}


@pytest.mark.parametrize("n,grid,thresh", SCENES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("numiters", [1, 3, 20])
def test_icp_gradient_wrt_targets_and_prev_pose(n, grid, thresh, mode, numiters):
    from e2ehip import icp
    tgt, tgt_n, src = R.scene(n, grid)
    T64, recs, g64, gp64 = _icp_reference(n, grid, thresh, mode, numiters)
    kw = dict(numiters=numiters, damp=DAMP, dist_thresh=thresh, **MODES[mode])
    w = R.weights((3, 4)).to(DEV)
    T_plain, tr_plain = icp.point_to_plane_icp(src.to(DEV), tgt.to(DEV), tgt_n.to(DEV), **kw)
    pose_plain, _ = icp.point_to_plane_icp(src.to(DEV), tgt.to(DEV), tgt_n.to(DEV), prev_pose=PREV.to(DEV), **kw)

    s0 = src.to(DEV).requires_grad_(True)                                  # today's call: the targets are constants
    T0, _ = icp.point_to_plane_icp(s0, tgt.to(DEV).requires_grad_(True), tgt_n.to(DEV), **kw)
    (T0[:3] * w).sum().backward()

    def run(with_prev):
        s, t, tn, p = (x.to(DEV).requires_grad_(True) for x in (src, tgt, tgt_n, PREV))
        out, trace = icp.point_to_plane_icp(s, t, tn, prev_pose=p if with_prev else None, target_gradient=True, **kw)
        assert out.grad_fn is not None
        (out[:3] * (w.float() if with_prev else w)).sum().backward()
        return out.detach(), trace, [s.grad, t.grad, tn.grad] + ([p.grad] if with_prev else [])

    T, trace, grads = run(False)
    assert T.dtype == torch.float64 and np.array_equal(T.cpu().numpy(), T_plain) and list(trace) == list(tr_plain)        # forward bit-identical
    assert len(trace.iterations) == len(recs)
    named = torch.zeros(tgt.shape[0], dtype=torch.bool)
    for it, r in zip(trace.iterations, recs):                             # the searches agree with the float64 ones, list for list
        assert it["cnt"] == r["cnt"] and torch.equal(it["idx"].cpu(), r["idx"])
        named[r["idx"][r["keep"]]] = True
        if "idx2" in r:
            assert it["cnt2"] == r["cnt2"] and torch.equal(it["idx2"].cpu(), r["idx2"])
            named[r["idx2"][r["keep2"]]] = True
    assert torch.equal(grads[0], s0.grad)                                 # g_src does not depend on the switch
    for name, got, want in zip(("src", "tgt", "tgt_n"), grads, g64):
        _check(f"icp d/d {name} ({numiters} it)", got, want, ICP_BOUND[name][numiters])
    assert (~named).any()
    assert float(grads[1][~named.to(DEV)].abs().max()) == 0.0 == float(grads[2][~named.to(DEV)].abs().max())            # rows no search named
    _, _, again = run(False)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))
    # with prev_pose: the pose fl32(T . prev_pose), and its gradient to prev_pose as well
    pose, trace_p, grads_p = run(True)
    assert pose.dtype == torch.float32 and torch.equal(pose, pose_plain) and list(trace_p) == list(tr_plain)
    for name, got, want in zip(("src", "tgt", "tgt_n", "prev_pose"), grads_p, gp64):
        _check(f"icp with prev_pose d/d {name} ({numiters} it)", got, want, ICP_BOUND[name][numiters])
    assert float(grads_p[1][~named.to(DEV)].abs().max()) == 0.0 == float(grads_p[2][~named.to(DEV)].abs().max())
    _, _, again_p = run(True)
    assert all(torch.equal(a, b) for a, b in zip(grads_p, again_p))


# ---------------------------------------------------------------------------------------------------------------------
# 3. ops.vertex_normal_maps: d/d pose
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X: 1x3x5 2.3e-8, 2x24x32 2.8e-8 (float64 sums of float32 factors, rounded once)
VERTEX_POSE_BOUND = 2.8e-7


@pytest.mark.parametrize("B,H,W", [(1, 3, 5), (2, 24, 32)])
def test_vertex_maps_gradient_wrt_pose(B, H, W):
    from e2ehip import _lib as L, ops
    from e2ehip.synthetic import icl_intrinsics
    g = torch.Generator().manual_seed(B * H)
    depth = 1.5 + torch.rand(B, H, W, generator=g)
    depth[:, 1:2, 2:4] = 0                                                 # a hole: Vg is 0 there whatever the pose
    K = icl_intrinsics(H, W)
    poses = torch.stack([R.se3_exp(torch.tensor([0.3, -0.2, 0.1, 0.2, -0.1, 0.3], dtype=torch.float64) * (1 + b)) for b in range(B)]).float()
    wv = P.weights((B, H, W, 3), 50)
    want = torch.zeros(B, 4, 4, dtype=torch.float64)
    for b in range(B):                                                    # the closed form: [sum g V^T | sum g] over the valid pixels
        V, _, valid = P.frame_maps(depth[b].double(), K, torch.eye(4))
        gm = (wv[b] * valid[..., None]).reshape(-1, 3)
        want[b, :3, :3], want[b, :3, 3] = gm.T @ V.reshape(-1, 3), gm.sum(0)
    Kd = K.to(DEV)[None].repeat(B, 1, 1)
    d, p = depth.to(DEV).requires_grad_(True), poses.to(DEV).requires_grad_(True)
    m = ops.vertex_normal_maps(d, Kd, p)
    assert not m["ng"].requires_grad and not m["alpha"].requires_grad
    (m["Vg"] * wv.float().to(DEV)).sum().backward()
    assert p.grad.shape == (B, 4, 4) and float(p.grad[:, 3].abs().max()) == 0.0
    _check(f"vertex maps d/d pose ({B}x{H}x{W})", p.grad, want, VERTEX_POSE_BOUND)
    # a pose that does not require grad: the depth gradient is the kernel's, bit for bit, either way
    d2, pd, wd = depth.to(DEV).requires_grad_(True), poses.to(DEV), wv.float().to(DEV).contiguous()
    (ops.vertex_normal_maps(d2, Kd, pd)["Vg"] * wd).sum().backward()
    direct = torch.empty_like(depth, device=DEV)
    L.call("e2e_vertex_maps_bwd", L.ptr(d2.detach()), L.ptr(Kd), L.ptr(pd), None, L.ptr(wd), L.ptr(direct), B, H, W, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(d2.grad, direct) and torch.equal(d.grad, direct)


# ---------------------------------------------------------------------------------------------------------------------
# 4. frame_to_model(map_tensors=..., prev_pose_gradient=True)
# ---------------------------------------------------------------------------------------------------------------------
FH, FW, DS = 24, 32, 4
FRAME_MODES = {"icp": dict(mode="icp"), "gradicp": dict(mode="gradicp", nu=200.0)}


def _corner(L, H, W):
    from e2ehip.synthetic import make_sequence
    colors, depths, K, poses = make_sequence(L, H, W, seed=3, step=0.02, noise=0.0, scene="corner")
    return colors[0], depths[0, ..., 0], K[0, 0], poses[0]


# measured on the MI355X (icp / gradicp), 3 it | 20 it: pose 4.9e-8 / 6.3e-8 | 1.5e-7 / 8.6e-8; d/d depth 1.3e-7 / 9.9e-8 | 1.8e-7 / 1.7e-7;
# d/d map points 1.4e-7 / 1.2e-7 | 1.7e-7 / 1.7e-7; d/d prev_pose 5.4e-8 / 3.7e-8 | 9.2e-8 / 8.2e-8
FRAME_BOUND = {"pose": 1.5e-6, "depth": 1.8e-6, "map points": 1.7e-6, "prev_pose": 9.2e-7}


@pytest.mark.parametrize("mode", list(FRAME_MODES))
@pytest.mark.parametrize("numiters", [3, 20])
def test_frame_to_model_map_and_prev_pose_gradient(mode, numiters):
    from e2ehip import icp
    from e2ehip.fusionmap import FusionMap
    colors, depths, K, poses = _corner(2, FH, FW)
    st, _ = opf.pointfusion_step(opf.empty_state(), colors[0], depths[0], K, poses[0])
    fm = FusionMap(3 * FH * FW, FH, FW, DEV)
    fm.load_state(st["points"].to(DEV), st["normals"].to(DEV), st["colors"].to(DEV), st["ccounts"].to(DEV))
    Kd = K.to(DEV)
    kw = dict(dsratio=DS, numiters=numiters, damp=DAMP, **FRAME_MODES[mode])
    pose_plain, tr_plain = icp.frame_to_model(fm, depths[1].to(DEV), Kd, poses[0].to(DEV), **kw)
    d, pts, p0 = (x.to(DEV).requires_grad_(True) for x in (depths[1], st["points"], poses[0]))
    pose, trace = icp.frame_to_model(fm, d, Kd, p0, map_tensors=(pts, st["normals"].to(DEV)), prev_pose_gradient=True, **kw)
    assert pose.grad_fn is not None and torch.equal(pose.detach(), pose_plain) and list(trace) == list(tr_plain)
    sel = fm.table("active")[::DS, 0].cpu()
    w = R.weights((3, 4))
    (pose[:3] * w.float().to(DEV)).sum().backward()

    d64, pts64, p64 = (x.double().requires_grad_(True) for x in (depths[1], st["points"], poses[0]))
    pose64, _ = C.localise(pts64, st["normals"], d64, K, p64, sel, C.forced_records(trace.iterations), DS, numiters=numiters, damp=DAMP,
                           **FRAME_MODES[mode])
    want = torch.autograd.grad((w * pose64[:3]).sum(), [d64, pts64, p64])
    _check(f"frame_to_model pose ({mode}, {numiters} it)", pose.detach(), pose64.detach(), FRAME_BOUND["pose"])
    for name, got, ref in zip(("depth", "map points", "prev_pose"), (d.grad, pts.grad, p0.grad), want):
        _check(f"frame_to_model d/d {name} ({mode}, {numiters} it)", got, ref, FRAME_BOUND[name])
    used = torch.zeros(st["points"].shape[0], dtype=torch.bool)
    used[sel] = True
    assert float(pts.grad[~used.to(DEV)].abs().max()) == 0.0 and float(pts.grad.abs().max()) > 0.0    # only the selected rows are reached
    # without the new arguments: today's call, whatever requires grad
    d1, p1 = depths[1].to(DEV).requires_grad_(True), poses[0].to(DEV).requires_grad_(True)
    pose1, _ = icp.frame_to_model(fm, d1, Kd, p1, **kw)
    (pose1[:3] * w.float().to(DEV)).sum().backward()
    assert p1.grad is None and torch.equal(pose1.detach(), pose_plain)


# ---------------------------------------------------------------------------------------------------------------------
# 5. three frames through PointFusion(odom=..., map_gradient=True, chain_gradient=True)
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(24, 32), (48, 64)]


class _Recorder:
    """Wraps e2ehip.icp.frame_to_model and FusionMap.step_differentiable while a sequence runs and keeps every discrete choice of the
    run in the form slam_chain_grad_ref.chain takes; `strip`: call both as the code before the chain gradient did."""

    def __init__(self, strip=False):
        self.steps, self.strip, self.saw_chain = [dict(unique=torch.zeros(0, 3, dtype=torch.int64), sel=None, records=None, normals=None)], strip, False

    def __enter__(self):
        import e2ehip.icp as icp_mod
        from e2ehip.fusionmap import FusionMap
        self.icp_mod, self.FusionMap = icp_mod, FusionMap
        self.real_ftm, self.real_step = icp_mod.frame_to_model, FusionMap.step_differentiable
        rec = self

        def frame_to_model(fmap, depth, K, prev_pose, **kw):
            rec.saw_chain |= "map_tensors" in kw or kw.get("prev_pose_gradient", False)
            if rec.strip:
                assert "map_tensors" not in kw and "prev_pose_gradient" not in kw
            normals = fmap.normals[:fmap.M].clone().cpu()
            pose, trace = rec.real_ftm(fmap, depth, K, prev_pose, **kw)
            rec.pending = dict(sel=fmap.table("active")[::kw["dsratio"], 0].cpu(), records=C.forced_records(trace.iterations), normals=normals)
            return pose, trace

        def step_differentiable(fm, rgb, depth, K, pose, prev=None, pose_gradient=False):
            if rec.strip:
                assert not pose_gradient
                out = rec.real_step(fm, rgb, depth, K, pose.detach(), prev)
            else:
                out = rec.real_step(fm, rgb, depth, K, pose, prev, pose_gradient)
            rec.steps.append(dict(unique=fm.table("unique").cpu(), **rec.pending))
            return out

        icp_mod.frame_to_model, FusionMap.step_differentiable = frame_to_model, step_differentiable
        return self

    def __exit__(self, *exc):
        self.icp_mod.frame_to_model, self.FusionMap.step_differentiable = self.real_ftm, self.real_step


def _run_sequence(H, W, odom, scalar, strip=False, **switches):
    """-> cloud tensors, poses (3,4,4), the recorded steps, d scalar / d depth and / d rgb per frame (None -> zeros)."""
    from gradslam.slam import PointFusion
    from gradslam.structures import RGBDImages
    rgbs, depths, K, poses = _corner(3, H, W)
    d = [depths[f].to(DEV).requires_grad_(True) for f in range(3)]
    c = [rgbs[f].to(DEV).requires_grad_(True) for f in range(3)]
    frames = RGBDImages(torch.stack(c)[None], torch.stack(d)[None, ..., None], K.to(DEV)[None, None], poses.to(DEV)[None])
    slam = PointFusion(odom=odom, dsratio=DS, numiters=20, damp=DAMP, map_gradient=True, device=DEV, **switches)
    with _Recorder(strip) as rec:
        cloud, est = slam(frames)
    assert rec.saw_chain == bool(switches.get("chain_gradient", False)) and len(rec.steps) == 3
    Pt, Cl, cc = cloud.points_list[0], cloud.colors_list[0], cloud.features_list[0].reshape(-1)
    s = sum((C.pose_weights(f).float().to(DEV) * est[0, f, :3]).sum() for f in (range(3) if scalar == "full" else [2]))
    if scalar == "full":
        s = s + sum((P.weights(tuple(t.shape), i).float().to(DEV) * t).sum() for i, t in enumerate((Pt, Cl, cc)))
    s.backward()
    grads = [_zero_if_none(t.grad, t) for t in d + c]
    return (Pt.detach(), Cl.detach(), cc.detach()), est[0].detach(), rec.steps, grads


# measured on the MI355X, the largest over both shapes and both odometries: d/d depth of frame 0 / 1 / 2 5.4e-7 / 6.9e-7 / 8.5e-7, d/d rgb
# 2.7e-7 / 2.6e-7 / 3.6e-7; the final map's points, colours and confidences 2.1e-7, 1.7e-7, 4.1e-7; the poses 2.2e-7
CHAIN_BOUND = {"depth": 8.5e-6, "rgb": 3.6e-6, "values": 4.1e-6, "poses": 2.2e-6}


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("odom", ["icp", "gradicp"])
def test_three_frame_chain_through_pointfusion(H, W, odom):
    rgbs, depths, K, poses = _corner(3, H, W)
    values, est, steps, grads = _run_sequence(H, W, odom, "full", chain_gradient=True)
    d64 = [x.double().requires_grad_(True) for x in depths]
    c64 = [x.double().requires_grad_(True) for x in rgbs]
    state, poses64 = C.chain(c64, d64, K, poses[0], steps, DS, numiters=20, damp=DAMP, mode=odom)
    want = torch.autograd.grad(C.scalar(state, poses64), d64 + c64)
    for k, t in zip(("points", "colors", "ccounts"), values):
        _check(f"chain final {k}", t, state[k].detach(), CHAIN_BOUND["values"])
    _check("chain poses", est, torch.stack(poses64).detach(), CHAIN_BOUND["poses"])
    for f in range(3):
        _check(f"chain frame {f} d/d depth", grads[f], want[f], CHAIN_BOUND["depth"])
        _check(f"chain frame {f} d/d rgb", grads[3 + f], want[3 + f], CHAIN_BOUND["rgb"])
    _, _, _, again = _run_sequence(H, W, odom, "full", chain_gradient=True)
    assert all(torch.equal(a, b) for a, b in zip(grads, again))


@pytest.mark.parametrize("odom", ["icp", "gradicp"])
def test_chain_switch_off_is_the_path_of_before(odom):
    H, W = SHAPES[0]
    values_on, est_on, _, _ = _run_sequence(H, W, odom, "full", chain_gradient=True)
    values, est, _, off = _run_sequence(H, W, odom, "full", chain_gradient=False)
    assert torch.equal(est, est_on) and all(torch.equal(a, b) for a, b in zip(values, values_on))       # the switch changes no value
    _, _, _, before = _run_sequence(H, W, odom, "full", strip=True)        # default switches, both calls made as before
    assert all(torch.equal(a, b) for a, b in zip(off, before))
    # the last frame's pose alone: it reaches the earlier frames' depth only through the map and the previous pose
    _, _, _, pose_off = _run_sequence(H, W, odom, "last pose", chain_gradient=False)
    _, _, _, pose_on = _run_sequence(H, W, odom, "last pose", chain_gradient=True)
    for f in (0, 1):
        assert float(pose_off[f].abs().max()) == 0.0 and float(pose_on[f].abs().max()) > 0.0, f"frame {f}"
    assert float(pose_off[2].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 6. train_depth's switch
# ---------------------------------------------------------------------------------------------------------------------
def _train_step(chain_gradient):
    from e2ehip.synthetic import make_sequence
    from oracle import depthnet
    from train_depth import Depth_Estimation, default_config
    cfg = default_config(64, 96, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.DATA.use_gt_pose = False
    cfg.MODEL.odom = "gradicp"
    cfg.LOSS.knn_points = False
    seq = make_sequence(2, 64, 96, seed=5, scene="corner")
    sd = depthnet.random_state_dict(0)
    sd["decoder.decoder.10.conv.weight"] = sd["decoder.decoder.10.conv.weight"] * 40.0       # depth with relief: the odometry has something to hold
    de = Depth_Estimation(cfg, sequence=seq, state_dict=sd, fused_losses=False)
    assert de.chain_gradient is False                                     # E2E_CHAIN_GRAD is off by default
    de.map_gradient, de.chain_gradient = True, chain_gradient
    seen = []

    def keep_depth(module, args):
        args[0].depth_image.retain_grad()
        seen.append(args[0].depth_image)
    handle = de.models["SLAM"].register_forward_pre_hook(keep_depth)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            log = de.train()
    finally:
        handle.remove()
    grads = torch.cat([p.grad.reshape(-1) for p in de.train_params if p.requires_grad and p.grad is not None]).clone()
    assert len(seen) == 1 and de.models["SLAM"].chain_gradient is chain_gradient and len(de.models["SLAM"].last_trace) >= 1
    per_frame = [0.0 if seen[0].grad is None else float(seen[0].grad[0, f].abs().max()) for f in range(2)]
    return log[0], grads, per_frame


def test_train_depth_chain_gradient_switch(monkeypatch):
    monkeypatch.delenv("E2E_CHAIN_GRAD", raising=False)
    loss_on, g_on, frames_on = _train_step(True)
    loss_off, g_off, frames_off = _train_step(False)
    print(f"loss {loss_on:.6f}; max |d loss / d depth| per frame into SLAM: on {frames_on}, off {frames_off}; "
          f"|g_on - g_off| / |g_off| {float((g_on - g_off).norm() / g_off.norm()):.3e}")
    assert np.isfinite(loss_on) and loss_on == loss_off                   # the forward is the same
    assert torch.isfinite(g_on).all() and torch.isfinite(g_off).all() and not torch.equal(g_on, g_off)
    # frame 0 is the source frame: nothing but the pose -> map point path reaches its depth through the SLAM module
    assert frames_off[0] == 0.0 and frames_on[0] > 0.0 and frames_on[1] > 0.0
