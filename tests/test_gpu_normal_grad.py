"""The normals' gradient (csrc/normal_maps_grad.hip e2e_normal_maps_bwd, csrc/pointfusion_grad.hip e2e_pf_fuse_normals_tape / e2e_pf_fuse_normals_bwd,
ops.vertex_normal_maps(normal_grad=True), FusionMap.step_differentiable(normal_gradient=True),
gradslam.slam.PointFusion(normal_gradient=True), train_depth's E2E_NORMAL_GRAD) against tests/normal_grad_ref.py, the float64 restatement
that tests/test_normal_grad_ref.py pins on the CPU.  The references are GIVEN every discrete choice of the GPU run (unique tables, target
selections, neighbour lists), so every element is compared, none excluded.

Every figure is the largest absolute difference relative to the largest entry of the compared float64 tensor; each bound is ten times
the figure measured on the MI355X (written next to it), and never above 1e-4, the project's figure for tensors compared with float64."""
import contextlib
import io

import numpy as np
import pytest
import torch

import icp_grad_ref as I
import normal_grad_ref as N
import pointfusion_grad_ref as P
import slam_chain_grad_ref as C
from test_gpu_slam_chain_grad import _check, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
POSE = I.se3_exp(torch.tensor([0.3, -0.2, 0.1, 0.2, -0.1, 0.3], dtype=F64)).float()


def _poses(B):
    return torch.stack([I.se3_exp(torch.tensor([0.3, -0.2, 0.1, 0.2, -0.1, 0.3], dtype=F64) * (1 + b)) for b in range(B)]).float()


def _scene(B, H, W):
    """-> depth (B,H,W), K (4,4): the 5x7 frame of every nrm == 0 case, or the frames of pointfusion_grad_ref.sequence (with its hole)."""
    from e2ehip.synthetic import icl_intrinsics
    if (H, W) == (5, 7):
        assert B == 1
        return N.degenerate_frame()[0][None], icl_intrinsics(5, 7)
    _, depths, K, _ = P.sequence(H, W)
    return depths[:B].clone(), K


def _map(H, W, state=None):
    from e2ehip.fusionmap import FusionMap
    fm = FusionMap(4 * H * W, H, W, DEV)
    if state is not None:
        fm.load_state(*(state[k].to(DEV) for k in ("points", "normals", "colors", "ccounts")))
    return fm


def _state(fm):
    return {k: t.clone().cpu() for k, t in zip(("points", "normals", "colors", "ccounts"), fm.live())}


# ---------------------------------------------------------------------------------------------------------------------
# 1. e2e_normal_maps_bwd
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X, the largest over the three modes and accumulate 0 / 1: 1x5x7 2.5e-8 (its nrm == 0 pixels alone 1.9e-8), 1x24x32
# 4.3e-8, 1x48x64 5.0e-8, 2x24x32 5.6e-8 -- float64 arithmetic on float32 inputs, rounded once on the store
NORMAL_MAPS_BOUND = 5.6e-7
KERNEL_SHAPES = [(1, 5, 7), (1, 24, 32), (1, 48, 64), (2, 24, 32)]


@pytest.mark.parametrize("B,H,W", KERNEL_SHAPES)
@pytest.mark.parametrize("mode", ["g_Nm", "g_Ng", "both"])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_normal_maps_bwd(B, H, W, mode, accumulate):
    from e2ehip import _lib as L
    depth, K = _scene(B, H, W)
    poses = _poses(B)
    gn = P.weights((B, H, W, 3), 31) if mode != "g_Ng" else None
    gg = P.weights((B, H, W, 3), 32) if mode != "g_Nm" else None
    prior = P.weights((B, H, W), 33)
    want = torch.stack([N.normal_maps_bwd_closed_form(depth[b].double(), K, poses[b], None if gn is None else gn[b], None if gg is None else gg[b])
                        for b in range(B)])
    assert torch.isfinite(want).all() and float(want.abs().max()) > 0
    if accumulate:
        want = want + prior
    dd, Kd, pd = depth.to(DEV).contiguous(), K.to(DEV)[None].repeat(B, 1, 1).contiguous(), poses.to(DEV).contiguous()
    gnd, ggd = (None if g is None else g.float().to(DEV).contiguous() for g in (gn, gg))

    def launch(a=gnd, b=ggd):
        out = prior.float().to(DEV).clone() if accumulate else torch.full((B, H, W), float("nan"), device=DEV)
        L.call("e2e_normal_maps_bwd", depth=L.ptr(dd), K=L.ptr(Kd), pose=L.ptr(pd), g_Nm=L.ptr(a), g_Ng=L.ptr(b), g_depth=L.ptr(out),
               accumulate=accumulate, B=B, H=H, W=W, stream=L.stream())
        torch.cuda.synchronize()
        return out

    got = launch()
    assert torch.isfinite(got).all()                                      # the nrm == 0 pixels too: finite, never NaN
    _check(f"e2e_normal_maps_bwd {B}x{H}x{W} {mode} accumulate={accumulate}", got, want, NORMAL_MAPS_BOUND)
    invalid = depth == 0
    assert invalid.any()
    assert torch.equal(got.cpu()[invalid], prior.float()[invalid] if accumulate else torch.zeros(int(invalid.sum())))
    if (H, W) == (5, 7):                                                   # the nrm == 0 pixels match on their own
        zero = torch.zeros(H, W, dtype=torch.bool)
        for h, w in N.degenerate_frame()[1]:
            zero[h, w] = True
        e = float((got.cpu()[0].double()[zero] - want[0][zero]).abs().max() / want.abs().max())
        print(f"  nrm == 0 pixels: rel {e:.3e}")
        assert e <= NORMAL_MAPS_BOUND
    assert torch.equal(launch(), got)                                     # a gather, no atomics: the same bits
    with pytest.raises(L.E2EError, match=r"e2e_normal_maps_bwd failed \(-1\)"):
        launch(None, None)


# ---------------------------------------------------------------------------------------------------------------------
# 2. ops.vertex_normal_maps(normal_grad=True)
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X (1x5x7 / 2x24x32): d/d depth 4.2e-8 / 3.6e-8, d/d pose 3.2e-8 / 8.3e-8
OPS_BOUND = {"depth": 4.2e-7, "pose": 8.3e-7}
OUT = ("V", "n", "Vg", "ng", "alpha")


@pytest.mark.parametrize("B,H,W", [(1, 5, 7), (2, 24, 32)])
def test_vertex_normal_maps_normal_grad(B, H, W):
    from e2ehip import ops
    depth, K = _scene(B, H, W)
    poses = _poses(B)
    w = {k: P.weights((B, H, W) if k == "alpha" else (B, H, W, 3), 40 + i) for i, k in enumerate(OUT)}
    d64, p64 = depth.double().requires_grad_(True), poses.double().requires_grad_(True)
    s = 0
    for b in range(B):
        V, _, _ = P.frame_maps(d64[b], K, torch.eye(4))
        Vg, alpha, _ = P.frame_maps(d64[b], K, p64[b])
        n, ng, _ = N.frame_normal_maps(d64[b], K, p64[b])
        s = s + sum((w[k][b] * t).sum() for k, t in zip(OUT, (V, n, Vg, ng, alpha)))
    want_d, want_p = torch.autograd.grad(s, [d64, p64])
    Kd = K.to(DEV)[None].repeat(B, 1, 1)

    def run(normal_grad, attach):
        d, p = depth.to(DEV).requires_grad_(attach), poses.to(DEV).requires_grad_(attach)
        return ops.vertex_normal_maps(d, Kd, p, alpha_grad=True, normal_grad=normal_grad), d, p

    m, d, p = run(True, True)
    assert m["n"].requires_grad and m["ng"].requires_grad
    sum((w[k].float().to(DEV) * m[k]).sum() for k in OUT).backward()
    _check(f"vertex_normal_maps(normal_grad) d/d depth ({B}x{H}x{W})", d.grad, want_d, OPS_BOUND["depth"])
    _check(f"vertex_normal_maps(normal_grad) d/d pose ({B}x{H}x{W})", p.grad, want_p, OPS_BOUND["pose"])
    assert float(p.grad[:, 3].abs().max()) == 0.0
    m_off, d_off, _ = run(False, True)
    assert not m_off["n"].requires_grad and not m_off["ng"].requires_grad
    assert all(torch.equal(m[k].detach(), m_off[k].detach()) for k in OUT)                            # the same bits in both modes
    # the normals alone: the pose gets the left 3x3 block and nothing else
    m2, d2, p2 = run(True, True)
    (w["ng"].float().to(DEV) * m2["ng"]).sum().backward()
    assert float(p2.grad[:, :3, 3].abs().max()) == 0.0 == float(p2.grad[:, 3].abs().max()) and float(p2.grad[:, :3, :3].abs().max()) > 0
    assert torch.isfinite(d2.grad).all() and float(d2.grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. one map step at the level of the entry points
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X, the largest over both shapes and accumulate 0 / 1: g_Ng 3.8e-8, g_prev_normals 6.6e-8, g_alpha 1.5e-7,
# g_prev_ccounts 1.4e-7 (float32 arithmetic on the same float32 inputs as the reference, which takes the differences first too)
STEP_BOUND = {"g_Ng": 3.8e-7, "g_prev_normals": 6.6e-7, "g_alpha": 1.5e-6, "g_prev_ccounts": 1.4e-6}
STEP_NAMES = tuple(STEP_BOUND)


def _normals_step_gpu(H, W, prev, rgb, depth, K, pose, accumulate, null=None, prior_seed=60):
    """maps -> associate -> tape -> normals tape -> fuse/append -> e2e_pf_fuse_normals_bwd, called by name.
    -> M_before, M_after, unique, the frame's ng and alpha (CPU), gN, the priors and the four outputs (None where `null` names it)."""
    from e2ehip import _lib as L
    fm = _map(H, W, prev)
    M0 = fm.M
    rgb, depth, K, pose = rgb.to(DEV), depth.to(DEV).contiguous(), K.to(DEV), pose.to(DEV)
    with torch.no_grad():
        maps = fm.frame_maps(depth, K, pose)
        fm.associate(maps, K, pose)
        tape = torch.empty(L.query("e2e_pf_fuse_tape_bytes", H, W), device=DEV, dtype=torch.uint8)
        L.call("e2e_pf_fuse_tape", map_points=L.ptr(fm.points), map_colors=L.ptr(fm.colors), map_ccounts=L.ptr(fm.ccounts), M=M0,
               map_capacity=fm.cap, depth=L.ptr(depth), workspace=L.ptr(fm.ws), H=H, W=W, tape=L.ptr(tape), stream=L.stream())
        nbytes = L.query("e2e_pf_fuse_normals_tape_bytes", H, W)
        assert 12 * H * W <= nbytes <= 12 * H * W + 256                   # O(H*W), whatever the map
        ntape = torch.empty(nbytes, device=DEV, dtype=torch.uint8)
        L.call("e2e_pf_fuse_normals_tape", tape=L.ptr(tape), map_normals=L.ptr(fm.normals), M=M0, ntape=L.ptr(ntape), H=H, W=W,
               stream=L.stream())
        fm.fuse_append(maps, rgb, depth)
    unique, M1 = fm.table("unique").cpu(), fm.M
    gN = P.weights((M1, 3), 50)
    shapes = {"g_Ng": (H, W, 3), "g_prev_normals": (M0, 3), "g_alpha": (H, W), "g_prev_ccounts": (M0,)}
    priors = {k: P.weights(shapes[k], prior_seed + i) for i, k in enumerate(STEP_NAMES)}
    out = {}
    for k in STEP_NAMES:
        if k == null:
            out[k] = None
        elif accumulate and k in ("g_alpha", "g_prev_ccounts"):
            out[k] = priors[k].float().to(DEV).clone()
        else:
            out[k] = torch.full(shapes[k], float("nan"), device=DEV)
    L.call("e2e_pf_fuse_normals_bwd", tape=L.ptr(tape), ntape=L.ptr(ntape), Ng=L.ptr(maps["ng"]), alpha=L.ptr(maps["alpha"]),
           g_normals=L.ptr(gN.float().to(DEV)), ccounts_after=L.ptr(fm.ccounts), M_before=M0, M_after=M1, g_Ng=L.ptr(out["g_Ng"]),
           g_prev_normals=L.ptr(out["g_prev_normals"]), g_alpha=L.ptr(out["g_alpha"]), g_prev_ccounts=L.ptr(out["g_prev_ccounts"]),
           accumulate=accumulate, H=H, W=W, stream=L.stream())
    torch.cuda.synchronize()
    frame = dict(ng=maps["ng"][0].cpu().double(), alpha=maps["alpha"][0].cpu().double(), valid=depth.cpu() != 0)
    return M0, M1, unique, frame, gN, priors, out


def _two_step_state(H, W):
    rgbs, depths, K, poses = P.sequence(H, W)
    fm = _map(H, W)
    for f in (0, 1):
        fm.step(rgbs[f].to(DEV), depths[f].to(DEV), K.to(DEV), poses[f].to(DEV))
    return _state(fm), (rgbs[2], depths[2], K, poses[2])


@pytest.mark.parametrize("H,W", [(24, 32), (48, 64)])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_one_step_normals_entry_points(H, W, accumulate):
    prev, (rgb, depth, K, pose) = _two_step_state(H, W)
    M0, M1, unique, frame, gN, priors, got = _normals_step_gpu(H, W, prev, rgb, depth, K, pose, accumulate)
    valid = int(frame["valid"].sum())
    assert 0 < unique.shape[0] < min(M0, valid) and M1 > M0 and valid < H * W                          # fused, appended, unmatched, invalid
    state64 = {k: v.double() for k, v in prev.items()}
    want = dict(zip(STEP_NAMES, (lambda r: (r[0], r[2], r[1], r[3]))(N.fuse_normals_bwd_closed_form(state64, frame, unique, gN))))
    for k in STEP_NAMES:
        assert torch.isfinite(got[k]).all(), f"{k}: an element was not written"
        w = want[k] + priors[k] if accumulate and k in ("g_alpha", "g_prev_ccounts") else want[k]
        _check(f"normals step {k} ({H}x{W}, accumulate={accumulate})", got[k], w, STEP_BOUND[k])
    assert float(got["g_Ng"].cpu()[~frame["valid"]].abs().max()) == 0.0
    # each output NULL in turn: the others are the same bits; all NULL is refused
    for null in STEP_NAMES:
        _, _, _, _, _, _, other = _normals_step_gpu(H, W, prev, rgb, depth, K, pose, accumulate, null=null)
        assert other[null] is None and all(torch.equal(other[k], got[k]) for k in STEP_NAMES if k != null), null


# measured on the MI355X: g_alpha 3.2e-8, g_prev_ccounts 3.2e-8 (three-term float32 dot products)
ZERO_BOUND = {"g_alpha": 3.2e-7, "g_prev_ccounts": 3.2e-7}


def test_zero_confidence_everywhere_takes_the_undivided_form():
    """As tests/test_gpu_pointfusion_grad.py's case of the same name: a surface 30 m away, alpha = 0 everywhere, every map row (the
    frame's interior) wins its own pixel, s = 0: g_alpha = gN . Ng, g_prev_ccounts = gN . N, g_Ng = g_prev_normals = 0 for the fused."""
    from e2ehip import ops
    from test_gpu_pointfusion_grad import _pose
    H, W = 16, 24
    g = torch.Generator().manual_seed(7)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 30.0 + 0.05 * torch.sin(xs / 3.0) * torch.cos(ys / 4.0)
    rgb, K, pose = torch.rand(H, W, 3, generator=g), P.sequence(H, W)[2], _pose(2.0, -3.0, 1.0)
    m = ops.vertex_normal_maps(depth.to(DEV)[None], K.to(DEV)[None], pose.to(DEV)[None])
    assert float(m["alpha"].max()) == 0.0
    inner = torch.zeros(H, W, dtype=torch.bool)
    inner[:-1, :-1] = True
    k = int(inner.sum())
    prev = {"points": m["Vg"][0].cpu()[inner], "normals": m["ng"][0].cpu()[inner], "colors": torch.rand(k, 3, generator=g), "ccounts": torch.zeros(k)}
    M0, M1, unique, frame, gN, _, got = _normals_step_gpu(H, W, prev, rgb, depth, K, pose, 0)
    assert unique.shape[0] == k and torch.equal(unique[:, 0], torch.arange(k)) and M1 == H * W
    want = N.fuse_normals_bwd_closed_form({kk: v.double() for kk, v in prev.items()}, frame, unique, gN)
    assert float(got["g_prev_normals"].abs().max()) == 0.0 and float(got["g_Ng"].cpu()[inner].abs().max()) == 0.0
    assert torch.equal(got["g_Ng"].cpu()[~inner], gN.float()[M0:])                                    # the appended pixels: copies
    _check("zero confidence g_alpha", got["g_alpha"], want[1], ZERO_BOUND["g_alpha"])
    _check("zero confidence g_prev_ccounts", got["g_prev_ccounts"], want[3], ZERO_BOUND["g_prev_ccounts"])


# ---------------------------------------------------------------------------------------------------------------------
# 4. FusionMap.step_differentiable(normal_gradient=True)
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X, d sum(w . normals) / d depth of frame 0 / 1 / 2: 24x32 1.6e-7 / 4.2e-7 / 1.9e-7, 48x64 2.2e-7 / 2.4e-7 / 3.2e-7
SEQ_BOUND = 4.2e-6


def _sequence_run(H, W, normal_gradient, scalar):
    rgbs, depths, K, poses = P.sequence(H, W)
    fm = _map(H, W)
    d = [depths[f].to(DEV).requires_grad_(True) for f in range(3)]
    prev, states, outs = None, [], None
    for f in range(3):
        kw = dict(normal_gradient=True) if normal_gradient else {}
        Pt, Nn, Cl, cc = fm.step_differentiable(rgbs[f].to(DEV), d[f], K.to(DEV), poses[f].to(DEV), prev=prev, **kw)
        prev = (Pt, Cl, cc, Nn) if normal_gradient else (Pt, Cl, cc)
        states.append(_state(fm))
        outs = (Pt, Nn, Cl, cc)
    if scalar == "normals":
        (P.weights(tuple(outs[1].shape), 70).float().to(DEV) * outs[1]).sum().backward()
    else:
        sum((P.weights(tuple(t.shape), i).float().to(DEV) * t).sum() for i, t in enumerate((outs[0], outs[2], outs[3]))).backward()
    return outs, states, [torch.zeros_like(t) if t.grad is None else t.grad for t in d]


@pytest.mark.parametrize("H,W", [(24, 32), (48, 64)])
def test_step_differentiable_normal_gradient(H, W):
    from test_gpu_pointfusion_grad import _plain_chain
    rgbs, depths, K, poses = P.sequence(H, W)
    plain_states, uniques = _plain_chain(H, W)
    outs, states, grads = _sequence_run(H, W, True, "normals")
    assert outs[1].requires_grad and outs[1].grad_fn is not None
    for f in range(3):                                                    # forward values and the resident state: FusionMap.step's, bit for bit
        assert all(torch.equal(states[f][k], plain_states[f][k]) for k in plain_states[f]), f"step {f}"
    assert all(torch.equal(t.detach().cpu(), plain_states[2][k]) for t, k in zip(outs, ("points", "normals", "colors", "ccounts")))
    d64 = [x.double().requires_grad_(True) for x in depths]
    state = N.empty_state()
    for f in range(3):
        state = N.step(state, rgbs[f].double(), d64[f], K, poses[f], uniques[f])
    want = torch.autograd.grad((P.weights(tuple(state["normals"].shape), 70) * state["normals"]).sum(), d64)
    for f in range(3):
        _check(f"step_differentiable d sum(w . normals) / d depth[{f}] ({H}x{W})", grads[f], want[f], SEQ_BOUND)
        assert float(grads[f].abs().max()) > 0
    # switch off: normals without a graph, and the gradients of the other three are the same bits either way
    outs_off, _, g_off = _sequence_run(H, W, False, "cloud")
    assert outs_off[1].grad_fn is None and not outs_off[1].requires_grad
    _, _, g_on = _sequence_run(H, W, True, "cloud")
    assert all(torch.equal(a, b) for a, b in zip(g_on, g_off))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the whole chain
# ---------------------------------------------------------------------------------------------------------------------
class _Recorder:
    """tests/test_gpu_slam_chain_grad.py's recorder with the keywords passed through: keeps every discrete choice of the run."""

    def __init__(self):
        self.steps = [dict(unique=torch.zeros(0, 3, dtype=torch.int64), sel=None, records=None, normals=None)]
        self.traces, self.normal_kw = [], []

    def __enter__(self):
        import e2ehip.icp as icp_mod
        from e2ehip.fusionmap import FusionMap
        self.icp_mod, self.FusionMap = icp_mod, FusionMap
        self.real_ftm, self.real_step = icp_mod.frame_to_model, FusionMap.step_differentiable
        rec = self

        def frame_to_model(fmap, depth, K, prev_pose, **kw):
            normals = fmap.normals[:fmap.M].clone().cpu()
            pose, trace = rec.real_ftm(fmap, depth, K, prev_pose, **kw)
            rec.traces.append(list(trace))
            rec.pending = dict(sel=fmap.table("active")[::kw["dsratio"], 0].cpu(), records=C.forced_records(trace.iterations), normals=normals)
            return pose, trace

        def step_differentiable(fm, *args, **kw):
            rec.normal_kw.append(kw.get("normal_gradient", False))
            out = rec.real_step(fm, *args, **kw)
            rec.steps.append(dict(unique=fm.table("unique").cpu(), **rec.pending))
            return out

        icp_mod.frame_to_model, FusionMap.step_differentiable = frame_to_model, step_differentiable
        return self

    def __exit__(self, *exc):
        self.icp_mod.frame_to_model, self.FusionMap.step_differentiable = self.real_ftm, self.real_step


def _run_chain(H, W, normal_gradient):
    from gradslam.slam import PointFusion
    from gradslam.structures import RGBDImages
    from test_gpu_slam_chain_grad import DAMP, DS, _corner
    rgbs, depths, K, poses = _corner(3, H, W)
    d = [depths[f].to(DEV).requires_grad_(True) for f in range(3)]
    frames = RGBDImages(torch.stack([c.to(DEV) for c in rgbs])[None], torch.stack(d)[None, ..., None], K.to(DEV)[None, None], poses.to(DEV)[None])
    kw = dict(normal_gradient=True) if normal_gradient else {}
    slam = PointFusion(odom="gradicp", dsratio=DS, numiters=20, damp=DAMP, map_gradient=True, chain_gradient=True, device=DEV, **kw)
    with _Recorder() as rec:
        cloud, est = slam(frames)
    assert len(rec.steps) == 3 and rec.normal_kw == [normal_gradient] * 2
    lists = (cloud.points_list[0], cloud.colors_list[0], cloud.features_list[0].reshape(-1))
    s = sum((C.pose_weights(f).float().to(DEV) * est[0, f, :3]).sum() for f in range(3))
    s = s + sum((P.weights(tuple(t.shape), i).float().to(DEV) * t).sum() for i, t in enumerate(lists))
    s.backward()
    values = [t.detach() for t in lists] + [cloud.normals_list[0].detach()]
    return values, est[0].detach(), rec, [torch.zeros_like(t) if t.grad is None else t.grad for t in d], cloud.normals_list[0].requires_grad


# measured on the MI355X: d/d depth of frame 0 / 1 / 2 4.0e-6 / 1.8e-6 / 8.1e-7 (without the normals' graph the same chain measures 5.4e-7
# / 6.9e-7 / 8.5e-7, tests/test_gpu_slam_chain_grad.py: frames 0 and 1 now also receive the localisation's d/d tgt_n, 2.9e-5 of ITS
# largest entry on record there, as about a third of their gradient); the normals' graph moves frame 0's gradient by 0.33
WHOLE_CHAIN_BOUND = 4.0e-5


def test_whole_chain_with_normal_gradient():
    from test_gpu_slam_chain_grad import DAMP, DS, _corner
    H, W = 24, 32
    rgbs, depths, K, poses = _corner(3, H, W)
    values, est, rec, grads, attached = _run_chain(H, W, True)
    assert attached
    d64 = [x.double().requires_grad_(True) for x in depths]
    state, poses64 = N.chain([c.double() for c in rgbs], d64, K, poses[0], rec.steps, DS, numiters=20, damp=DAMP, mode="gradicp")
    want = torch.autograd.grad(C.scalar(state, poses64), d64)
    for f in range(3):
        _check(f"whole chain frame {f} d/d depth", grads[f], want[f], WHOLE_CHAIN_BOUND)
    values_off, est_off, rec_off, grads_off, attached_off = _run_chain(H, W, False)
    assert not attached_off
    assert torch.equal(est, est_off) and all(torch.equal(a, b) for a, b in zip(values, values_off)) and rec.traces == rec_off.traces
    moved = _rel(grads_off[0], grads[0])
    print(f"frame 0: the normals' graph moves the depth gradient by {moved:.3e} of its largest entry, "
          f"{moved / WHOLE_CHAIN_BOUND:.1f} times the bound")
    assert moved > 10 * WHOLE_CHAIN_BOUND


# ---------------------------------------------------------------------------------------------------------------------
# 6. train_depth's switch
# ---------------------------------------------------------------------------------------------------------------------
TRAIN_H, TRAIN_W = 64, 96                                                 # the smallest frame the network's five stride-2 stages take (reflection
                                                                          # padding needs two rows at the deepest one): train_depth's other switch tests' shape


def _train_step(normal_gradient):
    from e2ehip.synthetic import make_sequence
    from oracle import depthnet
    from train_depth import Depth_Estimation, default_config
    cfg = default_config(TRAIN_H, TRAIN_W, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.DATA.use_gt_pose = False
    cfg.MODEL.odom = "gradicp"
    cfg.LOSS.knn_points = False
    seq = make_sequence(2, TRAIN_H, TRAIN_W, seed=5, scene="corner")
    sd = depthnet.random_state_dict(0)
    sd["decoder.decoder.10.conv.weight"] = sd["decoder.decoder.10.conv.weight"] * 40.0       # depth with relief: the odometry has something to hold
    de = Depth_Estimation(cfg, sequence=seq, state_dict=sd, fused_losses=False)
    assert de.normal_gradient is False                                    # E2E_NORMAL_GRAD is off by default
    de.map_gradient, de.chain_gradient, de.normal_gradient = True, True, normal_gradient
    with contextlib.redirect_stdout(io.StringIO()):
        log = de.train()
    grads = torch.cat([p.grad.reshape(-1) for p in de.train_params if p.requires_grad and p.grad is not None]).clone()
    assert de.models["SLAM"].normal_gradient is normal_gradient and de.models["SLAM"].chain_gradient is True
    return log[0], grads


def test_train_depth_normal_gradient_switch(monkeypatch):
    for name in ("E2E_NORMAL_GRAD", "E2E_CHAIN_GRAD", "E2E_MAP_GRAD"):
        monkeypatch.delenv(name, raising=False)
    loss_on, g_on = _train_step(True)
    loss_off, g_off = _train_step(False)
    print(f"loss {loss_on:.6f}; |g_on - g_off| / |g_off| {float((g_on - g_off).norm() / g_off.norm()):.3e}")
    assert np.isfinite(loss_on) and loss_on == loss_off                   # the forward is the same
    assert torch.isfinite(g_on).all() and torch.isfinite(g_off).all() and not torch.equal(g_on, g_off)
