"""The differentiable PointFusion map step (csrc/pointfusion_grad.hip, e2ehip/fusion_grad.py, gradslam.slam.PointFusion(map_gradient=True),
train_depth's E2E_MAP_GRAD) against tests/pointfusion_grad_ref.py, the float64 restatement that tests/test_pointfusion_grad_ref.py pins on
the CPU.  The reference is fed the `unique` table the GPU step itself found (FusionMap.table("unique"), which
tests/test_gpu_pointfusion_knn.py pins bit-exact to the oracle), so every element is compared, none excluded.

Scenes: e2ehip.synthetic.make_sequence(3, H, W, seed=5) with the hole depth[2:5, 3:9] = 0 in every frame, at 24x32 and 48x64 (at 48x64
step 3 has 2779 unique rows against 2826 similar ones: several map points contend for one pixel).

Every figure is the largest absolute difference relative to the largest entry of the compared float64 tensor; each bound is ten times
the figure measured on the MI355X (written next to it), and never above 1e-4, the project's figure for tensors compared with float64."""
import contextlib
import functools
import io
import math

import numpy as np
import pytest
import torch

import pointfusion_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(24, 32), (48, 64)]
NAMES = ("points", "colors", "ccounts")


def _rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def _check(name, got, want, bound):
    assert tuple(got.shape) == tuple(want.shape), f"{name}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    e = _rel(got, want)
    print(f"{name}: rel {e:.3e} (bound {bound:.1e}), max|ref| {float(want.abs().max()):.3e}")
    assert bound <= 1e-4
    assert e <= bound, f"{name}: {e:.3e} > {bound:.1e}"


def _pose(rx=0.0, ry=0.0, rz=0.0):
    a, b, c = (math.radians(v) for v in (rx, ry, rz))
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]], dtype=torch.float32)
    Ry = torch.tensor([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]], dtype=torch.float32)
    Rz = torch.tensor([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]], dtype=torch.float32)
    T = torch.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    return T


def _map(H, W, state=None):
    from e2ehip.fusionmap import FusionMap
    fm = FusionMap(4 * H * W, H, W, DEV)
    if state is not None:
        fm.load_state(*(state[k].to(DEV) for k in ("points", "normals", "colors", "ccounts")))
    return fm


def _state(fm):
    return {k: t.clone().cpu() for k, t in zip(("points", "normals", "colors", "ccounts"), fm.live())}


@functools.lru_cache(maxsize=None)
def _plain_chain(H, W):
    """FusionMap.step over the three frames: the map after every step and the unique table every step found (CPU tensors)."""
    rgbs, depths, K, poses = R.sequence(H, W)
    fm = _map(H, W)
    states, uniques = [], []
    for f in range(3):
        fm.step(rgbs[f].to(DEV), depths[f].to(DEV), K.to(DEV), poses[f].to(DEV))
        uniques.append(fm.table("unique").cpu())
        states.append(_state(fm))
    assert uniques[0].shape[0] == 0 and uniques[2].shape[0] == {(24, 32): 659, (48, 64): 2779}[H, W]
    return states, uniques


@functools.lru_cache(maxsize=None)
def _chain_reference(H, W):
    """float64: d R.scalar(final map) / d (depth, rgb) of every frame, with the GPU's tables."""
    rgbs, depths, K, poses = R.sequence(H, W)
    _, uniques = _plain_chain(H, W)
    d64 = [d.double().requires_grad_(True) for d in depths]
    c64 = [c.double().requires_grad_(True) for c in rgbs]
    state = R.chain(c64, d64, K, poses, uniques)
    grads = torch.autograd.grad(R.scalar(state), d64 + c64)
    return {k: v.detach() for k, v in state.items()}, grads[:3], grads[3:]


def _scalar32(points, colors, ccounts):
    """R.scalar on device tensors, with the same weights rounded to float32."""
    return sum((R.weights(tuple(t.shape), i).float().to(DEV) * t).sum() for i, t in enumerate((points, colors, ccounts.reshape(-1))))


# ---------------------------------------------------------------------------------------------------------------------
# 1. one step at the level of the entry points; 6. reproducible
# ---------------------------------------------------------------------------------------------------------------------
def _one_step_gpu(H, W, prev, rgb, depth, K, pose, up):
    """maps -> associate -> tape -> fuse/append -> e2e_pf_fuse_bwd -> e2e_vertex_maps_bwd + e2e_vertex_alpha_bwd, called by name.
    up: {name: (M_after, ...) gradient or None}.  -> M_after, unique, the five gradients."""
    from e2ehip import _lib as L, ops
    fm = _map(H, W, prev)
    M0 = fm.M
    rgb, depth, K, pose = rgb.to(DEV), depth.to(DEV).contiguous(), K.to(DEV), pose.to(DEV)
    with torch.no_grad():
        maps = fm.frame_maps(depth, K, pose)
        fm.associate(maps, K, pose)
        tape = torch.empty(L.query("e2e_pf_fuse_tape_bytes", H, W), device=DEV, dtype=torch.uint8)
        L.call("e2e_pf_fuse_tape", map_points=L.ptr(fm.points), map_colors=L.ptr(fm.colors), map_ccounts=L.ptr(fm.ccounts), M=M0,
               map_capacity=fm.cap, depth=L.ptr(depth), workspace=L.ptr(fm.ws), H=H, W=W, tape=L.ptr(tape), stream=L.stream())
        fm.fuse_append(maps, rgb, depth)
    unique, M1 = fm.table("unique").cpu(), fm.M
    g = {k: (None if v is None else v(M1).float().to(DEV)) for k, v in up.items()}
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    gVg, grgb, galpha, gpP, gpC, gpcc = nan(H, W, 3), nan(H, W, 3), nan(H, W), nan(M0, 3), nan(M0, 3), nan(M0)
    L.call("e2e_pf_fuse_bwd", tape=L.ptr(tape), Vg=L.ptr(maps["Vg"]), rgb=L.ptr(rgb), alpha=L.ptr(maps["alpha"]), g_points=L.ptr(g["points"]),
           g_colors=L.ptr(g["colors"]), g_ccounts=L.ptr(g["ccounts"]), ccounts_after=L.ptr(fm.ccounts), M_before=M0, M_after=M1,
           g_Vg=L.ptr(gVg), g_rgb=L.ptr(grgb), g_alpha=L.ptr(galpha), g_prev_points=L.ptr(gpP), g_prev_colors=L.ptr(gpC),
           g_prev_ccounts=L.ptr(gpcc), H=H, W=W, stream=L.stream())
    gd = nan(H, W)
    L.call("e2e_vertex_maps_bwd", L.ptr(depth), L.ptr(K), L.ptr(pose), None, L.ptr(gVg), L.ptr(gd), 1, H, W, L.stream())
    L.call("e2e_vertex_alpha_bwd", depth=L.ptr(depth), K=L.ptr(K), alpha=L.ptr(maps["alpha"]), g_alpha=L.ptr(galpha),
           alpha_den=float(ops.fusion_alpha_den(fm.sigma)), g_depth=L.ptr(gd), accumulate=1, B=1, H=H, W=W, stream=L.stream())
    torch.cuda.synchronize()
    return M1, unique, (gd, grgb, gpP, gpC, gpcc)


def _one_step_reference(prev, rgb, depth, K, pose, unique, up):
    d, c = depth.double().requires_grad_(True), rgb.double().requires_grad_(True)
    st = {k: prev[k].double().requires_grad_(True) for k in NAMES}
    out = R.step(st, c, d, K, pose, unique)
    s = sum((up[k](out[k].shape[0]) * out[k]).sum() for k in NAMES if up[k] is not None)
    return torch.autograd.grad(s, [d, c, st["points"], st["colors"], st["ccounts"]], allow_unused=True)


# measured on the MI355X, the largest over both shapes and the four upstream cases:
#   d/d depth 4.1e-7, d/d rgb 3.7e-7, d/d prev points 2.7e-7, d/d prev colors 3.7e-7, d/d prev ccounts 7.8e-6
# (prev ccounts: its entries are gP . (P - P') / s with |P - P'| of millimetres between float32 positions of metres -- the float64
# side recomputes Vg from the depth, the float32 forward rounded it to 2e-7 m -- and s about 4e-3; the largest entry is 1e4 to 1e5)
ONE_STEP_BOUND = {"depth": 4.1e-6, "rgb": 3.7e-6, "prev points": 2.7e-6, "prev colors": 3.7e-6, "prev ccounts": 7.8e-5}


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("null", [None, "points", "colors", "ccounts"])
def test_one_step_entry_points(H, W, null):
    rgbs, depths, K, poses = R.sequence(H, W)
    states, _ = _plain_chain(H, W)
    prev = states[1]                                                       # the map two frames built; frame 2 is the live one
    up = {k: (None if k == null else (lambda M, i=i, k=k: R.weights((M,) if k == "ccounts" else (M, 3), 10 + i))) for i, k in enumerate(NAMES)}
    M1, unique, got = _one_step_gpu(H, W, prev, rgbs[2], depths[2], K, poses[2], up)
    assert M1 == states[2]["points"].shape[0] and 0 < unique.shape[0] < int((depths[2] != 0).sum())        # fused, appended and invalid pixels
    want = _one_step_reference(prev, rgbs[2], depths[2], K, poses[2], unique, up)
    for name, g, w in zip(ONE_STEP_BOUND, got, want):
        assert torch.isfinite(g).all(), f"{name}: an element was not written"
        if w is None:                                                     # nothing upstream depends on it (colours with g_colors NULL)
            assert float(g.abs().max()) == 0.0, name
            continue
        _check(f"one step {name} (NULL: {null})", g, w, ONE_STEP_BOUND[name])
    _, _, again = _one_step_gpu(H, W, prev, rgbs[2], depths[2], K, poses[2], up)
    assert all(torch.equal(a, b) for a, b in zip(got, again))             # a gather, no atomics: bitwise reproducible


# ---------------------------------------------------------------------------------------------------------------------
# 2. forward equality
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
def test_forward_is_bitwise_the_plain_step(H, W):
    rgbs, depths, K, poses = R.sequence(H, W)
    states, uniques = _plain_chain(H, W)
    fm = _map(H, W)
    for f in range(3):
        d = depths[f].to(DEV).requires_grad_(True)
        P, Nn, C, cc = fm.step_differentiable(rgbs[f].to(DEV), d, K.to(DEV), poses[f].to(DEV))
        assert torch.equal(fm.table("unique").cpu(), uniques[f])
        live = _state(fm)
        for k, t in zip(("points", "normals", "colors", "ccounts"), (P, Nn, C, cc)):
            assert t.shape[0] == fm.M == states[f][k].shape[0], f"step {f}: map size"
            assert torch.equal(t.detach().cpu(), states[f][k]) and torch.equal(live[k], states[f][k]), f"step {f}: {k} differ from FusionMap.step"
        assert P.requires_grad and C.requires_grad and cc.requires_grad and not Nn.requires_grad
        assert P.data_ptr() != fm.points.data_ptr()                       # tensors of their own: a later in-place step cannot change them


# ---------------------------------------------------------------------------------------------------------------------
# 3. three-frame chain through the module; 6. reproducible
# ---------------------------------------------------------------------------------------------------------------------
def _frames(H, W, attach):
    from gradslam.structures import RGBDImages
    rgbs, depths, K, poses = R.sequence(H, W)
    d = [depths[f].to(DEV).requires_grad_(f in attach) for f in range(3)]
    c = [rgbs[f].to(DEV).requires_grad_(f in attach) for f in range(3)]
    frames = RGBDImages(torch.stack(c)[None], torch.stack(d)[None, ..., None], K.to(DEV)[None, None], poses.to(DEV)[None])
    return frames, d, c


# measured on the MI355X (24x32 / 48x64), the largest of the three frames: d/d depth 7.8e-7 / 7.5e-7, d/d rgb 2.7e-7 / 3.0e-7; the final
# map's values (points, colors, ccounts) 5.6e-7 / 5.6e-7
CHAIN_BOUND = {"depth": 7.8e-6, "rgb": 3.0e-6, "values": 5.6e-6}


@pytest.mark.parametrize("H,W", SHAPES)
def test_three_frame_chain_through_pointfusion(H, W):
    from gradslam.slam import PointFusion
    state64, gd64, gc64 = _chain_reference(H, W)
    grads = []
    for _ in range(2):
        frames, d, c = _frames(H, W, attach=(0, 1, 2))
        cloud, _ = PointFusion(odom="gt", map_gradient=True, device=DEV)(frames)
        P, C, cc = cloud.points_list[0], cloud.colors_list[0], cloud.features_list[0]
        assert P.requires_grad and C.requires_grad and cc.requires_grad and not cloud.normals_list[0].requires_grad
        _scalar32(P, C, cc).backward()
        grads.append([t.grad.clone() for t in d + c])
    for k, t in zip(NAMES, (P, C, cc.reshape(-1))):
        _check(f"chain final {k}", t.detach(), state64[k], CHAIN_BOUND["values"])
    for f in range(3):
        _check(f"chain frame {f} d/d depth", grads[0][f], gd64[f], CHAIN_BOUND["depth"])
        _check(f"chain frame {f} d/d rgb", grads[0][3 + f], gc64[f], CHAIN_BOUND["rgb"])
        assert float(grads[0][f].abs().max()) > 0 and float(grads[0][3 + f].abs().max()) > 0          # frames 1 and 2 are reached too
    assert all(torch.equal(a, b) for a, b in zip(*grads))


# ---------------------------------------------------------------------------------------------------------------------
# 4. image_recover_slam
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X (24x32 / 48x64): d/d depth 7.8e-7 / 7.4e-7, d/d rgb 1.9e-7 / 2.9e-7
RECOVER_BOUND = {"depth": 7.8e-6, "rgb": 2.9e-6}


class _PerFrame:
    """The three frames as an RGBDImages-like sequence whose frames are separate leaves (a stacked tensor's backward hands zeros to
    every frame it was stacked from, which would hide whether the graph reaches the earlier ones)."""

    def __init__(self, H, W, d, c):
        from gradslam.structures import RGBDImages
        _, _, K, poses = R.sequence(H, W)
        self.shape = (1, 3, H, W)
        self.frames = [RGBDImages(c[f][None, None], d[f][None, None, ..., None], K.to(DEV)[None, None], poses[f].to(DEV)[None, None]) for f in range(3)]

    def __getitem__(self, index):
        return self.frames[index[1]]


@pytest.mark.parametrize("H,W", SHAPES)
def test_image_recover_slam_reaches_the_last_frame(H, W):
    from gradslam.slam import PointFusion
    from slam.custom_slam import image_recover_slam
    _, gd64, gc64 = _chain_reference(H, W)             # the last frame's gradient does not depend on whether the earlier ones are attached
    _, d, c = _frames(H, W, attach=(0, 1, 2))
    cloud = image_recover_slam(_PerFrame(H, W, d, c), PointFusion(odom="gt", map_gradient=True, device=DEV), DEV)
    _scalar32(cloud.points_list[0], cloud.colors_list[0], cloud.features_list[0]).backward()
    _check("image_recover_slam d/d depth", d[2].grad, gd64[2], RECOVER_BOUND["depth"])
    _check("image_recover_slam d/d rgb", c[2].grad, gc64[2], RECOVER_BOUND["rgb"])
    assert all(t.grad is None for t in d[:2] + c[:2])


# ---------------------------------------------------------------------------------------------------------------------
# 5. default off; 7c. nothing requires grad
# ---------------------------------------------------------------------------------------------------------------------
def test_default_off_and_no_graph_take_the_plain_path():
    from gradslam.slam import PointFusion
    H, W = SHAPES[0]
    states, _ = _plain_chain(H, W)
    for kw, attach in ((dict(), (0, 1, 2)), (dict(map_gradient=False), (0, 1, 2)), (dict(map_gradient=True), ())):
        frames, d, c = _frames(H, W, attach)
        cloud, _ = PointFusion(odom="gt", device=DEV, **kw)(frames)
        fm = cloud._fusion_maps
        for name, lst, res in (("points", cloud.points_list, fm.points), ("normals", cloud.normals_list, fm.normals),
                               ("colors", cloud.colors_list, fm.colors), ("ccounts", cloud.features_list, fm.ccounts)):
            assert not lst[0].requires_grad, f"{kw}: {name} carries a graph"
            assert lst[0].data_ptr() == res.data_ptr()                    # today's zero-copy views of the resident rows
            assert torch.equal(lst[0].reshape(states[2][name].shape).cpu(), states[2][name])
    with torch.no_grad():                                                 # grad mode off: the plain path whatever requires grad
        frames, d, c = _frames(H, W, (0, 1, 2))
        cloud, _ = PointFusion(odom="gt", map_gradient=True, device=DEV)(frames)
        assert cloud.points_list[0].data_ptr() == cloud._fusion_maps.points.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# 7. edges
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X: camera turned away d/d depth 7.1e-8, d/d rgb 0 (an appended pixel's colour gradient is a copy of its row's)
AWAY_BOUND = {"depth": 7.1e-7, "rgb": 0.0}


def _edge_step(depth, pose):
    """A differentiable step of frame 1 (with `depth`, seen from `pose`) onto the map frame 0 built, every input attached."""
    H, W = SHAPES[0]
    rgbs, _, K, _ = R.sequence(H, W)
    states, _ = _plain_chain(H, W)
    fm = _map(H, W, states[0])
    prev = [states[0][k].to(DEV).requires_grad_(True) for k in NAMES]
    d, c = depth.to(DEV).requires_grad_(True), rgbs[1].to(DEV).requires_grad_(True)
    P, Nn, C, cc = fm.step_differentiable(c, d, K.to(DEV), pose.to(DEV), prev=tuple(prev))
    up = [R.weights(tuple(t.shape), 20 + i).float().to(DEV) for i, t in enumerate((P, C, cc))]
    sum((u * t).sum() for u, t in zip(up, (P, C, cc))).backward()
    return fm, states[0], (P, C, cc), up, d, c, prev


def test_camera_turned_away_is_a_pure_append():
    H, W = SHAPES[0]
    rgbs, depths, K, _ = R.sequence(H, W)
    pose = _pose(0, 180, 0)
    fm, st0, out, up, d, c, prev = _edge_step(depths[1], pose)
    M0 = st0["points"].shape[0]
    assert fm.table("active").shape[0] == 0 and fm.M == M0 + int((depths[1] != 0).sum())
    assert all(torch.equal(o[:M0].detach().cpu(), st0[k]) for o, k in zip(out, NAMES))               # the old rows are untouched
    assert all(torch.equal(p.grad, u[:M0]) for p, u in zip(prev, up))                                  # ... and pass their gradient through
    d64, c64 = depths[1].double().requires_grad_(True), rgbs[1].double().requires_grad_(True)
    new = R.step(R.empty_state(), c64, d64, K, pose, torch.zeros(0, 3, dtype=torch.int64))
    gd, gc = torch.autograd.grad(sum((u[M0:].double().cpu() * new[k]).sum() for u, k in zip(up, NAMES)), [d64, c64])
    _check("turned away d/d depth", d.grad, gd, AWAY_BOUND["depth"])
    _check("turned away d/d rgb", c.grad, gc, AWAY_BOUND["rgb"])


def test_all_zero_depth_changes_nothing():
    H, W = SHAPES[0]
    _, _, _, poses = R.sequence(H, W)
    fm, st0, out, up, d, c, prev = _edge_step(torch.zeros(H, W), poses[1])
    M0 = st0["points"].shape[0]
    assert fm.M == M0 and all(torch.equal(o.detach().cpu(), st0[k]) for o, k in zip(out, NAMES))      # an unchanged map
    assert float(d.grad.abs().max()) == 0.0 and float(c.grad.abs().max()) == 0.0
    assert all(torch.equal(p.grad, u) for p, u in zip(prev, up))


# measured on the MI355X: d/d depth 1.6e-7, d/d rgb 0 (copies of the appended rows' gradients), d/d prev ccounts 7.8e-8 (d/d prev points
# and colors are exactly zero on both sides)
ZERO_BOUND = {"depth": 1.6e-6, "rgb": 0.0, "prev ccounts": 7.8e-7}


def test_zero_confidence_everywhere_takes_the_undivided_form():
    """A surface 30 m away: alpha = exp(-1250) is 0 in float32 and in float64, so every map row and every pixel has confidence 0 and the
    forward's divisor is where(c + a == 0, 1, .) = 1: X' = c X + a X_f.  Every map row here wins its own pixel (the map is the frame's
    interior), the last row and column (zero normals) are appended."""
    from e2ehip import ops
    H, W = 16, 24
    g = torch.Generator().manual_seed(7)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = 30.0 + 0.05 * torch.sin(xs / 3.0) * torch.cos(ys / 4.0)
    rgb, K, pose = torch.rand(H, W, 3, generator=g), R.sequence(H, W)[2], _pose(2.0, -3.0, 1.0)
    m = ops.vertex_normal_maps(depth.to(DEV)[None], K.to(DEV)[None], pose.to(DEV)[None])
    assert float(m["alpha"].max()) == 0.0
    inner = torch.zeros(H, W, dtype=torch.bool)
    inner[:-1, :-1] = True
    prev = {"points": m["Vg"][0].cpu()[inner], "normals": m["ng"][0].cpu()[inner], "colors": torch.rand(int(inner.sum()), 3, generator=g),
            "ccounts": torch.zeros(int(inner.sum()))}
    up = {k: (lambda M, i=i, k=k: R.weights((M,) if k == "ccounts" else (M, 3), 40 + i)) for i, k in enumerate(NAMES)}
    M1, unique, got = _one_step_gpu(H, W, prev, rgb, depth, K, pose, up)
    assert unique.shape[0] == (H - 1) * (W - 1) and torch.equal(unique[:, 0], torch.arange((H - 1) * (W - 1))) and M1 == H * W
    want = _one_step_reference(prev, rgb, depth, K, pose, unique, up)
    gd, grgb, gpP, gpC, gpcc = got
    assert float(gpP.abs().max()) == 0.0 == float(gpC.abs().max()) and float(want[2].abs().max()) == 0.0 == float(want[3].abs().max())
    assert float(grgb[inner.to(DEV)].abs().max()) == 0.0 and float(gd[inner.to(DEV)].abs().max()) == 0.0     # a = 0: the fused pixels weigh nothing
    _check("zero confidence d/d depth", gd, want[0], ZERO_BOUND["depth"])
    _check("zero confidence d/d rgb", grgb, want[1], ZERO_BOUND["rgb"])
    _check("zero confidence d/d prev ccounts", gpcc, want[4], ZERO_BOUND["prev ccounts"])


# ---------------------------------------------------------------------------------------------------------------------
# 8. argument contracts
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    from e2ehip import _lib as L
    H, W = 8, 12
    fm = _map(H, W)
    f = lambda *s: torch.zeros(*s, device=DEV)
    tape = torch.zeros(L.query("e2e_pf_fuse_tape_bytes", H, W), device=DEV, dtype=torch.uint8)
    assert L.query("e2e_pf_fuse_tape_bytes", 0, W) == 0 and L.query("e2e_pf_fuse_tape_bytes", H, -1) == 0
    assert 36 * H * W <= tape.numel() <= 36 * H * W + 1024                # O(H*W), whatever the map
    depth, Vg, rgb, alpha, K = f(H, W), f(H, W, 3), f(H, W, 3), f(H, W), torch.eye(4, device=DEV)
    M = 5
    gP, gC, gcc, out3, out1 = f(M, 3), f(M, 3), f(M), torch.full((H, W, 3), 7.0, device=DEV), torch.full((H, W), 7.0, device=DEV)

    def refused(name, good, **bad):
        with pytest.raises(L.E2EError, match=rf"{name} failed \(-1\)"):
            L.call(name, **{**good, **bad})

    good = dict(map_points=L.ptr(fm.points), map_colors=L.ptr(fm.colors), map_ccounts=L.ptr(fm.ccounts), M=M, map_capacity=fm.cap,
                depth=L.ptr(depth), workspace=L.ptr(fm.ws), H=H, W=W, tape=L.ptr(tape), stream=L.stream())
    for bad in (dict(depth=None), dict(workspace=None), dict(tape=None), dict(map_points=None), dict(map_colors=None), dict(map_ccounts=None),
                dict(H=0), dict(W=-3), dict(M=-1), dict(M=fm.cap + 1)):
        refused("e2e_pf_fuse_tape", good, **bad)
    good = dict(tape=L.ptr(tape), Vg=L.ptr(Vg), rgb=L.ptr(rgb), alpha=L.ptr(alpha), g_points=L.ptr(gP), g_colors=L.ptr(gC), g_ccounts=L.ptr(gcc),
                ccounts_after=L.ptr(gcc), M_before=M, M_after=M, g_Vg=L.ptr(out3), g_rgb=None, g_alpha=L.ptr(out1), g_prev_points=L.ptr(gP.clone()),
                g_prev_colors=None, g_prev_ccounts=None, H=H, W=W, stream=L.stream())
    for bad in (dict(tape=None), dict(Vg=None), dict(rgb=None), dict(alpha=None), dict(H=0), dict(W=0), dict(M_before=-1), dict(M_after=M - 1),
                dict(ccounts_after=None), dict(g_Vg=None, g_alpha=None, g_prev_points=None)):
        refused("e2e_pf_fuse_bwd", good, **bad)
    good = dict(depth=L.ptr(depth), K=L.ptr(K), alpha=L.ptr(alpha), g_alpha=L.ptr(alpha), alpha_den=0.72, g_depth=L.ptr(out1), accumulate=0,
                B=1, H=H, W=W, stream=L.stream())
    for bad in (dict(depth=None), dict(K=None), dict(alpha=None), dict(g_alpha=None), dict(g_depth=None), dict(B=0), dict(H=0), dict(W=0),
                dict(alpha_den=0.0)):
        refused("e2e_vertex_alpha_bwd", good, **bad)
    torch.cuda.synchronize()
    assert float(out3.min()) == 7.0 == float(out1.max())                  # refused before any launch


# ---------------------------------------------------------------------------------------------------------------------
# ops.vertex_normal_maps(alpha_grad=...)
# ---------------------------------------------------------------------------------------------------------------------
# measured on the MI355X: alpha only 3.3e-7, alpha and Vg together 1.5e-7
ALPHA_BOUND = 3.3e-6


def test_alpha_gradient_is_opt_in():
    from e2ehip import ops
    H, W = SHAPES[0]
    rgbs, depths, K, poses = R.sequence(H, W)
    wa, wv = R.weights((H, W), 30), R.weights((H, W, 3), 31)
    d64 = depths[1].double().requires_grad_(True)
    Vg, alpha, _ = R.frame_maps(d64, K, poses[1])
    (ga,) = torch.autograd.grad((wa * alpha).sum(), d64, retain_graph=True)
    (gb,) = torch.autograd.grad((wa * alpha).sum() + (wv * Vg).sum(), d64)
    args = (K.to(DEV)[None], poses[1].to(DEV)[None])
    d = depths[1].to(DEV)[None].requires_grad_(True)
    assert not ops.vertex_normal_maps(d, *args)["alpha"].requires_grad                # the default stays non-differentiable
    m = ops.vertex_normal_maps(d, *args, alpha_grad=True)
    assert m["alpha"].requires_grad and not m["ng"].requires_grad and not m["n"].requires_grad
    (m["alpha"][0] * wa.float().to(DEV)).sum().backward()
    _check("alpha only d/d depth", d.grad[0], ga, ALPHA_BOUND)
    d.grad = None
    m = ops.vertex_normal_maps(d, *args, alpha_grad=True)
    ((m["alpha"][0] * wa.float().to(DEV)).sum() + (m["Vg"][0] * wv.float().to(DEV)).sum()).backward()
    _check("alpha + Vg d/d depth", d.grad[0], gb, ALPHA_BOUND)
    assert float(d.grad[0, 2:5, 3:9].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 9. the driver's switch
# ---------------------------------------------------------------------------------------------------------------------
def _train_step(map_gradient):
    from e2ehip.synthetic import make_sequence
    from oracle import depthnet
    from train_depth import Depth_Estimation, default_config
    cfg = default_config(64, 96, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.LOSS.knn_points = True
    de = Depth_Estimation(cfg, sequence=make_sequence(2, 64, 96, seed=5), state_dict=depthnet.random_state_dict(0), fused_losses=False)
    assert de.map_gradient is False                                       # E2E_MAP_GRAD is off by default
    de.map_gradient = map_gradient
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
    assert len(seen) == 1 and de.models["SLAM"].map_gradient is map_gradient
    per_frame = [0.0 if seen[0].grad is None else float(seen[0].grad[0, f].abs().max()) for f in range(2)]
    return log[0], grads, per_frame


def test_train_depth_map_gradient_switch():
    loss_on, g_on, frames_on = _train_step(True)
    loss_off, g_off, frames_off = _train_step(False)
    print(f"loss {loss_on:.6f}; max |d loss / d depth| per frame: on {frames_on}, off {frames_off}; "
          f"|g_on - g_off| / |g_off| {float((g_on - g_off).norm() / g_off.norm()):.3e}")
    assert np.isfinite(loss_on) and loss_on == loss_off                   # the forward is the same
    assert torch.isfinite(g_on).all() and not torch.equal(g_on, g_off)
    assert all(v > 0 for v in frames_on)                                  # every frame's depth is reached through the map
    assert frames_off[1] == 0.0                                           # before: nothing beyond the frame that met the empty map
