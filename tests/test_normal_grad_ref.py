"""Pins tests/normal_grad_ref.py, the float64 reference of the normals' gradient that tests/test_gpu_normal_grad.py compares the GPU
with.  CPU only.
  (a) its normal maps on float32 inputs are oracle.pointfusion.vertex_normal_maps' (float32) to 1e-5 of the largest entry;
  (b) the closed forms of include/e2eslam.h (e2e_normal_maps_bwd in its scatter and its gather form, the normals' fuse rule of
      e2e_pf_fuse_normals_bwd, the pose term of ng = R n) are what autograd finds, to 1e-12;
  (c) float64 central differences agree to 1e-6 on twenty depth entries of a 6x8 frame away from nrm == 0;
  (d) on the 5x7 frame that holds every nrm == 0 case all gradients are finite and are those the stated rule gives.

Measured here: (a) n 2.1e-7 / 1.5e-6, ng 2.2e-7 / 1.5e-6 (5x7 / 24x32: the oracle's float32 differences of neighbouring vertices);
(b) at most 3.5e-16; (c) 2.4e-10; the normals' graph adds 0.32 / 0.10 / 0 of the largest entry to the chain's depth gradient of frame
0 / 1 / 2 (the last frame's normals are read by no later localisation)."""
import pytest
import torch

import normal_grad_ref as N
import pointfusion_grad_ref as P
import icp_grad_ref as I
from oracle import pointfusion as opf

F64 = torch.float64
POSE = I.se3_exp(torch.tensor([0.3, -0.2, 0.1, 0.2, -0.1, 0.3], dtype=F64)).float()


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


def _intrinsics(H, W):
    from e2ehip.synthetic import icl_intrinsics
    return icl_intrinsics(H, W)


def _frame(H, W, seed, hole=True):
    g = torch.Generator().manual_seed(seed)
    depth = 1.5 + torch.rand(H, W, generator=g)
    if hole:
        depth[2:4, 3:5] = 0
    return depth, _intrinsics(H, W)


@pytest.mark.parametrize("H,W", [(5, 7), (24, 32)])
def test_normal_maps_are_the_oracles(H, W):
    depth, K = (N.degenerate_frame()[0], _intrinsics(5, 7)) if (H, W) == (5, 7) else _frame(H, W, 3)
    want = opf.vertex_normal_maps(depth, K, POSE)
    n, ng, valid = N.frame_normal_maps(depth.double(), K, POSE)
    for name, got, ref in (("n", n, want["n"]), ("ng", ng, want["ng"])):
        e = _rel(got, ref)
        print(f"{name} vs the float32 oracle ({H}x{W}): {e:.2e}")
        assert e <= 1e-5
    assert torch.equal(valid, depth != 0)


def _autograd_maps(depth, K, pose, wn, wng):
    d, p = depth.double().requires_grad_(True), pose.double().requires_grad_(True)
    n, ng, _ = N.frame_normal_maps(d, K, p)
    s = 0
    if wn is not None:
        s = s + (wn * n).sum()
    if wng is not None:
        s = s + (wng * ng).sum()
    grads = torch.autograd.grad(s, [d, p], allow_unused=True)
    return grads[0], grads[1], n.detach()


@pytest.mark.parametrize("mode", ["n", "ng", "both"])
@pytest.mark.parametrize("H,W", [(5, 7), (6, 8)])
def test_normal_map_closed_forms_are_the_autograd(H, W, mode):
    depth, K = (N.degenerate_frame()[0], _intrinsics(5, 7)) if (H, W) == (5, 7) else _frame(H, W, 11)
    wn = P.weights((H, W, 3), 1) if mode != "ng" else None
    wng = P.weights((H, W, 3), 2) if mode != "n" else None
    gd, gp, n = _autograd_maps(depth, K, POSE, wn, wng)
    assert torch.isfinite(gd).all()
    for name, f in (("scatter", N.normal_maps_bwd_closed_form), ("gather", N.normal_maps_bwd_gather)):
        got = f(depth.double(), K, POSE, wn, wng)
        e = _rel(got, gd)
        print(f"{name} form vs autograd ({H}x{W}, {mode}): {e:.2e}")
        assert e <= 1e-12
        assert float(got[depth == 0].abs().max()) == 0.0
    if wng is not None:                                                   # the pose term: the left 3x3 block, nothing else
        want = torch.zeros(4, 4, dtype=F64)
        want[:3, :3] = N.pose_term_closed_form(n, wng)
        assert _rel(gp, want) <= 1e-12 and float(gp[:, 3].abs().max()) == 0.0 == float(gp[3].abs().max())


def test_normal_map_gradient_is_the_central_difference():
    H, W = 6, 8
    depth, K = _frame(H, W, 11, hole=False)
    depth[3, 4] = 0                                                       # one invalid pixel
    wn, wng = P.weights((H, W, 3), 1), P.weights((H, W, 3), 2)
    gd, _, _ = _autograd_maps(depth, K, POSE, wn, wng)
    d64 = depth.double()

    def value(idx, delta):
        d = d64.clone()
        d[idx] += delta
        n, ng, _ = N.frame_normal_maps(d, K, POSE)
        return float((wn * n).sum() + (wng * ng).sum())

    # twenty entries away from the nrm == 0 pixels: not the last row or column, not the invalid pixel or one of its eight neighbours
    entries = [(h, w) for h in range(0, 5) for w in range(0, 7) if not (2 <= h <= 4 and 3 <= w <= 5)][3:23]
    _, _, is_zero = N._cross_adjoints(d64, K, POSE, None, None)
    assert len(entries) == 20 and all(float(d64[e]) != 0 and not bool(is_zero[e]) for e in entries)
    h, worst = 1e-6, 0.0
    for idx in entries:
        fd = (value(idx, h) - value(idx, -h)) / (2 * h)
        worst = max(worst, abs(fd - float(gd[idx])) / float(gd.abs().max()))
    print(f"central differences: {worst:.2e}")
    # unit normals of triangles whose sides are about 5e-3 long: third derivatives of order 1 / side^2 times h^2 = 1e-12 leave 4e-8,
    # the rounding of a float64 sum of 288 terms of order 1 over 2h leaves 2e-8, against a largest entry of order 1e2
    assert worst <= 1e-6


def test_degenerate_frame_is_finite_and_follows_the_rule():
    depth, zero = N.degenerate_frame()
    K = _intrinsics(5, 7)
    H, W = depth.shape
    assert depth[1, 2] != 0 and depth[1, 3] == 0 and depth[2, 2] == 0 and depth[3, 4] == 0
    d = depth.double()
    _, _, is_zero = N._cross_adjoints(d, K, POSE, None, None)
    assert sorted(zero) == sorted((int(h), int(w)) for h, w in (is_zero & (depth != 0)).nonzero().tolist())
    wn, wng = P.weights((H, W, 3), 1), P.weights((H, W, 3), 2)
    gd, gp, n = _autograd_maps(depth, K, POSE, wn, wng)
    assert torch.isfinite(gd).all() and torch.isfinite(gp).all() and torch.isfinite(n).all()
    assert float(n[is_zero].abs().max()) == 0.0                           # c = 0 over the constant 1
    assert _rel(N.normal_maps_bwd_closed_form(d, K, POSE, wn, wng), gd) <= 1e-12
    # at a nrm == 0 pixel gc = gn.  (1,2): dh = dv = -V, so g_dh + g_dv = dv x gn + gn x dh = 0 and the pixel sends nothing, to
    # itself or to anyone; last column: dh is the constant 0, so g_dv = gn x 0 = 0 and g_dh goes nowhere: nothing either.
    # So only pixels with nrm != 0 contribute, and zeroing the upstream gradient at the nrm == 0 pixels changes nothing.
    mask = (~is_zero).to(F64)[..., None]
    assert torch.equal(N.normal_maps_bwd_closed_form(d, K, POSE, wn * mask, wng * mask), N.normal_maps_bwd_closed_form(d, K, POSE, wn, wng))
    # the rule itself at (1,2), spelled out: gc = gn there, and the two cross products cancel
    g_dh, g_dv, _ = N._cross_adjoints(d, K, POSE, wn, wng)
    gn = wn[1, 2] + POSE.double()[:3, :3].T @ wng[1, 2]
    V = N._rays(K, H, W)[1, 2] * d[1, 2]
    assert _rel(g_dh[1, 2], N._cross(-V, gn)) <= 1e-12 and _rel(g_dv[1, 2], N._cross(gn, -V)) <= 1e-12
    assert float((g_dh[1, 2] + g_dv[1, 2]).abs().max()) == 0.0
    assert float(gd[depth == 0].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the normals' fuse rule
# ---------------------------------------------------------------------------------------------------------------------
def _two_step_state(H, W):
    """The float32 oracle's map after two steps of pointfusion_grad_ref.sequence and the third step's frame and unique table: fused,
    appended, unmatched and invalid pixels, rows that win a pixel and rows that do not."""
    rgbs, depths, K, poses = P.sequence(H, W)
    st = opf.empty_state()
    for f in (0, 1):
        st, _ = opf.pointfusion_step(st, rgbs[f], depths[f], K, poses[f])
    _, tab = opf.pointfusion_step(st, rgbs[2], depths[2], K, poses[2])
    return st, (rgbs[2], depths[2], K, poses[2]), tab["unique"]


@pytest.mark.parametrize("zero_confidence", [False, True])
def test_fuse_normals_closed_form_is_the_autograd(zero_confidence):
    H, W = 24, 32
    st, (rgb, depth, K, pose), unique = _two_step_state(H, W)
    M = st["points"].shape[0]
    assert 0 < unique.shape[0] < M
    state = {k: v.double() for k, v in st.items()}
    fr = N.frame(rgb.double(), depth.double(), K, pose)
    # The rule is algebra on the given table, so the values are free.  The scene's own normals agree between frames to 1e-5, and
    # autograd forms N/s - N'/s from two terms 1e5 times their difference: ITS float64 rounding would then be 2e-11 of the result.
    # Unit normals in general position and confidences of order 1 keep the reference's own error at the 1e-16 of its format.
    g = torch.Generator().manual_seed(3)
    state["normals"] = torch.nn.functional.normalize(torch.randn(M, 3, generator=g, dtype=F64), dim=1)
    state["ccounts"] = 0.5 + torch.rand(M, generator=g, dtype=F64)
    fr["alpha"] = (0.5 + torch.rand(H, W, generator=g, dtype=F64)) * fr["valid"]
    if zero_confidence:
        # every confidence 0, as in test_zero_confidence_everywhere_takes_the_undivided_form: the map is the rows that win a pixel (a
        # zero-confidence row that wins none sits on the jump of c N / where(c == 0, 1, c), where the rule passes nothing to c)
        order = torch.argsort(unique[:, 0])
        unique = unique[order]
        state = {k: v[unique[:, 0]] for k, v in state.items()}
        unique = torch.stack([torch.arange(unique.shape[0]), unique[:, 1], unique[:, 2]], 1)
        state["ccounts"] = torch.zeros_like(state["ccounts"])
        fr["alpha"] = torch.zeros_like(fr["alpha"])
    leaves = [state["normals"].requires_grad_(True), state["ccounts"].requires_grad_(True), fr["ng"].requires_grad_(True),
              fr["alpha"].requires_grad_(True)]
    out = N.fuse(state, fr, unique)
    gN = P.weights(tuple(out["normals"].shape), 7)
    want = torch.autograd.grad((gN * out["normals"]).sum(), leaves)
    g_ng, g_alpha, g_prevN, g_prevcc = N.fuse_normals_bwd_closed_form(state, fr, unique, gN)
    for name, got, ref in (("g_prev_normals", g_prevN, want[0]), ("g_prev_ccounts", g_prevcc, want[1]), ("g_ng", g_ng, want[2]),
                           ("g_alpha", g_alpha, want[3])):
        e = _rel(got, ref) if float(ref.abs().max()) > 0 else float(got.abs().max())
        print(f"{name} (zero confidence {zero_confidence}): {e:.2e}")
        assert e <= 1e-12 and torch.isfinite(got).all()
    if zero_confidence:
        assert float(g_prevN.abs().max()) == 0.0 and float(g_alpha.abs().max()) > 0.0 and float(g_prevcc.abs().max()) > 0.0


def test_chain_with_normals_moves_the_depth_gradient():
    """The extended chain runs on the discrete choices of slam_chain_grad_ref's free run and its normals are the oracle's; the
    normals' graph changes the depth gradient of every frame that built the map."""
    import slam_chain_grad_ref as C
    import test_slam_chain_grad_ref as T
    rgbs, depths, K, poses_gt = T._sequence()
    steps, st32, _, _ = T._free_run("gradicp")
    kw = dict(numiters=20, damp=T.DAMP, mode="gradicp", nu=200.0)
    d64 = [d.double().requires_grad_(True) for d in depths]
    state, poses = N.chain([c.double() for c in rgbs], d64, K, poses_gt[0], steps, T.DS, **kw)
    e = _rel(state["normals"].detach(), st32["normals"])
    print(f"final normals vs the float32 oracle: {e:.2e}")
    assert e <= 1e-5
    with_normals = torch.autograd.grad(C.scalar(state, poses), d64)
    state0, poses0 = C.chain([c.double() for c in rgbs], d64, K, poses_gt[0], steps, T.DS, **kw)
    without = torch.autograd.grad(C.scalar(state0, poses0), d64)
    # (slam_chain_grad_ref.chain localises against the oracle's float32 normals, this chain against its own float64 ones)
    assert all(_rel(a.detach(), b.detach()) <= 1e-5 for a, b in zip(poses, poses0))
    moved = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(with_normals, without)]
    print("share of the depth gradient the normals add:", [f"{m:.3f}" for m in moved])
    assert all(torch.isfinite(g).all() for g in with_normals) and moved[0] > 1e-3 and moved[1] > 1e-3
