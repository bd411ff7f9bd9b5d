"""Host-side half of tests/test_gpu_warp_photo_intrinsics.py: the gradient of the fused warp-photometric losses with respect to the camera
intrinsics K and inv_K (e2e_warp_photo_bwd_intrinsics, e2e_warp_photo_window_bwd_intrinsics, e2e_warp_photo_geo_bwd_intrinsics), of the two
operators (e2e_project3d_bwd_k, e2e_backproject_bwd_invk), and the CPU side of tensor_refine.learn_intrinsics.  Nothing here touches a GPU;
tests/test_warp_intrinsics_inputs.py proves what this docstring claims.

Scenes and admission are those of the family's reference modules, which this module imports and does not restate: the pair on
warp_contract_ref.fused_scene with warp_pose_ref.exclusions, the window on warp_window_ref (maps, candidates, first_min, window_case), the
geometric form on warp_geo_ref (maps, geometric_consistency, geo_case, admitted).  Their `maps` take K and inv_K from the scene they are
given, so a scene whose K and inv_K are leaves of the evaluation's dtype makes them variables of the same composition --
oracle.warp_loss.backproject -> project -> F.grid_sample -> photometric -- in float64 and float32.  K and inv_K are independent leaves: each
gradient is taken with the other held fixed, as the entry points define it.

Admission.  g_K and g_inv_K are sums over EVERY pixel, like g_T, so a case is admitted exactly where those modules admit a pose case: its
exclusion set is empty.  PAIR_CASES = warp_pose_ref.POSE_CASES; WINDOW_CASES = warp_window_ref.POSE_CASES at the modes of MODES, where the
one-source window with both flags off, (1,0,0), stands wherever (1,0,1) is admitted (one candidate: the same kink set without near-ties);
the geometric form is admitted by warp_geo_ref.admitted on the machine that runs the test, as in its own module.

Bound on max|g - a g64| of either matrix, the rule of warp_pose_ref.pose_bound: FACTOR x max|g32 - g64|, floored at FACTOR x 2^-24 x
max|g64|, raised to FACTOR x the largest max|g32 - g64| / max|g64| of that matrix over the admitted cases of the same form and
(pad, mask[, mode]) x this case's max|g64|, never above CAP x max|g64|.  All constants are warp_contract_ref's.

closed_form restates include/e2eslam.h's rule in float64 from the reference's own gradient of the sampling grid."""
import functools

import torch
import torch.nn.functional as F

import warp_contract_ref as R
import warp_geo_ref as G
import warp_pose_ref as P
import warp_window_ref as Wr
from oracle import warp_loss as wl
from warp_contract_ref import F32, F64

PAIR_CASES = list(P.POSE_CASES)
ZERO_CASE = P.ZERO_CASE                                               # every source index clamped: both gradients are exactly 0
EXPANDED_CASE = ((2, 9, 33), 1, 1)                                    # one (4,4) K / inv_K, the scene's first, behind both batch elements
PLAN_CASE = P.PLAN_CASE
MODES = [(2, 0, 0), (2, 1, 1), (1, 0, 0), (1, 1, 1)]                  # S = 2 and S = 1: flags off, min_reprojection + auto_masking
WINDOW_CASES = [c for c in Wr.POSE_CASES if c[3] in MODES] + [c[:3] + ((1, 0, 0),) for c in Wr.POSE_CASES if c[3] == (1, 0, 1)]
GEO_CASES = [(shape, pad, mask, mode) for shape in G.SHAPES for pad in (0, 1) for mask in (0, 1) for mode in MODES]
MATRICES = ("g_K", "g_invK")


def with_leaves(s, dt, expanded=False):
    """the scene with K and inv_K as leaves of dtype dt (expanded: the first (4,4) matrix of each behind every batch element)
    -> (scene for the modules' compositions, K leaf, inv_K leaf)"""
    Kl, iKl = (R.leaf(s[k][0] if expanded else s[k], dt) for k in ("K", "invK"))
    B = s["B"]
    s2 = dict(s, K=Kl.expand(B, 4, 4) if expanded else Kl, invK=iKl.expand(B, 4, 4) if expanded else iKl)
    return s2, Kl, iKl


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pair
# ---------------------------------------------------------------------------------------------------------------------------------------
def pair_composition(s, pad, use_mask, dt, expanded=False):
    B, H, W = s["B"], s["H"], s["W"]
    s2, Kl, iKl = with_leaves(s, dt, expanded)
    Tl, d = R.leaf(s["T"], dt), R.leaf(s["depth"], dt)
    pts = wl.backproject(d.view(B, 1, H, W), s2["invK"])
    grid, valid = wl.project(pts, s2["K"], Tl, H, W)
    synth = F.grid_sample(s["src"].to(dt), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=False)
    loss, _ = wl.masked_photometric_mean(synth, s["tgt"].to(dt), valid.to(dt), bool(use_mask))
    g_K, g_invK, g_T, g_d, g_grid = torch.autograd.grad(loss, (Kl, iKl, Tl, d, grid))
    return dict(loss=loss.detach(), g_K=g_K, g_invK=g_invK, g_T=g_T, g_depth=g_d, grid=grid.detach(), g_grid=g_grid, synth=synth.detach(),
                valid=valid.view(B, H, W), m=grid.detach().abs().amax(-1), pts=pts.detach(), K=s2["K"].detach(), invK=s2["invK"].detach())


@functools.lru_cache(maxsize=None)
def pair_case(shape, pad, use_mask, expanded=False):
    s = R.fused_scene(*shape)
    case = dict(scene=s, shape=shape, pad=pad, use_mask=use_mask, expanded=expanded, T=s["T"])
    for dt in (F64, F32):
        case[dt] = pair_composition(s, pad, use_mask, dt, expanded)
    case["grad_excluded"] = P.exclusions(s, case[F64], case[F32], pad, use_mask)
    return case


def closed_form(case):
    """the rule of include/e2eslam.h (e2e_warp_photo_bwd_intrinsics) in float64 from the reference's own g_grid:
    gc -> Pbar = sum gc [X;1]^T, Q = sum gc (d pix)^T -> g_K[:3,:] = Pbar T^T, g_inv_K[:3,:3] = P[:, :3]^T Q  -> (g_K, g_inv_K) (B,4,4)"""
    s, r = case["scene"], case[F64]
    B, H, W = case["shape"]
    K, T = r["K"], case["T"].double()
    Pm = torch.matmul(K, T)[:, :3, :]
    X = r["pts"]
    c = torch.matmul(Pm, X)
    z = c[:, 2] + 1e-7
    u, v = c[:, 0] / z, c[:, 1] / z
    gg = r["g_grid"].reshape(B, H * W, 2)
    gu, gv = gg[..., 0] * 2 / (W - 1), gg[..., 1] * 2 / (H - 1)
    gc = torch.stack([gu / z, gv / z, -(gu * u + gv * v) / z], 1)     # (B,3,N)
    Pbar = torch.matmul(gc, X.transpose(1, 2))                        # (B,3,4)
    dpix = s["depth"].double().view(B, 1, H * W) * wl.pixel_grid(B, H, W, F64)
    Q = torch.matmul(gc, dpix.transpose(1, 2))                        # (B,3,3)
    g_K, g_iK = torch.zeros(B, 4, 4, dtype=F64), torch.zeros(B, 4, 4, dtype=F64)
    g_K[:, :3, :] = torch.matmul(Pbar, T.transpose(1, 2))
    g_iK[:, :3, :3] = torch.matmul(Pm[:, :, :3].transpose(1, 2), Q)
    return g_K, g_iK


# ---------------------------------------------------------------------------------------------------------------------------------------
# the window and the geometric form
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _window_maps(shape, pad, use_mask, dt):
    s2, Kl, iKl = with_leaves(Wr.scene(*shape), dt)
    return s2, Kl, iKl, Wr.maps(s2, pad, use_mask, dt)


@functools.lru_cache(maxsize=None)
def window_case(shape, pad, use_mask, mode):
    """warp_window_ref.window_case (selection, exclusions, g_T, g_depth) plus g_K / g_invK of the same loss in both dtypes"""
    w = Wr.window_case(shape, pad, use_mask, mode)
    case = dict(scene=w["scene"], shape=shape, pad=pad, use_mask=use_mask, mode=mode, window=w, grad_excluded=w["grad_excluded"])
    for dt in (F64, F32):
        s2, Kl, iKl, base = _window_maps(shape, pad, use_mask, dt)
        pm, sel = Wr.first_min(Wr.candidates(base["rep"], base["idn"], mode, s2["noise"]))
        assert torch.equal(sel, w[dt]["select"])
        g = torch.autograd.grad(pm.mean(), (Kl, iKl), retain_graph=True)
        case[dt] = dict(g_K=g[0], g_invK=g[1], g_T=w[dt]["g_T"], g_depth=w[dt]["g_depth"], select=sel)
    return case


@functools.lru_cache(maxsize=None)
def _geo_maps(shape, pad, use_mask, dt):
    s2, Kl, iKl = with_leaves(G.scene(*shape), dt)
    return s2, Kl, iKl, G.maps(s2, pad, dt, use_mask)


@functools.lru_cache(maxsize=None)
def geo_case(shape, pad, use_mask, mode):
    """warp_geo_ref.geo_case (geo_min_valid = 0, G_LOSS) plus g_K / g_invK of g_loss[0] loss + sum_s g_loss[1 + s] G_s in both dtypes"""
    w = G.geo_case(shape, pad, use_mask, mode)
    S = mode[0]
    case = dict(scene=w["scene"], shape=shape, pad=pad, use_mask=use_mask, mode=mode, geo=w, admitted=G.admitted(w), g_loss=G.G_LOSS)
    for dt in (F64, F32):
        s2, Kl, iKl, base = _geo_maps(shape, pad, use_mask, dt)
        pm, sel = Wr.first_min(Wr.candidates(base["rep"], base["idn"], mode, s2["noise"]))
        total = G.G_LOSS[0] * pm.mean() + sum(G.G_LOSS[1 + k] * G.geometric_consistency(base["gsum"][k], base["n"][k], 0) for k in range(S))
        g = torch.autograd.grad(total, (Kl, iKl), retain_graph=True)
        case[dt] = dict(g_K=g[0], g_invK=g[1], g_T=w[dt]["g_T"], g_depth=w[dt]["g_depth"], g_ds=w[dt]["g_ds"], select=sel)
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------------------
def rel_error(case, which):
    g64, g32 = case[F64][which], case[F32][which].double()
    top = float(g64.abs().max())
    return float((g32 - g64).abs().max()) / top if top > 0 else 0.0


@functools.lru_cache(maxsize=None)
def pooled(form, which, pad, use_mask, mode=None):
    """the largest relative float32 error on matrix `which` over the admitted cases of this form and configuration"""
    if form == "pair":
        cases = [pair_case(*c) for c in PAIR_CASES if c[1:] == (pad, use_mask)]
    elif form == "window":
        cases = [window_case(*c) for c in WINDOW_CASES if c[1:] == (pad, use_mask, mode)]
    else:
        cases = [c for c in (geo_case(*k) for k in GEO_CASES if k[1:] == (pad, use_mask, mode)) if c["admitted"]]
    return max([rel_error(c, which) for c in cases] + [0.0])


def bound(form, case, which, a=1.0):
    """the bound on max|g - a g64| of matrix `which` ("g_K" | "g_invK") for the upstream factor a"""
    t64, t32 = a * case[F64][which], torch.tensor(a, dtype=F32) * case[F32][which]
    top = float(t64.abs().max())
    pool = pooled(form, which, case["pad"], case["use_mask"], case.get("mode"))
    return min(max(R.bound(t32, t64), R.FACTOR * pool * top), R.CAP * top)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the operators
# ---------------------------------------------------------------------------------------------------------------------------------------
OP_SHAPES = [(1, 3, 5), (2, 9, 33), (2, 17, 33), (1, 37, 53)]


@functools.lru_cache(maxsize=None)
def operator_case(B, H, W):
    """Project3D on the fused scene's own points with random upstream gradients, and BackprojectDepth with a random g_cam:
    float64 / float32 autograd with K (with and without g_z) and inv_K as leaves.  The scene's c2 lies in [0.5, 3.5], far above the clamp."""
    s = R.fused_scene(B, H, W)
    g = R.gen("I", B, H, W)
    N = H * W
    c = dict(scene=s, pts=wl.backproject(s["depth"].view(B, 1, H, W), s["invK"]), g_grid=torch.randn(B, H, W, 2, generator=g),
             g_z=torch.randn(B, H, W, generator=g), g_cam=torch.randn(B, 4, N, generator=g))
    for dt in (F64, F32):
        Kl, iKl = R.leaf(s["K"], dt), R.leaf(s["invK"], dt)
        grid, z, _ = wl.project(c["pts"].to(dt), Kl, s["T"].to(dt), H, W, geometric=True)
        a, b = (grid * c["g_grid"].to(dt)).sum(), (z.view(B, H, W) * c["g_z"].to(dt)).sum()
        g_plain, = torch.autograd.grad(a, Kl, retain_graph=True)
        g_with_z, = torch.autograd.grad(a + b, Kl)
        g_iK, = torch.autograd.grad((wl.backproject(s["depth"].to(dt).view(B, 1, H, W), iKl) * c["g_cam"].to(dt)).sum(), iKl)
        c[dt] = dict(g_K=g_plain, g_K_z=g_with_z, g_invK=g_iK, c2=torch.matmul(torch.matmul(Kl, s["T"].to(dt))[:, :3], c["pts"].to(dt))[:, 2].detach())
    return c


# ---------------------------------------------------------------------------------------------------------------------------------------
# learn_intrinsics on the CPU: torch.optim.Adam on the oracle loss, K_eff and its closed-form inverse built from the four factors
# ---------------------------------------------------------------------------------------------------------------------------------------
def intrinsics_from_factors(K, f):
    fx, fy, cx, cy = f[0] * K[:, 0, 0], f[1] * K[:, 1, 1], f[2] * K[:, 0, 2], f[3] * K[:, 1, 2]
    z, o = torch.zeros_like(fx), torch.ones_like(fx)
    K_eff = torch.stack([fx, z, cx, z, z, fy, cy, z, z, z, o, z, z, z, z, o], -1).view(-1, 4, 4)
    inv = torch.stack([1 / fx, z, -cx / fx, z, z, 1 / fy, -cy / fy, z, z, z, o, z, z, z, z, o], -1).view(-1, 4, 4)
    return K_eff, inv


# confirmed on the CPU before it was fixed: the loss falls from 0.0157 to 0.0008 and the focal error from 0.06 to 0.009; a perturbation of
# the inputs by one float32 ulp moves the final factors by 5e-7, a fortieth of the tolerance 3e-4 x steps x lr of the comparison
RECOVERY = dict(steps=12, lr=5e-3, init=(1.06, 1.06, 1.0, 1.0))


def recovery_scene():
    """a photo-consistent pair as in test_oft_reduces_the_loss_and_scale_learning_recovers_the_scale: the target is the source warped with
    the true depth and the true K, so the loss is ~0 at factors (1,1,1,1) -> (scene, src, tgt), frames (B,3,H,W)"""
    from synth import make_pair
    s = make_pair(96, 128, seed=3)
    src = s["src"].permute(0, 3, 1, 2)
    return s, src, wl.inverse_warp(s["depth"], src, s["K"], s["invK"], s["T"], "border")[0]


def cpu_learn_intrinsics(depth, src, tgt, K, T, steps, lr, init, padding_mode="border", use_mask=True):
    """-> (factors (4,), [loss per step]); src / tgt (B,3,H,W)"""
    f = torch.nn.Parameter(torch.tensor([float(v) for v in init]))
    opt = torch.optim.Adam([f], lr=lr)
    trace = []
    for _ in range(steps):
        opt.zero_grad()
        K_eff, inv = intrinsics_from_factors(K, f)
        synth, valid = wl.inverse_warp(depth, src, K_eff, inv, T, padding_mode)[:2]
        loss = wl.masked_photometric_mean(synth, tgt, valid, use_mask)[0]
        loss.backward()
        opt.step()
        trace.append(float(loss.detach()))
    return f.detach().clone(), trace
