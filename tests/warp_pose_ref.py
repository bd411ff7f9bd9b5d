"""Host-side half of tests/test_gpu_warp_photo_pose.py: the gradient of the fused warp-photometric loss with respect to the relative pose T.
The inputs are the scenes of tests/warp_contract_ref.py (fused_scene), the composition is the same one -- oracle.warp_loss.backproject ->
project -> F.grid_sample -> masked_photometric_mean -- evaluated in float64 and float32 on the CPU with T a leaf, g_T = autograd.grad(loss, T).
Nothing here touches a GPU; tests/test_warp_pose_inputs.py proves what this docstring claims.

Admission.  g_T is a sum over EVERY pixel, so no pixel can be left out of the comparison: a case is admitted only if the kink exclusions of
the fused pair's depth gradient (warp_contract_ref.fused_case(...)["grad_excluded"]: a source index within the band of an integer or of the
border clamp, y - x within the band of 0, an unclamped SSIM value within the band of 0 or 1, max|grid| within the band of 1) are EMPTY.
With the scenes as they are that holds for the cases of POSE_CASES below; (2,9,33) with zero padding (1 pixel) and (1,37,53) zeros / mask
(9 pixels) do not qualify.  The combinations then missing at a multi-tile shape with B = 2 (zero padding; mask on) come from one more
shape of fused_scene, OWN_SHAPE, chosen so that the condition holds.  (1,2,2) with border padding has g_T == 0 identically (every source
index is clamped): kept only as an exact-zero case.  `exclusions` restates the rule for a pose other than the scene's (one T behind both
batch elements); the input test holds it equal to fused_case's on every case that has both.

Bound on max|g_T - g64| (the rule of warp_contract_ref.bound, raised as fused_grad_bound raises it, for the same reason -- on a handful of
entries the float32 reference's largest error is the largest of a few samples): FACTOR x max|g32 - g64|, floored at FACTOR x 2^-24 x
max|g64|, raised to FACTOR x the largest max|g32 - g64| / max|g64| of any admitted pose case of the same (pad, mask) x this case's max|g64|,
and never above CAP x max|g64|.

Shapes: one column past a 32-wide tile (33), one row past an 8-high tile (9, 17), several tiles both ways (37 x 53), B = 2 with a
different (skewed) K and T per element."""
import functools

import torch
import torch.nn.functional as F

import warp_contract_ref as R
from oracle import warp_loss as wl
from warp_contract_ref import F32, F64

OWN_SHAPE = (2, 17, 33)
POSE_CASES = ([((1, 3, 5), pad, mask) for pad in (0, 1) for mask in (0, 1)]
              + [((2, 9, 33), 1, mask) for mask in (0, 1)]
              + [((1, 37, 53), 0, 0), ((1, 37, 53), 1, 0), ((1, 37, 53), 1, 1)]
              + [(OWN_SHAPE, pad, mask) for pad in (0, 1) for mask in (0, 1)])
ZERO_CASE = ((1, 2, 2), 1, 1)                                         # g_T == 0 identically
EXPANDED_CASE = ((2, 9, 33), 1, 1)                                    # one (4,4) T, the scene's first, behind both batch elements
PLAN_CASE = ((1, 37, 53), 1, 1)


def composition(s, pad, use_mask, dt, T=None):
    """the loss with T (default: the scene's; a (4,4) T is expanded over the batch) and the sampling grid as leaves ->
    dict(loss, T, g_T, grid, g_grid, synth, valid, m, pts)"""
    B, H, W = s["B"], s["H"], s["W"]
    Tl = R.leaf(s["T"] if T is None else T, dt)
    Tb = Tl.expand(B, 4, 4) if Tl.dim() == 2 else Tl
    pts = wl.backproject(s["depth"].to(dt).view(B, 1, H, W), s["invK"].to(dt))
    grid, valid = wl.project(pts, s["K"].to(dt), Tb, H, W)
    grid.retain_grad()
    synth = F.grid_sample(s["src"].to(dt), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=False)
    loss, _ = wl.masked_photometric_mean(synth, s["tgt"].to(dt), valid.to(dt), bool(use_mask))
    g_T, g_grid = torch.autograd.grad(loss, (Tl, grid))
    return dict(loss=loss.detach(), T=Tl.detach(), g_T=g_T, grid=grid.detach(), g_grid=g_grid, synth=synth.detach(), valid=valid.view(B, H, W),
                m=grid.detach().abs().amax(-1), pts=pts.detach())


def exclusions(s, r64, r32, pad, use_mask):
    """warp_contract_ref.fused_case's grad_excluded, from the two evaluations of `composition`"""
    H, W = s["H"], s["W"]
    vband = (r64["m"] - 1).abs() < R.band(r32["m"], r64["m"])
    idx = R.index_kink(r64["grid"][..., 0], W, pad, False) | R.index_kink(r64["grid"][..., 1], H, pad, False)
    m = r64["valid"][:, None].double() if use_mask else 1.0
    x, y = r64["synth"] * m, s["tgt"].double() * m
    d64, t64 = y - x, R.ssim_unclamped(x, y)
    m32 = r32["valid"][:, None] if use_mask else 1.0
    x32, y32 = r32["synth"] * m32, s["tgt"] * m32
    bd, bt = R.band(y32 - x32, d64), R.band(R.ssim_unclamped(x32, y32), t64)
    sign = ((d64 != 0) & (d64.abs() < bd)).any(1)
    gate = (((t64 != 0) & (t64.abs() < bt)) | ((t64 != 1) & ((t64 - 1).abs() < bt))).any(1)
    return idx | sign | R.dilate(gate, 1) | (R.dilate(vband, 2) if use_mask else torch.zeros_like(vband))


@functools.lru_cache(maxsize=None)
def pose_case(shape, pad, use_mask, expanded=False):
    s = R.fused_scene(*shape)
    T = s["T"][0] if expanded else None
    case = dict(scene=s, shape=shape, pad=pad, use_mask=use_mask, T=s["T"][0].expand(shape[0], 4, 4).contiguous() if expanded else s["T"])
    for dt in (F64, F32):
        case[dt] = composition(s, pad, use_mask, dt, T)
    case["grad_excluded"] = exclusions(s, case[F64], case[F32], pad, use_mask)
    return case


def rel_error(case):
    g64, g32 = case[F64]["g_T"], case[F32]["g_T"].double()
    return float((g32 - g64).abs().max()) / float(g64.abs().max())


@functools.lru_cache(maxsize=None)
def pooled(pad, use_mask):
    """the largest relative float32 error on g_T that any admitted pose case of this (pad, mask) shows"""
    return max(rel_error(pose_case(*c)) for c in POSE_CASES if c[1:] == (pad, use_mask))


def floor_cap(case, a=1.0):
    top = abs(a) * float(case[F64]["g_T"].abs().max())
    return R.FACTOR * R.EPS32 * top, R.CAP * top


def pose_bound(case, a=1.0):
    """the bound on max|g_T - a g64| for the upstream gradient a = g_loss[0]"""
    t64, t32 = a * case[F64]["g_T"], (torch.tensor(a, dtype=F32) * case[F32]["g_T"])
    top = float(t64.abs().max())
    return min(max(R.bound(t32, t64), R.FACTOR * pooled(case["pad"], case["use_mask"]) * top), R.CAP * top)


def closed_form(case):
    """the per-pixel formula of include/e2eslam.h (e2e_warp_photo_bwd_pose) in float64, from the reference's own gradient of the sampling grid:
    g_grid -> (gu, gv) -> (gc0, gc1, gc2); Pbar[r][j] = sum gc_r X_j | sum gc_r; g_T[k][j] = sum_{i<3} K[i][k] Pbar[i][j] -> (g_T (B,4,4), Pbar (B,3,4))"""
    s, r = case["scene"], case[F64]
    B, H, W = case["shape"]
    K, T = s["K"].double(), case["T"].double()
    P = torch.matmul(K, T)[:, :3, :]
    X = r["pts"]                                                      # (B,4,N): d cam | 1
    c = torch.matmul(P, X)
    z = c[:, 2] + 1e-7
    u, v = c[:, 0] / z, c[:, 1] / z
    gg = r["g_grid"].reshape(B, H * W, 2)
    gu, gv = gg[..., 0] * 2 / (W - 1), gg[..., 1] * 2 / (H - 1)
    gc = torch.stack([gu / z, gv / z, -(gu * u + gv * v) / z], 1)     # (B,3,N)
    Pbar = torch.matmul(gc, X.transpose(1, 2))                        # (B,3,4): the last column is sum gc, X's last row being 1
    return torch.matmul(K[:, :3, :].transpose(1, 2), Pbar), Pbar
