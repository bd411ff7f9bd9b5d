"""Host-side half of tests/test_gpu_warp_photo_window.py: the fused warp-photometric pair over a window of S = 1 or 2 source frames with the
candidate / minimum logic of the reference's train_depth.py:621-662 (e2e_warp_photo_window_fwd / _bwd).  The composition is that of
tests/warp_pose_ref.py per source -- oracle.warp_loss.backproject -> project -> F.grid_sample -> photometric of the masked images -- in
float64 and float32 on the CPU, with the depth and both poses as leaves; the candidates and their first minimum are formed here as
include/e2eslam.h states them.  Nothing touches a GPU; tests/test_warp_window_inputs.py proves what this docstring claims.

Scenes: gen("W", B, H, W, salt): depth rand * 2 + 1, two rigid(B, 0.15, 0.3, ...) poses, uniform images, tie noise randn * 1e-5 of shape
(B,2,H,W) (S = 1 takes its first plane).  The salts are CHOSEN (SALT): random seeds exclude up to 4.7 % of a case, and the
chosen ones stay under the cap whichever vector code path the CPU's math library takes.

Modes (S, min_reprojection, auto_masking): MODES.  Candidate order: identity candidates first (I_s + n_s per source with both flags, their
mean with auto-masking alone), then R_s per source with min-reprojection, else their mean.  select = the index of the first minimal one.

Exclusions of g_depth_tgt, the union of
  (a) each used source's kink set, warp_pose_ref.exclusions (a source index within the band of an integer or of the border clamp, y - x within
      the band of 0, an unclamped SSIM value within the band of 0 or 1, max|grid| within the band of 1);
  (b) near-ties of the selection, dilated by 1: 0 < gap64 < BAND x max|gap32 - gap64|, gap = the difference of the two smallest candidates
      (the float32 gap taken between the same two candidates).  A pixel counts only if those two candidates do not have identical values in
      the float32 and the float64 reference: fully masked 3x3 windows give exactly 0 against exactly the noise value on both sides, they are
      decided exactly and are compared.  Exact ties (gap64 == 0) are compared too: the first candidate wins.
`select` is compared for equality outside (b) (not dilated).  At most CAP_EXCLUDED = 2 % of the pixels of a case are excluded: the one-source
module's 1 %, doubled for two sources' kinks.  g_T sums every pixel, so a pose case is admitted only if its exclusion set is empty (POSE_CASES).

Bounds: warp_contract_ref.bound on everything but the gradients; g_depth_tgt and g_T by fused_grad_bound's rule -- the rule's own bound, raised to
FACTOR x the largest relative float32 error that any shape (g_T: any admitted pose case) of the same (pad, mask, mode) shows, times this case's
max|r64|, never above CAP x max|r64|.

Shapes: (1,3,5); (2,9,33): one row and one column past a 32x8 tile, B = 2 with distinct K and T; (2,17,33); (1,37,53): several tiles both ways."""
import functools
import itertools

import torch
import torch.nn.functional as F

import warp_contract_ref as R
import warp_pose_ref as P
from oracle import warp_loss as wl
from warp_contract_ref import F32, F64

SHAPES = [(1, 3, 5), (2, 9, 33), (2, 17, 33), (1, 37, 53)]
MODES = [(2, 0, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1), (1, 0, 1), (1, 1, 1)]           # (S, min_reprojection, auto_masking)
TRIVIAL = (2, 0, 0)                                                                   # one candidate
CAP_EXCLUDED = 0.02
SALT = {(1, 3, 5): 3, (2, 9, 33): 2, (2, 17, 33): 7, (1, 37, 53): 2}
CASES = [(shape, pad, mask, mode) for shape in SHAPES for pad in (0, 1) for mask in (0, 1) for mode in MODES]
G_LOSS = 1.3


def terms_of(mode):
    """E2E_TERM_AUTO_MASKING = 2, E2E_TERM_MIN_REPROJECTION = 4"""
    return (4 if mode[1] else 0) | (2 if mode[2] else 0)


@functools.lru_cache(maxsize=None)
def scene(B, H, W, salt=None):
    salt = SALT[(B, H, W)] if salt is None else salt
    g = R.gen("W", B, H, W, salt)
    K, invK = R.intrinsics(B, H, W, "W")
    return dict(B=B, H=H, W=W, K=K, invK=invK, depth=torch.rand(B, H, W, generator=g) * 2 + 1,
                T=[R.rigid(B, 0.15, 0.3, H, W, "W", salt, k) for k in range(2)],
                src=[torch.rand(B, 3, H, W, generator=g) for k in range(2)], tgt=torch.rand(B, 3, H, W, generator=g),
                noise=torch.randn(B, 2, H, W, generator=g) * 1e-5)


def maps(s, pad, use_mask, dt, Ts=None, srcs=None):
    """both sources' maps with the depth and the poses as leaves -> dict(d, T [2], rep (B,2,H,W), idn (B,2,H,W), per source: grid, m, synth, valid)"""
    B, H, W = s["B"], s["H"], s["W"]
    d = R.leaf(s["depth"], dt)
    Tl = [R.leaf(t, dt) for t in (s["T"] if Ts is None else Ts)]
    srcs = s["src"] if srcs is None else srcs
    tgt = s["tgt"].to(dt)
    out = dict(d=d, T=Tl, grid=[], m=[], synth=[], valid=[])
    rep, idn = [], []
    for src, T in zip(srcs, Tl):
        pts = wl.backproject(d.view(B, 1, H, W), s["invK"].to(dt))
        grid, valid = wl.project(pts, s["K"].to(dt), T.expand(B, 4, 4) if T.dim() == 2 else T, H, W)
        synth = F.grid_sample(src.to(dt), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=False)
        m = valid.to(dt) if use_mask else 1.0
        rep.append(wl.photometric(synth * m, tgt * m))
        idn.append(wl.photometric(src.to(dt) * m, tgt * m))
        out["grid"].append(grid.detach())
        out["m"].append(grid.detach().abs().amax(-1))
        out["synth"].append(synth.detach())
        out["valid"].append(valid.view(B, H, W))
    out["rep"], out["idn"] = torch.cat(rep, 1), torch.cat(idn, 1)
    return out


def candidates(rep, idn, mode, noise):
    S, minrep, auto = mode
    rep, idn = rep[:, :S], idn[:, :S]
    if not minrep:
        rep = rep.mean(1, keepdim=True)
    if not auto:
        return rep
    idn = idn + noise[:, :S].to(idn.dtype) if minrep else idn.mean(1, keepdim=True)
    return torch.cat((idn, rep), 1)


def n_identity(mode):
    S, minrep, auto = mode
    return (S if minrep else 1) if auto else 0


def first_min(c):
    """(the minimum, the index of the first candidate that has it); a NaN wins like in torch.min"""
    c_ = torch.where(torch.isnan(c), torch.full_like(c, -float("inf")), c)
    sel = (c_ == c_.amin(1, keepdim=True)).float().argmax(1)
    return c.gather(1, sel[:, None])[:, 0], sel


def evaluate(base, s, mode, dt, noise=None):
    """one mode on the maps of `maps` -> dict(cands, pmap, select, loss, g_depth, g_T [S])"""
    S = mode[0]
    c = candidates(base["rep"], base["idn"], mode, s["noise"] if noise is None else noise)
    pm, sel = first_min(c)
    loss = pm.mean()
    g = torch.autograd.grad(loss, [base["d"]] + base["T"][:S], retain_graph=True)
    return dict(cands=c.detach(), pmap=pm.detach(), select=sel, loss=loss.detach(), g_depth=g[0], g_T=list(g[1:]))


def near_ties(c64, c32):
    """(b) of the module docstring, not dilated; and the exact ties"""
    if c64.shape[1] == 1:
        z = torch.zeros_like(c64[:, 0], dtype=torch.bool)
        return z, z
    t64, o64 = c64.sort(dim=1, stable=True)
    t32 = torch.gather(c32, 1, o64).double()
    gap64, gap32 = t64[:, 1] - t64[:, 0], t32[:, 1] - t32[:, 0]
    same = (t32[:, 0] == t64[:, 0]) & (t32[:, 1] == t64[:, 1])
    return (gap64 != 0) & (gap64 < R.band(gap32, gap64)) & ~same, gap64 == 0


@functools.lru_cache(maxsize=None)
def base_case(shape, pad, use_mask, salt=None, expanded=False):
    """expanded: one (4,4) pose per source, the scene's first, behind every batch element"""
    s = scene(*shape, salt)
    c = dict(scene=s, shape=shape, pad=pad, use_mask=use_mask, T=[t[0] for t in s["T"]] if expanded else s["T"])
    for dt in (F64, F32):
        c[dt] = maps(s, pad, use_mask, dt, Ts=c["T"])
    c["kinks"], c["valid_band"] = [], []
    for k in range(2):
        r64, r32 = ({key: c[dt][key][k] for key in ("grid", "m", "synth", "valid")} for dt in (F64, F32))
        c["kinks"].append(P.exclusions(s, r64, r32, pad, use_mask))
        c["valid_band"].append((r64["m"] - 1).abs() < R.band(r32["m"], r64["m"]))
    return c


@functools.lru_cache(maxsize=None)
def window_case(shape, pad, use_mask, mode, salt=None, expanded=False):
    b = base_case(shape, pad, use_mask, salt, expanded)
    s, S = b["scene"], mode[0]
    case = dict(scene=s, shape=shape, pad=pad, use_mask=use_mask, mode=mode, base=b)
    for dt in (F64, F32):
        case[dt] = evaluate(b[dt], s, mode, dt)
    near, exact = near_ties(case[F64]["cands"], case[F32]["cands"].double())
    kinks = b["kinks"][0] | b["kinks"][1] if S == 2 else b["kinks"][0]
    vband = b["valid_band"][0] | b["valid_band"][1] if S == 2 else b["valid_band"][0]
    case.update(near=near, exact=exact, grad_excluded=kinks | R.dilate(near, 1), valid_band=vband,
                pmap_excluded=R.dilate(vband, 1) if use_mask else torch.zeros_like(vband))
    return case


def excluded_fraction(case):
    return float(case["grad_excluded"].sum()) / case["grad_excluded"].numel()


def _rel(a32, a64):
    top = float(a64.abs().max())
    return float((a32.double() - a64).abs().max()) / top if top > 0 else 0.0


@functools.lru_cache(maxsize=None)
def pooled_depth(pad, use_mask, mode):
    worst = 0.0
    for shape in SHAPES:
        c = window_case(shape, pad, use_mask, mode)
        keep = ~c["grad_excluded"]
        if keep.any():
            worst = max(worst, _rel(c[F32]["g_depth"][keep], c[F64]["g_depth"][keep]))
    return worst


def depth_bound(case, a=1.0):
    """the bound on max|g_depth_tgt - a g64| over the pixels that are compared"""
    keep = ~case["grad_excluded"]
    t64, t32 = a * case[F64]["g_depth"], torch.tensor(a, dtype=F32) * case[F32]["g_depth"]
    top = float(t64[keep].abs().max())
    return min(max(R.bound(t32, t64, keep), R.FACTOR * pooled_depth(case["pad"], case["use_mask"], case["mode"]) * top), R.CAP * top)


# the cases whose exclusion set is empty (tests/test_warp_window_inputs.py holds the list against the rule): g_T is compared on these
# The reference's float32 error -- hence every band -- moves a little with the CPU's math library, so the list holds the cases that stay empty under
# the AVX-512, AVX2 and SSE4.2 code paths of the library alike; with zero padding and the mask, S = 2 then remains at (1,3,5) only.
POSE_CASES = ([((1, 3, 5), pad, mask, mode) for pad in (0, 1) for mask in (0, 1) for mode in MODES]
              + [((2, 9, 33), 1, mask, mode) for mask in (0, 1) for mode in MODES]
              + [((2, 9, 33), 0, 0, mode) for mode in MODES if mode != (2, 1, 0)]
              + [((2, 9, 33), 0, 1, mode) for mode in MODES[4:]]
              + [((2, 17, 33), 0, 0, mode) for mode in MODES if mode != (2, 1, 0)]
              + [((2, 17, 33), 1, 1, mode) for mode in MODES if mode != (1, 0, 1)]
              + [((2, 17, 33), 0, 1, mode) for mode in MODES[4:]]
              + [((2, 17, 33), 1, 0, mode) for mode in ((2, 0, 0), (2, 0, 1), (1, 0, 1), (1, 1, 1))])


@functools.lru_cache(maxsize=None)
def pooled_pose(pad, use_mask, mode):
    worst = 0.0
    for c in POSE_CASES:
        if c[1:] == (pad, use_mask, mode):
            w = window_case(*c)
            worst = max([worst] + [_rel(g32, g64) for g32, g64 in zip(w[F32]["g_T"], w[F64]["g_T"])])
    return worst


def pose_bound(case, k, a=1.0):
    """the bound on max|g_T[k] - a g64| of source k"""
    t64, t32 = a * case[F64]["g_T"][k], torch.tensor(a, dtype=F32) * case[F32]["g_T"][k]
    top = float(t64.abs().max())
    return min(max(R.bound(t32, t64), R.FACTOR * pooled_pose(case["pad"], case["use_mask"], case["mode"]) * top), R.CAP * top)


def all_cases():
    return [window_case(*c) for c in CASES]


def survey(shape, salt):
    """what the choice of a salt looks at -> (largest excluded fraction, empty cases, selection flips outside (b), valid-band pixels, modes that
    lack a winner, exact ties)"""
    worst, empty, flips, vb, lacking, exact = 0.0, [], 0, 0, [], 0
    for pad, mask, mode in itertools.product((0, 1), (0, 1), MODES):
        c = window_case(shape, pad, mask, mode, salt)
        worst = max(worst, excluded_fraction(c))
        if not c["grad_excluded"].any():
            empty.append((pad, mask, mode))
        flips += int(((c[F64]["select"] != c[F32]["select"]) & ~c["near"]).sum())
        vb += int(c["valid_band"].sum())
        exact += int(c["exact"].sum())
        if mode != TRIVIAL and not both_winners(c):
            lacking.append((pad, mask, mode))
    return worst, empty, flips, vb, lacking, exact


def both_winners(case):
    """with auto-masking: an identity candidate wins somewhere and a reprojection candidate somewhere; with min-reprojection and S = 2 each
    source's reprojection map wins somewhere"""
    S, minrep, auto = case["mode"]
    sel, nI = case[F64]["select"], n_identity(case["mode"])
    ok = True
    if auto:
        ok = ok and bool((sel < nI).any()) and bool((sel >= nI).any())
    if minrep and S == 2:
        ok = ok and bool((sel == nI).any()) and bool((sel == nI + 1).any())
    return ok


EXPANDED_CASE = ((2, 9, 33), 1, 1, (2, 1, 1))                             # admitted like a pose case: its exclusion set is empty too


# the crafted case: one source's image is lifted by 10, so its reprojection map loses at every pixel (its L1 term alone is above 1.35, the
# other map is at most 1) while it still has texture, hence a gradient wherever it were given weight
CRAFTED = ((2, 9, 33), 1, 0, (2, 1, 0))


@functools.lru_cache(maxsize=None)
def crafted(winner):
    shape, pad, use_mask, mode = CRAFTED
    s = scene(*shape)
    srcs = list(s["src"])
    srcs[1 - winner] = srcs[1 - winner] + 10.0
    case = dict(scene=s, srcs=srcs, shape=shape, pad=pad, use_mask=use_mask, mode=mode)
    for dt in (F64, F32):
        case[dt] = evaluate(maps(s, pad, use_mask, dt, srcs=srcs), s, mode, dt)
    return case
