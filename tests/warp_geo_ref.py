"""Host-side half of tests/test_gpu_warp_photo_geo.py: the fused warp-photometric pair over a window of S = 1 or 2 source frames WITH the
geometric-consistency term of the reference's LOSS.geometric branch (e2e_warp_photo_geo_fwd / _bwd; train_depth.py:558-576,
view_synthesis.py:54-78, losses.py:84-95).  The composition per source is oracle.warp_loss.backproject -> project(geometric=True) ->
F.grid_sample (the image with align_corners=True, the source depth with False, as the reference does) -> photometric of the masked images and
the geometric consistency, restated here with the gate `n > geo_min_valid` as an argument; float64 and float32 on the CPU; leaves: the
depth, both source depths and both poses.  Candidates, modes and the first minimum are tests/warp_window_ref.py's.  Nothing touches a GPU;
tests/test_warp_geo_inputs.py proves what this docstring claims.

Scenes: warp_window_ref.scene plus source depths rand * 2 + 1 from gen("G", B, H, W, salt).  The salts are CHOSEN (SALT) so that every case
stays under the cap, no pixel of any case lies in a validity band (so n_s is decided), and the cases the pose comparison needs are empty.

What is differentiated: g_loss[0] loss[0] + sum_s g_loss[1 + s] G_s with G_LOSS, and geo_min_valid = 0 unless a test says otherwise.

Exclusions of g_depth_tgt, the union over the used sources of
  (a) the window module's kink set with the image index taken at align_corners=True (a source index within the band of an integer or of the
      border clamp, y - x within the band of 0, an unclamped SSIM value within the band of 0 or 1);
  (b) near-ties of the selection, dilated by 1 (warp_window_ref.near_ties);
  (c) the depth sample's index within the band of an integer or of the border clamp at align_corners=False;
  (d) wd - id within the band of 0 on a valid pixel;  (e) c2 within the band of 1e-3 on a valid pixel;
  (f) max|grid| within the band of 1, dilated by 2 -- always: the term multiplies by `valid` whatever use_mask says.
Exclusions of g_depth_src[s]: every source pixel that is a bilinear tap (align_corners=False, float64 position) of a target pixel in (d) or
in the undilated band of (f).  At most CAP_EXCLUDED = 2 % of the pixels of a case are excluded, for either gradient.
g_T, the loss and G_s sum every pixel: they are compared on the cases whose exclusion sets are all empty (`admitted`).

Bounds: warp_contract_ref.bound on everything but the gradients; the three gradients by fused_grad_bound's rule -- the rule's own bound, raised
to FACTOR x the largest relative float32 error that any shape (g_T: any admitted case) of the same (pad, mask, mode) shows, times this case's
max|r64|, never above CAP x max|r64|.

Shapes: the family's (1,3,5); (2,9,33): one row and one column past a 32x8 tile, B = 2 with distinct K and T, which catches a scatter that
crosses batch elements or sources; (2,17,33); (1,37,53): several tiles both ways."""
import functools
import itertools

import torch
import torch.nn.functional as F

import warp_contract_ref as R
import warp_window_ref as Wr
from oracle import warp_loss as wl
from warp_contract_ref import F32, F64

SHAPES, MODES = Wr.SHAPES, Wr.MODES
CAP_EXCLUDED = Wr.CAP_EXCLUDED
SALT = {(1, 3, 5): 3, (2, 9, 33): 4, (2, 17, 33): 1, (1, 37, 53): 7}
N_VALID = {(1, 3, 5): (4, 8), (2, 9, 33): (402, 474), (2, 17, 33): (763, 949), (1, 37, 53): (1633, 1540)}      # n_0, n_1 of those scenes
GATE_SHAPE = (2, 9, 33)                                               # n_0 < n_1: geo_min_valid = n_0 closes source 0 alone
CASES = [(shape, pad, mask, mode) for shape in SHAPES for pad in (0, 1) for mask in (0, 1) for mode in MODES]
G_LOSS = (1.3, 0.7, 1.9)
ZCLAMP = 1e-3


@functools.lru_cache(maxsize=None)
def scene(B, H, W, salt=None):
    salt = SALT[(B, H, W)] if salt is None else salt
    s = dict(Wr.scene(B, H, W, salt))
    g = R.gen("G", B, H, W, salt)
    s["dsrc"] = [torch.rand(B, H, W, generator=g) * 2 + 1 for k in range(2)]
    return s


def maps(s, pad, dt, use_mask, Ts=None):
    """both sources' maps with the depth, the source depths and the poses as leaves -> dict(d, T [2], ds [2], rep, idn (B,2,H,W), per source:
    grid, m, synth, valid, wd, id, c2 (detached), gsum = sum(diff valid) (graph), n = sum(valid) (int))"""
    B, H, W = s["B"], s["H"], s["W"]
    d = R.leaf(s["depth"], dt)
    Tl = [R.leaf(t, dt) for t in (s["T"] if Ts is None else Ts)]
    dsl = [R.leaf(x, dt) for x in s["dsrc"]]
    tgt, K = s["tgt"].to(dt), s["K"].to(dt)
    out = dict(d=d, T=Tl, ds=dsl, grid=[], m=[], synth=[], valid=[], wd=[], id=[], c2=[], gsum=[], n=[])
    rep, idn = [], []
    for k, (src, T) in enumerate(zip(s["src"], Tl)):
        Tb = T.expand(B, 4, 4) if T.dim() == 2 else T
        pts = wl.backproject(d.view(B, 1, H, W), s["invK"].to(dt))
        grid, wd, valid = wl.project(pts, K, Tb, H, W, geometric=True)
        synth = F.grid_sample(src.to(dt), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=True)
        idp = F.grid_sample(dsl[k].view(B, 1, H, W), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=False)
        v = valid.to(dt)
        m = v if use_mask else 1.0
        rep.append(wl.photometric(synth * m, tgt * m))
        idn.append(wl.photometric(src.to(dt) * m, tgt * m))
        diff = ((wd - idp).abs() / (wd + idp)).clamp(0, 1)                # losses.py:84-95
        out["gsum"].append((diff * v).sum())
        out["n"].append(int(valid.sum()))
        out["grid"].append(grid.detach())
        out["m"].append(grid.detach().abs().amax(-1))
        out["synth"].append(synth.detach())
        out["valid"].append(valid.view(B, H, W))
        out["wd"].append(wd.detach().view(B, H, W))
        out["id"].append(idp.detach().view(B, H, W))
        out["c2"].append(torch.matmul(torch.matmul(K, Tb)[:, :3], pts)[:, 2].detach().view(B, H, W))
    out["rep"], out["idn"] = torch.cat(rep, 1), torch.cat(idn, 1)
    return out


def geometric_consistency(gsum, n, geo_min_valid):
    """losses.py:84-95 with the gate as an argument: sum(diff mask) / sum(mask) if sum(mask) > geo_min_valid, else 0 (no gradient)"""
    return gsum / n if n > geo_min_valid else gsum * 0


def evaluate(base, s, mode, dt, geo_min_valid=0, g_loss=G_LOSS):
    """one mode on the maps of `maps` -> dict(cands, pmap, select, loss, G [S], g_depth, g_T [S], g_ds [S]); the gradients are those of
    g_loss[0] loss + sum_s g_loss[1 + s] G_s"""
    S = mode[0]
    c = Wr.candidates(base["rep"], base["idn"], mode, s["noise"])
    pm, sel = Wr.first_min(c)
    loss = pm.mean()
    G = [geometric_consistency(base["gsum"][k], base["n"][k], geo_min_valid) for k in range(S)]
    total = g_loss[0] * loss + sum(g_loss[1 + k] * G[k] for k in range(S))
    leaves = [base["d"]] + base["T"][:S] + base["ds"][:S]
    g = torch.autograd.grad(total, leaves, retain_graph=True, allow_unused=True)
    g = [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, g)]
    return dict(cands=c.detach(), pmap=pm.detach(), select=sel, loss=loss.detach(), G=[x.detach() for x in G], g_depth=g[0],
                g_T=g[1:1 + S], g_ds=g[1 + S:])


def _band_on(q32, q64, on):
    return R.band(q32[on], q64[on]) if on.any() else 0.0


def photo_kinks(s, r64, r32, pad, use_mask):
    """(a) of the module docstring: warp_pose_ref.exclusions with the image index at align_corners=True and without the validity band"""
    H, W = s["H"], s["W"]
    idx = R.index_kink(r64["grid"][..., 0], W, pad, True) | R.index_kink(r64["grid"][..., 1], H, pad, True)
    m = r64["valid"][:, None].double() if use_mask else 1.0
    x, y = r64["synth"] * m, s["tgt"].double() * m
    d64, t64 = y - x, R.ssim_unclamped(x, y)
    m32 = r32["valid"][:, None] if use_mask else 1.0
    x32, y32 = r32["synth"] * m32, s["tgt"] * m32
    bd, bt = R.band(y32 - x32, d64), R.band(R.ssim_unclamped(x32, y32), t64)
    sign = ((d64 != 0) & (d64.abs() < bd)).any(1)
    gate = (((t64 != 0) & (t64.abs() < bt)) | ((t64 != 1) & ((t64 - 1).abs() < bt))).any(1)
    return idx | sign | R.dilate(gate, 1)


def geo_kinks(s, r64, r32, pad):
    """(c) - (f) of the module docstring -> dict(idx, sign, zclamp, vband) of (B,H,W) masks"""
    H, W = s["H"], s["W"]
    on = r64["valid"] > 0
    idx = R.index_kink(r64["grid"][..., 0], W, pad, False) | R.index_kink(r64["grid"][..., 1], H, pad, False)
    q64, q32 = r64["wd"] - r64["id"], r32["wd"] - r32["id"]
    sign = on & (q64.abs() < _band_on(q32, q64, on))
    zclamp = on & ((r64["c2"] - ZCLAMP).abs() < _band_on(r32["c2"], r64["c2"], on))
    vband = (r64["m"] - 1).abs() < R.band(r32["m"], r64["m"])
    return dict(idx=idx, sign=sign, zclamp=zclamp, vband=vband)


def footprint(grid64, H, W, pad, mask):
    """the source pixels (B,H,W) that are bilinear taps (align_corners=False) of the target pixels in `mask`"""
    B = grid64.shape[0]
    ix, iy = R.source_index(grid64[..., 0], W, False, F64), R.source_index(grid64[..., 1], H, False, F64)
    if pad == 1:
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    x0, y0 = ix.floor().long(), iy.floor().long()
    bi = torch.arange(B)[:, None, None].expand(B, H, W)
    out = torch.zeros(B, H, W, dtype=torch.bool)
    for dy, dx in itertools.product((0, 1), (0, 1)):
        x, y = x0 + dx, y0 + dy
        ok = mask & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        out[bi[ok], y[ok], x[ok]] = True
    return out


@functools.lru_cache(maxsize=None)
def base_case(shape, pad, use_mask, salt=None, expanded=False):
    """expanded: one (4,4) pose per source, the scene's first, behind every batch element"""
    s = scene(*shape, salt)
    c = dict(scene=s, shape=shape, pad=pad, use_mask=use_mask, T=[t[0] for t in s["T"]] if expanded else s["T"])
    for dt in (F64, F32):
        c[dt] = maps(s, pad, dt, use_mask, Ts=c["T"])
    c["photo"], c["geo"], c["src_excluded"] = [], [], []
    B, H, W = shape
    for k in range(2):
        r64, r32 = ({key: c[dt][key][k] for key in ("grid", "m", "synth", "valid", "wd", "id", "c2")} for dt in (F64, F32))
        c["photo"].append(photo_kinks(s, r64, r32, pad, use_mask))
        gk = geo_kinks(s, r64, r32, pad)
        c["geo"].append(gk)
        c["src_excluded"].append(footprint(r64["grid"], H, W, pad, gk["sign"] | gk["vband"]))
    return c


def _assemble(case, b, S):
    near, exact = Wr.near_ties(case[F64]["cands"], case[F32]["cands"].double())
    ex = R.dilate(near, 1)
    vband = torch.zeros_like(near)
    for k in range(S):
        gk = b["geo"][k]
        ex = ex | b["photo"][k] | gk["idx"] | gk["sign"] | gk["zclamp"] | R.dilate(gk["vband"], 2)
        vband = vband | gk["vband"]
    case.update(near=near, exact=exact, grad_excluded=ex, valid_band=vband, src_excluded=b["src_excluded"][:S], geo=b["geo"][:S],
                pmap_excluded=R.dilate(vband, 1) if case["use_mask"] else torch.zeros_like(vband))
    return case


@functools.lru_cache(maxsize=None)
def geo_case(shape, pad, use_mask, mode, salt=None, expanded=False, geo_min_valid=0, g_loss=G_LOSS):
    b = base_case(shape, pad, use_mask, salt, expanded)
    s, S = b["scene"], mode[0]
    case = dict(scene=s, shape=shape, pad=pad, use_mask=use_mask, mode=mode, base=b, g_loss=g_loss, geo_min_valid=geo_min_valid, n=b[F64]["n"][:S])
    for dt in (F64, F32):
        case[dt] = evaluate(b[dt], s, mode, dt, geo_min_valid, g_loss)
    return _assemble(case, b, S)


def excluded_fraction(case):
    """the largest excluded fraction of the case: of g_depth_tgt, or of one source's g_depth_src"""
    sets = [case["grad_excluded"]] + list(case["src_excluded"])
    return max(float(x.sum()) / x.numel() for x in sets)


def admitted(case):
    """g_T, the loss and G_s sum every pixel: compared only when nothing is excluded"""
    return not case["grad_excluded"].any() and not any(x.any() for x in case["src_excluded"])


def _rel(a32, a64):
    top = float(a64.abs().max()) if a64.numel() else 0.0
    return float((a32.double() - a64).abs().max()) / top if top > 0 else 0.0


def _keeps(c, kind):
    S = c["mode"][0]
    if kind == "g_depth":
        return [(c[F32]["g_depth"], c[F64]["g_depth"], ~c["grad_excluded"])]
    if kind == "g_ds":
        return [(c[F32]["g_ds"][k], c[F64]["g_ds"][k], ~c["src_excluded"][k]) for k in range(S)]
    return [(c[F32]["g_T"][k], c[F64]["g_T"][k], None) for k in range(S)] if admitted(c) else []


@functools.lru_cache(maxsize=None)
def pooled(kind, pad, use_mask, mode):
    """the largest relative float32 error of gradient `kind` (g_depth | g_ds | g_T) over the shapes of this (pad, mask, mode)"""
    worst = 0.0
    for shape in SHAPES:
        for a32, a64, keep in _keeps(geo_case(shape, pad, use_mask, mode), kind):
            worst = max(worst, _rel(a32, a64) if keep is None else _rel(a32[keep], a64[keep]))
    return worst


def grad_bound(case, kind, k=0, pool=None):
    """the bound on max|gpu - r64| of g_depth, g_ds[k] or g_T[k] over the elements that are compared -> (bound, keep or None)"""
    if kind == "g_depth":
        t32, t64, keep = case[F32]["g_depth"], case[F64]["g_depth"], ~case["grad_excluded"]
    elif kind == "g_ds":
        t32, t64, keep = case[F32]["g_ds"][k], case[F64]["g_ds"][k], ~case["src_excluded"][k]
    else:
        t32, t64, keep = case[F32]["g_T"][k], case[F64]["g_T"][k], None
    top = float((t64 if keep is None else t64[keep]).abs().max())
    pool = pooled(kind, case["pad"], case["use_mask"], case["mode"]) if pool is None else pool
    return min(max(R.bound(t32, t64, keep), R.FACTOR * pool * top), R.CAP * top), keep


def survey(shape, salt):
    """what the choice of a salt looks at -> (largest excluded fraction, admitted cases, valid-band pixels, selection flips outside the
    near-ties, (n_0, n_1) with border padding)"""
    worst, adm, vb, flips = 0.0, [], 0, 0
    for pad, mask, mode in itertools.product((0, 1), (0, 1), MODES):
        c = geo_case(shape, pad, mask, mode, salt)
        worst = max(worst, excluded_fraction(c))
        if admitted(c):
            adm.append((pad, mask, mode))
        vb += int(c["valid_band"].sum())
        flips += int(((c[F64]["select"] != c[F32]["select"]) & ~c["near"]).sum())
    return worst, adm, vb, flips, tuple(base_case(shape, 1, 1, salt)[F64]["n"])


EXPANDED_CASE = ((2, 9, 33), 1, 1, (2, 1, 1), 3, True)                  # (shape, pad, mask, mode, salt, expanded): its own salt, admitted


# ---------------------------------------------------------------------------------------------------------------------------------------
# the two crafted scenes: only the geometric term is differentiated (g_loss[0] = 0), so only (c) - (f) are excluded
# ---------------------------------------------------------------------------------------------------------------------------------------
CRAFTED_SHAPES = [(2, 9, 33), (2, 17, 33)]
CRAFTED_MODE, CRAFTED_G_LOSS = (2, 0, 0), (0.0, 1.0, 1.7)
CRAFTED_SALT = 2


@functools.lru_cache(maxsize=None)
def crafted(kind, shape, pad, salt=CRAFTED_SALT):
    """kind "behind": a two-layer depth (2x2 checker of 1 + 0.4 rand and 2.6 + 0.4 rand) and T = rigid(0.05, 0.05) with -2 added to the z
    translation: part of the valid pixels has c2 < 1e-3, where no gradient flows through wd but the one through the sampling position does;
    kind "pileup": the same T with +20 in z: every pixel is valid and all of them land on a few source pixels, a heavy many-to-one sum"""
    B, H, W = shape
    s = dict(scene(B, H, W, salt))
    g = R.gen("C", kind, B, H, W, salt)
    if kind == "behind":
        yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        far = ((yy // 2 + xx // 2) % 2 == 1)[None].expand(B, H, W)
        r = torch.rand(B, H, W, generator=g)
        s["depth"] = torch.where(far, 2.6 + 0.4 * r, 1 + 0.4 * r)
    Ts = []
    for k in range(2):
        T = R.rigid(B, 0.05, 0.05, "C", kind, H, W, salt, k)
        T[:, 2, 3] += -2.0 if kind == "behind" else 20.0
        Ts.append(T)
    s["T"] = Ts
    S = CRAFTED_MODE[0]
    b = dict(scene=s, shape=shape, pad=pad, use_mask=1, T=Ts)
    for dt in (F64, F32):
        b[dt] = maps(s, pad, dt, 1, Ts=Ts)
    case = dict(scene=s, shape=shape, pad=pad, use_mask=1, mode=CRAFTED_MODE, base=b, g_loss=CRAFTED_G_LOSS, geo_min_valid=0, n=b[F64]["n"][:S])
    for dt in (F64, F32):
        case[dt] = evaluate(b[dt], s, CRAFTED_MODE, dt, 0, CRAFTED_G_LOSS)
    ex = torch.zeros(B, H, W, dtype=torch.bool)
    case["src_excluded"], case["geo"] = [], []
    for k in range(S):
        r64, r32 = ({key: b[dt][key][k] for key in ("grid", "m", "synth", "valid", "wd", "id", "c2")} for dt in (F64, F32))
        gk = geo_kinks(s, r64, r32, pad)
        ex = ex | gk["idx"] | gk["sign"] | gk["zclamp"] | R.dilate(gk["vband"], 2)
        case["geo"].append(gk)
        case["src_excluded"].append(footprint(r64["grid"], H, W, pad, gk["sign"] | gk["vband"]))
    vband = case["geo"][0]["vband"] | case["geo"][1]["vband"]
    case.update(grad_excluded=ex, near=torch.zeros_like(ex), valid_band=vband, pmap_excluded=R.dilate(vband, 1))      # one candidate: no ties
    return case


def crafted_bound(case, kind, k=0):
    """the rule's own bound: a crafted scene has no other shape to pool with"""
    return grad_bound(case, kind, k, pool=0.0)
