"""Host-side half of tests/test_gpu_lossgrad_contracts.py: the one-launch loss-and-gradient family of csrc/warp_photo_fused.hip
(e2e_warp_photo_lossgrad, _hostgeo, _chain, _chain_flush and the workspace query).  The scenes, the float64 reference, the rule for bounds
and the kink exclusions are those of tests/warp_contract_ref.py (fused_scene, fused_case, bound, band): include/e2eslam.h promises this
family "the same semantics as e2e_warp_photo_fwd followed by e2e_warp_photo_bwd with upstream gradients (w_photo, w_reg)".  Nothing here
touches a GPU; tests/test_lossgrad_contract_inputs.py proves what this docstring claims.

Shapes.  The kernel's tile is 32 x 16 with two rows per thread.  LG_SHAPES = the pair's four shapes (H = 2 and 3: smaller than the halo;
H = 9: a thread's second row is dead in the only tile row; (1,37,53): 3 x 2 tiles, ragged both ways) + (2,17,33), one row and one column
past a tile, + (3,49,161): 6 x 4 x 3 = 72 workgroups, so that eight of the chained form's 64 slots take two workgroups.

A second float32 sample.  The kernel does not evaluate backproject -> project but the header's folded form c = d * (M [x,y,1]^T) + p4,
M = (K T)[:3,:3] inv_K[:3,:3], p4 = (K T)[:3,3].  `folded` is the same composition with that geometry: form "device" with M and p4 formed
in float32 from the float32 matrices (what the kernel does when it is given K, inv_K and T), form "host" with the twelve numbers formed in
float64 and rounded to float32 (what e2ehip.fused.LossGradPlan.set_host_geometry hands to the _hostgeo entry point; its formula is
restated in `geometry12`, not imported).  The float64 reference stays fused_case's.  The float32 error of a tensor is the larger of the
errors of the two float32 formulations -- fused_case's and the folded one of the form the entry point under test uses.

Bounds (warp_contract_ref.FACTOR, EPS32, CAP; no constant of this module's own):
  * g_depth_tgt: warp_contract_ref.fused_grad_bound's rule -- the rule's own bound or, where larger, FACTOR x the largest relative float32
    error of any LG_SHAPES case of the same (pad, mask, reg_kind, upstream pair) x this case's max|r64|, never above CAP x max|r64|.
  * g_depth_src: warp_contract_ref.bound (the regulariser does not depend on the geometry: one float32 formulation).
  * loss_out[0], loss_out[1]: a scalar's float32 error is ONE sample and falls as low as 3e-9 relative on these cases, where no float32 sum
    can follow.  They are bounded as the 2 x 2 gradient is, for the same reason: the rule's own bound or, where larger, FACTOR x the largest
    |l32 - l64| / |l64| of any LG_SHAPES case of the same (pad, mask) -- for the regulariser: of the same reg_kind -- x |l64|, never above
    CAP x |l64|.
  * loss_out[1] with reg_kind = 0 is exactly 0: both the second-stage kernel and the chained form's finalisation write 0 (the header says so).
Exclusions: fused_case's grad_excluded, reg_excluded_t and reg_excluded_s unchanged.  `scene_case` restates fused_case for a scene that
fused_scene does not produce (one image behind both batch elements, the overflow scene); the input test holds the two equal on every
LG_SHAPES case.

Overflow.  `overflow_scene` trips the chained form's documented flag ("a per-workgroup sum ... above 2.6e8 / #workgroups turns the loss
into NaN") by values alone: the (1,37,53) scene with reg_kind 2 and ri_t = depth + 2000, every workgroup's regulariser sum about
(pixels of the tile) x 4e6.  That is 10 to 47 times the limit, so a limit ten times too large still raises the flag for five of the six
workgroups: a second scene, ri_t = depth + 700, puts every workgroup's sum between the limit and ten times the limit.  `tile_sums` gives the per-tile sums of both loss maps of any case from its float64 reference."""
import functools

import torch
import torch.nn.functional as F

import warp_contract_ref as R
from oracle import warp_loss as wl
from warp_contract_ref import F32, F64

LG_SHAPES = R.FUSED_SHAPES + [(2, 17, 33), (3, 49, 161)]
PADS, MASKS, REGS = (0, 1), (0, 1), (0, 1, 2)
FORMS = ("device", "host")
HOSTGEO_SHAPES = [s for s in LG_SHAPES if s[0] == 1]
EXPAND_SHAPES = [s for s in LG_SHAPES if s[0] == 2]                  # one image behind both batch elements (sb = 0)
CHAIN_CASES = [((1, 37, 53), "host"), ((3, 49, 161), "device")]
CHAIN_STEPS = [(0, 0), (0, 1), (1, 0), (1, 1)]                        # (pad, use_mask) of the four steps of a chain
CHAIN_SETS = [(6, -1), (7, 6), (0, 7), (1, 0)]                        # (set_cur, set_prev): set 7 and the wrap back to 0
OVERFLOW_SHAPE, OVERFLOW_REG, OVERFLOW_LIMIT = (1, 37, 53), 2, 2.6e8  # the limit is the header's: 2.6e8 / #workgroups per workgroup sum
OVERFLOW_OFFSETS = (2000.0, 700.0)                                    # ri_t - depth: far above the limit; every workgroup between 1 x and 10 x the limit


def workspace_floats(B, H, W):
    """include/e2eslam.h: two partial sums per 32 x 8 block of pixels, rounded up to even, then 8 slot sets of 129 64-bit words"""
    if B <= 0 or H <= 0 or W <= 0:
        return 0
    return (2 * B * -(-W // 32) * -(-H // 8) + 1) // 2 * 2 + 2 * 8 * 129


def chain_offset(B, H, W):
    """where the slot sets begin in the workspace, in floats"""
    return workspace_floats(B, H, W) - 2 * 8 * 129


def workgroups(shape, tile_h, tile_w):
    B, H, W = shape
    return B * -(-H // tile_h) * -(-W // tile_w)


# ---------------------------------------------------------------------------------------------------------------------------------------
# scenes other than fused_scene's
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expanded_scene(B, H, W):
    """fused_scene with the first source and target image behind every batch element (views of stride 0, as the device gets them)"""
    s = dict(R.fused_scene(B, H, W))
    s["src"], s["tgt"] = s["src"][:1].expand(B, -1, -1, -1), s["tgt"][:1].expand(B, -1, -1, -1)
    return s


@functools.lru_cache(maxsize=None)
def overflow_scene(offset=OVERFLOW_OFFSETS[0]):
    s = dict(R.fused_scene(*OVERFLOW_SHAPE))
    s["ri_t"] = s["depth"] + offset
    return s


def scene_case(s, pad, use_mask, reg_kind):
    """warp_contract_ref.fused_case, restated for any scene"""
    B, H, W = s["B"], s["H"], s["W"]
    case = dict(scene=s, pad=pad, use_mask=use_mask, reg_kind=reg_kind)
    for dt in (F64, F32):
        d, ds = R.leaf(s["depth"], dt), R.leaf(s["d_src"], dt)
        pts = wl.backproject(d.view(B, 1, H, W), s["invK"].to(dt))
        grid, valid = wl.project(pts, s["K"].to(dt), s["T"].to(dt), H, W)
        synth = F.grid_sample(s["src"].to(dt), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=False)
        loss, pmap = wl.masked_photometric_mean(synth, s["tgt"].to(dt), valid.to(dt), bool(use_mask))
        r = dict(grid=grid.detach(), m=grid.detach().abs().amax(-1), synth=synth.detach(), valid=valid.view(B, H, W), pmap=pmap.detach().view(B, H, W),
                 loss=loss.detach(), g_photo=torch.autograd.grad(loss, d)[0])
        if reg_kind:
            reg = wl.depth_regularizer(s["ri_t"].to(dt), d, R.REG_NAME[reg_kind]) + wl.depth_regularizer(s["ri_s"].to(dt), ds, R.REG_NAME[reg_kind])
            r["reg"] = reg.detach()
            r["g_reg_t"], r["g_reg_s"] = torch.autograd.grad(reg, (d, ds))
        case[dt] = r
    r64, r32 = case[F64], case[F32]
    none = torch.zeros(B, H, W, dtype=torch.bool)
    vband = (r64["m"] - 1).abs() < R.band(r32["m"], r64["m"])
    idx = R.index_kink(r64["grid"][..., 0], W, pad, False) | R.index_kink(r64["grid"][..., 1], H, pad, False)
    m64 = r64["valid"][:, None].double() if use_mask else 1.0
    m32 = r32["valid"][:, None] if use_mask else 1.0
    x, y = r64["synth"] * m64, s["tgt"].double() * m64
    x32, y32 = r32["synth"] * m32, s["tgt"] * m32
    d64, t64 = y - x, R.ssim_unclamped(x, y)
    bd, bt = R.band(y32 - x32, d64), R.band(R.ssim_unclamped(x32, y32), t64)
    sign = ((d64 != 0) & (d64.abs() < bd)).any(1)
    gate = (((t64 != 0) & (t64.abs() < bt)) | ((t64 != 1) & ((t64 - 1).abs() < bt))).any(1)
    case["valid_band"] = vband
    case["pmap_excluded"] = R.dilate(vband, 1) if use_mask else none
    case["grad_excluded"] = idx | sign | R.dilate(gate, 1) | (R.dilate(vband, 2) if use_mask else none)
    e_t, e_s = s["ri_t"].double() - s["depth"].double(), s["ri_s"].double() - s["d_src"].double()
    case["reg_excluded_t"] = (e_t != 0) & (e_t.abs() < R.band(s["ri_t"] - s["depth"], e_t)) if reg_kind == 1 else none
    case["reg_excluded_s"] = (e_s != 0) & (e_s.abs() < R.band(s["ri_s"] - s["d_src"], e_s)) if reg_kind == 1 else none
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# the folded geometry
# ---------------------------------------------------------------------------------------------------------------------------------------
def geometry12(s, form):
    """(B,12): the rows of M = (K T)[:3,:3] inv_K[:3,:3], then p4 = (K T)[:3,3].  "device": float32 arithmetic on the float32 matrices;
    "host": float64 arithmetic, rounded to float32 (LossGradPlan.set_host_geometry's formula); "f64": float64, not rounded"""
    dt = F32 if form == "device" else F64
    K, T, inv_K = s["K"].to(dt), s["T"].to(dt), s["invK"].to(dt)
    P = torch.matmul(K, T)[:, :3]
    M = torch.matmul(P[:, :, :3], inv_K[:, :3, :3])
    geo = torch.cat([M.reshape(-1, 9), P[:, :, 3]], 1)
    return geo.float() if form == "host" else geo


def folded(s, geo, pad, use_mask, dt):
    """the composition with c = d * (M [x,y,1]^T) + p4 in place of backproject -> project, in dtype dt -> dict(loss, g_photo, valid, grid, pmap)"""
    B, H, W = s["B"], s["H"], s["W"]
    geo = geo.to(dt)
    M, p4 = geo[:, :9].reshape(B, 3, 3), geo[:, 9:].reshape(B, 3, 1)
    d = R.leaf(s["depth"], dt)
    c = d.view(B, 1, -1) * torch.matmul(M, wl.pixel_grid(B, H, W, dt)) + p4
    pix = (c[:, :2] / (c[:, 2:3] + 1e-7)).view(B, 2, H, W).permute(0, 2, 3, 1)
    grid = (torch.stack([pix[..., 0] / (W - 1), pix[..., 1] / (H - 1)], -1) - 0.5) * 2
    valid = (grid.abs().max(dim=-1)[0] <= 1).unsqueeze(1).to(dt)
    synth = F.grid_sample(s["src"].to(dt), grid, mode="bilinear", padding_mode=R.PAD_NAME[pad], align_corners=False)
    loss, pmap = wl.masked_photometric_mean(synth, s["tgt"].to(dt), valid, bool(use_mask))
    return dict(loss=loss.detach(), g_photo=torch.autograd.grad(loss, d)[0], valid=valid.view(B, H, W), grid=grid.detach(), pmap=pmap.detach().view(B, H, W))


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _folded32(shape, pad, use_mask, expanded, form):
    s = expanded_scene(*shape) if expanded else R.fused_scene(*shape)
    return folded(s, geometry12(s, form), pad, use_mask, F32)


@functools.lru_cache(maxsize=None)
def lg_case(shape, pad, use_mask, reg_kind, expanded=False):
    """fused_case (or its restatement for the expanded scene) + the two folded float32 samples under "folded" """
    c = dict(scene_case(expanded_scene(*shape), pad, use_mask, reg_kind) if expanded else R.fused_case(shape, pad, use_mask, reg_kind))
    c["shape"], c["expanded"] = shape, expanded
    c["folded"] = {form: _folded32(shape, pad, use_mask, expanded, form) for form in FORMS}
    return c


LG_CASES = [(shape, pad, mask, reg) for shape in LG_SHAPES for pad in PADS for mask in MASKS for reg in REGS]
HOSTGEO_CASES = [(shape, pad, mask, reg) for shape in HOSTGEO_SHAPES for pad in PADS for mask in MASKS for reg in (0, 2)]
EXPAND_CASES = [(shape, pad, mask, reg) for shape in EXPAND_SHAPES for pad in PADS for mask in MASKS for reg in REGS]


def grad_keep(case, g_loss):
    """the pixels at which g_depth_tgt is compared"""
    return ~(case["grad_excluded"] | (case["reg_excluded_t"] if g_loss[1] else torch.zeros_like(case["grad_excluded"])))


def grad_samples(case, g_loss, form):
    """g_depth_tgt of the two float32 formulations"""
    alt = {**case, F32: {**case[F32], "g_photo": case["folded"][form]["g_photo"]}}
    return [R.fused_grads(case, g_loss, F32)[0], R.fused_grads(alt, g_loss, F32)[0]]


def _rel(samples, r64, keep=None):
    """the largest max|r32 - r64| / max|r64| of the float32 samples (0 where the reference vanishes)"""
    r64 = torch.as_tensor(r64).double()
    a = r64[keep] if keep is not None else r64
    top = float(a.abs().max()) if a.numel() else 0.0
    if top == 0:
        return 0.0
    return max(float(((b.double()[keep] if keep is not None else b.double()) - a).abs().max()) for b in samples) / top


@functools.lru_cache(maxsize=None)
def pooled_grad(pad, use_mask, reg_kind, g_loss, form):
    out = 0.0
    for shape in LG_SHAPES:
        c = lg_case(shape, pad, use_mask, reg_kind)
        out = max(out, _rel(grad_samples(c, g_loss, form), R.fused_grads(c, g_loss, F64)[0], grad_keep(c, g_loss)))
    return out


def grad_bound(case, g_loss, form):
    """the bound on max|g_depth_tgt - r64| over grad_keep(case, g_loss)"""
    keep = grad_keep(case, g_loss)
    t64 = R.fused_grads(case, g_loss, F64)[0]
    top = float(t64[keep].abs().max())
    own = max(R.bound(t32, t64, keep) for t32 in grad_samples(case, g_loss, form))
    return min(max(own, R.FACTOR * pooled_grad(case["pad"], case["use_mask"], case["reg_kind"], tuple(g_loss), form) * top), R.CAP * top)


def src_grad_bound(case, g_loss):
    s64, s32 = R.fused_grads(case, g_loss, F64)[1], R.fused_grads(case, g_loss, F32)[1]
    return R.bound(s32, s64, ~case["reg_excluded_s"])


def loss_samples(case, form):
    return [case[F32]["loss"], case["folded"][form]["loss"]]


@functools.lru_cache(maxsize=None)
def pooled_loss(pad, use_mask, form):
    return max(_rel(loss_samples(c, form), c[F64]["loss"]) for c in (lg_case(shape, pad, use_mask, 0) for shape in LG_SHAPES))


@functools.lru_cache(maxsize=None)
def pooled_reg(reg_kind):
    return max(_rel([c[F32]["reg"]], c[F64]["reg"]) for c in (lg_case(shape, 0, 0, reg_kind) for shape in LG_SHAPES))


def loss_bound(case, form):
    """the bound on |loss_out[0] - l64|"""
    l64 = case[F64]["loss"]
    top = abs(float(l64))
    own = max(R.bound(l32, l64) for l32 in loss_samples(case, form))
    return min(max(own, R.FACTOR * pooled_loss(case["pad"], case["use_mask"], form) * top), R.CAP * top)


def reg_bound(case):
    """the bound on |loss_out[1] - reg64| (reg_kind != 0)"""
    l64 = case[F64]["reg"]
    top = abs(float(l64))
    return min(max(R.bound(case[F32]["reg"], l64), R.FACTOR * pooled_reg(case["reg_kind"]) * top), R.CAP * top)


# ---------------------------------------------------------------------------------------------------------------------------------------
# per-tile sums of the two loss maps (what a workgroup adds to its slot in the chained form)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _tiles(m, tile_h, tile_w):
    B, H, W = m.shape
    m = F.pad(m, (0, -W % tile_w, 0, -H % tile_h))
    return m.view(B, m.shape[1] // tile_h, tile_h, m.shape[2] // tile_w, tile_w).sum((2, 4))


def tile_sums(case, tile_h, tile_w):
    """(photometric, regulariser or None), each (B, tile rows, tile columns), from the float64 reference of the case"""
    s, reg_kind = case["scene"], case["reg_kind"]
    photo = _tiles(case[F64]["pmap"], tile_h, tile_w)
    if not reg_kind:
        return photo, None
    e_t, e_s = s["ri_t"].double() - s["depth"].double(), s["ri_s"].double() - s["d_src"].double()
    return photo, _tiles(e_t ** 2 + e_s ** 2 if reg_kind == 2 else e_t.abs() + e_s.abs(), tile_h, tile_w)


@functools.lru_cache(maxsize=None)
def overflow_case(offset=OVERFLOW_OFFSETS[0], pad=1, use_mask=1):
    return scene_case(overflow_scene(offset), pad, use_mask, OVERFLOW_REG)
