"""Host-side half of tests/test_gpu_warp_photo_contracts.py: the inputs of every case, their float64 and float32 references (oracle.warp_loss
and torch.nn.functional.grid_sample on the CPU, gradients by autograd), the bound each comparison gets and the kink exclusions.  Nothing here
touches a GPU, so tests/test_warp_contract_inputs.py can prove without one that every case excludes what it may and holds the edges it claims.

Bound (one per compared tensor, from the references alone): FACTOR x max|r32 - r64|, floored at FACTOR x 2^-24 x max|r64| and capped at
CAP x max|r64|.  Exclusion bands: BAND x max|q32 - q64| of the quantity q whose kink it is (max|grid| against 1, a source index against an
integer or the border clamp, y - x against 0, c2 against 1e-3, the unclamped SSIM value against 0 and 1), q taken from the reference.

Two readings this module fixes, because the rule above does not decide them:
  * An element that sits EXACTLY on a kink in the float64 reference and whose two operands are identical there (y == x, all-zero windows: the
    SSIM value is exactly 0, y - x is exactly 0) is compared, not excluded: both sides are specified (clamp passes the gradient on its closed
    edge, sign(0) = 0) and the function has its extremum there, so the gradient vanishes whichever way a gate rounds.
  * With y == x every compared tensor is identically zero, so max|r64| is zero (or float64 rounding noise) and says nothing about the size of
    the terms that cancel; and the float32 reference is exactly zero too, but only because its operands are bit-identical and its sequence of
    operations is symmetric in them (it stays within 4e-6 even one ulp beside y == x) -- an FMA-contracted evaluation has no such symmetry,
    and in a flat window (variance 8e-4 under a mean of 0.9 in the 3 x 3 case) one ulp of E[x^2], 6e-8, is 2.4e-5 of 2 sigma + C2.  The
    float32 reference cannot measure that, so FACTOR x its error is not a bound a correct kernel can meet there: those cases are bounded by
    the cap, CAP x max|r64| of the companion case (the same x and upstream gradients with an independent y, whose terms have the same size).
  * The fused pair's g_depth_tgt is the end of the longest chain here, and on a 2 x 2 image the float32 reference's largest error is the
    largest of four samples.  Its bound is the rule's, or, where that is larger, FACTOR x the largest max|r32 - r64| / max|r64| that the
    reference shows on any shape of the same configuration, times this case's max|r64|; never more than the cap (fused_grad_bound)."""
import functools
import zlib

import torch
import torch.nn.functional as F

from oracle import warp_loss as wl

F64, F32 = torch.float64, torch.float32
FACTOR, BAND, CAP, EPS32 = 8.0, 16.0, 1e-4, 2.0 ** -24
PAD_NAME = {0: "zeros", 1: "border"}                     # E2E_PADDING_ZEROS / E2E_PADDING_BORDER


# seeds chosen (tests/test_warp_contract_inputs.py checks the outcome) so that every case holds its planted edges and excludes at most 1 %
SALT = {("E", 1, 37, 53): 2}


def gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_()


def bound(r32, r64, keep=None):
    """the bound on max|gpu - r64| over `keep` (default: everything)"""
    r32, r64 = torch.as_tensor(r32).double(), torch.as_tensor(r64).double()
    if keep is not None:
        r32, r64 = r32[keep], r64[keep]
    if r64.numel() == 0:
        return 0.0
    top = float(r64.abs().max())
    return min(max(FACTOR * float((r32 - r64).abs().max()), FACTOR * EPS32 * top), CAP * top)


def band(q32, q64):
    return BAND * float((q32.double() - q64).abs().max())


def dilate(mask, r):
    """mask (B,H,W) or (B,C,H,W) bool -> true wherever the (2r+1)^2 window holds a true element"""
    m = mask.float() if mask.dim() == 4 else mask.float()[:, None]
    m = F.max_pool2d(m, 2 * r + 1, 1, r) > 0
    return m if mask.dim() == 4 else m[:, 0]


def intrinsics(B, H, W, *seed):
    """a different K per batch element with a nonzero skew -> (K, inv_K) (B,4,4) float32"""
    g = gen("K", B, H, W, *seed)
    K = torch.zeros(B, 4, 4, dtype=F64)
    r = torch.rand(B, 5, generator=g, dtype=F64)
    K[:, 0, 0] = (W - 1) * (0.8 + 0.3 * r[:, 0])
    K[:, 1, 1] = (H - 1) * (0.8 + 0.3 * r[:, 1])
    K[:, 0, 1] = 0.05 * K[:, 0, 0] * (0.5 + r[:, 2])
    K[:, 0, 2] = (W - 1) / 2 + r[:, 3] - 0.5
    K[:, 1, 2] = (H - 1) / 2 + r[:, 4] - 0.5
    K[:, 2, 2] = K[:, 3, 3] = 1
    return K.float(), torch.linalg.inv(K).float()


def rigid(B, angle, tmax, *seed):
    """general rigid transforms (B,4,4) float32: `angle` rad about a random skew axis, translation uniform in [-tmax, tmax]^3"""
    g = gen("T", B, *seed)
    w = torch.randn(B, 3, generator=g, dtype=F64)
    w = w / w.norm(dim=1, keepdim=True) * angle
    S = torch.zeros(B, 3, 3, dtype=F64)
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 2] = -w[:, 2], w[:, 1], -w[:, 0]
    S = S - S.transpose(1, 2)
    T = torch.eye(4, dtype=F64).repeat(B, 1, 1)
    T[:, :3, :3] = torch.linalg.matrix_exp(S)
    T[:, :3, 3] = (torch.rand(B, 3, generator=g, dtype=F64) * 2 - 1) * tmax
    return T.float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. backproject
# ---------------------------------------------------------------------------------------------------------------------------------------
BHW_SHAPES = [(1, 2, 2), (2, 3, 5), (2, 9, 33), (1, 683, 768)]        # the last: 2049 x 256 pixels, one block past the launch cap


@functools.lru_cache(maxsize=None)
def backproject_case(B, H, W):
    g = gen("A", B, H, W)
    N = H * W
    depth = torch.rand(B, 1, H, W, generator=g) * 3 + 0.1
    depth.view(-1)[1::3] *= -1.0
    depth.view(-1)[::5] = 0.0
    K, invK = intrinsics(B, H, W)
    g_cam = torch.randn(B, 4, N, generator=g)
    case = dict(B=B, H=H, W=W, depth=depth, invK=invK, g_cam=g_cam)
    for dt in (F64, F32):
        d = leaf(depth, dt)
        cam = wl.backproject(d, invK.to(dt))
        (cam * g_cam.to(dt)).sum().backward()
        case[dt] = dict(cam=cam.detach(), g_depth=d.grad.reshape(B, N))
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. project3d
# ---------------------------------------------------------------------------------------------------------------------------------------
ZCLAMP = 1e-3
BELOW = (8e-4, 9.5e-4, 3e-4, 6e-4)                                    # 0 < c2 < 1e-3
ABOVE = (1.03e-3, 1.1e-3, 1.05e-3, 1.2e-3)                            # just above the clamp
ORDINARY, BEHIND, NEAR_BELOW, NEAR_ABOVE = 0, 1, 2, 3


@functools.lru_cache(maxsize=None)
def project_case(B, H, W):
    """points that project to pixels spread over [-0.15, 1.15] of the image (grid in [-1.3, 1.3]) at depths 0.5 .. 3, w in {1, 0.5, 2}; the
    small shapes also hold points behind the camera and on either side of z_out's clamp.  The clamp-side points lie within a few centimetres
    of the camera centre (the translation is small), so that c2 ~ 1e-3 is computed from small terms: 1/z amplifies every absolute rounding
    error of the projection 1000 times, and with metre-sized terms no float32 evaluation, the reference's included, stays inside the cap.
    They are compared as a group of their own (`near`), so their looser bound does not cover for the ordinary points."""
    g = gen("B", B, H, W, SALT.get(("B", B, H, W), 0))
    N = H * W
    K, _ = intrinsics(B, H, W)
    T = rigid(B, 0.3, 0.04, H, W)
    P = torch.matmul(K.double(), T.double())[:, :3, :]
    u = (torch.rand(B, N, generator=g, dtype=F64) * 1.3 - 0.15) * (W - 1)
    v = (torch.rand(B, N, generator=g, dtype=F64) * 1.3 - 0.15) * (H - 1)
    c2 = torch.rand(B, N, generator=g, dtype=F64) * 2.5 + 0.5
    kind = torch.zeros(B, N, dtype=torch.long)
    if N < 10000:
        h = 1 if N < 10 else (2 if N < 100 else 4)
        for b in range(B):
            where = torch.randperm(N, generator=g)[:3 * h]
            for k in range(h):
                i, j, l = where[3 * k:3 * k + 3]
                kind[b, i], c2[b, i] = BEHIND, -c2[b, i]
                kind[b, j], c2[b, j] = NEAR_BELOW, BELOW[(k + b) % 4]
                kind[b, l], c2[b, l] = NEAR_ABOVE, ABOVE[(k + b) % 4]
    w = torch.tensor([1.0, 0.5, 2.0], dtype=F64)[torch.arange(N) % 3].repeat(B, 1)
    c = torch.stack([u * c2, v * c2, c2], 1)
    X = torch.linalg.solve(P[:, :, :3], c - P[:, :, 3:] * w[:, None, :])
    points = torch.cat([X, w[:, None, :]], 1).float()
    near = kind >= NEAR_BELOW
    g_grid = torch.randn(B, H, W, 2, generator=g)
    g_grid[near.view(B, H, W)] *= 1e-3                                 # d grid / d point is 1000 times larger there
    g_z = torch.randn(B, H, W, generator=g)
    case = dict(B=B, H=H, W=W, points=points, K=K, T=T, g_grid=g_grid, g_z=g_z, kind=kind, near=near)
    for dt in (F64, F32):
        p = leaf(points, dt)
        grid, z, valid = wl.project(p, K.to(dt), T.to(dt), H, W, geometric=True)
        l_grid = (grid * g_grid.to(dt)).sum()
        gp, = torch.autograd.grad(l_grid, p, retain_graph=True)
        gpz, = torch.autograd.grad(l_grid + (z.view(B, H, W) * g_z.to(dt)).sum(), p)
        cz = torch.matmul(torch.matmul(K.to(dt), T.to(dt))[:, 2:3, :], p.detach())[:, 0]      # z_out before its clamp
        case[dt] = dict(grid=grid.detach(), z=z.detach().view(B, N), valid=valid.view(B, N), m=grid.detach().abs().amax(-1).view(B, N),
                        c2=cz, g_points=gp, g_points_z=gpz)
    r64, r32 = case[F64], case[F32]
    case["valid_band"], case["gate_band"] = torch.zeros(B, N, dtype=torch.bool), torch.zeros(B, N, dtype=torch.bool)
    for grp in (near, ~near):                                          # each group's band from its own reference error
        if grp.any():
            case["valid_band"] |= grp & ((r64["m"] - 1).abs() < band(r32["m"][grp], r64["m"][grp]))
            case["gate_band"] |= grp & ((r64["c2"] - ZCLAMP).abs() < band(r32["c2"][grp], r64["c2"][grp]))
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. grid_sample
# ---------------------------------------------------------------------------------------------------------------------------------------
GS_SHAPES = [(1, 1, 1, 1, 2, 3), (2, 5, 11, 19, 6, 9), (1, 3, 6, 9, 11, 19), (2, 2, 40, 56, 40, 56)]
GS_LOOP = (1, 1, 7, 9, 683, 768)                                      # second trip of the sampling loops
GS_CONVERT = (1, 3, 592, 592, 5, 7)                                   # second trip of the fixed-point conversion (border, align off only)
LAYOUTS = ("nchw", "nhwc", "cols", "expand")                          # expand: one image behind both batch elements (sb = 0), so B = 2 only
GS_CASES = [(s, l) for s in GS_SHAPES for l in LAYOUTS if l != "expand" or s[0] == 2]


def layout_base(layout, B, C, Hi, Wi, g):
    """the memory behind a (B,C,Hi,Wi) view: dense, channels last, every second column of a buffer twice as wide, one image for every batch element"""
    shape = {"nchw": (B, C, Hi, Wi), "nhwc": (B, Hi, Wi, C), "cols": (B, C, Hi, 2 * Wi), "expand": (1, C, Hi, Wi)}[layout]
    return torch.rand(shape, generator=g) * 2 - 0.5


def layout_view(layout, base, B):
    if layout == "nhwc":
        return base.permute(0, 3, 1, 2)
    if layout == "cols":
        return base[..., ::2]
    if layout == "expand":
        return base.expand(B, -1, -1, -1)
    return base


def source_index(gc, size, align, dt):
    gc = gc.to(dt)
    return (gc + 1) / 2 * (size - 1) if align else ((gc + 1) * size - 1) / 2


def index_kink(gc, size, pad, align):
    """the grid coordinates whose float64 source index lies within the band of an integer at which the sampler's slope jumps: 0 .. size-1
    (with border padding the first and last are the clamp), and -1 and size as well with zero padding"""
    i64, i32 = source_index(gc, size, align, F64), source_index(gc, size, align, F32)
    near = i64.round()
    lo, hi = (0, size - 1) if pad == 1 else (-1, size)
    return ((i64 - near).abs() < band(i32, i64)) & (near >= lo) & (near <= hi)


@functools.lru_cache(maxsize=None)
def grid_sample_case(shape, layout, pad, align):
    B, C, Hi, Wi, Ho, Wo = shape
    g = gen("C", shape, layout)                                       # the same image and grid for every padding / alignment
    No = Ho * Wo
    base = layout_base(layout, B, C, Hi, Wi, g)
    grid = (torch.rand(B, No, 2, generator=g) * 2.6 - 1.3)
    planted = torch.zeros(B, No, dtype=torch.bool)
    n_pl = min(int(0.04 * B * No), 64)               # under 5 % of the case: the 2 x 3 grid has room for none
    for k in range(n_pl):                                              # the tail of batch element 0: pixel centres, then +-1
        sizes = torch.tensor([Wi, Hi], dtype=F64)
        if k % 2 == 0:
            px = (torch.rand(2, generator=g, dtype=F64) * sizes).floor()
            gc = px / (sizes - 1).clamp(min=1) * 2 - 1 if align else (2 * px + 1) / sizes - 1
        else:
            gc = torch.tensor([[1.0, -1.0], [-1.0, 1.0], [1.0, 0.3], [-0.7, -1.0]], dtype=F64)[(k // 2) % 4]
        grid[0, No - 1 - k] = gc.float()
        planted[0, No - 1 - k] = True
    grid = grid.view(B, Ho, Wo, 2)
    g_out = torch.randn(B, C, Ho, Wo, generator=g)
    case = dict(shape=shape, layout=layout, base=base, grid=grid, g_out=g_out, planted=planted.view(B, Ho, Wo))
    for dt in (F64, F32):
        inp = leaf(layout_view(layout, base, B), dt)
        gr = leaf(grid, dt)
        out = F.grid_sample(inp, gr, mode="bilinear", padding_mode=PAD_NAME[pad], align_corners=bool(align))
        (out * g_out.to(dt)).sum().backward()
        case[dt] = dict(out=out.detach(), g_grid=gr.grad, g_input=inp.grad)
    kink = torch.stack([index_kink(grid[..., 0], Wi, pad, align), index_kink(grid[..., 1], Hi, pad, align)], -1)
    case["kink"] = kink & ~case["planted"][..., None]                  # what the rule excludes among the uniform samples
    case["keep"] = ~kink & ~case["planted"][..., None]                 # the g_grid elements that are compared
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. photometric
# ---------------------------------------------------------------------------------------------------------------------------------------
PH_SHAPES = [(1, 1, 2, 2), (2, 3, 2, 5), (1, 3, 5, 2), (1, 3, 3, 3), (2, 4, 9, 33), (1, 3, 17, 65)]
PH_KINDS = ("uniform", "masked", "same", "randn")
PH_UPSTREAM = ("p", "s", "ps")                                        # g_pmap only, g_ssim only, both


def ssim_unclamped(x, y):
    """oracle.warp_loss.ssim before its clamp (tests/test_warp_contract_inputs.py holds the two together bit for bit): the quantity whose distance
    to 0 and 1 decides whether the clamp's gate is a kink"""
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    x = F.pad(x, (1, 1, 1, 1), mode="reflect")
    y = F.pad(y, (1, 1, 1, 1), mode="reflect")
    mu_x = F.avg_pool2d(x, 3, 1)
    mu_y = F.avg_pool2d(y, 3, 1)
    sigma_x = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
    sigma_y = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
    sigma_xy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    return (1 - n / d) / 2


def zero_region(H, W):
    """what a validity mask leaves: a 5 x 5 block (as much of it as the image holds, column 0 kept) and, on the wider images, the last column"""
    m = torch.zeros(H, W, dtype=torch.bool)
    r0 = 1 if H > 6 else 0
    m[r0:r0 + 5, 1:6] = True
    if W >= 7:
        m[:, W - 1] = True
    return m


def clamp_kink(x, y):
    """(B,C,H,W): windows whose unclamped SSIM value is within the band of 0 or 1 without being exactly on it"""
    t64, t32 = ssim_unclamped(x.double(), y.double()), ssim_unclamped(x.float(), y.float())
    bt = band(t32, t64)
    return ((t64 != 0) & (t64.abs() < bt)) | ((t64 != 1) & ((t64 - 1).abs() < bt))


def l1_kink(x, y):
    d64, d32 = y.double() - x.double(), y.float() - x.float()
    return (d64 != 0) & (d64.abs() < band(d32, d64))


def _photometric_refs(x, y, g_pmap, g_ssim):
    out = {}
    for dt in (F64, F32):
        xx, yy = leaf(x, dt), leaf(y, dt)
        s, p = wl.ssim(xx, yy), wl.photometric(xx, yy)
        r = dict(ssim=s.detach(), pmap=p.detach())
        for up in PH_UPSTREAM:
            loss = ((p * g_pmap.to(dt)).sum() if "p" in up else 0) + ((s * g_ssim.to(dt)).sum() if "s" in up else 0)
            r["gx_" + up], r["gy_" + up] = torch.autograd.grad(loss, (xx, yy), retain_graph=True)
        out[dt] = r
    return out


@functools.lru_cache(maxsize=None)
def photometric_case(shape, kind):
    B, C, H, W = shape
    g = gen("D", shape)                                               # x and the upstream gradients are the same for every kind
    x = torch.rand(B, C, H, W, generator=g)
    y = torch.rand(B, C, H, W, generator=g)
    g_pmap = torch.randn(B, 1, H, W, generator=g)
    g_ssim = torch.randn(B, C, H, W, generator=g)
    if kind == "randn":
        x, y = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    elif kind == "same":
        y = x.clone()
    elif kind == "masked":
        zero = zero_region(H, W)
        x, y = x.masked_fill(zero, 0.0), y.masked_fill(zero, 0.0)
    case = dict(shape=shape, kind=kind, x=x, y=y, g_pmap=g_pmap, g_ssim=g_ssim)
    case.update(_photometric_refs(x, y, g_pmap, g_ssim))
    gate = dilate(clamp_kink(x, y), 1)
    sign = l1_kink(x, y)
    case["excluded"] = {"p": gate | sign, "s": gate, "ps": gate | sign}
    if kind == "same":                                                # see the module docstring
        case["bound"] = {k: CAP * float(v.abs().max()) for k, v in photometric_case(shape, "uniform")[F64].items()}
    else:
        case["bound"] = {k: bound(case[F32][k], case[F64][k], None if k in ("ssim", "pmap") else ~case["excluded"][k[3:]]) for k in case[F64]}
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. the fused pair
# ---------------------------------------------------------------------------------------------------------------------------------------
FUSED_SHAPES = [(1, 2, 2), (1, 3, 5), (2, 9, 33), (1, 37, 53)]
G_LOSS = ((1.3, 0.07), (0.0, 1.0), (1.0, 0.0))
REG_NAME = {1: "l1", 2: "l2"}


@functools.lru_cache(maxsize=None)
def fused_scene(B, H, W):
    g = gen("E", B, H, W, SALT.get(("E", B, H, W), 0))
    K, invK = intrinsics(B, H, W, "E")
    depth = torch.rand(B, H, W, generator=g) * 2 + 1
    d_src = torch.rand(B, H, W, generator=g) * 2 + 1
    return dict(B=B, H=H, W=W, K=K, invK=invK, T=rigid(B, 0.15, 0.3, H, W, "E"), depth=depth, d_src=d_src,
                ri_t=depth + 0.2 * torch.randn(B, H, W, generator=g), ri_s=d_src + 0.2 * torch.randn(B, H, W, generator=g),
                src=torch.rand(B, 3, H, W, generator=g), tgt=torch.rand(B, 3, H, W, generator=g))


@functools.lru_cache(maxsize=None)
def fused_case(shape, pad, use_mask, reg_kind):
    """the float64 / float32 composition backproject -> project -> grid_sample -> masked photometric mean (+ regulariser), its gradients wrt
    both depths for unit upstream gradients (the loss is linear in g_loss), and the pixels each comparison leaves out"""
    B, H, W = shape
    s = fused_scene(B, H, W)
    case = dict(scene=s, pad=pad, use_mask=use_mask, reg_kind=reg_kind)
    for dt in (F64, F32):
        d, ds = leaf(s["depth"], dt), leaf(s["d_src"], dt)
        pts = wl.backproject(d.view(B, 1, H, W), s["invK"].to(dt))
        grid, valid = wl.project(pts, s["K"].to(dt), s["T"].to(dt), H, W)
        synth = F.grid_sample(s["src"].to(dt), grid, mode="bilinear", padding_mode=PAD_NAME[pad], align_corners=False)
        loss, pmap = wl.masked_photometric_mean(synth, s["tgt"].to(dt), valid.to(dt), bool(use_mask))
        r = dict(grid=grid.detach(), m=grid.detach().abs().amax(-1), synth=synth.detach(), valid=valid.view(B, H, W), pmap=pmap.detach().view(B, H, W),
                 loss=loss.detach(), g_photo=torch.autograd.grad(loss, d)[0])
        if reg_kind:
            reg = wl.depth_regularizer(s["ri_t"].to(dt), d, REG_NAME[reg_kind]) + wl.depth_regularizer(s["ri_s"].to(dt), ds, REG_NAME[reg_kind])
            r["reg"] = reg.detach()
            r["g_reg_t"], r["g_reg_s"] = torch.autograd.grad(reg, (d, ds))
        case[dt] = r
    r64, r32 = case[F64], case[F32]
    vband = (r64["m"] - 1).abs() < band(r32["m"], r64["m"])
    idx = index_kink(r64["grid"][..., 0], W, pad, False) | index_kink(r64["grid"][..., 1], H, pad, False)
    m = r64["valid"][:, None].double() if use_mask else 1.0
    x, y = r64["synth"] * m, s["tgt"].double() * m
    d64, t64 = y - x, ssim_unclamped(x, y)
    x32, y32 = r32["synth"] * (r32["valid"][:, None] if use_mask else 1.0), s["tgt"] * (r32["valid"][:, None] if use_mask else 1.0)
    bd, bt = band(y32 - x32, d64), band(ssim_unclamped(x32, y32), t64)
    sign = ((d64 != 0) & (d64.abs() < bd)).any(1)
    gate = (((t64 != 0) & (t64.abs() < bt)) | ((t64 != 1) & ((t64 - 1).abs() < bt))).any(1)
    case["valid_band"] = vband
    case["pmap_excluded"] = dilate(vband, 1) if use_mask else torch.zeros_like(vband)
    case["grad_excluded"] = idx | sign | dilate(gate, 1) | (dilate(vband, 2) if use_mask else torch.zeros_like(vband))
    e_t, e_s = s["ri_t"].double() - s["depth"].double(), s["ri_s"].double() - s["d_src"].double()
    case["reg_excluded_t"] = (e_t != 0) & (e_t.abs() < band(s["ri_t"] - s["depth"], e_t)) if reg_kind == 1 else torch.zeros_like(vband)
    case["reg_excluded_s"] = (e_s != 0) & (e_s.abs() < band(s["ri_s"] - s["d_src"], e_s)) if reg_kind == 1 else torch.zeros_like(vband)
    return case


def fused_grads(case, g_loss, dt):
    """(g_depth_tgt, g_depth_src or None) for upstream gradients g_loss, combined in dtype dt"""
    r, (a, b) = case[dt], g_loss
    if not case["reg_kind"]:
        return a * r["g_photo"], None
    return a * r["g_photo"] + b * r["g_reg_t"], b * r["g_reg_s"]


def fused_grad_bound(case, g_loss, keep):
    """the bound on g_depth_tgt (module docstring): the rule's own, or the relative one pooled over the shapes of this configuration"""
    t64, t32 = fused_grads(case, g_loss, F64)[0], fused_grads(case, g_loss, F32)[0]
    top = float(t64[keep].abs().max())
    pooled = 0.0
    for shape in FUSED_SHAPES:
        c = fused_case(shape, case["pad"], case["use_mask"], case["reg_kind"])
        k = ~(c["grad_excluded"] | (c["reg_excluded_t"] if g_loss[1] else torch.zeros_like(c["grad_excluded"])))
        a, b = fused_grads(c, g_loss, F64)[0][k], fused_grads(c, g_loss, F32)[0][k]
        if float(a.abs().max()) > 0:
            pooled = max(pooled, float((b.double() - a).abs().max()) / float(a.abs().max()))
    return min(max(bound(t32, t64, keep), FACTOR * pooled * top), CAP * top)
