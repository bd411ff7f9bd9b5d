"""Float64 reference of the contract include/e2eslam.h states for csrc/disp_pyramid_smooth.hip (host only; no tests in this file):

    e2e_disp_pyramid_smoothness_lossgrad   per present scale K: img_K = F.avg_pool2d(img, (H / hK, W / wK)) in float64, loss_K =
                                           oracle.warp_loss.normalised_smoothness(dispK, img_K); loss_out[4] = sum_K weightK loss_K;
                                           g_dispK = weightK d loss_K / d dispK by autograd in float64

and a second formulation written from the structure the kernel uses (formulation(): raw sums scaled by |inv|, the gradient
sign(inv) gn inv - raw |inv| inv / N, no autograd), which tests/test_pyramid_smoothness_inputs.py holds against the first in float64, runs
in float32 as an emulation of the term, and runs with seeded faults.

BOUNDS (derived from the operation count, U = 2^-24 the unit roundoff of fp32, first order; none is a measured number of the kernel).
Images lie in [0, 1], so a box mean c lies in [0, 1], a sum of three channel differences in [0, 3] and the argument of exp in [-1, 0].
  box mean    n = fy fx terms added one after the other in some fixed order (n - 1 roundings on any term) and one division: relative
              n U, absolute n U (c <= 1); a scale of the image's own size takes the pixel itself: BOX = n if n > 1 else 0
  argument    a = (|dc0| + |dc1| + |dc2|) / 3: every difference 2 BOX U + U, two additions (2 U of a sum <= 3), the division (1):
              absolute (3 (2 BOX + 1) + 6) / 3 + 1 = 2 BOX + 4 in U
  exp         the allowance the project has recorded for a transcendental over such arguments (tests/test_gpu_depth_aux_contracts.py:
              expf over -mean_c |dI| in [-1, 0] read 0.42 .. 1.01 U): torch's fp32 exp on the CPU against float64 over the case's own
              arguments, and twice that is allowed; the argument's absolute error becomes the same relative error of the weight
  weight      times k = 1 / (B h (w - 1)) or 1 / (B (h - 1) w), rounded once from float64 (1), the product (1):
              W_REL = EXP + (2 BOX + 4 + 2) U
  raw         sum_e k w |d_p - d_q|: the difference (1), the product (1), and SUM = 12 roundings on any term (three terms a lane, a
              six-level tree over the wave, four waves; the tiles in float64): relative W_REL + 14 U, every term positive
  inv         the plane's sum of d (1 term a lane, the tree, the waves: 9), the mean rounded to fp32 (1), + 1e-7 (1), 1 / x (1): 12 U
  loss_K      sum_b |inv_b| raw_b in float64, rounded once:  relative W_REL + 27 U
  total       sum_K weightK loss_K in float64, rounded once: sum_K |weightK| tol_K + U |total| (the weights are fp32 numbers)
  gradient    g_p = weight (|inv| gn_p - coef), gn_p the signed sum of the <= 4 weighted edges of p with MAG_p = sum |k w| over them
              (W_REL each, three additions), coef = raw |inv| inv / N (W_REL + 14, the rounding to fp32 1, 12 + 12, two products: W_REL
              + 41), one fused multiply-add and the product with the weight (2):
              |weight| ((W_REL + 17 U) |inv| MAG_p + (W_REL + 43 U) |coef|)
The signs: the kernel takes an edge's sign from d_p - d_q in fp32, which is exact; every case but `flat` keeps every pair of neighbouring
NORMALISED disparities 2^-16 apart (min_gap), so neither side can see a zero the other does not, and no element is excluded anywhere."""
import zlib

import torch
import torch.nn.functional as F

from oracle import warp_loss

EPS = 2.0 ** -24
GAP = 2.0 ** -16
TILE = (8, 32)                      # csrc/disp_pyramid_smooth.hip: a workgroup owns 8 rows x 32 columns of one plane
SLOTS = 4
WEIGHTS = {0: 0.75, 1: -1.5, 2: 0.3125, 3: 2.25}         # distinct, exact in fp32, one of them negative

_FOUR = {0: (32, 64), 1: (16, 32), 2: (8, 16), 3: (4, 8)}
# B, (H, W), {slot: (h, w)}; salt: added to the seed so that the case meets the 2^-16 condition (tests/test_pyramid_smoothness_inputs.py)
CASES = {
    "four": dict(B=2, size=(32, 64), scales=_FOUR, salt=0),
    "zero_two": dict(B=2, size=(32, 64), scales={0: (32, 64), 2: (8, 16)}, salt=0),
    # more than one tile and ragged edges on both axes
    "ragged": dict(B=1, size=(36, 132), scales={0: (36, 132), 1: (18, 66)}, salt=0),
    # every pixel on a border, fy != fx
    "two_by_two": dict(B=2, size=(8, 16), scales={0: (4, 4), 1: (2, 2)}, salt=0),
    "anisotropic": dict(B=1, size=(30, 40), scales={0: (15, 10)}, salt=0),
    # the image is handed over as an NCHW view of NHWC memory
    "strided": dict(B=2, size=(32, 64), scales=_FOUR, salt=0, nhwc=True),
    # every disparity a constant per plane: the loss and every gradient element are exactly 0
    "flat": dict(B=2, size=(32, 64), scales=_FOUR, salt=0, flat=True),
}


def inputs(name):
    """the float32 operands of a case on the CPU: ({slot: disp (B,1,h,w)} = sigmoid(randn), img (B,3,H,W) uniform in [0, 1])"""
    c = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("pyramid_smoothness", name)).encode()) + c["salt"])
    disps = {}
    for k, (h, w) in sorted(c["scales"].items()):
        d = torch.sigmoid(torch.randn(c["B"], 1, h, w, generator=gen))
        if c.get("flat"):
            d = torch.full_like(d, 0.0) + (0.125 + 0.0625 * k + 0.25 * torch.arange(c["B"], dtype=torch.float32).view(-1, 1, 1, 1))
        disps[k] = d
    return disps, torch.rand(c["B"], 3, *c["size"], generator=gen)


def weights(name):
    return {k: WEIGHTS[k] for k in CASES[name]["scales"]}


def box(img, shape):
    """(B,3,H,W) -> (B,3,h,w): the mean of every (H / h) x (W / w) block"""
    return F.avg_pool2d(img, (img.shape[2] // shape[0], img.shape[3] // shape[1]))


def reference(disps, img, wts):
    """-> dict(loss {slot: float64 0-dim}, total, grad {slot: (B,1,h,w) float64, weighted})"""
    leaves = {k: d.double().requires_grad_(True) for k, d in disps.items()}
    loss = {k: warp_loss.normalised_smoothness(leaves[k], box(img.double(), d.shape[2:])) for k, d in disps.items()}
    total = sum(wts[k] * loss[k] for k in sorted(loss))
    grads = torch.autograd.grad(total, [leaves[k] for k in sorted(leaves)])
    return dict(loss={k: v.detach() for k, v in loss.items()}, total=total.detach(), grad=dict(zip(sorted(leaves), grads)))


def edge_weights(img_k):
    """exp(-mean_c |d img|) of the x-edges (B,1,h,w-1) and the y-edges (B,1,h-1,w), and the arguments"""
    ax = (img_k[:, :, :, :-1] - img_k[:, :, :, 1:]).abs().sum(1, keepdim=True) / 3
    ay = (img_k[:, :, :-1, :] - img_k[:, :, 1:, :]).abs().sum(1, keepdim=True) / 3
    return torch.exp(-ax), torch.exp(-ay), ax, ay


def formulation(disps, img, wts, dtype=torch.float64, fault=None):
    """The term as the kernel structures it, in `dtype`: per plane raw = sum_e k w |d_p - d_q| and gn_p = the signed sum of the edges of
    p, from the RAW disparities; then loss = sum_b |inv_b| raw_b and g = weight (sign(inv) gn inv - raw |inv| inv / N).  Same return
    value as reference().  fault: None, or one of
      "halo"        the x-edges that cross a tile's right border (column TILE[1] j - 1 to TILE[1] j) are dropped
      "square_box"  the box mean is taken over fx x fx instead of fy x fx (rows beyond the block's own are the next block's)
      "no_mean"     the mean's own term of the gradient is left out
      "swap"        the weights of the first two present scales are exchanged"""
    keys = sorted(disps)
    if fault == "swap":
        wts = {**wts, keys[0]: wts[keys[1]], keys[1]: wts[keys[0]]}
    loss, grad = {}, {}
    for k in keys:
        d = disps[k].to(dtype)
        B, _, h, w = d.shape
        im = img.to(dtype)
        fy, fx = im.shape[2] // h, im.shape[3] // w
        if fault == "square_box":                                               # fx rows from the block's first row, clipped to the image
            rows = (torch.arange(h)[:, None] * fy + torch.arange(fx)[None, :]).clamp(max=im.shape[2] - 1)
            img_k = im[:, :, rows, :].mean(3).reshape(B, 3, h, w, fx).mean(4)
        else:
            img_k = box(im, (h, w))
        wx, wy, _, _ = edge_weights(img_k)
        wx, wy = wx / (B * h * (w - 1)), wy / (B * (h - 1) * w)
        if fault == "halo":
            wx = wx.clone()
            wx[:, :, :, TILE[1] - 1::TILE[1]] = 0
        ex, ey = d[:, :, :, :-1] - d[:, :, :, 1:], d[:, :, :-1, :] - d[:, :, 1:, :]
        raw = (wx * ex.abs()).sum((1, 2, 3)) + (wy * ey.abs()).sum((1, 2, 3))   # (B,)
        gn = torch.zeros_like(d)
        sx, sy = wx * torch.sign(ex), wy * torch.sign(ey)
        gn[:, :, :, :-1] += sx
        gn[:, :, :, 1:] -= sx
        gn[:, :, :-1, :] += sy
        gn[:, :, 1:, :] -= sy
        inv = 1 / (d.mean((1, 2, 3)) + 1e-7)
        loss[k] = (inv.abs() * raw).sum()
        mean_term = 0 if fault == "no_mean" else (raw * inv.abs() * inv / (h * w)).view(B, 1, 1, 1)
        grad[k] = wts[k] * (torch.sign(inv).view(B, 1, 1, 1) * gn * inv.view(B, 1, 1, 1) - mean_term)
    return dict(loss=loss, total=sum(wts[k] * loss[k] for k in keys), grad=grad)


def min_gap(disps):
    """the smallest |n_p - n_q| over every pair of neighbouring normalised disparities of every scale (float64)"""
    gaps = []
    for d in disps.values():
        n = d.double() / (d.double().mean((2, 3), keepdim=True) + 1e-7)
        gaps += [(n[:, :, :, :-1] - n[:, :, :, 1:]).abs().min(), (n[:, :, :-1, :] - n[:, :, 1:, :]).abs().min()]
    return float(min(gaps))


def exp_ulps(args64):
    """worst error of torch's fp32 exp on the CPU against float64 over the fp32 roundings of -args64, relative, in units of U"""
    x = (-args64).float()
    ref = torch.exp(x.double())
    return float(((torch.exp(x).double() - ref).abs() / ref).max()) / EPS


def bounds(disps, img, wts):
    """-> dict(loss {slot: absolute tolerance}, total, grad {slot: (B,1,h,w) absolute tolerance}), from float64 quantities alone"""
    ref = reference(disps, img, wts)
    out = dict(loss={}, grad={})
    for k, d in disps.items():
        d = d.double()
        B, _, h, w = d.shape
        n = (img.shape[2] // h) * (img.shape[3] // w)
        wx, wy, ax, ay = edge_weights(box(img.double(), (h, w)))
        w_rel = 2 * max(exp_ulps(ax), exp_ulps(ay)) * EPS + (2 * (n if n > 1 else 0) + 6) * EPS
        wx, wy = wx / (B * h * (w - 1)), wy / (B * (h - 1) * w)
        mag = torch.zeros_like(d)
        mag[:, :, :, :-1] += wx
        mag[:, :, :, 1:] += wx
        mag[:, :, :-1, :] += wy
        mag[:, :, 1:, :] += wy
        ex, ey = d[:, :, :, :-1] - d[:, :, :, 1:], d[:, :, :-1, :] - d[:, :, 1:, :]
        raw = (wx * ex.abs()).sum((1, 2, 3)) + (wy * ey.abs()).sum((1, 2, 3))
        inv = (1 / (d.mean((1, 2, 3)) + 1e-7)).view(B, 1, 1, 1)
        coef = (raw.view(B, 1, 1, 1) * inv.abs() * inv / (h * w)).abs()
        out["loss"][k] = (w_rel + 27 * EPS) * ref["loss"][k].abs()
        out["grad"][k] = abs(wts[k]) * ((w_rel + 17 * EPS) * inv.abs() * mag + (w_rel + 43 * EPS) * coef)
    out["total"] = sum(abs(wts[k]) * out["loss"][k] for k in disps) + EPS * ref["total"].abs()
    return out


_CACHE = {}


def case(name):
    """everything a test needs of a case, computed once and shared: dict(disps, img, weights, ref, bounds)"""
    if name not in _CACHE:
        disps, img = inputs(name)
        wts = weights(name)
        _CACHE[name] = dict(disps=disps, img=img, weights=wts, ref=reference(disps, img, wts), bounds=bounds(disps, img, wts))
    return _CACHE[name]


def worst(got, c):
    """{quantity: the largest |got - ref| / tolerance}; got = dict(loss {slot: x}, total, grad {slot: tensor})"""
    ref, tol = c["ref"], c["bounds"]
    out = {"total": float((torch.as_tensor(got["total"]).double() - ref["total"]).abs() / tol["total"])}
    for k in ref["loss"]:
        out[f"loss{k}"] = float((torch.as_tensor(got["loss"][k]).double() - ref["loss"][k]).abs() / tol["loss"][k])
        if got.get("grad") is not None:
            out[f"g_disp{k}"] = float(((got["grad"][k].double() - ref["grad"][k]).abs() / tol["grad"][k]).max())
    return out
