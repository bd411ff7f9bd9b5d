"""Float64 references of the contracts include/e2eslam.h states for csrc/disp_pyramid.hip (host only; no tests in this file), written
from the header's comment with explicit index arithmetic (no F.interpolate):

    e2e_disp_pyramid_depth_fwd   sy = max((y + 0.5) h / H - 0.5, 0), y0 = floor(sy), y1 = min(y0 + 1, h - 1), wy = sy - y0 (same in x);
                                 u = the four-weight sum; depth = scale / (lo + (hi - lo) u) for every present scale -> (S,B,1,H,W)
    e2e_disp_pyramid_depth_bwd   g_u = -g_depth scale (hi - lo) / (lo + (hi - lo) u)^2; g_d[j,i] = sum over the fine pixels whose stencil
                                 touches (j,i) of their weight on it times g_u

y0 is taken in INTEGER arithmetic (floor(((2y + 1) h - H) / 2H)), so the stencil and the footprint of a coarse index are exact statements
about indices; tests/test_disp_pyramid_inputs.py holds all of it against float64 F.interpolate, autograd and a brute-force table.

BOUNDS (derived from the operation count, eps = 2^-24 the unit roundoff of fp32; none of them is a measured number).  Disparities are
drawn from [D_LO, D_HI] = [0.1, 0.9] and every case has hi >= 10 lo, which the counts below use.
  forward, |gpu - r64| <= FWD * eps * |r64| element by element:
    u         4 products of an exact weight and a disparity, 3 sums, all terms positive                       4
    span      1/min and 1/max from the fp32 limits (1 each), their difference (hi + lo)/(hi - lo) <= 1.25,
              rounded to fp32 (1); lo: 2                                                                        2.25
    den       fma(span, u, lo): max(2, 2.25 + 4) + 1                                                            7.25
    depth     scale rounded to fp32 (1), one division (1)                                                       9.25  -> FWD = 10
  ratios that are no power of two add the fp32 rounding of the weights (1 - wy, the product: 3) and of sy: r = h / H rounded and one
  fused multiply-add, |d sy| <= 2 eps h, so |d u| <= (D_HI - D_LO) 2 eps (h + w) and |d u| / u <= 16 eps (h + w):  FWD = 13 + 16 (h + w).
  backward, |gpu - r64| <= eps * (BWD * A_w + SY * A_1) with A_w[j,i] = sum of weight |g_u| and A_1[j,i] = sum of |g_u| over the footprint:
    g_u       den^2 (2 * 7.25 + 1), scale * span (1 + 2.25 + 1), the product with g (1), the division (1)       21.75 -> 22
    the sum   n terms, each one fused multiply-add, then the lanes' tree: at most n roundings on any term        n = the largest footprint
  and for the other ratios 3 (the weight) + 32 (h + w) (den^2 through u) more on A_w, and SY = 2 (h + w): the weight itself moves by
  |d sy| in each axis."""
import zlib

import torch

EPS = 2.0 ** -24
D_LO, D_HI = 0.1, 0.9
FWD_TILE = (4, 64)                  # csrc/disp_pyramid.hip: a forward workgroup writes 4 rows x 64 columns of one plane
BWD_THREADS = 256                   # a backward workgroup: 256 lanes, lanes_per_pixel() of them to a coarse pixel

# B, (H, W), {slot: (h, w)}, (min_depth, max_depth), scale, the regimes the case is there for
CASES = {
    "factor2": dict(B=1, size=(8, 12), scales={0: (4, 6)}, limits=(0.1, 80.0), scale=1.0, reaches={"clamped_sy", "clamped_y1"}),
    # factor 8: 16-wide footprints, one coarse pixel to a whole wave
    "factor8": dict(B=2, size=(24, 40), scales={0: (3, 5)}, limits=(0.5, 10.0), scale=6.9, reaches={"clamped_sy", "clamped_y1", "wave_per_pixel"}),
    # no integer ratio: the weights and sy round in fp32
    "ragged": dict(B=1, size=(13, 17), scales={0: (5, 7)}, limits=(0.1, 80.0), scale=1.0, reaches={"clamped_sy", "clamped_y1", "inexact"}),
    # every index clamped: one coarse pixel owns the whole image
    "one_pixel": dict(B=1, size=(4, 4), scales={0: (1, 1)}, limits=(0.1, 80.0), scale=6.9, reaches={"clamped_sy", "clamped_y1", "all_clamped"}),
    # more than one tile both ways, both edges ragged: column 64 (the forward tile's edge) lies inside the footprints of coarse columns
    # 31 and 32, and a backward workgroup (256 / 8 = 32 coarse pixels) ends inside a coarse row of 33
    "tiles": dict(B=1, size=(18, 66), scales={0: (9, 33)}, limits=(0.1, 80.0), scale=1.0,
                  reaches={"clamped_sy", "clamped_y1", "multi_tile", "tile_edge"}),
    # the identity: bitwise e2e_disp_range_depth_fwd / _bwd
    "identity": dict(B=1, size=(8, 12), scales={0: (8, 12)}, limits=(0.1, 80.0), scale=6.9, reaches={"identity"}),
    # one launch over the four scales of a 32 x 64 image, then with absent scales
    "four": dict(B=2, size=(32, 64), scales={0: (32, 64), 1: (16, 32), 2: (8, 16), 3: (4, 8)}, limits=(0.1, 80.0), scale=1.0,
                 reaches={"clamped_sy", "clamped_y1", "multi_tile", "identity"}),
    "zero_two": dict(B=2, size=(32, 64), scales={0: (32, 64), 2: (8, 16)}, limits=(0.1, 80.0), scale=1.0, reaches={"absent", "multi_tile"}),
    "three": dict(B=2, size=(32, 64), scales={3: (4, 8)}, limits=(0.5, 10.0), scale=6.9, reaches={"absent", "wave_per_pixel"}),
}


def inputs(name):
    """the float32 operands of a case on the CPU, from a seed that depends on the case alone: {slot: disp (B,1,h,w)} in [D_LO, D_HI] and
    the gradient g (S,B,1,H,W) of the depths"""
    c = CASES[name]
    gen = torch.Generator().manual_seed(zlib.crc32(repr(("disp_pyramid", name)).encode()))
    disps = {k: torch.rand(c["B"], 1, h, w, generator=gen) * (D_HI - D_LO) + D_LO for k, (h, w) in sorted(c["scales"].items())}
    return disps, torch.randn(len(disps), c["B"], 1, *c["size"], generator=gen)


# ---- one axis ------------------------------------------------------------------------------------------------------------------------
def stencil(n, N):
    """for every fine index y < N on an axis of n coarse samples: (y0, y1, wy) -- int64, int64, float64"""
    y = torch.arange(N, dtype=torch.int64)
    num = (2 * y + 1) * n - N                                   # sy = num / 2N before the clamp
    y0 = torch.where(num < 0, torch.zeros_like(y), torch.div(num, 2 * N, rounding_mode="floor"))
    sy = torch.clamp(num.double() / (2 * N), min=0.0)
    return y0, torch.clamp(y0 + 1, max=n - 1), sy - y0.double()


def footprint(j, n, N):
    """(first, last) fine index whose stencil touches coarse index j -- y0 in {j - 1, j} -- in closed form; the brute-force table of
    tests/test_disp_pyramid_inputs.py holds it against stencil().  j = 1 starts at 0 as well: the indices whose sy was clamped to 0 have
    y0 = 0 and y1 = 1 (with weight 0 on it)."""
    ceil_div = lambda a, b: -((-a) // b)
    first = 0 if j <= 1 else max(0, ceil_div(N * (2 * j - 1) - n, 2 * n))
    last = min(N - 1, ceil_div(N * (2 * j + 3) - n, 2 * n) - 1)
    return first, last


def axis_matrix(n, N):
    """(n, N) float64: entry (j, y) is the weight of coarse index j in the stencil of fine index y (both taps where y1 was clamped)"""
    y0, y1, wy = stencil(n, N)
    M = torch.zeros(n, N, dtype=torch.float64)
    y = torch.arange(N)
    M.index_put_((y0, y), 1 - wy, accumulate=True)
    M.index_put_((y1, y), wy, accumulate=True)
    return M


# ---- the two contracts ----------------------------------------------------------------------------------------------------------------
def upsample(d, size):
    """(B,1,h,w) -> (B,1,H,W) float64 by the four-weight formula"""
    (y0, y1, wy), (x0, x1, wx) = stencil(d.shape[2], size[0]), stencil(d.shape[3], size[1])
    d = d.double()
    wy, wx = wy[:, None], wx[None, :]
    g = lambda a, b: d[:, :, a[:, None], b[None, :]]
    return (1 - wy) * (1 - wx) * g(y0, x0) + (1 - wy) * wx * g(y0, x1) + wy * (1 - wx) * g(y1, x0) + wy * wx * g(y1, x1)


def _limits(min_depth, max_depth):
    return 1 / torch.tensor(max_depth, dtype=torch.float64), 1 / torch.tensor(min_depth, dtype=torch.float64)


def pyramid_depth(disps, size, min_depth, max_depth, scale):
    """{slot: (B,1,h,w)} -> (S,B,1,H,W) float64, the present scales in ascending order"""
    lo, hi = _limits(min_depth, max_depth)
    return torch.stack([scale / (lo + (hi - lo) * upsample(disps[k], size)) for k in sorted(disps)])


def g_u(g, disps, size, min_depth, max_depth, scale):
    lo, hi = _limits(min_depth, max_depth)
    u = torch.stack([upsample(disps[k], size) for k in sorted(disps)])
    return -g.double() * scale * (hi - lo) / (lo + (hi - lo) * u) ** 2


def gather(gu, shape, size, drop=None, weighted=True):
    """the adjoint's second half for one scale: (B,1,H,W) -> (B,1,h,w), g_d[j,i] = sum over the footprint of weight * gu.  drop = (y, x):
    that fine pixel is left out of every footprint.  weighted=False: the plain sum over the footprint (weight 1 wherever the stencil
    touches)."""
    My, Mx = axis_matrix(shape[0], size[0]), axis_matrix(shape[1], size[1])
    if not weighted:
        for M, n, N in ((My, shape[0], size[0]), (Mx, shape[1], size[1])):
            M.zero_()
            for j in range(n):
                first, last = footprint(j, n, N)
                M[j, first:last + 1] = 1
    gu = gu.double().clone()
    if drop is not None:
        gu[:, :, drop[0], drop[1]] = 0
    return My @ gu @ Mx.T


def pyramid_depth_bwd(g, disps, size, min_depth, max_depth, scale):
    """-> {slot: g_disp (B,1,h,w)} float64"""
    gu = g_u(g, disps, size, min_depth, max_depth, scale)
    return {k: gather(gu[s], disps[k].shape[2:], size) for s, k in enumerate(sorted(disps))}


# ---- the derived bounds ---------------------------------------------------------------------------------------------------------------
def exact_ratio(shape, size):
    """both ratios are powers of two: sy and every weight are exact in fp32"""
    pow2 = lambda n, N: N % n == 0 and (N // n) & (N // n - 1) == 0
    return pow2(shape[0], size[0]) and pow2(shape[1], size[1])


def largest_footprint(shape, size):
    side = lambda n, N: max(b - a + 1 for a, b in (footprint(j, n, N) for j in range(n)))
    return side(shape[0], size[0]) * side(shape[1], size[1])


def fwd_ops(shape, size):
    return 10 if exact_ratio(shape, size) else 13 + 16 * (shape[0] + shape[1])


def bwd_tolerance(gu, shape, size):
    """(B,1,h,w) float64: the absolute bound of every element of g_disp, from this scale's g_u (B,1,H,W)"""
    a_w = gather(gu.abs(), shape, size)
    n = largest_footprint(shape, size)
    if exact_ratio(shape, size):
        return EPS * (22 + n) * a_w
    hw = shape[0] + shape[1]
    return EPS * ((25 + n + 32 * hw) * a_w + 2 * hw * gather(gu.abs(), shape, size, weighted=False))


def lanes_per_pixel(shape, size):
    """csrc/disp_pyramid.hip, dp_lpp_shift: the footprint candidates (2 ceil(f) + 3 a side) at about eight a lane, a power of two <= 64"""
    n = (2 * -(-size[0] // shape[0]) + 3) * (2 * -(-size[1] // shape[1]) + 3)
    lanes = 1
    while lanes < 64 and 8 * lanes < n:
        lanes *= 2
    return lanes
