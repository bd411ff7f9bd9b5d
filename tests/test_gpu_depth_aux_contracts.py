"""The C entry points of csrc/depth_ops.hip and csrc/aux_losses.hip against float64 references written from the comments of
include/e2eslam.h -- called through e2ehip._lib, not through the Python wrappers.

Conventions of every case
  * Reference: a few lines of float64 torch on the CPU.
  * Write coverage: every output is NaN-filled, SENT elements longer than the contract needs (one float4 store) and must come back
    finite over the contract's elements and NaN behind them; workspaces are allocated at exactly their query's size + sentinel.
  * Exact cases: small integers / dyadic fractions whose partial sums stay below 2^24, so that every summation order is exact in
    fp32: equality with the fp64 result rounded to fp32 (one ulp where the kernel ends with a scale or a division).
  * Random cases: U = 2^-24;  element-wise |err| <= (r + 1) U |ref| with r the fp32 roundings of the header's formula (against the
    sum of the magnitudes of the terms where they cancel);  reductions |err| <= (ceil(n / 256) + 16) U sum |term| (+ the terms' own
    roundings).  No bound is fitted to an observed result.
  * Inputs keep 2^-10 away from every kink (asserted on the fp64 side); ties get their own cases with exactly equal values.
  * Refusals raise E2EError and leave the outputs NaN.

Math functions: worst error of torch fp32 on the CPU against fp64, measured over the inputs of the cases that use them, in units of
U relative to the result (1 U is half an ulp at the bottom of a binade, so a correctly rounded function reads up to 1.0 U -- plus the
rounding of the fp32 argument nowhere: both sides take the same fp32 argument).  Each case measures its own figure again and allows
twice that on top of its rounding count.
  expf  over -mean_c |dI| of test_smoothness: (1,1,2,2) 0.42 U, arguments down to -0.44; (2,3,3,5) 0.85 U, -0.67; (1,3,37,53) 0.97 U,
        -0.83; (1,2,5,26219) 1.01 U, -0.97
  logf  over the kept gt and pred of test_depth_metrics, relative to max(|log|, 2^-10): n = 7: 0.85 U (arguments 0.99 .. 5.24);
        n = 65543: 1.01 U (0.45 .. 8.88)
  sqrtf over Adam's second moments after each of the four steps of test_adam_steps: n = 1: 0.55 U; 3: 0.78 U; 4: 0.82 U; 5: 0.86 U;
        1027: 1.03 U; 2097175: 1.07 U (arguments 0 .. 0.49)

entry point                          cases
e2e_median_workspace_bytes           test_median_*
e2e_median_lower                     test_median_sizes, test_median_edges, test_median_nan, test_median_refusals
e2e_depth_scale_workspace_bytes      test_depth_scale_*
e2e_depth_scale_fwd                  test_depth_scale_chain, test_depth_scale_refusals
e2e_depth_scale_bwd                  test_depth_scale_chain, test_depth_scale_bwd_exact
e2e_depth_scale_bwd_at               test_depth_scale_bwd_at, test_depth_scale_bwd_exact, test_depth_scale_refusals
e2e_depth_fixed_scale_fwd / _bwd     test_depth_fixed_scale, test_depth_fixed_scale_refusals
e2e_reduce_workspace_floats          test_mean_diff*, test_depth_metrics*
e2e_mean_diff_fwd / _bwd             test_mean_diff, test_mean_diff_exact, test_mean_diff_refusals
e2e_depth_metrics                    test_depth_metrics, test_depth_metrics_exact_counts, test_depth_metrics_refusals
e2e_adam_step                        test_adam_steps, test_adam_forms_agree, test_adam_refusals
e2e_adam_step_mean                   test_adam_participants, test_adam_forms_agree, test_adam_refusals
e2e_adam_step_resident               test_adam_resident_counter, test_adam_participants, test_adam_forms_agree, test_adam_refusals
e2e_aux_workspace_floats             every aux_losses case
e2e_smoothness_lossgrad              test_smoothness, test_smoothness_exact, test_smoothness_refusals
e2e_geometric_consistency_lossgrad   test_geometric_consistency, test_geometric_gate, test_geometric_refusals
e2e_masked_l1_lossgrad               test_masked_l1, test_masked_l1_exact
e2e_min_reprojection_lossgrad        test_min_reprojection, test_min_reprojection_exact, test_min_reprojection_ties_nan
e2e_disp_blend_fwd / _bwd            test_disp_blend
e2e_masked_mean_lossgrad             test_masked_mean, test_masked_mean_exact
e2e_mask_mul                         test_mask_mul
e2e_channel_mean                     test_channel_mean
e2e_mean_normalize                   test_mean_normalize, test_mean_normalize_exact
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 4
U = 2.0 ** -24
MARGIN = 2.0 ** -10
NAN = float("nan")
f32 = ctypes.c_float


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _out(n, init=None):
    """n floats + NaN sentinel; NaN-filled unless `init` (an accumulate / in-place input) is given"""
    buf = torch.full((n + SENT,), NAN, device=DEV)
    if init is not None:
        buf[:n] = init.flatten().to(DEV)
    return buf


def _written(buf, n, what, nan_ok=False):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    if not nan_ok:
        bad = int((~torch.isfinite(buf[:n])).sum())
        assert bad == 0, f"{what}: {bad} of {n} elements not written (or not finite)"


def _untouched(*bufs):
    for b in bufs:
        assert torch.isnan(b).all(), "a refused call wrote its output"


def _refused(name, *args):
    L = _L()
    with pytest.raises(L.E2EError):
        L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def _f32(ref64):
    """the fp64 result rounded to fp32"""
    return ref64.double().float()


def _ulp_eq(got, ref64, ulps, what):
    """got (fp32, cpu) within `ulps` units in the last place of the fp64 result rounded to fp32"""
    r = _f32(ref64)
    if ulps == 0:
        assert torch.equal(got, r), f"{what}: {got} != {r}"
        return
    spacing = (torch.nextafter(r.abs(), torch.full_like(r, math.inf)) - r.abs()).double()
    d = (got.double() - r.double()).abs()
    assert (d <= ulps * spacing).all(), f"{what}: {got} vs {r} ({(d / spacing).max().item():.1f} ulp)"


def _within(got, ref64, bound64, what):
    """|got - ref| <= bound element-wise (bound computed from the case's own fp64 data)"""
    d = (got.double().cpu() - ref64).abs()
    over = d > bound64
    assert not over.any(), (f"{what}: {int(over.sum())} of {d.numel()} outside the bound; worst err / bound = "
                            f"{(d / bound64.clamp_min(1e-300)).max().item():.2f}, max |err| {d.max().item():.3e}")


def _red_bound(n, mags64):
    """any fixed association of n terms in workgroups of 256"""
    return (math.ceil(n / 256) + 16) * U * mags64.sum()


def _fn_ulps(fn, x32, floor=0.0):
    """worst error of torch's fp32 fn on the CPU against fp64 over x32, relative to max(|fn|, floor), in units of U"""
    ref = fn(x32.double())
    return ((fn(x32).double() - ref).abs() / ref.abs().clamp_min(floor).clamp_min(1e-300)).max().item() / U


def _marks(n, lo, hi, g, mark):
    """small integers in [lo, hi] with distinct larger values at element 0, n - 1, the last n % 4 elements and both sides of the
    256-element boundary: a dropped, doubled or misplaced element at any of them changes an exact sum"""
    x = torch.randint(lo, hi + 1, (n,), generator=g).float()
    pos = [0, n - 1, 255, 256] + [n - 1 - j for j in range(n % 4)]
    for j, p in enumerate(sorted({p for p in pos if 0 <= p < n})):
        x[p] = mark + j
    return x


# =======================================================================================================================================
# depth_ops.hip
# =======================================================================================================================================
MED_BINS = 2048


def _median(x):
    """e2e_median_lower on x (cpu fp32): value (cpu, 1 element), index, count"""
    L = _L()
    nb = L.load().e2e_median_workspace_bytes()
    assert nb == (3 * MED_BINS + 8) * 4
    ws, val = _out(nb // 4), _out(1)
    xd = x.to(DEV)
    L.call("e2e_median_lower", L.ptr(xd), x.numel(), L.ptr(val), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(val, 1, "median", nan_ok=True)
    assert torch.isnan(ws[nb // 4:]).all(), "median workspace: written past its size"
    state = ws[:nb // 4].view(torch.int32)[3 * MED_BINS:3 * MED_BINS + 5].cpu()       # prefix, rank, key, index, count
    return val[:1].cpu(), int(state[3]), int(state[4])


def _median_check(x, what, sign_of_zero=True):
    got, index, count = _median(x)
    ref = torch.median(x)
    if sign_of_zero:
        assert got.view(torch.int32).item() == ref.view(torch.int32).item(), f"{what}: {got.item()!r} != {ref.item()!r}"
        holders = (x.view(torch.int32) == ref.view(torch.int32)).nonzero().flatten()
        assert index == int(holders[0]) and count == holders.numel(), f"{what}: index {index}, count {count}; holders {holders[:4]}..."
    else:
        assert got.item() == ref.item(), f"{what}: {got.item()!r} != {ref.item()!r}"


# 24577 = 96 * 256 + 1: the histogram passes run on at most 96 workgroups (sgrid(n, 96)), so one thread takes a second element
@pytest.mark.parametrize("n", [1, 2, 3, 4, 255, 256, 257, 24577])
def test_median_sizes(n):
    g = torch.Generator().manual_seed(n)
    _median_check(torch.randn(n, generator=g), f"randn n={n}")
    _median_check(torch.randint(1, 8, (n,), generator=g).float() - 4.5, f"heavy ties n={n}")


def test_median_edges():
    g = torch.Generator().manual_seed(3)
    inf = math.inf
    _median_check(torch.full((257,), 1.375), "all equal")
    _median_check(torch.tensor([2.0, 1.0] * 128), "two values, even n: the lower one")
    _median_check(torch.tensor([2.0, 1.0]), "n = 2: the lower one")
    _median_check(-torch.rand(1001, generator=g) - 0.5, "negative values")
    _median_check(torch.tensor([inf, -1.0, -inf, 3.0, inf, -inf, inf]), "infinities, median finite... or not")
    _median_check(torch.tensor([inf, inf, -inf, 3.0, inf]), "median +inf")
    _median_check(torch.tensor([-inf, inf, -inf, 3.0, -inf]), "median -inf")
    # equal in the top 11 bits (sign, exponent, two mantissa bits): pass 1 decides; equal in the top 22: pass 2 decides
    _median_check(1.0 + torch.rand(3001, generator=g) * 0.25, "top 11 bits equal")
    _median_check((0x3F800000 + torch.randint(0, 1024, (3001,), generator=g)).to(torch.int32).view(torch.float32), "top 22 bits equal")
    _median_check(torch.tensor([-0.0, 0.0, -0.0, 0.0, -1.0, 1.0]), "+0.0 and -0.0", sign_of_zero=False)
    _median_check(torch.tensor([0.0, -0.0, 0.0, -0.0, 0.0]), "zeros only", sign_of_zero=False)


def test_median_nan():
    """include/e2eslam.h: NaN inputs order by their bit pattern -- sign clear above +inf, sign set below -inf -- so the result is NaN
    only when the rank falls among them (torch.median returns NaN as soon as one is present)"""
    inf = math.inf
    got, index, count = _median(torch.tensor([1.0, NAN, 3.0, 2.0, inf]))
    assert got.item() == 3.0 and (index, count) == (2, 1)
    x = torch.tensor([1.0, 0.0, 3.0, 2.0, -inf])
    x.view(torch.int32)[1] = 0xFFC00000 - (1 << 32)                       # a NaN with the sign bit set
    got, _, _ = _median(x)
    assert got.item() == 1.0
    got, index, count = _median(torch.tensor([NAN, 1.0, NAN, NAN, 2.0]))
    assert math.isnan(got.item()) and (index, count) == (0, 3)


def test_median_refusals():
    L = _L()
    x, val, ws = torch.ones(8, device=DEV), _out(1), _out(L.load().e2e_median_workspace_bytes() // 4)
    for args in ((None, 8, L.ptr(val), L.ptr(ws)), (L.ptr(x), 0, L.ptr(val), L.ptr(ws)), (L.ptr(x), -1, L.ptr(val), L.ptr(ws)),
                 (L.ptr(x), 0xFFFFFFFF, L.ptr(val), L.ptr(ws)), (L.ptr(x), 8, None, L.ptr(ws)), (L.ptr(x), 8, L.ptr(val), None)):
        _refused("e2e_median_lower", *args)
    _untouched(val, ws)


# ---------------------------------------------------------------------------------------------------------------------------------------
# scale chain.  Launch caps: histogram passes 96 workgroups, scaling pass and backward 1024, dot partials 512: 262151 = 1024 * 256 + 7
# ---------------------------------------------------------------------------------------------------------------------------------------
OVER_1024 = 1024 * 256 + 7


def _tied_disp(n, k, g):
    """n disparities of which exactly k hold the value 0.5, placed so that the lower median of 1 / disp is 2.0"""
    m = n - k
    hi = m // 2                                                # disp > 0.5: the smaller deltas
    d = torch.cat([torch.full((k,), 0.5), 0.55 + 0.25 * torch.rand(hi, generator=g), 0.3 + 0.15 * torch.rand(m - hi, generator=g)])
    return d[torch.randperm(n, generator=g)]


def _scale_ref(disp, mgt, gdep, holders):
    """fp64: delta, median, ratio, depth and g_disp with the median's gradient shared by `holders` (indices)"""
    delta = 1 / disp.double()
    med = delta[holders[0]] if holders.numel() else None
    ratio = mgt / med
    share = torch.zeros_like(delta)
    S = (gdep.double() * delta).sum()
    share.index_add_(0, holders, torch.full((holders.numel(),), float(-(ratio / med) * S / holders.numel()), dtype=torch.float64))
    return delta, med, ratio, ratio * delta, -delta ** 2 * (ratio * gdep.double() + share), share, S


def _scale_bound(n, delta, ratio, med, gdep, share, nh):
    """g_disp = -delta^2 (rho g + share): <= 10 roundings on the two cancelling terms, and the reduction error of S = sum(g delta)
    carried into the share of the nh elements that receive it"""
    s_err = _red_bound(n, (gdep.double() * delta).abs()) + U * (gdep.double() * delta).abs().sum()
    return delta ** 2 * (11 * U * ((ratio * gdep.double()).abs() + share.abs()) + (share != 0) * abs(ratio / med) / nh * s_err)


def _scale_fwd(disp, mgt, with_ratio=True):
    L = _L()
    n = disp.numel()
    nb = L.load().e2e_depth_scale_workspace_bytes()
    ws = _out(nb // 4)
    t = dict(n=n, nb=nb, ws=ws, disp=disp.to(DEV), mgt=torch.tensor([mgt], device=DEV), delta=_out(n), depth=_out(n), med=_out(1),
             ratio=_out(1) if with_ratio else None)
    L.call("e2e_depth_scale_fwd", L.ptr(t["disp"]), L.ptr(t["mgt"]), L.ptr(t["delta"]), L.ptr(t["depth"]), L.ptr(t["med"]), L.ptr(t["ratio"]),
           L.ptr(ws), n, L.stream())
    torch.cuda.synchronize()
    for key in ("delta", "depth"):
        _written(t[key], n, key)
    _written(t["med"], 1, "median_delta")
    if with_ratio:
        _written(t["ratio"], 1, "ratio")
    assert torch.isnan(ws[nb // 4:]).all(), "scale-chain workspace: written past its size"
    return t


def _scale_bwd(t, gdep_d, elements=None):
    L = _L()
    n = t["n"]
    gd = _out(n)
    if elements is None:
        L.call("e2e_depth_scale_bwd", L.ptr(gdep_d), L.ptr(t["delta"]), L.ptr(t["mgt"]), L.ptr(t["med"]), L.ptr(gd), L.ptr(t["ws"]), n, L.stream())
    else:
        el = torch.tensor(elements, dtype=torch.int32, device=DEV)
        L.call("e2e_depth_scale_bwd_at", L.ptr(gdep_d), L.ptr(t["delta"]), L.ptr(t["mgt"]), L.ptr(t["med"]), L.ptr(el), len(elements), L.ptr(gd),
               L.ptr(t["ws"]), n, L.stream())
    torch.cuda.synchronize()
    _written(gd, n, "g_disp")
    assert torch.isnan(t["ws"][t["nb"] // 4:]).all(), "scale-chain workspace: written past its size"
    return gd[:n].cpu()


SCALE = [(1, 1), (5, 1), (5, 2), (5, 3), (1024, 1), (1024, 2), (1024, 64), (OVER_1024, 1), (OVER_1024, 3), (OVER_1024, 64)]


@pytest.mark.parametrize("n,k", SCALE, ids=[f"n{n}-ties{k}" for n, k in SCALE])
def test_depth_scale_chain(n, k):
    g = torch.Generator().manual_seed(n + k)
    disp, mgt = _tied_disp(n, k, g), 1.7
    gdep = torch.randn(n, generator=g)
    d32 = 1 / disp                                                        # correctly rounded on both sides: the kernel's deltas
    holders = (d32 == torch.median(d32)).nonzero().flatten()
    assert holders.numel() == k and torch.median(d32).item() == 2.0
    delta, med, ratio, depth, gref, share, S = _scale_ref(disp, torch.tensor(mgt).double(), gdep, holders)
    t = _scale_fwd(disp, mgt, with_ratio=(k != 2))
    assert torch.equal(t["delta"][:n].cpu(), d32)                         # 1 rounding, both IEEE divisions
    assert t["med"][:1].cpu().item() == 2.0
    state = t["ws"][:t["nb"] // 4].view(torch.int32)[3 * MED_BINS:3 * MED_BINS + 5].cpu()
    assert (int(state[3]), int(state[4])) == (int(holders[0]), k), "the forward's workspace: index and count of the median's holders"
    if k != 2:
        _within(t["ratio"][:1], ratio.reshape(1), 3 * U * ratio.abs().reshape(1), "ratio")       # fp32 m_gt (given), median, division
    _within(t["depth"][:n], depth, 5 * U * depth.abs(), "depth")          # delta 1, ratio 2, product 1
    gdep_d = gdep.to(DEV)
    got = _scale_bwd(t, gdep_d)
    _within(got, gref, _scale_bound(n, delta, ratio, med, gdep, share, k), "g_disp")
    assert torch.equal(_scale_bwd(t, gdep_d), got), "a second backward on the same forward workspace differs"


@pytest.mark.parametrize("n", [5, 1024, OVER_1024])
def test_depth_scale_bwd_at(n):
    g = torch.Generator().manual_seed(n)
    disp, mgt = _tied_disp(n, 1, g), float(torch.tensor(0.9))             # the fp32 scalar the device holds
    gdep = torch.randn(n, generator=g)
    holder = int((disp == 0.5).nonzero()[0])
    other = (holder + 1) % n                                              # does not hold the median
    t = _scale_fwd(disp, mgt)
    gdep_d = gdep.to(DEV)
    named = [[holder], [other, holder]] + ([[int(i) for i in torch.randperm(n, generator=g)[:64]]] if n >= 64 else [[0, 1, 2, 3, 4]])
    for elements in named:
        idx = torch.tensor(elements)
        delta, med, ratio, depth, gref, share, S = _scale_ref(disp, torch.tensor(mgt).double(), gdep, idx)
        med = delta[holder]                                               # the median stays the median, whoever is named
        ratio = mgt / med
        share = torch.zeros_like(delta)
        share[idx] = -(ratio / med) * S / len(elements)
        gref = -delta ** 2 * (ratio * gdep.double() + share)
        _within(_scale_bwd(t, gdep_d, elements), gref, _scale_bound(n, delta, ratio, med, gdep, share, len(elements)), f"g_disp at {len(elements)}")
    # no element named: e2e_depth_scale_bwd
    L = _L()
    gd = _out(n)
    L.call("e2e_depth_scale_bwd_at", L.ptr(gdep_d), L.ptr(t["delta"]), L.ptr(t["mgt"]), L.ptr(t["med"]), None, 0, L.ptr(gd), L.ptr(t["ws"]), n, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(gd[:n].cpu(), _scale_bwd(t, gdep_d))


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [5, 1024, OVER_1024])
def test_depth_scale_bwd_exact(n, k):
    """S = sum(g_depth * delta) in exact arithmetic: disparities that are powers of two (delta in {0.5, 1, 2, 4}), non-zero integer
    gradients with distinct values at the marked places, median_gt = 4 against a median of 2 (rho = 2, rho / median = 1) and 1 or 2
    elements sharing the gradient: every operation of the chain is exact, so g_disp must equal the fp64 result bit for bit at every
    element -- one term of S dropped, doubled or misplaced moves the share by at least 0.25"""
    g = torch.Generator().manual_seed(3 * n + k)
    m = n - k
    hi = m // 2
    disp = torch.cat([torch.full((k,), 0.5), 2.0 ** torch.randint(0, 2, (hi,), generator=g).float(), torch.full((m - hi,), 0.25)])
    disp = disp[torch.randperm(n, generator=g)]
    gdep = _marks(n, 1, 3, g, 5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    d32 = 1 / disp
    holders = (d32 == 2.0).nonzero().flatten()
    assert holders.numel() == k and torch.median(d32).item() == 2.0
    S = (gdep.double() * d32.double()).sum()
    assert (gdep.double() * d32.double()).abs().sum() < 2 ** 24 and abs(S) < 2 ** 21
    delta, med, ratio, depth, gref, share, _ = _scale_ref(disp, torch.tensor(4.0).double(), gdep, holders)
    assert ratio.item() == 2.0 and (share[holders] == -S / k).all()
    t = _scale_fwd(disp, 4.0)
    assert t["ratio"][0].item() == 2.0
    _ulp_eq(t["depth"][:n].cpu(), depth, 0, "exact depth")
    gdep_d = gdep.to(DEV)
    _ulp_eq(_scale_bwd(t, gdep_d), gref, 0, f"exact g_disp (n={n}, {k} holders)")
    other = int((d32 != 2.0).nonzero()[-1])
    for elements in ([int(holders[0])], [other, int(holders[0])]):
        sh = torch.zeros(n, dtype=torch.float64)
        sh[torch.tensor(elements)] = -S / len(elements)
        _ulp_eq(_scale_bwd(t, gdep_d, elements), -delta ** 2 * (2.0 * gdep.double() + sh), 0, f"exact g_disp at {elements}")


def test_depth_scale_refusals():
    L = _L()
    n = 8
    x = torch.ones(n, device=DEV)
    one = torch.ones(1, device=DEV)
    el = torch.zeros(65, dtype=torch.int32, device=DEV)
    ws = _out(L.load().e2e_depth_scale_workspace_bytes() // 4)
    delta, depth, med, gd = _out(n), _out(n), _out(1), _out(n)
    P = L.ptr
    fwd = [P(x), P(one), P(delta), P(depth), P(med), None, P(ws), n]
    for i in (0, 1, 2, 3, 4, 6):
        _refused("e2e_depth_scale_fwd", *[None if j == i else a for j, a in enumerate(fwd)])
    for bad_n in (0, -3, 0xFFFFFFFF):
        _refused("e2e_depth_scale_fwd", *fwd[:7], bad_n)
    bwd = [P(x), P(x), P(one), P(one), P(gd), P(ws), n]
    for i in range(6):
        _refused("e2e_depth_scale_bwd", *[None if j == i else a for j, a in enumerate(bwd)])
    _refused("e2e_depth_scale_bwd", *bwd[:6], 0)
    at = lambda e, ne: [P(x), P(x), P(one), P(one), e, ne, P(gd), P(ws), n]
    _refused("e2e_depth_scale_bwd_at", *at(P(el), 65))
    _refused("e2e_depth_scale_bwd_at", *at(P(el), -1))
    _refused("e2e_depth_scale_bwd_at", *at(None, 1))
    _untouched(ws, delta, depth, med, gd)


@pytest.mark.parametrize("scale", [1.0, 0.37])
@pytest.mark.parametrize("n", [1, 5, OVER_1024])                          # both kernels run on at most 1024 workgroups
def test_depth_fixed_scale(n, scale):
    L = _L()
    g = torch.Generator().manual_seed(n)
    disp = 0.2 + torch.rand(n, generator=g)
    gdep = torch.randn(n, generator=g)
    s64 = float(torch.tensor(scale))                                      # the fp32 scalar the library receives
    delta = 1 / disp.double()
    disp_d, gdep_d = disp.to(DEV), gdep.to(DEV)
    for with_delta in (True, False):
        dl, dp = (_out(n) if with_delta else None), _out(n)
        L.call("e2e_depth_fixed_scale_fwd", L.ptr(disp_d), f32(scale), L.ptr(dl), L.ptr(dp), n, L.stream())
        torch.cuda.synchronize()
        _written(dp, n, "depth")
        _within(dp[:n], delta * s64, 3 * U * (delta * s64).abs(), "depth")                      # 1 / disp, * scale
        if with_delta:
            _written(dl, n, "delta")
            assert torch.equal(dl[:n].cpu(), 1 / disp)
    gd = _out(n)
    L.call("e2e_depth_fixed_scale_bwd", L.ptr(gdep_d), L.ptr(disp_d), f32(scale), L.ptr(gd), n, L.stream())
    torch.cuda.synchronize()
    _written(gd, n, "g_disp")
    ref = -(gdep.double() * s64) / disp.double() ** 2
    _within(gd[:n], ref, 6 * U * ref.abs(), "g_disp")                     # g * scale, the square (or two reciprocal factors), the quotient: <= 5


def test_depth_fixed_scale_refusals():
    L = _L()
    x, a, b = torch.ones(4, device=DEV), _out(4), _out(4)
    P = L.ptr
    _refused("e2e_depth_fixed_scale_fwd", None, f32(1.0), P(a), P(b), 4)
    _refused("e2e_depth_fixed_scale_fwd", P(x), f32(1.0), P(a), None, 4)
    _refused("e2e_depth_fixed_scale_fwd", P(x), f32(1.0), P(a), P(b), 0)
    _refused("e2e_depth_fixed_scale_bwd", None, P(x), f32(1.0), P(a), 4)
    _refused("e2e_depth_fixed_scale_bwd", P(x), None, f32(1.0), P(a), 4)
    _refused("e2e_depth_fixed_scale_bwd", P(x), P(x), f32(1.0), None, 4)
    _refused("e2e_depth_fixed_scale_bwd", P(x), P(x), f32(1.0), P(a), -1)
    _untouched(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------------
# mean |a - b| / mean (a - b)^2.  Forward partials on at most 512 workgroups, backward on 1024.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _mean_diff(a, b, kind, gout):
    L = _L()
    n = a.numel()
    nws = L.load().e2e_reduce_workspace_floats()
    ws, out, gb = _out(nws), _out(1), _out(n)
    ad, bd, gd = a.to(DEV), b.to(DEV), torch.tensor([gout], device=DEV)
    L.call("e2e_mean_diff_fwd", L.ptr(ad), L.ptr(bd), n, kind, L.ptr(out), L.ptr(ws), L.stream())
    L.call("e2e_mean_diff_bwd", L.ptr(ad), L.ptr(bd), L.ptr(gd), n, kind, L.ptr(gb), L.stream())
    torch.cuda.synchronize()
    _written(out, 1, "mean diff")
    _written(gb, n, "g_b")
    assert torch.isnan(ws[nws:]).all(), "reduce workspace: written past its size"
    return out[:1].cpu(), gb[:n].cpu()


def _diff_inputs(n, g):
    """a - b at least 2^-10 from 0, except exact zeros at a few places (their l1 gradient is 0)"""
    b = torch.randn(n, generator=g)
    e = (MARGIN * 2 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    a = b + e
    a[::7] = b[::7]
    e64 = a.double() - b.double()
    assert ((e64.abs() >= MARGIN) | (e64 == 0)).all() and (e64 == 0).any()
    return a, b, e64


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", [1, 257, OVER_1024])
def test_mean_diff(n, kind):
    g = torch.Generator().manual_seed(n)
    a, b, e = _diff_inputs(n, g)
    for gout in (1.0, -2.75):
        out, gb = _mean_diff(a, b, kind, gout)
        terms = e.abs() if kind == 1 else e * e
        # terms: the difference (1) [and its square (1)]; the sum; the final scale and the conversion (2)
        _within(out, (terms.sum() / n).reshape(1), ((_red_bound(n, terms) + (2 + kind) * U * terms.sum()) / n).reshape(1), "mean diff")
        if kind == 1:
            ref = -torch.sign(e) * gout / n
            _within(gb, ref, 2 * U * ref.abs(), "g_b (l1)")                                     # g / n
        else:
            ref = -2 * e * gout / n
            _within(gb, ref, 4 * U * ref.abs(), "g_b (l2)")                                     # g / n, a - b, the product


@pytest.mark.parametrize("kind", [1, 2])
@pytest.mark.parametrize("n", [1, 5, 257, OVER_1024])
def test_mean_diff_exact(n, kind):
    g = torch.Generator().manual_seed(n)
    a = _marks(n, -3, 3, g, 11)
    b = torch.randint(-1, 2, (n,), generator=g).float()
    e = a.double() - b.double()
    terms = e.abs() if kind == 1 else e * e
    assert terms.sum() < 2 ** 24
    out, gb = _mean_diff(a, b, kind, 1.0)
    _ulp_eq(out, (terms.sum() / n).reshape(1), 1, f"exact mean diff n={n}")


def test_mean_diff_refusals():
    L = _L()
    x, out, ws, gb = torch.ones(4, device=DEV), _out(1), _out(L.load().e2e_reduce_workspace_floats()), _out(4)
    P = L.ptr
    for kind in (0, 3, -1):
        _refused("e2e_mean_diff_fwd", P(x), P(x), 4, kind, P(out), P(ws))
        _refused("e2e_mean_diff_bwd", P(x), P(x), P(x), 4, kind, P(gb))
    _refused("e2e_mean_diff_fwd", None, P(x), 4, 1, P(out), P(ws))
    _refused("e2e_mean_diff_fwd", P(x), None, 4, 1, P(out), P(ws))
    _refused("e2e_mean_diff_fwd", P(x), P(x), 0, 1, P(out), P(ws))
    _refused("e2e_mean_diff_fwd", P(x), P(x), 4, 1, None, P(ws))
    _refused("e2e_mean_diff_fwd", P(x), P(x), 4, 1, P(out), None)
    _refused("e2e_mean_diff_bwd", P(x), P(x), None, 4, 1, P(gb))
    _refused("e2e_mean_diff_bwd", P(x), P(x), P(x), 4, 1, None)
    _refused("e2e_mean_diff_bwd", P(x), P(x), P(x), 0, 1, P(gb))
    _untouched(out, ws, gb)


# ---------------------------------------------------------------------------------------------------------------------------------------
# depth metrics: partials on at most 256 workgroups (65543 = 256 * 256 + 7)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _metrics(gt, pred, mask_zero):
    L = _L()
    nws = L.load().e2e_reduce_workspace_floats()
    ws, out = _out(nws), _out(7)
    gd, pd = gt.to(DEV), pred.to(DEV)
    L.call("e2e_depth_metrics", L.ptr(gd), L.ptr(pd), gt.numel(), mask_zero, L.ptr(out), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(out, 7, "out7")
    assert torch.isnan(ws[nws:]).all(), "reduce workspace: written past its size"
    return out[:7].cpu()


def _metrics_inputs(n, g, holes):
    gt = 1 + 3 * torch.rand(n, generator=g)
    ratio = torch.exp((torch.rand(n, generator=g) - 0.5) * 1.6)          # max(gt / pred, pred / gt) up to 2.2: all three thresholds matter
    pred = gt * ratio
    for _ in range(8):                                                    # move the few ratios near a threshold away from it
        th = torch.maximum(gt.double() / pred.double(), pred.double() / gt.double())
        near = sum(((th - t).abs() < 4 * MARGIN) for t in (1.25, 1.25 ** 2, 1.25 ** 3)) > 0
        if not near.any():
            break
        pred[near] = pred[near] * 1.03
    if holes is not None:
        gt[holes] = 0.0
    return gt, pred


@pytest.mark.parametrize("mode", ["all", "holes", "one_kept"])
@pytest.mark.parametrize("n", [7, 256 * 256 + 7])
def test_depth_metrics(n, mode):
    g = torch.Generator().manual_seed(n)
    holes = None if mode == "all" else ((torch.rand(n, generator=g) < 0.3) if mode == "holes" else (torch.arange(n) != n // 2))
    gt, pred = _metrics_inputs(n, g, holes)
    keep = gt != 0
    G, P = gt.double()[keep], pred.double()[keep]
    m = int(keep.sum())
    th = torch.maximum(G / P, P / G)
    for t in (1.25, 1.25 ** 2, 1.25 ** 3):
        assert ((th - t).abs() >= MARGIN).all()
    e, le = G - P, torch.log(G) - torch.log(P)
    # logf: measured here over this case's own arguments, relative to max(|log|, 2^-10); twice that is allowed per logarithm
    lg = 2 * max(_fn_ulps(torch.log, gt[keep], MARGIN), _fn_ulps(torch.log, pred[keep], MARGIN)) * U
    dle = lg * (torch.log(G).abs().clamp_min(MARGIN) + torch.log(P).abs().clamp_min(MARGIN)) + U * le.abs()
    terms = [e.abs() / G, e * e / G, e * e, le * le, (th < 1.25).double(), (th < 1.25 ** 2).double(), (th < 1.25 ** 3).double()]
    # each term's own roundings: e (1) then |e| / g (1); e e (1) / g (1); e e; the logarithms' error into le^2; counts exact
    own = [2 * U * terms[0], 4 * U * terms[1], 3 * U * terms[2], 2 * le.abs() * dle + dle * dle + U * terms[3], 0 * th, 0 * th, 0 * th]
    got = _metrics(gt, pred, 0 if mode == "all" else 1)
    for i, name in enumerate(("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")):
        mean = terms[i].sum() / m
        bound = (_red_bound(m, terms[i]) + own[i].sum()) / m + 2 * U * mean
        if i in (2, 3):                                                   # sqrt of the mean (in double on the device): d sqrt = d / (2 sqrt)
            bound = bound / (2 * torch.sqrt(mean)) + U * torch.sqrt(mean)
            mean = torch.sqrt(mean)
        _within(got[i:i + 1], mean.reshape(1), bound.reshape(1), name)


@pytest.mark.parametrize("mask_zero", [0, 1])
def test_depth_metrics_exact_counts(mask_zero):
    """gt / pred in {1, 1.125, 1.5, 1.75, 2} and their reciprocals -- all dyadic pairs, far from the thresholds: the three counts, the kept
    count and the integer-valued sums of (gt - pred)^2 are exact"""
    n = 256 * 256 + 7
    g = torch.Generator().manual_seed(mask_zero)
    pairs = torch.tensor([[8, 8], [9, 8], [12, 8], [14, 8], [16, 8], [8, 9], [8, 12], [8, 14], [8, 16]]).float()
    pick = torch.randint(0, 9, (n,), generator=g)
    for j, p in enumerate((0, n - 1, n - 2, n - 3, 255, 256)):
        pick[p] = (j % 4) + 1
    gt, pred = pairs[pick, 0].clone(), pairs[pick, 1].clone()
    if mask_zero:
        gt[3::5] = 0.0
        gt[0], gt[n - 1] = 0.0, 0.0
    keep = (gt != 0) if mask_zero else torch.ones(n, dtype=torch.bool)
    G, P = gt.double()[keep], pred.double()[keep]
    th = torch.maximum(G / P, P / G)
    got = _metrics(gt, pred, mask_zero)
    m = int(keep.sum())
    for i, t in ((4, 1.25), (5, 1.25 ** 2), (6, 1.25 ** 3)):
        _ulp_eq(got[i:i + 1], ((th < t).double().sum() / m).reshape(1), 1, f"a{i - 3}")
    _ulp_eq(got[2:3], torch.sqrt(((G - P) ** 2).sum() / m).reshape(1), 1, "rmse")


def test_depth_metrics_refusals():
    L = _L()
    x, out, ws = torch.ones(4, device=DEV), _out(7), _out(L.load().e2e_reduce_workspace_floats())
    P = L.ptr
    _refused("e2e_depth_metrics", None, P(x), 4, 0, P(out), P(ws))
    _refused("e2e_depth_metrics", P(x), None, 4, 0, P(out), P(ws))
    _refused("e2e_depth_metrics", P(x), P(x), 0, 0, P(out), P(ws))
    _refused("e2e_depth_metrics", P(x), P(x), 4, 0, None, P(ws))
    _refused("e2e_depth_metrics", P(x), P(x), 4, 0, P(out), None)
    _untouched(out, ws)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Adam.  One thread per float4 on at most 2048 workgroups: 2048 * 256 * 4 + 20 + 3 elements give a second iteration and a tail of 3.
# ---------------------------------------------------------------------------------------------------------------------------------------
ADAM_OVER = 2048 * 256 * 4 + 20 + 3
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
B1F, B2F, EPSF = (float(torch.tensor(v)) for v in (B1, B2, EPS))          # the fp32 scalars the library receives


def _schedule_row(t):
    """{lr / (1 - beta1^t), sqrt(1 - beta2^t)}: doubles rounded to fp32, from the fp32 betas and lr the entry point receives"""
    lr = float(torch.tensor(LR))
    return float(torch.tensor(lr / (1.0 - B1F ** t))), float(torch.tensor(math.sqrt(1.0 - B2F ** t)))


class _Adam:
    """device state of one flat buffer, every array with its sentinel; `off` floats of misalignment for the refusals"""

    def __init__(self, n, g):
        self.n = n
        self.p0, self.m0, self.v0 = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), 0.01 * torch.rand(n, generator=g)
        self.reset()

    def reset(self):
        self.p, self.m, self.v = _out(self.n, self.p0), _out(self.n, self.m0), _out(self.n, self.v0)

    def check(self):
        for b, w in ((self.p, "params"), (self.m, "exp_avg"), (self.v, "exp_avg_sq")):
            _written(b, self.n, w)

    def state(self):
        return [b[:self.n].cpu() for b in (self.p, self.m, self.v)]


def _adam_call(s, grad_d, form, step, part=None, sched=None, counter=None, sched_len=0):
    L = _L()
    P = L.ptr
    if form == "step":
        L.call("e2e_adam_step", P(s.p), P(grad_d), P(s.m), P(s.v), s.n, f32(LR), f32(B1), f32(B2), f32(EPS), step, L.stream())
    elif form == "mean":
        L.call("e2e_adam_step_mean", P(s.p), P(grad_d), P(part), P(s.m), P(s.v), s.n, f32(LR), f32(B1), f32(B2), f32(EPS), step, L.stream())
    else:
        L.call("e2e_adam_step_resident", P(s.p), P(grad_d), P(part), P(s.m), P(s.v), s.n, f32(B1), f32(B2), f32(EPS), P(sched), sched_len,
               P(counter), L.stream())
    torch.cuda.synchronize()
    s.check()


def _adam_ref(p, m, v, g, t, cnt=1.0, carry=None):
    """one fp64 step from the fp32 state (p, m, v); returns the new fp64 state and element-wise bounds on |device - new| for a device
    whose state before the step lay within `carry` = (ep, em, ev) of (p, m, v) (None: the same state).  First order in U:
    m' = m + (1 - b1)(g - m): g / cnt, the difference, 1 - b1 (fp32), the product, the sum -- on the cancelling |g| + |m|: 6 U; the
         map contracts (b1 < 1), so the carried error enters at most once:  em' = em + 6 U (|g| + |m|)
    v' = b2 v + (1 - b2) g g: all terms positive, <= 8 roundings counting g / cnt twice:  ev' = ev + 9 U v'
    p' = p - step (m' / den), den = sqrt(v') / bc2 + eps: em' / den from the first moment; from the second, ev' through the root
         (ev' / (2 sqrt(v') bc2), relative to den), the root itself (measured over this step's v', twice allowed), the two quotients,
         the sum and the product (5 U) on |m' / den|; the difference (U |p'|); and the carried ep"""
    step_size, bc2 = _schedule_row(t)
    one_b1, one_b2 = float(torch.tensor(1.0) - torch.tensor(B1)), float(torch.tensor(1.0) - torch.tensor(B2))
    zero = torch.zeros(p.numel(), dtype=torch.float64)
    ep, em, ev = carry if carry is not None else (zero, zero, zero)
    p, m, v, g = p.double(), m.double(), v.double(), g.double() / cnt
    m2 = m + one_b1 * (g - m)
    v2 = v * B2F + one_b2 * g * g
    root = torch.sqrt(v2)
    den = root / bc2 + EPSF
    p2 = p - step_size * (m2 / den)
    sq = 2 * _fn_ulps(torch.sqrt, _f32(v2)) * U
    bm = em + 6 * U * (g.abs() + m.abs())
    bv = ev + 9 * U * v2
    through_root = torch.where(v2 > 0, bv / (2 * root.clamp_min(1e-300) * bc2 * den), zero)
    bp = ep + U * p2.abs() + step_size * (bm / den + (m2 / den).abs() * (5 * U + sq + through_root))
    return (p2, m2, v2), (bp, bm, bv)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, ADAM_OVER])
def test_adam_steps(n):
    """four consecutive e2e_adam_step calls against an fp64 Adam that carries its OWN state, rounded to fp32 after every step; the bound
    of step k is the one _adam_ref propagates from the bounds of step k - 1 plus that rounding of the reference (U |state|)"""
    g = torch.Generator().manual_seed(n)
    s = _Adam(n, g)
    zero = n // 2 if n > 1 else None                                      # a zero gradient on zero moments: the parameter must not move
    if zero is not None:
        s.m0[zero], s.v0[zero] = 0.0, 0.0
    s.reset()
    ref, carry = [s.p0, s.m0, s.v0], None
    for t in range(1, 5):
        grad = torch.randn(n, generator=g) * (0.1 + t)
        if zero is not None:
            grad[zero] = 0.0
        new, bounds = _adam_ref(*ref, grad, t, carry=carry)
        _adam_call(s, grad.to(DEV), "step", t)
        for i, (got, what) in enumerate(zip(s.state(), ("params", "exp_avg", "exp_avg_sq"))):
            _within(got, new[i], bounds[i], f"{what} after step {t}")
        ref = [_f32(x) for x in new]
        carry = [b + (x - r.double()).abs() for b, x, r in zip(bounds, new, ref)]
    assert zero is None or s.state()[0][zero] == s.p0[zero]


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, ADAM_OVER])
def test_adam_forms_agree(n):
    """equal inputs: e2e_adam_step, _mean (participants 1) and _resident (counter at the same step) give the same bits"""
    g = torch.Generator().manual_seed(n + 1)
    s = _Adam(n, g)
    grad_d = torch.randn(n, generator=g).to(DEV)
    one = torch.ones(1, device=DEV)
    sched = torch.tensor([v for t in range(1, 6) for v in _schedule_row(t)], device=DEV)
    results = []
    for form in ("step", "mean", "resident", "resident_null"):
        s.reset()
        counter = torch.tensor([3, -77], dtype=torch.int32, device=DEV)
        _adam_call(s, grad_d, form.split("_")[0], 3, part=None if form == "resident_null" else one, sched=sched, counter=counter, sched_len=5)
        results.append(s.state())
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert torch.equal(a, b)


@pytest.mark.parametrize("n", [5, 1027])
def test_adam_participants(n):
    """grad_sums / max(participants, 1): 4 divides, 0 behaves as 1"""
    g = torch.Generator().manual_seed(n + 2)
    s = _Adam(n, g)
    grad = torch.randn(n, generator=g)
    grad_d = grad.to(DEV)
    sched = torch.tensor([v for t in range(1, 3) for v in _schedule_row(t)], device=DEV)
    for form in ("mean", "resident"):
        got = {}
        for cnt in (0.0, 1.0, 4.0):
            s.reset()
            counter = torch.tensor([2, -77], dtype=torch.int32, device=DEV)
            _adam_call(s, grad_d, form, 2, part=torch.tensor([cnt], device=DEV), sched=sched, counter=counter, sched_len=2)
            got[cnt] = s.state()
        for a, b in zip(got[0.0], got[1.0]):
            assert torch.equal(a, b), "participants = 0 must behave as 1"
        new, bounds = _adam_ref(s.p0, s.m0, s.v0, grad, 2, cnt=4.0)
        for i, what in enumerate(("params", "exp_avg", "exp_avg_sq")):
            _within(got[4.0][i], new[i], bounds[i], f"{form}, 4 participants: {what}")


def test_adam_resident_counter():
    """the counter starts at 1 and advances by exactly 1 per call; 0 and schedule_len + 5 use the first and the last row; a schedule that
    is 8- but not 16-byte aligned is accepted"""
    n, slen = 1027, 4
    g = torch.Generator().manual_seed(9)
    s = _Adam(n, g)
    grad_d = torch.randn(n, generator=g).to(DEV)
    rows = torch.tensor([v for t in range(1, slen + 1) for v in _schedule_row(t)])
    base = torch.full((2 + 2 * slen + SENT,), NAN, device=DEV)
    base[2:2 + 2 * slen] = rows.to(DEV)
    sched = base[2:]
    assert sched.data_ptr() % 16 == 8
    counter = torch.tensor([1, -77], dtype=torch.int32, device=DEV)
    for t in range(1, 4):
        expect = _Adam(n, torch.Generator().manual_seed(9))
        expect.p, expect.m, expect.v = (b.clone() for b in (s.p, s.m, s.v))
        _adam_call(expect, grad_d, "step", t)
        _adam_call(s, grad_d, "resident", 0, sched=sched, counter=counter, sched_len=slen)
        assert counter.cpu().tolist() == [t + 1, -77]
        for a, b in zip(s.state(), expect.state()):
            assert torch.equal(a, b), f"resident step {t} differs from e2e_adam_step(step = {t})"
    for start, row in ((0, 1), (-3, 1), (slen + 5, slen)):
        s.reset()
        counter = torch.tensor([start, -77], dtype=torch.int32, device=DEV)
        _adam_call(s, grad_d, "resident", 0, sched=sched, counter=counter, sched_len=slen)
        assert counter.cpu().tolist() == [start + 1, -77]
        got = s.state()
        s.reset()
        _adam_call(s, grad_d, "step", row)
        for a, b in zip(got, s.state()):
            assert torch.equal(a, b), f"counter {start} must use schedule row {row}"
    assert torch.isnan(base[:2]).all() and torch.isnan(base[2 + 2 * slen:]).all()


def test_adam_refusals():
    L = _L()
    P = L.ptr
    n = 8
    bufs = [_out(n + 4) for _ in range(4)]                                # params, grads, exp_avg, exp_avg_sq
    one = torch.ones(1, device=DEV)
    sched = torch.full((8,), NAN, device=DEV)
    counter = torch.tensor([1], dtype=torch.int32, device=DEV)
    ok = [P(b) for b in bufs]

    def forms(p, gr, m, v, nn=n, step=1):
        return (("e2e_adam_step", (p, gr, m, v, nn, f32(LR), f32(B1), f32(B2), f32(EPS), step)),
                ("e2e_adam_step_mean", (p, gr, P(one), m, v, nn, f32(LR), f32(B1), f32(B2), f32(EPS), step)),
                ("e2e_adam_step_resident", (p, gr, P(one), m, v, nn, f32(B1), f32(B2), f32(EPS), P(sched), 4, P(counter))))

    for i in range(4):
        for name, args in forms(*[None if j == i else a for j, a in enumerate(ok)]):
            _refused(name, *args)
        for name, args in forms(*[P(bufs[j][1:]) if j == i else a for j, a in enumerate(ok)]):     # 4 bytes off a 16-byte boundary
            _refused(name, *args)
    for name, args in forms(*ok, nn=0):
        _refused(name, *args)
    for name, args in forms(*ok, step=0)[:2]:
        _refused(name, *args)
    _refused("e2e_adam_step_mean", ok[0], ok[1], None, ok[2], ok[3], n, f32(LR), f32(B1), f32(B2), f32(EPS), 1)
    res = lambda sc, sl, ct: (ok[0], ok[1], None, ok[2], ok[3], n, f32(B1), f32(B2), f32(EPS), sc, sl, ct)
    _refused("e2e_adam_step_resident", *res(None, 4, P(counter)))
    _refused("e2e_adam_step_resident", *res(P(sched), 0, P(counter)))
    _refused("e2e_adam_step_resident", *res(P(sched), 4, None))
    _refused("e2e_adam_step_resident", *res(P(sched[1:]), 3, P(counter)))                       # 4 bytes off an 8-byte boundary
    _untouched(*bufs)
    assert counter.item() == 1


# =======================================================================================================================================
# aux_losses.hip
# =======================================================================================================================================
def _aux_ws():
    n = _L().load().e2e_aux_workspace_floats()
    return _out(n), n


def _nchw_view(t, nhwc):
    """device tensor indexed (B, C, H, W): contiguous, or a permuted view of NHWC memory"""
    return t.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2) if nhwc else t.contiguous().to(DEV)


# ---- smoothness: one pixel per thread on at most 512 workgroups: (1, 2, 5, 26219) has 131095 > 512 * 256 pixels -------------------------
def _smooth_inputs(B, C, H, W, g, flat_image=False, qmax=200):
    """disp with every horizontal and vertical neighbour difference at least 2^-10 from 0"""
    q = torch.randint(2, qmax, (B, 1, H, W), generator=g)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    q = q * 2 + ((yy + xx) % 2)                                           # neighbours differ in parity: never equal
    disp = q.float() * (2.0 ** -8)                                        # differences are multiples of 2^-8
    img = torch.full((B, C, H, W), 0.5) if flat_image else torch.rand(B, C, H, W, generator=g)
    return disp, img


def _smooth_ref(disp, img):
    d = disp.double().requires_grad_(True)
    I = img.double()
    ex, ey = d[:, :, :, :-1] - d[:, :, :, 1:], d[:, :, :-1, :] - d[:, :, 1:, :]
    assert (ex.abs() >= MARGIN).all() and (ey.abs() >= MARGIN).all()
    ax, ay = (I[:, :, :, :-1] - I[:, :, :, 1:]).abs().mean(1, keepdim=True), (I[:, :, :-1, :] - I[:, :, 1:, :]).abs().mean(1, keepdim=True)
    tx, ty = ex.abs() * torch.exp(-ax), ey.abs() * torch.exp(-ay)
    lx, ly = tx.mean(), ty.mean()
    gr, = torch.autograd.grad(lx + ly, d)
    # the magnitudes of the <= 4 cancelling edge weights of each pixel's gradient
    mag = torch.zeros_like(d)
    wx, wy = torch.exp(-ax) / tx.numel(), torch.exp(-ay) / ty.numel()
    mag[:, :, :, :-1] += wx; mag[:, :, :, 1:] += wx; mag[:, :, :-1, :] += wy; mag[:, :, 1:, :] += wy
    return lx.detach(), ly.detach(), gr, tx.detach(), ty.detach(), mag.detach(), ax, ay


def _smooth_run(disp, img_view, B, C, H, W, with_grad=True):
    L = _L()
    ws, nws = _aux_ws()
    loss, gd = _out(2), (_out(B * H * W) if with_grad else None)
    dd = disp.to(DEV)
    L.call("e2e_smoothness_lossgrad", L.ptr(dd), L.ptr(img_view), L.strides4(img_view), B, C, H, W, L.ptr(loss), L.ptr(gd), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(loss, 2, "smoothness terms")
    assert torch.isnan(ws[nws:]).all(), "aux workspace: written past its size"
    if with_grad:
        _written(gd, B * H * W, "g_disp")
    return loss[:2].cpu(), gd[:B * H * W].cpu().reshape(B, 1, H, W) if with_grad else None


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc_view"])
@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 3, 3, 5), (1, 3, 37, 53), (1, 2, 5, 26219)], ids=str)
def test_smoothness(shape, nhwc):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    disp, img = _smooth_inputs(B, C, H, W, g)
    lx, ly, gr, tx, ty, mag, ax, ay = _smooth_ref(disp, img)
    # expf: measured over this case's own arguments; twice that is allowed.  Edge weight: C differences (1 each) summed (C - 1), the
    # mean (1: scaled by 1 / C, a second rounding for 1 / C itself) -- an ABSOLUTE error of the argument <= (2 C + 2) U max|a|, which
    # the exponential turns into the same relative error of the weight
    ex = 2 * max(_fn_ulps(torch.exp, (-ax).float()), _fn_ulps(torch.exp, (-ay).float())) * U
    w_rel = ex + (2 * C + 2) * U * 1.0
    loss, gd = _smooth_run(disp, _nchw_view(img, nhwc), B, C, H, W)
    for i, (ref, terms) in enumerate(((lx, tx), (ly, ty))):
        n = terms.numel()
        # a term: the disparity difference (exact: multiples of 2^-8), the weight, the product (1)
        bound = (_red_bound(B * H * W, terms) + (w_rel + U) * terms.sum()) / n + 2 * U * ref
        _within(loss[i:i + 1], ref.reshape(1), bound.reshape(1), ("x term", "y term")[i])
    # gradient: each of the <= 4 addends is scale (1) * sign * weight (w_rel) and the product (1), then <= 3 additions
    _within(gd, gr, (w_rel + 6 * U) * mag, "g_disp")
    loss2, none = _smooth_run(disp, _nchw_view(img, nhwc), B, C, H, W, with_grad=False)
    assert torch.equal(loss2, loss), "g_disp = NULL changes the loss"


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 3, 3, 5), (1, 3, 37, 53), (1, 2, 5, 26219)], ids=str)
def test_smoothness_exact(shape):
    """a constant image: every edge weight is exp(-0) = 1 and the two terms are exact sums of multiples of 2^-8"""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + 1)
    disp, img = _smooth_inputs(B, C, H, W, g, flat_image=True, qmax=20)
    lx, ly, gr, tx, ty, mag, ax, ay = _smooth_ref(disp, img)
    assert tx.sum() * 256 < 2 ** 24 and ty.sum() * 256 < 2 ** 24
    loss, gd = _smooth_run(disp, _nchw_view(img, False), B, C, H, W)
    _ulp_eq(loss, torch.stack([lx, ly]), 1, "exact smoothness terms")
    _within(gd, gr, 4 * U * mag, "g_disp")                                # the two scales (1 each), <= 3 additions of equal-magnitude terms


def test_smoothness_refusals():
    L = _L()
    P = L.ptr
    x = torch.ones(1, 1, 4, 4, device=DEV)
    ws, _ = _aux_ws()
    loss, gd = _out(2), _out(16)
    st = L.strides4(x)
    for B, C, H, W in ((1, 1, 1, 4), (1, 1, 4, 1), (0, 1, 4, 4), (1, 0, 4, 4)):
        _refused("e2e_smoothness_lossgrad", P(x), P(x), st, B, C, H, W, P(loss), P(gd), P(ws))
    _refused("e2e_smoothness_lossgrad", None, P(x), st, 1, 1, 4, 4, P(loss), P(gd), P(ws))
    _refused("e2e_smoothness_lossgrad", P(x), None, st, 1, 1, 4, 4, P(loss), P(gd), P(ws))
    _refused("e2e_smoothness_lossgrad", P(x), P(x), st, 1, 1, 4, 4, None, P(gd), P(ws))
    _refused("e2e_smoothness_lossgrad", P(x), P(x), st, 1, 1, 4, 4, P(loss), P(gd), None)
    _untouched(ws, loss, gd)


# ---- geometric consistency: partials on at most 512 workgroups, the scaling pass on 2048: 524301 = 2048 * 256 + 13 ----------------------
GEOM_OVER = 2048 * 256 + 13


def _geom_inputs(n, g, dyadic=False):
    """a, b with |a - b| >= 2^-10 and the clamp argument |a - b| / (a + b) at least 2^-10 from 0 and 1; every 11th pair has a negative
    member, which puts the argument above 1 (clamped: zero gradient)"""
    if dyadic:                                                            # a + b = 8: the quotient is a multiple of 2^-3
        a = torch.randint(1, 8, (n,), generator=g).float()
        a[a == 4] = 5.0
        b = 8 - a
    else:
        a = 1 + 3 * torch.rand(n, generator=g)
        b = a * (1 + (0.01 + 0.5 * torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float())
        a[::11], b[::11] = 3.0 + torch.rand(len(a[::11]), generator=g), -1.0 - 0.5 * torch.rand(len(a[::11]), generator=g)
    return a, b


def _geom_ref(a, b, m):
    A, Bb = a.double().requires_grad_(True), b.double().requires_grad_(True)
    M = m.double()
    q = (A - Bb).abs() / (A + Bb)
    assert ((A - Bb).abs() >= MARGIN).all() and (q >= MARGIN).all() and ((q - 1).abs() >= MARGIN).all()
    f = q.clamp(0, 1)
    msum = M.sum()
    gate = bool(msum > 10000)
    loss = (f * M).sum() / msum if gate else torch.zeros((), dtype=torch.float64)
    if gate:
        ga, gb = torch.autograd.grad(loss, (A, Bb))
    else:
        ga, gb = torch.zeros_like(A), torch.zeros_like(A)
    return loss.detach(), msum, gate, ga, gb, (f * M).detach(), q.detach()


def _geom_run(a, b, m, with_grad=True):
    L = _L()
    n = a.numel()
    ws, nws = _aux_ws()
    stats = _out(3)
    ga, gb = (_out(n), _out(n)) if with_grad else (None, None)
    ad, bd, md = a.to(DEV), b.to(DEV), m.to(DEV)
    L.call("e2e_geometric_consistency_lossgrad", L.ptr(ad), L.ptr(bd), L.ptr(md), n, L.ptr(stats), L.ptr(ga), L.ptr(gb), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(stats, 3, "stats")
    assert torch.isnan(ws[nws:]).all(), "aux workspace: written past its size"
    if with_grad:
        _written(ga, n, "g_warped")
        _written(gb, n, "g_interpolated")
        return stats[:3].cpu(), ga[:n].cpu(), gb[:n].cpu()
    return stats[:3].cpu(), None, None


@pytest.mark.parametrize("mask", ["binary", "weights"])
@pytest.mark.parametrize("n", [20011, GEOM_OVER])
def test_geometric_consistency(n, mask):
    g = torch.Generator().manual_seed(n)
    a, b = _geom_inputs(n, g)
    m = (torch.rand(n, generator=g) < 0.8).float() if mask == "binary" else 0.25 + torch.rand(n, generator=g)
    loss, msum, gate, ga, gb, terms, q = _geom_ref(a, b, m)
    assert gate and (q > 1).any()
    stats, gota, gotb = _geom_run(a, b, m)
    # a term: a - b (1), a + b (1), the quotient (1), the product with the mask (1); the mask sum: its own reduction
    num_b = _red_bound(n, terms) + 5 * U * terms.sum()
    den_b = _red_bound(n, m.double())
    _within(stats[0:1], loss.reshape(1), (num_b / msum + loss * den_b / msum + 2 * U * loss).reshape(1), "loss")
    _within(stats[1:2], msum.reshape(1), (den_b + U * msum).reshape(1), "sum(mask)")
    _within(stats[2:3], (1 / msum).reshape(1), ((den_b / msum + 2 * U) / msum).reshape(1), "normaliser")
    # d f / d a = m (sign (a + b) - |a - b|) / (a + b)^2 / sum(m): cancellation between sign * den and |a - b|
    A, Bb, M = a.double(), b.double(), m.double()
    mag = M * ((A + Bb).abs() + (A - Bb).abs()) / (A + Bb) ** 2 / msum
    bound = (9 * U + den_b / msum) * mag                                  # a - b, a + b, their difference, den^2, 1 / den^2 or the quotient,
    _within(gota, ga, bound, "g_warped")                                  # two products, the normaliser (2) -- and the mask sum's error
    _within(gotb, gb, bound, "g_interpolated")
    assert (gota[q > 1] == 0).all() and (gotb[q > 1] == 0).all(), "an element clamped at 1 has no gradient"
    stats2, _, _ = _geom_run(a, b, m, with_grad=False)
    assert torch.equal(stats2, stats), "gradient pointers NULL change the statistics"


@pytest.mark.parametrize("ones", [10000, 10001])
def test_geometric_gate(ones):
    """sum(mask) > 10000 decides on the device: exactly 10000 closes the gate (loss, normaliser and gradients 0), 10001 opens it.  The
    inputs are dyadic (a + b = 8): the loss numerator is an exact sum of multiples of 2^-3"""
    n = 20011
    g = torch.Generator().manual_seed(ones)
    a, b = _geom_inputs(n, g, dyadic=True)
    m = torch.zeros(n)
    m[torch.randperm(n, generator=g)[:ones]] = 1.0
    loss, msum, gate, ga, gb, terms, q = _geom_ref(a, b, m)
    assert int(msum) == ones and gate == (ones > 10000)
    stats, gota, gotb = _geom_run(a, b, m)
    assert stats[1].item() == float(ones)
    if not gate:
        assert stats[0].item() == 0.0 and stats[2].item() == 0.0
        assert (gota == 0).all() and (gotb == 0).all()
    else:
        _ulp_eq(stats[0:1], loss.reshape(1), 1, "exact loss")
        _ulp_eq(stats[2:3], (1 / msum).reshape(1), 1, "normaliser")
        assert (gota[m == 0] == 0).all() and (gota[m == 1] != 0).all()


def test_geometric_refusals():
    L = _L()
    P = L.ptr
    x = torch.ones(4, device=DEV)
    ws, _ = _aux_ws()
    stats, ga, gb = _out(3), _out(4), _out(4)
    _refused("e2e_geometric_consistency_lossgrad", P(x), P(x), P(x), 4, P(stats), P(ga), None, P(ws))
    _refused("e2e_geometric_consistency_lossgrad", P(x), P(x), P(x), 4, P(stats), None, P(gb), P(ws))
    _refused("e2e_geometric_consistency_lossgrad", None, P(x), P(x), 4, P(stats), P(ga), P(gb), P(ws))
    _refused("e2e_geometric_consistency_lossgrad", P(x), None, P(x), 4, P(stats), P(ga), P(gb), P(ws))
    _refused("e2e_geometric_consistency_lossgrad", P(x), P(x), None, 4, P(stats), P(ga), P(gb), P(ws))
    _refused("e2e_geometric_consistency_lossgrad", P(x), P(x), P(x), 0, P(stats), P(ga), P(gb), P(ws))
    _refused("e2e_geometric_consistency_lossgrad", P(x), P(x), P(x), 4, None, P(ga), P(gb), P(ws))
    _refused("e2e_geometric_consistency_lossgrad", P(x), P(x), P(x), 4, P(stats), P(ga), P(gb), None)
    _untouched(ws, stats, ga, gb)


# ---- masked l1: at most 512 workgroups: 131085 = 512 * 256 + 13 -------------------------------------------------------------------------
def _masked_l1_run(p, gt, m, with_grad=True):
    L = _L()
    n = p.numel()
    ws, nws = _aux_ws()
    loss, gp = _out(1), (_out(n) if with_grad else None)
    pd, gd, md = p.to(DEV), gt.to(DEV), m.to(DEV)
    L.call("e2e_masked_l1_lossgrad", L.ptr(pd), L.ptr(gd), L.ptr(md), n, L.ptr(loss), L.ptr(gp), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(loss, 1, "loss")
    assert torch.isnan(ws[nws:]).all(), "aux workspace: written past its size"
    if with_grad:
        _written(gp, n, "g_prediction")
    return loss[:1].cpu(), gp[:n].cpu() if with_grad else None


@pytest.mark.parametrize("mask", ["sparse", "zero"])
@pytest.mark.parametrize("n", [1, 257, 512 * 256 + 13])
def test_masked_l1(n, mask):
    g = torch.Generator().manual_seed(n)
    p = 1 + torch.rand(n, generator=g)
    m = (torch.rand(n, generator=g) < 0.4).float() if mask == "sparse" else torch.zeros(n)
    if mask == "sparse":
        m[0] = 1.0
    e_want = (4 * MARGIN + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    gt = torch.where(m != 0, p * m - e_want, 0.5 + torch.rand(n, generator=g))       # unmasked: e = -gt, away from 0 as well
    e = p.double() * m.double() - gt.double()
    assert (e.abs() >= MARGIN).all()
    ref = e.abs().mean()
    gref = torch.sign(e) * m.double() / n
    loss, gp = _masked_l1_run(p, gt, m)
    _within(loss, ref.reshape(1), ((_red_bound(n, e.abs()) + 3 * U * (p.double() * m.double()).abs().sum() + 3 * U * gt.double().abs().sum()) / n
                                   + 2 * U * ref).reshape(1), "loss")   # p m (1) - gt (1) on the cancelling magnitudes
    _within(gp, gref, 3 * U * gref.abs(), "g_prediction")                 # 1 / n (1), * mask (1)
    if mask == "zero":
        assert (gp == 0).all()
    loss2, _ = _masked_l1_run(p, gt, m, with_grad=False)
    assert torch.equal(loss2, loss)


@pytest.mark.parametrize("n", [1, 5, 257, 512 * 256 + 13])
def test_masked_l1_exact(n):
    g = torch.Generator().manual_seed(n)
    p = _marks(n, 1, 6, g, 17)
    m = torch.randint(0, 2, (n,), generator=g).float()
    m[0], m[n - 1] = 1.0, 1.0
    gt = torch.randint(-3, 0, (n,), generator=g).float()                  # p m - gt >= 1
    e = p.double() * m.double() - gt.double()
    assert e.abs().sum() < 2 ** 24
    loss, gp = _masked_l1_run(p, gt, m)
    _ulp_eq(loss, e.abs().mean().reshape(1), 1, "exact masked l1")
    _ulp_eq(gp, torch.sign(e) * m.double() / n, 1, "g_prediction")


# ---- minimum reprojection: at most 512 workgroups: (2, C, 257, 257) has 132098 pixels, not a multiple of 256 ----------------------------
def _min_reproj_run(err, with_grad=True):
    L = _L()
    B, C, H, W = err.shape
    ws, nws = _aux_ws()
    loss, ge = _out(1), (_out(err.numel()) if with_grad else None)
    ed = err.contiguous().to(DEV)
    L.call("e2e_min_reprojection_lossgrad", L.ptr(ed), B, C, H, W, L.ptr(loss), L.ptr(ge), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(loss, 1, "loss", nan_ok=True)
    assert torch.isnan(ws[nws:]).all(), "aux workspace: written past its size"
    if with_grad:
        _written(ge, err.numel(), "g_errors")
    return loss[:1].cpu(), ge[:err.numel()].cpu().reshape(err.shape) if with_grad else None


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 1, 3, 5), (2, 2, 9, 31), (2, 5, 9, 31), (2, 2, 257, 257)], ids=str)
def test_min_reprojection(shape):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    err = torch.rand(shape, generator=g)
    mn, arg = err.double().min(1)
    n = B * H * W
    gref = torch.zeros(shape, dtype=torch.float64).scatter_(1, arg.unsqueeze(1), 1.0 / n)
    loss, ge = _min_reproj_run(err)
    _within(loss, mn.mean().reshape(1), (_red_bound(n, mn) / n + 2 * U * mn.mean()).reshape(1), "loss")
    _ulp_eq(ge, gref, 0, "g_errors")                                      # 1 / n: one correctly rounded value, or 0
    loss2, _ = _min_reproj_run(err, with_grad=False)
    assert torch.equal(loss2, loss)


@pytest.mark.parametrize("shape", [(1, 1, 1, 5), (2, 5, 7, 37), (2, 2, 257, 257)], ids=str)
def test_min_reprojection_exact(shape):
    """integer minima of at least 1 with distinct values at pixel 0, n - 1, the last n % 4 pixels and both sides of pixel 256; the other
    channels lie 0 .. 2 above the minimum (ties go to the first): an exact sum, under and over the 512-workgroup cap"""
    B, C, H, W = shape
    n = B * H * W
    g = torch.Generator().manual_seed(n + C)
    mn = _marks(n, 1, 6, g, 17).view(B, 1, H, W)
    off = torch.randint(0, 3, shape, generator=g).float()
    off.scatter_(1, torch.randint(0, C, (B, 1, H, W), generator=g), 0.0)
    err = mn + off
    first = (err == mn).float().argmax(1)
    assert torch.equal(err.min(1)[0], mn[:, 0]) and mn.sum() < 2 ** 24
    loss, ge = _min_reproj_run(err)
    _ulp_eq(loss, mn.double().mean().reshape(1), 1, "exact loss")
    _ulp_eq(ge, torch.zeros(shape, dtype=torch.float64).scatter_(1, first.unsqueeze(1), 1.0 / n), 0, "g_errors")


def test_min_reprojection_ties_nan():
    """small integers: the loss is an exact sum; ties go to the FIRST minimal channel; a NaN wins like in torch.min"""
    B, C, H, W = 2, 5, 7, 37
    g = torch.Generator().manual_seed(1)
    err = torch.randint(0, 3, (B, C, H, W), generator=g).float()           # three values over five channels: ties everywhere
    err[0, :, 0, 0] = 2.0
    err[1, :, H - 1, W - 1] = torch.tensor([5.0, 4.0, 4.0, 7.0, 4.0])
    mn, arg = err.min(1)                                                  # torch's CPU argmin of min(dim): the first minimum
    first = (err == mn.unsqueeze(1)).float().argmax(1)
    assert torch.equal(arg, first)
    n = B * H * W
    loss, ge = _min_reproj_run(err)
    _ulp_eq(loss, mn.double().mean().reshape(1), 1, "exact loss")
    _ulp_eq(ge, torch.zeros(err.shape, dtype=torch.float64).scatter_(1, first.unsqueeze(1), 1.0 / n), 0, "g_errors on ties")
    err[0, 2, 3, 4] = NAN
    err[1, 1, 0, 5], err[1, 3, 0, 5] = NAN, NAN
    mn, arg = err.min(1)
    assert math.isnan(mn[0, 3, 4].item()) and arg[0, 3, 4].item() == 2 and arg[1, 0, 5].item() == 1
    loss, ge = _min_reproj_run(err)
    assert math.isnan(loss.item())
    _ulp_eq(ge, torch.zeros(err.shape, dtype=torch.float64).scatter_(1, arg.unsqueeze(1), 1.0 / n), 0, "g_errors with NaN")


# ---- dual-disparity blend ---------------------------------------------------------------------------------------------------------------
def _blend64(d, H, W):
    """the header's formula in fp64: l = 1 - clip(20 (y / (H - 1) - 0.05), 0, 1) per ROW (linspace(0, 1, 1) = 0), r = flip_w(l) = l"""
    left, right = d[0], torch.flip(d[1], [1])
    middle = 0.5 * (left + right)
    t = torch.linspace(0, 1, H, dtype=torch.float64)
    l = (1 - torch.clip(20 * (t - 0.05), 0, 1)).unsqueeze(1).expand(H, W)
    return l * left + l * right + (1 - l - l) * middle, (left.abs() + right.abs() + middle.abs())


# the issue's H x W grid, and 513 x 1025 = 525825 > 2048 * 256 elements: both kernels run on at most 2048 workgroups
@pytest.mark.parametrize("H,W", [(H, W) for H in (1, 2, 21, 40) for W in (1, 7, 64)] + [(513, 1025)])
def test_disp_blend(H, W):
    L = _L()
    g = torch.Generator().manual_seed(100 * H + W)
    d = torch.rand(2, H, W, generator=g) + 0.1
    gout = torch.randn(H, W, generator=g)
    ref, mag = _blend64(d.double(), H, W)
    out, gd = _out(H * W), _out(2 * H * W)
    dd, god = d.to(DEV), gout.to(DEV)
    for args in ((None, H, W, L.ptr(out)), (L.ptr(dd), 0, W, L.ptr(out)), (L.ptr(dd), H, 0, L.ptr(out)), (L.ptr(dd), H, W, None)):
        _refused("e2e_disp_blend_fwd", *args)
    for args in ((None, H, W, L.ptr(gd)), (L.ptr(god), 0, W, L.ptr(gd)), (L.ptr(god), H, 0, L.ptr(gd)), (L.ptr(god), H, W, None)):
        _refused("e2e_disp_blend_bwd", *args)
    _untouched(out, gd)
    L.call("e2e_disp_blend_fwd", L.ptr(dd), H, W, L.ptr(out), L.stream())
    L.call("e2e_disp_blend_bwd", L.ptr(god), H, W, L.ptr(gd), L.stream())
    torch.cuda.synchronize()
    _written(out, H * W, "blend")
    _written(gd, 2 * H * W, "g_disp_pair")
    # The mask is a constant of the row and the same fp32 l multiplies all three terms: l left + l right + (1 - 2 l) middle = middle for
    # ANY l, so the mask's own fp32 error cancels and only the roundings of the evaluation remain -- middle (1), the three products (3),
    # 1 - l - l (2), the two sums (2): 8, on the magnitudes of the three terms (l and |1 - 2 l| are at most 1)
    _within(out[:H * W].reshape(H, W), ref, 9 * U * mag, "blend")
    # adjoint: both halves receive g (l + (1 - 2 l) / 2) = g / 2 for any l: 1 - l - l (2), the sum (1), the product (1), on |g| (l + |1 - 2 l| / 2)
    # <= 1.5 |g|
    D = d.double().requires_grad_(True)
    gref, = torch.autograd.grad(_blend64(D, H, W)[0], D, gout.double())
    got = gd[:2 * H * W].reshape(2, H, W)
    _within(got, gref, 5 * U * 1.5 * torch.stack([gout.double().abs(), torch.flip(gout.double().abs(), [1])]), "g_disp_pair")
    # <g, blend(d)> = <blend_bwd(g), d> in fp64, on the device's own forward and adjoint: the two element-wise bounds, summed
    lhs, rhs = (gout.double() * out[:H * W].reshape(H, W).double().cpu()).sum(), (got.double().cpu() * d.double()).sum()
    assert abs(lhs - rhs) <= (9 * U * (gout.double().abs() * mag).sum() + 5 * U * 1.5 * (gout.double().abs() * (d[0].double() + torch.flip(d[1].double(), [1]))).sum())


# ---- masked mean: partials on at most 512 workgroups, the gradient on 2048 --------------------------------------------------------------
def _masked_mean_run(v, gate, weight, with_grad=True):
    L = _L()
    n = v.numel()
    ws, nws = _aux_ws()
    out3, gv = _out(3), (_out(n) if with_grad else None)
    vd, gd = v.to(DEV), gate.to(DEV)
    L.call("e2e_masked_mean_lossgrad", L.ptr(vd), L.ptr(gd), n, f32(weight), L.ptr(out3), L.ptr(gv), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(out3, 3, "out3", nan_ok=True)
    assert torch.isnan(ws[nws:]).all(), "aux workspace: written past its size"
    if with_grad:
        _written(gv, n, "g_values")
    return out3[:3].cpu(), gv[:n].cpu() if with_grad else None


@pytest.mark.parametrize("weight", [1.0, 0.37])
@pytest.mark.parametrize("n", [1, 257, GEOM_OVER])
def test_masked_mean(n, weight):
    """gate != 0 selects: negative, tiny (1e-30) and subnormal (1e-40) gates count, -0.0 and +0.0 do not"""
    g = torch.Generator().manual_seed(n)
    v = torch.randn(n, generator=g)
    gate = torch.where(torch.rand(n, generator=g) < 0.6, 0.5 + torch.rand(n, generator=g), torch.zeros(n))
    for j, val in enumerate((-2.0, 1e-30, -1e-30, 1e-40, -0.0)):
        if j < n:
            gate[(j * 37) % n] = val
    sel = gate.double() != 0
    if not sel.any():
        gate[0] = -1.0
        sel = gate.double() != 0
    cnt = int(sel.sum())
    w64 = float(torch.tensor(weight))
    ref = v.double()[sel].sum() / cnt
    out3, gv = _masked_mean_run(v, gate, weight)
    _within(out3[0:1], ref.reshape(1), (_red_bound(n, v.double()[sel].abs()) / cnt + 2 * U * ref.abs()).reshape(1), "mean")
    assert out3[1].item() == float(cnt)
    _ulp_eq(out3[2:3], torch.tensor([w64 / cnt], dtype=torch.float64), 1, "weight / count")
    _ulp_eq(gv, sel.double() * (w64 / cnt), 1, "g_values")
    assert (gv[~sel] == 0).all()
    out3b, _ = _masked_mean_run(v, gate, weight, with_grad=False)
    assert torch.equal(out3b, out3)


@pytest.mark.parametrize("n", [1, 5, 257, GEOM_OVER])
def test_masked_mean_exact(n):
    g = torch.Generator().manual_seed(n)
    v = _marks(n, -4, 4, g, 9)
    gate = torch.randint(-1, 2, (n,), generator=g).float()
    gate[0], gate[n - 1] = 1.0, -1.0
    sel = gate != 0
    out3, gv = _masked_mean_run(v, gate, 1.0)
    _ulp_eq(out3[0:1], (v.double()[sel].sum() / int(sel.sum())).reshape(1), 1, "exact mean")
    assert out3[1].item() == float(sel.sum())
    # the empty selection: NaN mean, count 0, normaliser 0 and an all-zero gradient
    out3, gv = _masked_mean_run(v, torch.zeros(n), 2.0)
    assert math.isnan(out3[0].item()) and out3[1].item() == 0.0 and out3[2].item() == 0.0 and (gv == 0).all()
    # a single selected element
    one = torch.zeros(n)
    one[n // 2] = -3.0
    out3, gv = _masked_mean_run(v, one, 2.0)
    assert out3.tolist() == [v[n // 2].item(), 1.0, 2.0] and gv[n // 2].item() == 2.0 and int((gv != 0).sum()) == 1


def test_masked_mean_refusals():
    L = _L()
    P = L.ptr
    x = torch.ones(4, device=DEV)
    ws, _ = _aux_ws()
    out3, gv = _out(3), _out(4)
    _refused("e2e_masked_mean_lossgrad", None, P(x), 4, f32(1.0), P(out3), P(gv), P(ws))
    _refused("e2e_masked_mean_lossgrad", P(x), None, 4, f32(1.0), P(out3), P(gv), P(ws))
    _refused("e2e_masked_mean_lossgrad", P(x), P(x), 0, f32(1.0), P(out3), P(gv), P(ws))
    _refused("e2e_masked_mean_lossgrad", P(x), P(x), 4, f32(1.0), None, P(gv), P(ws))
    _refused("e2e_masked_mean_lossgrad", P(x), P(x), 4, f32(1.0), P(out3), P(gv), None)
    _refused("e2e_masked_l1_lossgrad", None, P(x), P(x), 4, P(out3), P(gv), P(ws))
    _refused("e2e_masked_l1_lossgrad", P(x), None, P(x), 4, P(out3), P(gv), P(ws))
    _refused("e2e_masked_l1_lossgrad", P(x), P(x), None, 4, P(out3), P(gv), P(ws))
    _refused("e2e_masked_l1_lossgrad", P(x), P(x), P(x), 0, P(out3), P(gv), P(ws))
    _refused("e2e_masked_l1_lossgrad", P(x), P(x), P(x), 4, None, P(gv), P(ws))
    _refused("e2e_masked_l1_lossgrad", P(x), P(x), P(x), 4, P(out3), P(gv), None)
    for B, C, H, W in ((0, 1, 2, 2), (1, 0, 2, 2), (1, 1, 0, 2), (1, 1, 2, 0)):
        _refused("e2e_min_reprojection_lossgrad", P(x), B, C, H, W, P(out3), P(gv), P(ws))
    _refused("e2e_min_reprojection_lossgrad", None, 1, 1, 2, 2, P(out3), P(gv), P(ws))
    _refused("e2e_min_reprojection_lossgrad", P(x), 1, 1, 2, 2, None, P(gv), P(ws))
    _refused("e2e_min_reprojection_lossgrad", P(x), 1, 1, 2, 2, P(out3), P(gv), None)
    _untouched(ws, out3, gv)


# ---- image-space helpers: at most 2048 workgroups -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc_view"])
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 1, 1), (2, 3, 295, 297)], ids=str)       # the last: 525690 > 2048 * 256 elements
def test_mask_mul(shape, nhwc):
    L = _L()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, mask = torch.randn(shape, generator=g), torch.rand(B, 1, H, W, generator=g)
    xv, md = _nchw_view(x, nhwc), mask.to(DEV)
    out = _out(x.numel())
    L.call("e2e_mask_mul", L.ptr(xv), L.strides4(xv), L.ptr(md), B, C, H, W, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    _written(out, x.numel(), "out")
    _ulp_eq(out[:x.numel()].cpu().reshape(shape), x.double() * mask.double(), 0, "x * mask")      # one product: correctly rounded
    if not nhwc:
        o2 = _out(x.numel())
        for args in ((None, L.strides4(xv), L.ptr(md), B, C, H, W, L.ptr(o2)), (L.ptr(xv), L.strides4(xv), None, B, C, H, W, L.ptr(o2)),
                     (L.ptr(xv), L.strides4(xv), L.ptr(md), B, C, H, W, None), (L.ptr(xv), L.strides4(xv), L.ptr(md), 0, C, H, W, L.ptr(o2)),
                     (L.ptr(xv), L.strides4(xv), L.ptr(md), B, 0, H, W, L.ptr(o2)), (L.ptr(xv), L.strides4(xv), L.ptr(md), B, C, 0, W, L.ptr(o2)),
                     (L.ptr(xv), L.strides4(xv), L.ptr(md), B, C, H, 0, L.ptr(o2))):
            _refused("e2e_mask_mul", *args)
        _untouched(o2)


@pytest.mark.parametrize("shape", [(2, 1, 3, 5), (2, 2, 3, 5), (3, 5, 7, 9), (1, 2, 1, 2048 * 256 + 5)], ids=str)
def test_channel_mean(shape):
    L = _L()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) % 1000)
    x, gy = torch.randn(shape, generator=g), torch.randn(B, 1, H, W, generator=g)
    xd, gyd = x.to(DEV), gy.to(DEV)
    out, adj = _out(B * H * W), _out(x.numel())
    L.call("e2e_channel_mean", L.ptr(xd), B, C, H, W, 0, L.ptr(out), L.stream())
    L.call("e2e_channel_mean", L.ptr(gyd), B, C, H, W, 1, L.ptr(adj), L.stream())
    torch.cuda.synchronize()
    _written(out, B * H * W, "mean")
    _written(adj, x.numel(), "adjoint")
    got, gadj = out[:B * H * W].cpu().reshape(B, 1, H, W), adj[:x.numel()].cpu().reshape(shape)
    # C - 1 additions, the factor 1 / C (1) and the product (1), on the magnitudes
    _within(got, x.double().mean(1, keepdim=True), (C + 2) * U * x.double().abs().mean(1, keepdim=True), "channel mean")
    ref_adj = (gy.double() / C).expand(shape)
    _within(gadj, ref_adj, 3 * U * ref_adj.abs(), "adjoint")
    # <gy, mean(x)> = <adjoint(gy), x>, in fp64 on the device's own results
    lhs, rhs = (gy.double() * got.double()).sum(), (gadj.double() * x.double()).sum()
    assert abs(lhs - rhs) <= (C + 5) * U * (gy.double().abs() * x.double().abs().mean(1, keepdim=True)).sum()
    if C == 2 and H == 3:                                                 # exact: small integers, C a power of two
        xi = torch.randint(-8, 9, shape, generator=g).float()
        o = _out(B * H * W)
        xid = xi.to(DEV)
        L.call("e2e_channel_mean", L.ptr(xid), B, C, H, W, 0, L.ptr(o), L.stream())
        torch.cuda.synchronize()
        _ulp_eq(o[:B * H * W].cpu().reshape(B, 1, H, W), xi.double().mean(1, keepdim=True), 0, "exact channel mean")
        o2 = _out(4)
        for args in ((None, B, C, H, W, 0, L.ptr(o2)), (L.ptr(xid), B, C, H, W, 0, None), (L.ptr(xid), 0, C, H, W, 0, L.ptr(o2)),
                     (L.ptr(xid), B, 0, H, W, 1, L.ptr(o2)), (L.ptr(xid), B, C, 0, W, 0, L.ptr(o2)), (L.ptr(xid), B, C, H, 0, 1, L.ptr(o2))):
            _refused("e2e_channel_mean", *args)
        _untouched(o2)


def _mean_normalize_run(d, gup, B, H, W):
    L = _L()
    n = B * H * W
    ws, out = _out(B * 130), _out(n)
    dd, gd = d.to(DEV), (gup.to(DEV) if gup is not None else None)
    L.call("e2e_mean_normalize", L.ptr(dd), L.ptr(gd), B, H, W, L.ptr(out), L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    _written(out, n, "out")
    assert torch.isnan(ws[B * 130:]).all(), "workspace: written past B * 130 floats"
    return out[:n].cpu().reshape(B, 1, H, W)


# per image 64 workgroups of 256 threads: 64 * 256 + 5 elements give one thread a second one; the normalising pass runs on at most 2048
# workgroups over all images: 3 x 180229 = 540687 > 2048 * 256 elements
@pytest.mark.parametrize("HW", [(1, 1), (7, 9), (1, 64 * 256 + 5), (1, 11 * 64 * 256 + 5)], ids=str)
@pytest.mark.parametrize("B", [1, 3])
def test_mean_normalize(B, HW):
    H, W = HW
    n = H * W
    g = torch.Generator().manual_seed(B * 1000 + n % 997)
    d, gup = torch.rand(B, 1, H, W, generator=g) + 0.05, torch.randn(B, 1, H, W, generator=g)
    D = d.double().requires_grad_(True)
    den = D.mean((2, 3), keepdim=True) + float(torch.tensor(1e-7))
    ref = D / den
    gref, = torch.autograd.grad(ref, D, gup.double())
    den = den.detach()
    # the mean's error (reduction, / HW, + 1e-7f: 3 roundings) relative to den, then the quotient (1)
    sum_b = torch.stack([_red_bound(n, d.double()[b].abs().flatten()) for b in range(B)]).reshape(B, 1, 1, 1) / n
    rel_den = sum_b / den + 4 * U
    _within(_mean_normalize_run(d, None, B, H, W), ref.detach(), (rel_den + 2 * U) * ref.detach().abs(), "d / (mean + eps)")
    # adjoint g / den - sum(g d) / (HW den^2): cancellation, bounded on the two magnitudes; sum(g d) has its own reduction error
    t1 = gup.double().abs() / den
    sgd = (gup.double() * d.double()).sum((2, 3), keepdim=True)
    sgd_b = torch.stack([_red_bound(n, (gup.double() * d.double())[b].abs().flatten()) + U * (gup.double() * d.double())[b].abs().sum()
                         for b in range(B)]).reshape(B, 1, 1, 1)
    t2 = sgd.abs() / (n * den ** 2)
    bound = (rel_den + 3 * U) * t1 + (2 * rel_den + 6 * U) * t2 + sgd_b / (n * den ** 2)
    _within(_mean_normalize_run(d, gup, B, H, W), gref, bound.expand_as(gref), "adjoint")


def test_mean_normalize_exact():
    """dyadic images whose sum is HW / 4 exactly, marked at the ends and at the 256-element boundary: 1 / (0.25 + 1e-7f) of each"""
    B, H, W = 2, 1, 64 * 256 + 4
    n = H * W
    g = torch.Generator().manual_seed(4)
    d = torch.full((B, 1, H, W), 0.25)
    for b in range(B):
        for p, q in ((0, n - 1), (255, 256), (n - 2, n - 3)):
            d[b, 0, 0, p], d[b, 0, 0, q] = 0.25 + (b + 1) * 0.125, 0.25 - (b + 1) * 0.125
    assert (d.double().sum((2, 3)) == n / 4).all()
    den = torch.tensor(0.25) + torch.tensor(1e-7)                         # fp32, as the device forms it from the exact mean
    got = _mean_normalize_run(d, None, B, H, W)
    _ulp_eq(got, d.double() / den.double(), 0, "exact mean normalise")
    L = _L()
    x, ws, out = torch.ones(4, device=DEV), _out(130), _out(4)
    for args in ((None, None, 1, 2, 2, L.ptr(out), L.ptr(ws)), (L.ptr(x), None, 1, 2, 2, None, L.ptr(ws)), (L.ptr(x), None, 1, 2, 2, L.ptr(out), None),
                 (L.ptr(x), None, 0, 2, 2, L.ptr(out), L.ptr(ws)), (L.ptr(x), None, 1, 0, 2, L.ptr(out), L.ptr(ws)),
                 (L.ptr(x), None, 1, 2, 0, L.ptr(out), L.ptr(ws))):
        _refused("e2e_mean_normalize", *args)
    _untouched(ws, out)
