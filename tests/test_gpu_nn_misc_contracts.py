"""The C entry points of csrc/nn_misc.hip against float64 references written from the comments of include/e2eslam.h -- called through
e2ehip._lib, not through the Python wrappers.  Same conventions as tests/test_gpu_depth_aux_contracts.py:

  * float64 torch on the CPU as the reference (F.max_pool2d and its autograd, F.interpolate + torch.cat, the header's formulas);
  * every output NaN-filled (index bytes: 0xFF) with a sentinel of SENT elements behind it, workspaces at exactly their query's size;
  * exact cases on small integers (partial sums below 2^24: any summation order is exact), equality with the fp64 result rounded to fp32;
  * random cases with U = 2^-24: element-wise (r + 1) U on the magnitudes of the terms, reductions (ceil(n / 256) + 16) U sum |term|;
  * refusals raise E2EError and leave the outputs untouched.

sqrtf (e2e_bn_fold): worst error of torch fp32 on the CPU against fp64 over var + eps of test_bn_fold's own channels (arguments in
[1e-5, 1.6]), relative to the result in units of U: C = 1: 0.05 U; C = 64: 0.88 U; C = 257: 0.93 U (correctly rounded: at most 1 U).
Each case measures it again and allows twice that.

entry point                          cases
e2e_maxpool3x3s2_fwd / _bwd          test_maxpool, test_maxpool_over_the_grid_cap, test_maxpool_refusals
e2e_maxpool3x3s2_fwd_idx / _bwd_idx  test_maxpool, test_maxpool_over_the_grid_cap, test_maxpool_refusals
e2e_bn_fold                          test_bn_fold
e2e_affine_fwd                       test_affine_fwd, test_affine_refusals
e2e_affine_bwd_workspace_floats      test_affine_bwd, test_affine_bwd_exact
e2e_affine_bwd                       test_affine_bwd, test_affine_bwd_exact, test_affine_refusals
e2e_upsample2_concat                 test_upsample2_concat
e2e_copy_batch_prepare               test_copy_batched, test_copy_batched_many_items, test_copy_batch_prepare_malformed
e2e_copy_batched                     test_copy_batched, test_copy_batched_many_items
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 4
U = 2.0 ** -24
NAN = float("nan")
f32 = ctypes.c_float


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _out(n, init=None):
    """n floats + NaN sentinel; NaN-filled unless `init` (an accumulate input) is given"""
    buf = torch.full((n + SENT,), NAN, device=DEV)
    if init is not None:
        buf[:n] = init.flatten().to(DEV)
    return buf


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    bad = int((~torch.isfinite(buf[:n])).sum())
    assert bad == 0, f"{what}: {bad} of {n} elements not written (or not finite)"


def _untouched(*bufs):
    for b in bufs:
        assert (torch.isnan(b) if b.is_floating_point() else b == 0xFF).all(), "a refused call wrote its output"


def _refused(name, *args):
    L = _L()
    with pytest.raises(L.E2EError):
        L.call(name, *args, L.stream())
    torch.cuda.synchronize()


def _bits_eq(got, ref64, what):
    """got (fp32) equals the fp64 result rounded to fp32"""
    r = ref64.double().float()
    assert torch.equal(got.cpu(), r), f"{what}: {int((got.cpu() != r).sum())} of {r.numel()} elements differ"


def _within(got, ref64, bound64, what):
    d = (got.double().cpu() - ref64).abs()
    over = d > bound64
    assert not over.any(), (f"{what}: {int(over.sum())} of {d.numel()} outside the bound; worst err / bound = "
                            f"{(d / bound64.clamp_min(1e-300)).max().item():.2f}, max |err| {d.max().item():.3e}")


def _red_bound(n, mags64, dim=0):
    """any fixed association of n terms in groups of 256"""
    return (math.ceil(n / 256) + 16) * U * mags64.sum(dim)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# max-pool 3 x 3 / 2 / pad 1
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pool_ref(x, dy):
    """x (B,H,W,C) fp32 -> fp64 y (NHWC), kh * 3 + kw of ATen's first maximum, d/dx of <dy, y> and the same for |dy| (the magnitudes)"""
    B, H, W, C = x.shape
    X = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    Y, idx = F.max_pool2d(X, 3, 2, 1, return_indices=True)
    Ho, Wo = Y.shape[2:]
    oh, ow = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    pos = (torch.div(idx, W, rounding_mode="floor") - (2 * oh - 1)) * 3 + (idx % W - (2 * ow - 1))
    assert (pos >= 0).all() and (pos <= 8).all()
    DY = dy.double().permute(0, 3, 1, 2)
    dx, = torch.autograd.grad(Y, X, DY, retain_graph=True)
    mag, = torch.autograd.grad(Y, X, DY.abs())
    return _nhwc(Y.detach()), _nhwc(pos).to(torch.uint8), _nhwc(dx), _nhwc(mag)


def _pool_inputs(B, H, W, C, g, ties=True):
    """behind a ReLU: exact zeros and, from a grid of five values, exact ties inside every window -- at zero and at non-zero values"""
    x = torch.randint(-2, 3, (B, H, W, C), generator=g).clamp_min(0).float() * 0.75 if ties else F.relu(torch.randn(B, H, W, C, generator=g))
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return x, torch.randn(B, Ho, Wo, C, generator=g), torch.randn(B, H, W, C, generator=g)


def _pool_fwd(x_d, B, H, W, C, idx_form):
    L = _L()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n = B * Ho * Wo * C
    y = _out(n)
    am = torch.full((n + SENT,), 0xFF, dtype=torch.uint8, device=DEV) if idx_form else None
    if idx_form:
        L.call("e2e_maxpool3x3s2_fwd_idx", L.ptr(x_d), L.ptr(y), L.ptr(am), B, H, W, C, L.stream())
    else:
        L.call("e2e_maxpool3x3s2_fwd", L.ptr(x_d), L.ptr(y), B, H, W, C, L.stream())
    torch.cuda.synchronize()
    _written(y, n, "y")
    if idx_form:
        assert (am[n:] == 0xFF).all(), "argmax: written past the end"
        assert (am[:n] <= 8).all(), "argmax: bytes not written (or out of range)"
    return y[:n].reshape(B, Ho, Wo, C), am


def _pool_bwd(x_d, am, dy_d, dx0, B, H, W, C, acc, relu, x_null=False):
    L = _L()
    n = B * H * W * C
    dx = _out(n, dx0 if acc else None)
    if am is not None:
        L.call("e2e_maxpool3x3s2_bwd_idx", L.ptr(None if x_null else x_d), L.ptr(am), L.ptr(dy_d), L.ptr(dx), B, H, W, C, acc, relu, L.stream())
    else:
        L.call("e2e_maxpool3x3s2_bwd", L.ptr(x_d), L.ptr(dy_d), L.ptr(dx), B, H, W, C, acc, relu, L.stream())
    torch.cuda.synchronize()
    _written(dx, n, "dx")
    return dx[:n].reshape(B, H, W, C)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("HW", [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (4, 5), (7, 9)], ids=str)
def test_maxpool(HW, C, B):
    """every window of (1,1) .. (3,3) hangs over a border; (4,5) and (7,9) add interior windows and, with even H, a last row that only the
    bottom window row reaches"""
    H, W = HW
    g = torch.Generator().manual_seed(100 * H + 10 * W + C + B)
    x, dy, dx0 = _pool_inputs(B, H, W, C, g)
    y_ref, pos_ref, dx_ref, mag = _pool_ref(x, dy)
    x_d, dy_d = x.to(DEV), dy.to(DEV)
    for idx_form in (False, True):
        y, am = _pool_fwd(x_d, B, H, W, C, idx_form)
        _bits_eq(y, y_ref, "y")
        if idx_form:
            assert torch.equal(am[:y.numel()].cpu().reshape(pos_ref.shape), pos_ref), "argmax bytes differ from kh * 3 + kw of ATen's first maximum"
        for acc in (0, 1):
            for relu in (0, 1):
                ref = dx_ref * ((x > 0).double() if relu else 1) + (dx0.double() if acc else 0)
                # <= 4 addends in a fixed order, + the old value: <= 4 roundings on the magnitudes
                bound = 5 * U * (mag + (dx0.double().abs() if acc else 0))
                _within(_pool_bwd(x_d, am, dy_d, dx0, B, H, W, C, acc, relu), ref, bound, f"dx (idx={idx_form}, acc={acc}, relu={relu})")
        if idx_form:
            _within(_pool_bwd(x_d, am, dy_d, dx0, B, H, W, C, 0, 0, x_null=True), dx_ref, 5 * U * mag, "dx (idx form, x = NULL)")


# forward: 4 channels per thread on at most 4096 workgroups; backward: one 2 x 2 input block x 4 channels per thread on at most 8192.
# A single row of 4194311 pixels x 4 channels has 2097156 > 8192 * 256 blocks and as many outputs.
POOL_OVER = (1, 1, 8192 * 256 * 2 + 7, 4)


@functools.lru_cache(maxsize=None)
def _pool_over_case():
    B, H, W, C = POOL_OVER
    g = torch.Generator().manual_seed(5)
    x, dy, dx0 = _pool_inputs(B, H, W, C, g, ties=False)
    return (x, dy) + _pool_ref(x, dy)


@pytest.mark.parametrize("idx_form", [False, True], ids=["rescan", "idx"])
def test_maxpool_over_the_grid_cap(idx_form):
    B, H, W, C = POOL_OVER
    x, dy, y_ref, pos_ref, dx_ref, mag = _pool_over_case()
    x_d, dy_d = x.to(DEV), dy.to(DEV)
    y, am = _pool_fwd(x_d, B, H, W, C, idx_form)
    _bits_eq(y, y_ref, "y")
    if idx_form:
        assert torch.equal(am[:y.numel()].cpu().reshape(pos_ref.shape), pos_ref)
    _within(_pool_bwd(x_d, am, dy_d, None, B, H, W, C, 0, 0), dx_ref, 5 * U * mag, "dx")


def test_maxpool_refusals():
    L = _L()
    P = L.ptr
    x = torch.ones(1, 4, 4, 8, device=DEV)
    y, dx = _out(2 * 2 * 8), _out(4 * 4 * 8)
    am = torch.full((2 * 2 * 8 + SENT,), 0xFF, dtype=torch.uint8, device=DEV)
    dy = torch.ones(1, 2, 2, 8, device=DEV)
    for B, H, W, C in ((1, 4, 4, 6), (1, 4, 4, 2), (1, 4, 4, 0), (0, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8)):
        _refused("e2e_maxpool3x3s2_fwd", P(x), P(y), B, H, W, C)
        _refused("e2e_maxpool3x3s2_fwd_idx", P(x), P(y), P(am), B, H, W, C)
        _refused("e2e_maxpool3x3s2_bwd", P(x), P(dy), P(dx), B, H, W, C, 0, 0)
        _refused("e2e_maxpool3x3s2_bwd_idx", P(x), P(am), P(dy), P(dx), B, H, W, C, 0, 0)
    _refused("e2e_maxpool3x3s2_fwd", None, P(y), 1, 4, 4, 8)
    _refused("e2e_maxpool3x3s2_fwd", P(x), None, 1, 4, 4, 8)
    _refused("e2e_maxpool3x3s2_fwd_idx", None, P(y), P(am), 1, 4, 4, 8)
    _refused("e2e_maxpool3x3s2_fwd_idx", P(x), None, P(am), 1, 4, 4, 8)
    _refused("e2e_maxpool3x3s2_fwd_idx", P(x), P(y), None, 1, 4, 4, 8)
    _refused("e2e_maxpool3x3s2_bwd", None, P(dy), P(dx), 1, 4, 4, 8, 0, 0)
    _refused("e2e_maxpool3x3s2_bwd", P(x), None, P(dx), 1, 4, 4, 8, 0, 0)
    _refused("e2e_maxpool3x3s2_bwd", P(x), P(dy), None, 1, 4, 4, 8, 0, 0)
    _refused("e2e_maxpool3x3s2_bwd_idx", None, P(am), P(dy), P(dx), 1, 4, 4, 8, 0, 1)           # mul_relu reads x
    _refused("e2e_maxpool3x3s2_bwd_idx", P(x), None, P(dy), P(dx), 1, 4, 4, 8, 0, 0)
    _refused("e2e_maxpool3x3s2_bwd_idx", P(x), P(am), None, P(dx), 1, 4, 4, 8, 0, 0)
    _refused("e2e_maxpool3x3s2_bwd_idx", P(x), P(am), P(dy), None, 1, 4, 4, 8, 0, 0)
    _untouched(y, dx, am)


# ---------------------------------------------------------------------------------------------------------------------------------------
# eval-mode BatchNorm with a trainable affine
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rstd", [True, False])
@pytest.mark.parametrize("C", [1, 64, 257])
def test_bn_fold(C, with_rstd):
    L = _L()
    g = torch.Generator().manual_seed(C)
    gamma, beta, mean = torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    var = 0.1 + 1.5 * torch.rand(C, generator=g)
    var[C // 2] = 0.0                                                     # a variance of 0: rstd = 1 / sqrt(eps)
    eps = float(torch.tensor(1e-5))
    dev = [t.to(DEV) for t in (gamma, beta, mean, var)]
    scale, shift, rstd = _out(C), _out(C), (_out(C) if with_rstd else None)
    L.call("e2e_bn_fold", *[L.ptr(t) for t in dev], f32(1e-5), L.ptr(scale), L.ptr(shift), L.ptr(rstd), C, L.stream())
    torch.cuda.synchronize()
    r = 1 / torch.sqrt(var.double() + eps)
    s = gamma.double() * r
    arg = var + torch.tensor(1e-5)
    sq = 2 * ((torch.sqrt(arg).double() - torch.sqrt(arg.double())).abs() / torch.sqrt(arg.double())).max().item()    # measured, twice allowed
    r_rel = 0.5 * U + sq + U                                              # var + eps (half its error survives the root), the root, 1 / x
    _written(scale, C, "scale")
    _written(shift, C, "shift")
    _within(scale[:C], s, (r_rel + 2 * U) * s.abs(), "scale")             # ... and gamma * r
    # shift = beta - mean * scale: bounded on |beta| + |mean scale|
    _within(shift[:C], beta.double() - mean.double() * s, (r_rel + 4 * U) * (mean.double() * s).abs() + 2 * U * beta.double().abs(), "shift")
    if with_rstd:
        _written(rstd, C, "rstd")
        _within(rstd[:C], r, (r_rel + U) * r, "rstd")
    else:
        bad = _out(C)
        for i in range(6):
            args = [L.ptr(t) for t in dev] + [f32(1e-5), L.ptr(bad), L.ptr(bad), None, C]
            args[i if i < 4 else i + 1] = None
            _refused("e2e_bn_fold", *args)
        _refused("e2e_bn_fold", *[L.ptr(t) for t in dev], f32(1e-5), L.ptr(bad), L.ptr(bad), None, 0)
        _untouched(bad)


# at most 4096 workgroups of 256 elements: 3 x 349527 = 1048581 elements give a second iteration
@pytest.mark.parametrize("C,P", [(1, 37), (3, 37), (64, 37), (3, 349527), (1, 4096 * 256 + 5)])
def test_affine_fwd(C, P):
    L = _L()
    n = C * P
    g = torch.Generator().manual_seed(C + P)
    z, res = torch.randn(n, generator=g), torch.randn(n, generator=g)
    scale, shift = torch.randn(C, generator=g), torch.randn(C, generator=g)
    zd, rd, scd, shd = (t.to(DEV) for t in (z, res, scale, shift))
    for has_shift in (0, 1):
        for has_res in (0, 1):
            for relu in (0, 1):
                y = _out(n)
                L.call("e2e_affine_fwd", L.ptr(zd), L.ptr(scd), L.ptr(shd if has_shift else None), L.ptr(rd if has_res else None), relu, L.ptr(y),
                       n, C, L.stream())
                torch.cuda.synchronize()
                _written(y, n, "y")
                t0 = z.double().view(P, C) * scale.double()
                t1 = shift.double().expand(P, C) if has_shift else torch.zeros(P, C, dtype=torch.float64)
                t2 = res.double().view(P, C) if has_res else torch.zeros(P, C, dtype=torch.float64)
                v = t0 + t1 + t2
                # the product, the two sums: 3 roundings on the magnitudes of the cancelling terms; ReLU is a contraction, so the bound
                # holds across its kink
                _within(y[:n].reshape(P, C), F.relu(v) if relu else v, 4 * U * (t0.abs() + t1.abs() + t2.abs()),
                        f"y (shift={has_shift}, residual={has_res}, relu={relu})")


AFF_C = [1, 2, 63, 64, 65, 130]
AFF_P = [1, 3, 4, 5, 191, 193, 256, 1000, 64 * 256 + 7]


def _affine_bwd_run(dy_d, z_d, mean_d, rstd_d, P, C, want, acc, old):
    """want: 'both', 'dgamma' or 'dbeta'; returns (dgamma, dbeta) on the cpu (None where not asked for)"""
    L = _L()
    nws = L.load().e2e_affine_bwd_workspace_floats(C)
    ws = _out(nws)
    dg = _out(C, old[0] if acc else None) if want != "dbeta" else None
    db = _out(C, old[1] if acc else None) if want != "dgamma" else None
    L.call("e2e_affine_bwd", L.ptr(dy_d), L.ptr(z_d), L.ptr(mean_d), L.ptr(rstd_d), P, C, L.ptr(dg), L.ptr(db), acc, L.ptr(ws), L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws:]).all(), "workspace: written past e2e_affine_bwd_workspace_floats(C)"
    for b, w in ((dg, "dgamma"), (db, "dbeta")):
        if b is not None:
            _written(b, C, w)
    return (dg[:C].cpu() if dg is not None else None), (db[:C].cpu() if db is not None else None)


@pytest.mark.parametrize("P", AFF_P)
@pytest.mark.parametrize("C", AFF_C)
def test_affine_bwd(C, P):
    g = torch.Generator().manual_seed(1000 * C + P % 1000)
    dy, z = torch.randn(P, C, generator=g), torch.randn(P, C, generator=g)
    mean, rstd = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    old = (torch.randn(C, generator=g), torch.randn(C, generator=g))
    dy_d, z_d, mean_d, rstd_d = (t.to(DEV) for t in (dy, z, mean, rstd))
    for stats in ((False,) if C == 1 else (True, False)):                 # the single-channel form takes no statistics
        m64, r64 = (mean.double(), rstd.double()) if stats else (torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64))
        tg = dy.double() * (z.double() - m64) * r64
        refs = (tg.sum(0), dy.double().sum(0))
        # a d gamma term: z - mean (1, on |z| + |mean|), * rstd (1), the multiply-add (1)
        own = (3 * U * (dy.double().abs() * (z.double().abs() + m64.abs()) * r64).sum(0), torch.zeros(C, dtype=torch.float64))
        mags = (tg.abs(), dy.double().abs())
        for want, acc in (("both", 0), ("both", 1), ("dgamma", 1), ("dgamma", 0), ("dbeta", 0), ("dbeta", 1)):
            got = _affine_bwd_run(dy_d, z_d, mean_d if stats else None, rstd_d if stats else None, P, C, want, acc, old)
            for i, name in enumerate(("dgamma", "dbeta")):
                if got[i] is None:
                    continue
                ref = refs[i] + (old[i].double() if acc else 0)
                bound = _red_bound(P, mags[i]) + own[i] + (U * (old[i].double().abs() + mags[i].sum(0)) if acc else 0)
                _within(got[i], ref, bound, f"{name} (stats={stats}, {want}, accumulate={acc})")


@pytest.mark.parametrize("P", AFF_P)
def test_affine_bwd_exact(P):
    """small integers, mean an integer and rstd a power of two, distinct values in the first and last pixel, the last P % 4 pixels and on
    both sides of pixel 256: sums below 2^24, exact in every order; accumulation onto integers is exact too"""
    for C in (1, 2, 65):
        g = torch.Generator().manual_seed(P + C)
        dy, z = torch.randint(-3, 4, (P, C), generator=g).float(), torch.randint(-3, 4, (P, C), generator=g).float()
        for j, p in enumerate(sorted({p for p in [0, P - 1, 255, 256] + [P - 1 - k for k in range(P % 4)] if 0 <= p < P})):
            z[p], dy[p] = 5.0 + j, 1.0 + (j % 3)
        stats = C > 1
        mean, rstd = torch.randint(-2, 3, (C,), generator=g).float(), torch.full((C,), 0.5)
        old = (torch.randint(-9, 10, (C,), generator=g).float(), torch.randint(-9, 10, (C,), generator=g).float())
        tg = dy.double() * (z.double() - (mean.double() if stats else 0)) * (0.5 if stats else 1)
        assert tg.abs().sum(0).max() < 2 ** 24
        dev = [t.to(DEV) for t in (dy, z, mean, rstd)]
        for acc in (0, 1):
            dg, db = _affine_bwd_run(dev[0], dev[1], dev[2] if stats else None, dev[3] if stats else None, P, C, "both", acc, old)
            _bits_eq(dg, tg.sum(0) + (old[0].double() if acc else 0), f"exact dgamma (C={C}, accumulate={acc})")
            _bits_eq(db, dy.double().sum(0) + (old[1].double() if acc else 0), f"exact dbeta (C={C}, accumulate={acc})")


def test_affine_refusals():
    L = _L()
    P = L.ptr
    x, c1 = torch.ones(8, device=DEV), torch.ones(1, device=DEV)
    y, dg, db = _out(8), _out(2), _out(2)
    ws = _out(L.load().e2e_affine_bwd_workspace_floats(2))
    _refused("e2e_affine_fwd", None, P(x), None, None, 0, P(y), 8, 2)
    _refused("e2e_affine_fwd", P(x), None, None, None, 0, P(y), 8, 2)
    _refused("e2e_affine_fwd", P(x), P(x), None, None, 0, None, 8, 2)
    _refused("e2e_affine_fwd", P(x), P(x), None, None, 0, P(y), 0, 2)
    _refused("e2e_affine_fwd", P(x), P(x), None, None, 0, P(y), 8, 0)
    _refused("e2e_affine_fwd", P(x), P(x), None, None, 0, P(y), 8, 3)                            # n % C != 0
    _refused("e2e_affine_bwd", None, P(x), None, None, 4, 2, P(dg), P(db), 0, P(ws))
    _refused("e2e_affine_bwd", P(x), None, None, None, 4, 2, P(dg), P(db), 0, P(ws))
    _refused("e2e_affine_bwd", P(x), P(x), None, None, 4, 2, P(dg), P(db), 0, None)
    _refused("e2e_affine_bwd", P(x), P(x), None, None, 0, 2, P(dg), P(db), 0, P(ws))
    _refused("e2e_affine_bwd", P(x), P(x), None, None, 4, 0, P(dg), P(db), 0, P(ws))
    _refused("e2e_affine_bwd", P(x), P(x), None, None, 4, 2, None, None, 0, P(ws))               # neither output
    _refused("e2e_affine_bwd", P(x), P(x), P(c1), None, 8, 1, P(dg), P(db), 0, P(ws))            # statistics with C = 1
    _refused("e2e_affine_bwd", P(x), P(x), None, P(c1), 8, 1, P(dg), P(db), 0, P(ws))
    _untouched(y, dg, db, ws)


# ---------------------------------------------------------------------------------------------------------------------------------------
# nearest x2 upsample + concat: at most 4096 workgroups of 256 elements; (1, 64, 65, 32 + 32) has 1064960 output elements
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,h,w,C1,C2", [(B, h, w, C1, C2) for C1, C2 in ((1, 0), (3, 0), (32, 64), (5, 7)) for h, w in ((1, 1), (3, 5)) for B in (1, 2)]
                         + [(1, 64, 65, 32, 32)])
def test_upsample2_concat(B, h, w, C1, C2):
    L = _L()
    g = torch.Generator().manual_seed(B + h + w + C1 + C2)
    x = torch.randn(B, h, w, C1, generator=g)
    skip = torch.randn(B, 2 * h, 2 * w, C2, generator=g) if C2 else None
    ref = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    if C2:
        ref = torch.cat([ref, skip.permute(0, 3, 1, 2)], 1)
    ref = _nhwc(ref)
    n = ref.numel()
    y = _out(n)
    xd, sd = x.to(DEV), (skip.to(DEV) if C2 else None)
    L.call("e2e_upsample2_concat", L.ptr(xd), L.ptr(sd), L.ptr(y), B, h, w, C1, C2, L.stream())
    torch.cuda.synchronize()
    _written(y, n, "y")
    assert torch.equal(y[:n].cpu().reshape(ref.shape), ref)
    if h == 1 and B == 1:
        bad = _out(n)
        for args in ((None, L.ptr(sd), L.ptr(bad), B, h, w, C1, C2), (L.ptr(xd), L.ptr(sd), None, B, h, w, C1, C2), (L.ptr(xd), L.ptr(sd), L.ptr(bad), 0, h, w, C1, C2),
                     (L.ptr(xd), L.ptr(sd), L.ptr(bad), B, 0, w, C1, C2), (L.ptr(xd), L.ptr(sd), L.ptr(bad), B, h, 0, C1, C2),
                     (L.ptr(xd), L.ptr(sd), L.ptr(bad), B, h, w, 0, C2), (L.ptr(xd), L.ptr(sd), L.ptr(bad), B, h, w, C1, -1),
                     (L.ptr(xd), None, L.ptr(bad), B, h, w, C1, 4)):                            # channels to concatenate, no skip tensor
            _refused("e2e_upsample2_concat", *args)
        _untouched(bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# batched copy: a work item is 16384 bytes of one copy, on at most 8192 workgroups
# ---------------------------------------------------------------------------------------------------------------------------------------
GAP = 8                                                                   # int32 words (32 bytes) of sentinel on either side of a destination


def _copy_run(sizes):
    """one table of copies of `sizes` bytes out of one source arena into one destination arena whose gaps hold sentinels"""
    L = _L()
    words = [s // 4 for s in sizes]
    total_w = sum(words)
    src = torch.arange(1, total_w + 1, dtype=torch.int32, device=DEV)
    dst = torch.full((GAP + sum(wd + GAP for wd in words),), -1, dtype=torch.int32, device=DEV)
    arr = (L.CopyDesc * len(sizes))()
    so, do, spans = 0, GAP, []
    for i, (s, wd) in enumerate(zip(sizes, words)):
        arr[i].src, arr[i].dst, arr[i].bytes, arr[i].first_item = src.data_ptr() + 4 * so, dst.data_ptr() + 4 * do, s, -1
        spans.append((so, do, wd))
        so, do = so + wd, do + wd + GAP
    total = L.load().e2e_copy_batch_prepare(arr, len(sizes))
    assert total == sum(-(-s // 16384) for s in sizes)
    first = 0
    for i, s in enumerate(sizes):
        assert arr[i].first_item == first
        first += -(-s // 16384)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.call("e2e_copy_batched", L.ptr(table), len(sizes), total, L.stream())
    torch.cuda.synchronize()
    keep = torch.ones(dst.numel(), dtype=torch.bool, device=DEV)
    for so, do, wd in spans:
        assert torch.equal(dst[do:do + wd], src[so:so + wd]), f"copy of {wd * 4} bytes differs"
        keep[do:do + wd] = False
    assert (dst[keep] == -1).all(), "written outside a destination"
    return table, total


def test_copy_batched():
    _copy_run([16, 16368, 16384, 16400, 5 * 16384 + 16])
    _copy_run([16400, 16])
    for s in (16, 16384, 5 * 16384 + 16):
        _copy_run([s])                                                    # a table with a single descriptor


def test_copy_batched_many_items():
    """8195 + 1 + 2 items on 8192 workgroups: some take a second item, in another descriptor"""
    table, total = _copy_run([8194 * 16384 + 32, 16, 16400])
    assert total == 8198
    L = _L()
    _refused("e2e_copy_batched", None, 3, total)
    _refused("e2e_copy_batched", L.ptr(table), 0, total)
    _refused("e2e_copy_batched", L.ptr(table), 3, 0)


def test_copy_batch_prepare_malformed():
    """-1 for a NULL pointer, a size that is not a positive multiple of 16, a pointer off a 16-byte boundary -- and for no table at all"""
    L = _L()
    lib = L.load()
    buf = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = buf.data_ptr()
    good = (p, p + 128, 64)
    for bad in ((None, p + 128, 64), (p, None, 64), (p, p + 128, 0), (p, p + 128, -16), (p, p + 128, 24), (p + 4, p + 128, 64), (p, p + 132, 64)):
        for where in (0, 1):
            arr = (L.CopyDesc * 2)()
            for i in range(2):
                arr[i].src, arr[i].dst, arr[i].bytes = bad if i == where else good
            assert lib.e2e_copy_batch_prepare(arr, 2) == -1, (bad, where)
    arr = (L.CopyDesc * 1)()
    arr[0].src, arr[0].dst, arr[0].bytes = good
    assert lib.e2e_copy_batch_prepare(arr, 1) == 1 and arr[0].first_item == 0
    assert lib.e2e_copy_batch_prepare(arr, 0) == -1 and lib.e2e_copy_batch_prepare(None, 1) == -1
