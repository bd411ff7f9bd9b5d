"""The two entry points of csrc/disp_pyramid.hip, called straight through e2ehip._lib, against the float64 references of
tests/disp_pyramid_ref.py (written from the contract include/e2eslam.h states; tests/test_disp_pyramid_inputs.py qualifies them):

  A. e2e_disp_pyramid_depth_fwd / _bwd on every case of the reference module: factor 2, factor 8 (a wave to a coarse pixel), a ratio
     that is no integer, one coarse pixel (every index clamped), more than one tile with ragged edges, the identity, and one launch
     over four, two and one scale of a 32 x 64 image with the other slots NULL;
  B. where the scale has the full size: bit-equal to e2e_disp_range_depth_fwd / _bwd;
  C. the arguments the header rules out: E2EError, nothing written.

Every output is NaN-filled and followed by a NaN sentinel (the entry points take no workspace); the buffers of absent scales are handed
over as well and must stay untouched.  Each call is made twice and the results compared bit for bit.  The bounds are the derived ones of
the reference module: forward |gpu - r64| <= fwd_ops * 2^-24 * |r64| element by element, backward |gpu - r64| <= bwd_tolerance."""
import pytest
import torch

import disp_pyramid_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
SLOTS = range(4)


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _out(n):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV)


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _untouched(buf, what):
    assert torch.isnan(buf).all(), f"{what}: written although it was refused or not asked for"


def _common(L, c, disps):
    """the arguments both directions share: disp0 .. disp3 (NULL where the case has no such scale) and the sizes"""
    args = dict(B=c["B"], H=c["size"][0], W=c["size"][1], min_depth=c["limits"][0], max_depth=c["limits"][1], scale=c["scale"])
    for k in SLOTS:
        args[f"disp{k}"] = L.ptr(disps.get(k))
        args[f"h{k}"], args[f"w{k}"] = c["scales"].get(k, (0, 0))
    return args


def _run(L, c, disps, g):
    """one forward and one backward call -> (depth (S,B,1,H,W), {slot: g_disp})"""
    S, n = len(disps), len(disps) * c["B"] * c["size"][0] * c["size"][1]
    depth = _out(n)
    gd = {k: _out(disps[k].numel() if k in disps else 16) for k in SLOTS}
    common = _common(L, c, disps)
    L.call("e2e_disp_pyramid_depth_fwd", depth=L.ptr(depth), stream=L.stream(), **common)
    L.call("e2e_disp_pyramid_depth_bwd", g_depth=L.ptr(g), stream=L.stream(), **{f"g_disp{k}": L.ptr(gd[k]) for k in SLOTS}, **common)
    torch.cuda.synchronize()
    _written(depth, n, "depth")
    for k in SLOTS:
        if k in disps:
            _written(gd[k], disps[k].numel(), f"g_disp{k}")
        else:
            _untouched(gd[k], f"g_disp{k} of an absent scale")
    return depth[:n].view(S, c["B"], 1, *c["size"]), {k: gd[k][:disps[k].numel()].view_as(disps[k]) for k in disps}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_pyramid_depth(name):
    L = _L()
    c = R.CASES[name]
    cpu_disps, cpu_g = R.inputs(name)
    disps, g = {k: v.to(DEV) for k, v in cpu_disps.items()}, cpu_g.to(DEV)
    depth, gd = _run(L, c, disps, g)
    depth2, gd2 = _run(L, c, disps, g)
    assert torch.equal(depth, depth2) and all(torch.equal(gd[k], gd2[k]) for k in gd), "two calls differ"
    args = (c["size"], *c["limits"], c["scale"])
    ref, ref_g, gu = R.pyramid_depth(cpu_disps, *args), R.pyramid_depth_bwd(cpu_g, cpu_disps, *args), R.g_u(cpu_g, cpu_disps, *args)
    for s, k in enumerate(sorted(disps)):
        shape = tuple(disps[k].shape[2:])
        ef = ((depth[s].cpu().double() - ref[s]).abs() / (R.fwd_ops(shape, c["size"]) * R.EPS * ref[s].abs())).max()
        eb = ((gd[k].cpu().double() - ref_g[k]).abs() / R.bwd_tolerance(gu[s], shape, c["size"])).max()
        print(f"disp_pyramid {name} scale {k} {shape} -> {c['size']}: fwd {float(ef):.3g} bwd {float(eb):.3g} of their bounds")
        assert ef <= 1 and eb <= 1, (name, k, float(ef), float(eb))
        if shape == tuple(c["size"]):                                          # B: the identity, bit for bit
            n = disps[k].numel()
            d1, g1 = _out(n), _out(n)
            one = dict(disp=L.ptr(disps[k]), min_depth=c["limits"][0], max_depth=c["limits"][1], scale=c["scale"], n=n, stream=L.stream())
            L.call("e2e_disp_range_depth_fwd", depth=L.ptr(d1), **one)
            L.call("e2e_disp_range_depth_bwd", g_depth=L.ptr(g[s].contiguous()), g_disp=L.ptr(g1), **one)
            torch.cuda.synchronize()
            assert torch.equal(depth[s].reshape(-1).view(torch.int32), d1[:n].view(torch.int32)), "identity: depth differs from e2e_disp_range_depth_fwd"
            assert torch.equal(gd[k].reshape(-1).view(torch.int32), g1[:n].view(torch.int32)), "identity: g_disp differs from e2e_disp_range_depth_bwd"


def test_refusals_write_nothing():
    L = _L()
    c = R.CASES["zero_two"]
    cpu_disps, cpu_g = R.inputs("zero_two")
    disps, g = {k: v.to(DEV) for k, v in cpu_disps.items()}, cpu_g.to(DEV)
    ok = _common(L, c, disps)
    n = len(disps) * c["B"] * c["size"][0] * c["size"][1]
    bad = [dict(disp0=None, disp2=None),                                       # no scale present
           dict(h0=33), dict(w2=65), dict(h2=0), dict(w0=-1), dict(B=0), dict(H=0), dict(W=0), dict(H=31), dict(W=63),
           dict(min_depth=0.0), dict(min_depth=-1.0), dict(max_depth=0.1), dict(min_depth=80.0, max_depth=0.1)]
    for change in bad:
        depth = _out(n)
        gd = {k: _out(disps[k].numel() if k in disps else 16) for k in SLOTS}
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_pyramid_depth_fwd", depth=L.ptr(depth), stream=L.stream(), **{**ok, **change})
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_pyramid_depth_bwd", g_depth=L.ptr(g), stream=L.stream(), **{f"g_disp{k}": L.ptr(gd[k]) for k in SLOTS}, **{**ok, **change})
        torch.cuda.synchronize()
        _untouched(depth, f"depth after {change}")
        for k in SLOTS:
            _untouched(gd[k], f"g_disp{k} after {change}")
    with pytest.raises(L.E2EError):                                            # the NULL outputs
        L.call("e2e_disp_pyramid_depth_fwd", depth=None, stream=L.stream(), **ok)
    gd = {k: _out(disps[k].numel() if k in disps else 16) for k in SLOTS}
    with pytest.raises(L.E2EError):
        L.call("e2e_disp_pyramid_depth_bwd", g_depth=None, stream=L.stream(), **{f"g_disp{k}": L.ptr(gd[k]) for k in SLOTS}, **ok)
    with pytest.raises(L.E2EError):                                            # a present scale without its gradient buffer
        L.call("e2e_disp_pyramid_depth_bwd", g_depth=L.ptr(g), stream=L.stream(),
               **{f"g_disp{k}": (None if k == 2 else L.ptr(gd[k])) for k in SLOTS}, **ok)
    torch.cuda.synchronize()
    for k in SLOTS:
        _untouched(gd[k], f"g_disp{k} after a NULL output")
