"""The five entry points of csrc/disp_heads.hip, called straight through e2ehip._lib, against the float64 references of
tests/disp_head_ref.py (written from the contracts include/e2eslam.h states; tests/test_disp_head_ref.py qualifies every input used here):

  A. e2e_disp_head_fwd: Cin 16 / 32 / 64 / 128 x six shapes x act 0 / 3 / 4 x bias given / NULL;
  B. e2e_disp_head_workspace_floats + e2e_disp_head_bwd: the same cases x every NULL combination of dx / dw / dbias;
  C. e2e_disp_range_depth_fwd / _bwd;
  D. the arguments the header rules out: E2EError, nothing written.

Every output and the workspace are NaN-filled and followed by a NaN sentinel, the workspace allocated at exactly the size its query
returns: each case also checks that every element meant to be written was written, that nothing past any end was, and that an output
passed as NULL stays untouched.  Every call is made twice and the results compared bit for bit.  Bounds are the project's own: forward
max |gpu - r64| / max |r64| < 2e-5 (conv_fwd_ref.BOUND), gradients < 5e-5 (test_gpu_conv_bwd_contracts.GRAD_BOUND)."""
import itertools

import pytest
import torch

import disp_head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64


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


def _fwd(L, t, bias, act, shape, Cin):
    B, H, W = shape
    y = _out(B * H * W)
    L.call("e2e_disp_head_fwd", x=L.ptr(t["x"]), w=L.ptr(t["w"]), bias=L.ptr(bias), y=L.ptr(y), B=B, H=H, W=W, Cin=Cin, act=act, stream=L.stream())
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("Cin", R.CINS)
def test_head_forward(Cin, shape):
    L = _L()
    B, H, W = shape
    cpu = R.head_inputs(Cin, B, H, W)
    t = {k: v.to(DEV) for k, v in cpu.items()}
    for act in R.ACTS:
        for bias in ("bias", None):
            y = _fwd(L, t, t[bias] if bias else None, act, shape, Cin)
            _written(y, B * H * W, "y")
            assert torch.equal(y[:B * H * W], _fwd(L, t, t[bias] if bias else None, act, shape, Cin)[:B * H * W]), "two calls differ"
            e = R.rel(y[:B * H * W].cpu().view(B, H, W), R.head_fwd(cpu["x"], cpu["w"], cpu[bias] if bias else None, act))
            print(f"disp_head_fwd Cin={Cin} {shape} act={act} bias={bias}: {e:.3g}")
            assert e < R.BOUND


def _bwd(L, t, y, act, shape, Cin, want):
    B, H, W = shape
    n = {"dx": B * H * W * Cin, "dw": 9 * Cin, "dbias": 1}
    nws = L.query("e2e_disp_head_workspace_floats", B=B, H=H, W=W, Cin=Cin)
    bufs = {k: _out(n[k]) for k in n}
    ws = _out(nws)
    L.call("e2e_disp_head_bwd", dy=L.ptr(t["dy"]), y=L.ptr(y), x=L.ptr(t["x"]), w=L.ptr(t["w"]), workspace=L.ptr(ws), B=B, H=H, W=W, Cin=Cin, act=act,
           stream=L.stream(), **{k: (L.ptr(bufs[k]) if k in want else None) for k in n})
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws:]).all(), "workspace: written past the size its query returned"
    for k in n:
        if k in want:
            _written(bufs[k], n[k], k)
        else:
            _untouched(bufs[k], k)
    return {k: bufs[k][:n[k]] for k in want}


@pytest.mark.parametrize("shape", R.SHAPES)
@pytest.mark.parametrize("Cin", R.CINS)
def test_head_backward(Cin, shape):
    L = _L()
    B, H, W = shape
    cpu = R.head_inputs(Cin, B, H, W)
    t = {k: v.to(DEV) for k, v in cpu.items()}
    nws = L.query("e2e_disp_head_workspace_floats", B=B, H=H, W=W, Cin=Cin)
    assert 0 < nws <= 2048 * (9 * Cin + 1) and nws % (9 * Cin + 1) == 0 and nws // (9 * Cin + 1) <= B * H * W
    views = {"dx": (B, H, W, Cin), "dw": (1, Cin, 3, 3), "dbias": (1,)}
    for act in R.ACTS:
        y32 = R.head_fwd(cpu["x"], cpu["w"], cpu["bias"], act).float()                   # the saved output the contract takes
        ref = dict(zip(("dx", "dw", "dbias"), R.head_bwd(cpu["dy"], y32, cpu["x"], cpu["w"], act)))
        y = y32.to(DEV)
        for r in range(4):
            for want in itertools.combinations(("dx", "dw", "dbias"), r):
                got = _bwd(L, t, y, act, shape, Cin, want)
                again = _bwd(L, t, y, act, shape, Cin, want)
                for k in want:
                    assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
                    e = R.rel(got[k].cpu().view(views[k]), ref[k])
                    if len(want) in (1, 3):
                        print(f"disp_head_bwd Cin={Cin} {shape} act={act} {'+'.join(want)} {k}: {e:.3g}")
                    assert e < R.GRAD_BOUND, (k, want, act, e)


@pytest.mark.parametrize("n,limits,scale", R.RANGE_CASES)
def test_range_depth(n, limits, scale):
    L = _L()
    cpu = R.range_inputs(n, limits, scale)
    t = {k: v.to(DEV) for k, v in cpu.items()}

    def run():
        depth, gd = _out(n), _out(n)
        L.call("e2e_disp_range_depth_fwd", disp=L.ptr(t["disp"]), min_depth=limits[0], max_depth=limits[1], scale=scale, depth=L.ptr(depth), n=n,
               stream=L.stream())
        L.call("e2e_disp_range_depth_bwd", g_depth=L.ptr(t["g"]), disp=L.ptr(t["disp"]), min_depth=limits[0], max_depth=limits[1], scale=scale,
               g_disp=L.ptr(gd), n=n, stream=L.stream())
        torch.cuda.synchronize()
        _written(depth, n, "depth")
        _written(gd, n, "g_disp")
        return depth[:n], gd[:n]
    (d, g), (d2, g2) = run(), run()
    assert torch.equal(d, d2) and torch.equal(g, g2), "two calls differ"
    ef, eb = R.rel(d.cpu(), R.range_depth(cpu["disp"], *limits, scale)), R.rel(g.cpu(), R.range_depth_bwd(cpu["g"], cpu["disp"], *limits, scale))
    print(f"disp_range_depth n={n} {limits} scale={scale}: fwd {ef:.3g} bwd {eb:.3g}")
    assert ef < R.BOUND and eb < R.GRAD_BOUND


def test_refusals_write_nothing():
    L = _L()
    B, H, W, Cin = 1, 4, 5, 16
    x, w, bias = torch.randn(B, H, W, 128, device=DEV), torch.randn(1, 128, 3, 3, device=DEV), torch.randn(1, device=DEV)
    dy, yv = torch.randn(B, H, W, device=DEV), torch.rand(B, H, W, device=DEV)
    ok_f = dict(x=L.ptr(x), w=L.ptr(w), bias=L.ptr(bias), B=B, H=H, W=W, Cin=Cin, act=4)
    bad = [dict(Cin=8), dict(Cin=48), dict(act=1), dict(act=2), dict(H=1), dict(W=1), dict(B=0), dict(x=None), dict(w=None)]
    for change in bad:
        y = _out(B * H * W)
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_head_fwd", y=L.ptr(y), stream=L.stream(), **{**ok_f, **change})
        torch.cuda.synchronize()
        _untouched(y, f"y after {change}")
    with pytest.raises(L.E2EError):
        L.call("e2e_disp_head_fwd", y=None, stream=L.stream(), **ok_f)
    ok_b = dict(dy=L.ptr(dy), y=L.ptr(yv), x=L.ptr(x), w=L.ptr(w), B=B, H=H, W=W, Cin=Cin, act=4)
    nws = L.query("e2e_disp_head_workspace_floats", B=B, H=H, W=W, Cin=Cin)
    for change in bad + [dict(dy=None), dict(y=None), dict(workspace=None)]:
        dx, dw, db, ws = _out(B * H * W * 128), _out(9 * 128), _out(1), _out(nws)
        args = {**ok_b, "workspace": L.ptr(ws), **change}
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_head_bwd", dx=L.ptr(dx), dw=L.ptr(dw), dbias=L.ptr(db), stream=L.stream(), **args)
        torch.cuda.synchronize()
        for name, b in (("dx", dx), ("dw", dw), ("dbias", db), ("workspace", ws)):
            _untouched(b, f"{name} after {change}")
    assert L.query("e2e_disp_head_workspace_floats", B=B, H=H, W=W, Cin=48) == 0
    disp, g = torch.rand(63, device=DEV), torch.randn(63, device=DEV)
    for change in (dict(disp=None), dict(n=0), dict(min_depth=0.0), dict(min_depth=80.0, max_depth=0.1)):
        out = _out(63)
        args = {**dict(disp=L.ptr(disp), min_depth=0.1, max_depth=80.0, scale=1.0, n=63), **change}
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_range_depth_fwd", depth=L.ptr(out), stream=L.stream(), **args)
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_range_depth_bwd", g_depth=L.ptr(g), g_disp=L.ptr(out), stream=L.stream(), **args)
        torch.cuda.synchronize()
        _untouched(out, f"range depth after {change}")
