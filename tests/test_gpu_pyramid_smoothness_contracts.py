"""e2e_disp_pyramid_smoothness_lossgrad and its workspace query (csrc/disp_pyramid_smooth.hip), called straight through e2ehip._lib,
against the float64 reference of tests/pyramid_smoothness_ref.py (F.avg_pool2d + oracle.warp_loss.normalised_smoothness + autograd;
tests/test_pyramid_smoothness_inputs.py qualifies it) under that module's derived bounds:

  A. every case of the reference module with distinct, non-trivial weights per slot: the four scales of a 32 x 64 image in one call, two of
     them with the other slots NULL, more than one tile with ragged edges, 2 x 2 planes with fy != fx, an anisotropic box, the image as an
     NCHW view of NHWC memory;
  B. constant planes: the loss is exactly 0 and every gradient element exactly +-0;
  C. the loss-only call (all g_disp NULL): loss_out has the bits of the call with gradients, no g_disp is touched;
  D. the arguments the header rules out: E2EError, nothing written, and the workspace query answers 0 to the sizes it can judge.

Every output is NaN-filled and followed by a 64-float NaN sentinel, the workspace has exactly the queried size plus a sentinel, the
buffers of absent scales are handed over as well and must stay NaN.  Each call is made twice and the results compared bit for bit."""
import pytest
import torch

import pyramid_smoothness_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
SLOTS = range(R.SLOTS)
REGULAR = [n for n in sorted(R.CASES) if not R.CASES[n].get("flat")]


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


def _image(name, img):
    img = img.to(DEV)
    return img.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if R.CASES[name].get("nhwc") else img


def _sizes(c):
    out = {}
    for k in SLOTS:
        out[f"h{k}"], out[f"w{k}"] = c["scales"].get(k, (0, 0))
    return out


def _args(L, name, disps, img):
    c = R.CASES[name]
    args = dict(B=c["B"], H=c["size"][0], W=c["size"][1], img=L.ptr(img), img_strides=L.strides4(img), stream=L.stream(), **_sizes(c))
    for k in SLOTS:
        args[f"disp{k}"] = L.ptr(disps.get(k))
        args[f"weight{k}"] = R.WEIGHTS[k]
    return args


def _buffers(L, name, disps):
    c = R.CASES[name]
    nws = L.query("e2e_disp_pyramid_smoothness_workspace_floats", B=c["B"], **_sizes(c))
    assert nws > 0
    return _out(5), {k: _out(disps[k].numel() if k in disps else 16) for k in SLOTS}, _out(nws), nws


def _run(L, name, disps, img, with_grad=True):
    """one call -> (loss_out (5,), {slot: g_disp} or None)"""
    loss, gd, ws, nws = _buffers(L, name, disps)
    L.call("e2e_disp_pyramid_smoothness_lossgrad", loss_out=L.ptr(loss), workspace=L.ptr(ws),
           **{f"g_disp{k}": (L.ptr(gd[k]) if with_grad else None) for k in SLOTS}, **_args(L, name, disps, img))
    torch.cuda.synchronize()
    _written(loss, 5, "loss_out")
    assert torch.isnan(ws[nws:]).all(), "workspace: written past its queried size"
    for k in SLOTS:
        if k in disps and with_grad:
            _written(gd[k], disps[k].numel(), f"g_disp{k}")
        else:
            _untouched(gd[k], f"g_disp{k} of an absent scale or of the loss-only call")
    return loss[:5].clone(), ({k: gd[k][:disps[k].numel()].view_as(disps[k]) for k in disps} if with_grad else None)


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", REGULAR)
def test_lossgrad_against_float64(name):
    L = _L()
    c = R.case(name)
    disps, img = {k: v.to(DEV) for k, v in c["disps"].items()}, _image(name, c["img"])
    loss, gd = _run(L, name, disps, img)
    loss2, gd2 = _run(L, name, disps, img)
    assert torch.equal(_bits(loss), _bits(loss2)) and all(torch.equal(_bits(gd[k]), _bits(gd2[k])) for k in gd), "two calls differ"
    for k in SLOTS:
        if k not in disps:
            assert float(loss[k]) == 0, f"loss_out[{k}] of an absent slot"
    got = dict(loss={k: loss[k].cpu() for k in disps}, total=loss[4].cpu(), grad={k: gd[k].cpu() for k in disps})
    worst = R.worst(got, c)
    print(f"disp_pyramid_smoothness {name}: of the bounds: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 1, worst
    only, none = _run(L, name, disps, img, with_grad=False)                   # C: the loss alone
    assert none is None and torch.equal(_bits(only), _bits(loss)), "the loss-only call gives other bits"


def test_constant_planes_are_exact():
    L = _L()
    c = R.case("flat")
    disps, img = {k: v.to(DEV) for k, v in c["disps"].items()}, c["img"].to(DEV)
    loss, gd = _run(L, "flat", disps, img)
    assert torch.equal(loss, torch.zeros(5, device=DEV)), loss
    for k in disps:
        assert torch.equal(gd[k], torch.zeros_like(gd[k])), f"g_disp{k}: not exactly zero on constant planes"


def test_refusals_write_nothing():
    L = _L()
    name = "zero_two"
    c = R.case(name)
    disps, img = {k: v.to(DEV) for k, v in c["disps"].items()}, c["img"].to(DEV)
    ok = _args(L, name, disps, img)
    huge = L.Strides(2 ** 62, 2 ** 62, 2 ** 62, 1)                            # 1 * 2^62 + 2 * 2^62 + 31 * 2^62 does not fit an int64_t
    bad = [dict(img=None), dict(loss_out=None), dict(workspace=None),
           dict(disp0=None, disp2=None),                                       # no scale present
           dict(h0=1), dict(w2=1), dict(h2=0), dict(w0=-1), dict(h0=33), dict(w2=65),
           dict(h0=24), dict(w0=48), dict(h2=5), dict(w2=12),                  # sizes that do not divide 32 x 64
           dict(g_disp2=None), dict(g_disp0=None),                             # some present scales with a gradient buffer, not all
           dict(B=0), dict(H=0), dict(W=0), dict(B=32768),                     # S * B = 65536
           dict(img_strides=huge)]
    for change in bad:
        loss, gd, ws, nws = _buffers(L, name, disps)
        args = {**ok, "loss_out": L.ptr(loss), "workspace": L.ptr(ws), **{f"g_disp{k}": L.ptr(gd[k]) for k in SLOTS}, **change}
        with pytest.raises(L.E2EError):
            L.call("e2e_disp_pyramid_smoothness_lossgrad", **args)
        torch.cuda.synchronize()
        _untouched(loss, f"loss_out after {change}")
        _untouched(ws, f"workspace after {change}")
        for k in SLOTS:
            _untouched(gd[k], f"g_disp{k} after {change}")


def test_workspace_query():
    L = _L()
    q = lambda **kw: L.query("e2e_disp_pyramid_smoothness_workspace_floats", **{**_sizes(R.CASES["zero_two"]), "B": 2, **kw})
    th, tw = R.TILE
    tiles = lambda h, w: -(-h // th) * -(-w // tw)
    assert q() == 2 * 2 * (tiles(32, 64) + tiles(8, 16))                      # two partial sums a tile and plane, nothing per pixel
    for change in (dict(B=0), dict(B=-3), dict(h0=1), dict(w2=1), dict(h2=0), dict(w0=-1), dict(h0=0, w0=0, h2=0, w2=0), dict(B=32768)):
        assert q(**change) == 0, change
