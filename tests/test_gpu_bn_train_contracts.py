"""The three entry points of csrc/bn_train.hip, called straight through e2ehip._lib, against the float64 reference of
tests/bn_train_ref.py (tests/test_bn_train_ref.py holds that reference to torch.nn.BatchNorm2d in float64 and qualifies the inputs):

  A. e2e_bn_train_fwd on the nine cases x gamma positive / mixed signs x momentum 0.1 / -1 (two successive calls, counter from 0 and 7),
     and its NULL forms (no running buffers, no gamma / beta);
  B. e2e_bn_train_workspace_floats + e2e_bn_train_bwd on the same cases, fed with the DEVICE forward's y, save_mean and save_rstd:
     everything at once, dz only, the sums only, accumulate = 1 onto non-zero buffers, gamma NULL, y NULL;
  C. forward + backward recorded into one torch.cuda.graph on a side stream and replayed twice with momentum = -1;
  D. the arguments the header rules out: E2EError, nothing written.

Every output and the workspace are NaN-filled and followed by a NaN guard band, the workspace allocated at exactly the size its query
returns; every call is made twice and the results compared bit for bit.

Bounds (the project's own for this kind of kernel): forward, save_mean, save_rstd, running buffers max |gpu - r64| < 2e-5 of that
output's maximum; gradients 5e-5 -- dz element (p, c) against |gamma_c| rstd_c max |g| (in case (a) dz is the difference of nearly equal
terms), dgamma / dbeta against the reference's maximum over channels, widened by exactly what the undecidable ReLU elements of that
channel could contribute; undecidable elements are left out of the dz / dresidual comparison and no other element is exempt.  Each
case prints its worst error per output next to the error of torch's own fp32 CPU evaluation under the same measure."""
import functools

import numpy as np
import pytest
import torch

import bn_train_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
NAMES = sorted(R.CASES)


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _out(n):
    return torch.full((n + GUARD,), float("nan"), device=DEV)


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _untouched(buf, what):
    assert torch.isnan(buf).all(), f"{what}: written although it was refused or not asked for"


def _dims(name):
    (B, H, W, C), relu, has_res, _ = R.CASES[name]
    return B * H * W, C, relu, has_res


@functools.lru_cache(maxsize=None)
def _dev(name):
    return {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in R.inputs(name).items()}


@functools.lru_cache(maxsize=None)
def _ref_fwd(name, gamma_key, affine=True):
    P, C, relu, has_res = _dims(name)
    t = R.inputs(name)
    return R.fwd(t["z"], t[gamma_key] if affine else None, t["beta"] if affine else None, t["residual"] if has_res else None, relu, R.EPS, 0.1,
                 None, None, None)


def _guarded(values):
    """values (C,) followed by a NaN guard band"""
    buf = _out(values.numel())
    buf[:values.numel()] = values
    return buf


def _fwd(L, name, gamma_key="gamma", momentum=0.1, state=None, affine=True):
    """One call.  state: None (no running buffers) or (running_mean, running_var, counter) device buffers that the call updates."""
    P, C, relu, has_res = _dims(name)
    t = _dev(name)
    nws = L.query("e2e_bn_train_workspace_floats", P=P, C=C)
    y, mean, rstd, ws = _out(P * C), _out(C), _out(C), _out(nws)
    rm, rv, nbt = state if state is not None else (None, None, None)
    L.call("e2e_bn_train_fwd", z=L.ptr(t["z"]), gamma=L.ptr(t[gamma_key]) if affine else None, beta=L.ptr(t["beta"]) if affine else None,
           residual=L.ptr(t["residual"]) if has_res else None, relu=int(relu), eps=R.EPS, momentum=momentum, running_mean=L.ptr(rm),
           running_var=L.ptr(rv), num_batches_tracked=L.ptr(nbt), y=L.ptr(y), save_mean=L.ptr(mean), save_rstd=L.ptr(rstd), P=P, C=C,
           workspace=L.ptr(ws), stream=L.stream())
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws:]).all(), "workspace: written past the size its query returned"
    _written(y, P * C, "y")
    _written(mean, C, "save_mean")
    _written(rstd, C, "save_rstd")
    return {"y": y[:P * C].view(P, C), "save_mean": mean[:C], "save_rstd": rstd[:C]}


def _state(name, nbt0):
    t = _dev(name)
    return _guarded(t["running_mean"]), _guarded(t["running_var"]), torch.tensor([nbt0, -77, -77], dtype=torch.int64, device=DEV)


@functools.lru_cache(maxsize=None)
def _torch_fp32(name, gamma_key):
    """torch's own fp32 evaluation on the CPU (forward, running buffers from count 7 at momentum 0.1, gradients)."""
    (B, H, W, C), relu, has_res, _ = R.CASES[name]
    t = R.inputs(name)
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=0.1).train()
    with torch.no_grad():
        for dst, k in ((bn.weight, gamma_key), (bn.bias, "beta"), (bn.running_mean, "running_mean"), (bn.running_var, "running_var")):
            dst.copy_(torch.from_numpy(np.array(t[k])))
    nchw = lambda a: torch.from_numpy(np.array(a)).view(B, H, W, C).permute(0, 3, 1, 2)
    z = nchw(t["z"]).clone().requires_grad_(True)
    res = nchw(t["residual"]).clone().requires_grad_(True) if has_res else None
    y = bn(z)
    y = y + res if has_res else y
    y = torch.relu(y) if relu else y
    y.backward(nchw(t["dy"]))
    flat = lambda a: a.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy()
    return {"y": flat(y), "dz": flat(z.grad), "dresidual": flat(res.grad) if has_res else None, "dgamma": bn.weight.grad.numpy(),
            "dbeta": bn.bias.grad.numpy(), "running_mean": bn.running_mean.numpy(), "running_var": bn.running_var.numpy()}


def _grad_errors(got, ref, P, C):
    """{output: worst error in units of its bound's scale} for the outputs in `got`."""
    keep = ~ref["undecidable"]
    e = {}
    if got.get("dz") is not None:
        e["dz"] = float((np.abs(got["dz"] - ref["dz"]) / ref["dz_scale"])[keep].max())
    if got.get("dresidual") is not None:
        e["dresidual"] = float(np.abs(got["dresidual"] - ref["dresidual"])[keep].max() / np.abs(ref["dresidual"]).max())
    for k in ("dgamma", "dbeta"):
        if got.get(k) is not None:
            scale = np.abs(ref[k]).max()
            over = np.abs(got[k] - ref[k]) - ref["und_" + k]           # what the undecidable elements of the channel cannot explain
            e[k] = float(over.max() / scale)
    return e


@pytest.mark.parametrize("name", NAMES)
def test_forward(name):
    L = _L()
    P, C, relu, has_res = _dims(name)
    t = R.inputs(name)
    worst = {}
    for gamma_key in ("gamma", "gamma_mixed"):
        ref, first = _ref_fwd(name, gamma_key), None
        for momentum in (0.1, -1.0):
            for nbt0 in (0, 7):
                sa, sb = _state(name, nbt0), _state(name, nbt0)
                want = {"running_mean": t["running_mean"], "running_var": t["running_var"], "num_batches_tracked": nbt0}
                for call in range(2):                                  # two successive calls on the same buffers
                    got, again = _fwd(L, name, gamma_key, momentum, sa), _fwd(L, name, gamma_key, momentum, sb)
                    want = R.running(ref["save_mean"], ref["var"], P, momentum, want["running_mean"], want["running_var"], want["num_batches_tracked"])
                    for k in got:
                        assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
                        if first is None:
                            worst[k] = max(worst.get(k, 0.0), R.rel(got[k].cpu().numpy(), ref[k]))
                        else:                                          # y and the batch statistics do not depend on the running side
                            assert torch.equal(got[k], first[k]), f"{k} changed with momentum / the counter"
                    first = first or got
                    for i, k in enumerate(("running_mean", "running_var")):
                        _written(sa[i], C, k)
                        assert torch.equal(sa[i][:C], sb[i][:C]), f"{k}: two calls differ"
                        worst[k] = max(worst.get(k, 0.0), R.rel(sa[i][:C].cpu().numpy(), want[k]))
                    assert sa[2].tolist() == [nbt0 + call + 1, -77, -77], "num_batches_tracked"
    tf = _torch_fp32(name, "gamma")
    r7 = R.running(ref["save_mean"], ref["var"], P, 0.1, t["running_mean"], t["running_var"], 7)
    torch_err = {"y": R.rel(tf["y"], _ref_fwd(name, "gamma")["y"]), "running_mean": R.rel(tf["running_mean"], r7["running_mean"]),
                 "running_var": R.rel(tf["running_var"], r7["running_var"])}
    print(f"bn_train_fwd case {name} P={P} C={C}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items())
          + " | torch fp32 cpu: " + " ".join(f"{k}={v:.2e}" for k, v in torch_err.items()))
    for k, v in worst.items():
        assert v < R.BOUND, (k, v)


@pytest.mark.parametrize("name", NAMES)
def test_forward_null_forms(name):
    L = _L()
    P, C, relu, has_res = _dims(name)
    # no running buffers: same y and statistics, nothing else touched (there is nothing else)
    ref = _ref_fwd(name, "gamma")
    got, again = _fwd(L, name), _fwd(L, name)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
        assert R.rel(got[k].cpu().numpy(), ref[k]) < R.BOUND, k
    # no gamma / beta: 1 / 0
    ref = _ref_fwd(name, "gamma", affine=False)
    got = _fwd(L, name, affine=False, state=_state(name, 3))
    for k in got:
        assert R.rel(got[k].cpu().numpy(), ref[k]) < R.BOUND, k


def _bwd(L, name, fw, want, gamma_key="gamma", accumulate=None, use_y=True):
    """One call.  fw: the device forward's outputs; want: the outputs asked for; accumulate: {name: initial (C,) tensor} or None."""
    P, C, relu, has_res = _dims(name)
    t = _dev(name)
    n = {"dz": P * C, "dresidual": P * C, "dgamma": C, "dbeta": C}
    nws = L.query("e2e_bn_train_workspace_floats", P=P, C=C)
    bufs = {k: _out(n[k]) for k in n}
    if accumulate:
        for k, v in accumulate.items():
            bufs[k][:C] = v
    ws = _out(nws)
    L.call("e2e_bn_train_bwd", dy=L.ptr(t["dy"]), y=L.ptr(fw["y"]) if (relu and use_y) else None, z=L.ptr(t["z"]),
           gamma=L.ptr(t[gamma_key]) if gamma_key else None, save_mean=L.ptr(fw["save_mean"]), save_rstd=L.ptr(fw["save_rstd"]), P=P, C=C,
           accumulate=1 if accumulate else 0, workspace=L.ptr(ws), stream=L.stream(), **{k: (L.ptr(bufs[k]) if k in want else None) for k in n})
    torch.cuda.synchronize()
    assert torch.isnan(ws[nws:]).all(), "workspace: written past the size its query returned"
    for k in n:
        if k in want:
            _written(bufs[k], n[k], k)
        else:
            _untouched(bufs[k], k)
    return {k: bufs[k][:n[k]].view(-1, C) if n[k] > C else bufs[k][:C] for k in want}


def _ref_bwd(name, gamma_key, relu_mask=True):
    P, C, relu, has_res = _dims(name)
    t = R.inputs(name)
    f = _ref_fwd(name, gamma_key or "gamma")
    use = relu and relu_mask
    return R.bwd(t["dy"], (f["pre"] > 0) if use else None, t["z"], t[gamma_key] if gamma_key else None, f["save_mean"], f["save_rstd"],
                 f["undecidable"] if use else None) | {"undecidable": f["undecidable"] if use else np.zeros((P, C), bool)}


FORMS = (("dz", "dresidual", "dgamma", "dbeta"), ("dz",), ("dgamma", "dbeta"), ("dresidual",), ("dz", "dbeta"))


@pytest.mark.parametrize("name", NAMES)
def test_backward(name):
    L = _L()
    P, C, relu, has_res = _dims(name)
    nws = L.query("e2e_bn_train_workspace_floats", P=P, C=C)
    assert 2 * C < nws <= 2 * 1024 * C + 2 * C and (nws - 2 * C) % (2 * C) == 0
    worst = {}

    def check(got, ref, tag):
        for k, e in _grad_errors({k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}, ref, P, C).items():
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < R.GRAD_BOUND, (tag, k, e)

    for gamma_key in ("gamma", "gamma_mixed"):
        fw = _fwd(L, name, gamma_key)
        ref = _ref_bwd(name, gamma_key)
        for want in FORMS:
            got, again = _bwd(L, name, fw, want, gamma_key), _bwd(L, name, fw, want, gamma_key)
            for k in want:
                assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
            check(got, ref, (gamma_key, want))
        # accumulate = 1 onto non-zero buffers: the sums are ADDED, in fp32
        g = torch.Generator().manual_seed(5)
        init = {k: torch.randn(C, generator=g).to(DEV) for k in ("dgamma", "dbeta")}
        got = _bwd(L, name, fw, ("dz", "dgamma", "dbeta"), gamma_key, accumulate=init)
        plain = _bwd(L, name, fw, ("dgamma", "dbeta"), gamma_key)
        for k in init:
            assert torch.equal(got[k], init[k] + plain[k]), f"{k}: accumulate is not initial + sum"
    # gamma NULL: 1
    fw = _fwd(L, name, "gamma")
    check(_bwd(L, name, fw, FORMS[0], None), _ref_bwd(name, None), "gamma NULL")
    # y NULL: no mask, whatever the forward did
    check(_bwd(L, name, fw, FORMS[0], "gamma", use_y=False), _ref_bwd(name, "gamma", relu_mask=False), "y NULL")
    tf, rb = _torch_fp32(name, "gamma"), _ref_bwd(name, "gamma")
    torch_err = _grad_errors({k: tf[k] for k in FORMS[0] if tf[k] is not None}, rb, P, C)
    print(f"bn_train_bwd case {name} P={P} C={C} slices={(nws - 2 * C) // (2 * C)}: " + " ".join(f"{k}={v:.2e}" for k, v in worst.items())
          + " | torch fp32 cpu: " + " ".join(f"{k}={v:.2e}" for k, v in torch_err.items()))


def test_graph_capture_replays_the_counter():
    """The six launches of a forward and a backward are a linear chain: recorded on a side stream into ONE graph and replayed twice
    with momentum = -1, the counter has advanced by 2 and every buffer equals two eager calls bit for bit."""
    L = _L()
    name = "h"
    P, C, relu, has_res = _dims(name)
    t = _dev(name)
    nws = L.query("e2e_bn_train_workspace_floats", P=P, C=C)

    def buffers():
        rm, rv, nbt = _state(name, 7)
        return {"rm": rm, "rv": rv, "nbt": nbt, "y": _out(P * C), "mean": _out(C), "rstd": _out(C), "ws": _out(nws), "dz": _out(P * C),
                "dres": _out(P * C), "dg": _out(C), "db": _out(C)}

    def step(b):
        st = L.stream()
        L.call("e2e_bn_train_fwd", z=L.ptr(t["z"]), gamma=L.ptr(t["gamma"]), beta=L.ptr(t["beta"]), residual=L.ptr(t["residual"]), relu=1, eps=R.EPS,
               momentum=-1.0, running_mean=L.ptr(b["rm"]), running_var=L.ptr(b["rv"]), num_batches_tracked=L.ptr(b["nbt"]), y=L.ptr(b["y"]),
               save_mean=L.ptr(b["mean"]), save_rstd=L.ptr(b["rstd"]), P=P, C=C, workspace=L.ptr(b["ws"]), stream=st)
        L.call("e2e_bn_train_bwd", dy=L.ptr(t["dy"]), y=L.ptr(b["y"]), z=L.ptr(t["z"]), gamma=L.ptr(t["gamma"]), save_mean=L.ptr(b["mean"]),
               save_rstd=L.ptr(b["rstd"]), P=P, C=C, dz=L.ptr(b["dz"]), dresidual=L.ptr(b["dres"]), dgamma=L.ptr(b["dg"]), dbeta=L.ptr(b["db"]),
               accumulate=0, workspace=L.ptr(b["ws"]), stream=st)

    eager, rec = buffers(), buffers()
    step(eager)
    step(eager)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(rec)
    torch.cuda.synchronize()
    assert rec["nbt"].tolist() == [7, -77, -77], "capturing must not run anything"
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert rec["nbt"].tolist() == eager["nbt"].tolist() == [9, -77, -77]
    for k in ("rm", "rv", "y", "mean", "rstd", "dz", "dres", "dg", "db"):
        assert torch.equal(rec[k].view(torch.int32), eager[k].view(torch.int32)), f"{k}: the replayed graph and two eager calls differ"
    ref = R.inputs(name)
    f = _ref_fwd(name, "gamma")
    want = R.running(f["save_mean"], f["var"], P, -1.0, ref["running_mean"], ref["running_var"], 7)
    want = R.running(f["save_mean"], f["var"], P, -1.0, want["running_mean"], want["running_var"], 8)
    assert R.rel(rec["rm"][:C].cpu().numpy(), want["running_mean"]) < R.BOUND and R.rel(rec["rv"][:C].cpu().numpy(), want["running_var"]) < R.BOUND


def test_refusals_write_nothing():
    L = _L()
    P, C = 15, 8
    z, res, dy = (torch.randn(P * 16, device=DEV) for _ in range(3))
    gamma, beta = torch.rand(16, device=DEV) + 0.5, torch.randn(16, device=DEV)
    nws = L.query("e2e_bn_train_workspace_floats", P=P, C=C)
    assert nws > 0
    for bad in (dict(P=1, C=8), dict(P=0, C=8), dict(P=15, C=0), dict(P=15, C=6), dict(P=15, C=-4)):
        assert L.query("e2e_bn_train_workspace_floats", **bad) == 0

    def fwd_case(change, drop=()):
        rm, rv, nbt = _guarded(torch.zeros(C, device=DEV)), _guarded(torch.ones(C, device=DEV)), torch.tensor([5], dtype=torch.int64, device=DEV)
        y, mean, rstd, ws = _out(P * 16), _out(16), _out(16), _out(nws)
        args = dict(z=L.ptr(z), gamma=L.ptr(gamma), beta=L.ptr(beta), residual=L.ptr(res), relu=1, eps=R.EPS, momentum=0.1, running_mean=L.ptr(rm),
                    running_var=L.ptr(rv), num_batches_tracked=L.ptr(nbt), y=L.ptr(y), save_mean=L.ptr(mean), save_rstd=L.ptr(rstd), P=P, C=C,
                    workspace=L.ptr(ws), stream=L.stream())
        args.update(change)
        with pytest.raises(L.E2EError):
            L.call("e2e_bn_train_fwd", **args)
        torch.cuda.synchronize()
        for what, b in (("y", y), ("save_mean", mean), ("save_rstd", rstd), ("workspace", ws)):
            _untouched(b, f"{what} after {change}")
        assert torch.equal(rm[:C], torch.zeros(C, device=DEV)) and torch.equal(rv[:C], torch.ones(C, device=DEV)) and int(nbt) == 5, change

    for change in (dict(z=None), dict(y=None), dict(workspace=None), dict(P=1), dict(P=0), dict(C=0), dict(C=-8), dict(C=6), dict(C=10),
                   dict(eps=0.0), dict(eps=-1e-5), dict(running_mean=None), dict(running_var=None), dict(num_batches_tracked=None),
                   dict(running_mean=None, running_var=None), dict(running_var=None, num_batches_tracked=None), dict(save_mean=None),
                   dict(save_rstd=None)):
        fwd_case(change)

    y, mean, rstd = torch.rand(P * 16, device=DEV), torch.randn(16, device=DEV), torch.rand(16, device=DEV) + 0.5

    def bwd_case(change):
        dz, dres, dg, db, ws = _out(P * 16), _out(P * 16), _out(16), _out(16), _out(nws)
        args = dict(dy=L.ptr(dy), y=L.ptr(y), z=L.ptr(z), gamma=L.ptr(gamma), save_mean=L.ptr(mean), save_rstd=L.ptr(rstd), P=P, C=C, dz=L.ptr(dz),
                    dresidual=L.ptr(dres), dgamma=L.ptr(dg), dbeta=L.ptr(db), accumulate=0, workspace=L.ptr(ws), stream=L.stream())
        args.update(change)
        with pytest.raises(L.E2EError):
            L.call("e2e_bn_train_bwd", **args)
        torch.cuda.synchronize()
        for what, b in (("dz", dz), ("dresidual", dres), ("dgamma", dg), ("dbeta", db), ("workspace", ws)):
            _untouched(b, f"{what} after {change}")

    for change in (dict(dy=None), dict(z=None), dict(workspace=None), dict(save_mean=None), dict(save_rstd=None), dict(P=1), dict(P=0), dict(C=0),
                   dict(C=6), dict(C=-8), dict(dz=None, dresidual=None, dgamma=None, dbeta=None)):
        bwd_case(change)
