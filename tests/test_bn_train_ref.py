"""Host-only: the float64 reference of tests/bn_train_ref.py against torch.nn.BatchNorm2d in float64, on every case the device
contracts use -- forward, autograd gradients, the running buffers, num_batches_tracked, momentum=None over two calls -- and the input
qualification: the elements whose ReLU an fp32 evaluation cannot decide are at most 1e-3 of a case."""
import numpy as np
import pytest
import torch

import bn_train_ref as R

TOL = 1e-10          # float64 against float64: of the output's maximum


def _torch_bn(name, momentum, gamma_key="gamma", nbt=0, calls=1):
    (B, H, W, C), relu, has_res, _ = R.CASES[name]
    t = R.inputs(name)
    bn = torch.nn.BatchNorm2d(C, eps=R.EPS, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(np.array(t[gamma_key])))
        bn.bias.copy_(torch.from_numpy(np.array(t["beta"])))
        bn.running_mean.copy_(torch.from_numpy(np.array(t["running_mean"])))
        bn.running_var.copy_(torch.from_numpy(np.array(t["running_var"])))
        bn.num_batches_tracked.fill_(nbt)
    nchw = lambda a: torch.from_numpy(np.array(a)).double().view(B, H, W, C).permute(0, 3, 1, 2)
    z = nchw(t["z"]).clone().requires_grad_(True)
    res = nchw(t["residual"]).clone().requires_grad_(True) if has_res else None
    for _ in range(calls):
        bn.zero_grad()
        z.grad = None
        if res is not None:
            res.grad = None
        y = bn(z)
        if res is not None:
            y = y + res
        if relu:
            y = torch.relu(y)
        y.backward(nchw(t["dy"]))
    flat = lambda a: a.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy()
    return {"y": flat(y), "dz": flat(z.grad), "dresidual": flat(res.grad) if has_res else None, "dgamma": bn.weight.grad.numpy(),
            "dbeta": bn.bias.grad.numpy(), "running_mean": bn.running_mean.numpy(), "running_var": bn.running_var.numpy(),
            "num_batches_tracked": int(bn.num_batches_tracked)}


def _ref(name, momentum, gamma_key="gamma", nbt=0, calls=1):
    (B, H, W, C), relu, has_res, _ = R.CASES[name]
    t = R.inputs(name)
    rm, rv = t["running_mean"], t["running_var"]
    for _ in range(calls):
        f = R.fwd(t["z"], t[gamma_key], t["beta"], t["residual"] if has_res else None, relu, R.EPS, -1.0 if momentum is None else momentum,
                  rm, rv, nbt)
        rm, rv, nbt = f["running_mean"], f["running_var"], f["num_batches_tracked"]
    b = R.bwd(t["dy"], (f["pre"] > 0) if relu else None, t["z"], t[gamma_key], f["save_mean"], f["save_rstd"], f["undecidable"])
    return f, b


@pytest.mark.parametrize("gamma_key", ["gamma", "gamma_mixed"])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_reference_is_torch_batchnorm_in_float64(name, gamma_key):
    has_res = R.CASES[name][2]
    want = _torch_bn(name, 0.1, gamma_key, nbt=7)
    f, b = _ref(name, 0.1, gamma_key, nbt=7)
    got = {**f, **b}
    for k in ("y", "dz", "dgamma", "dbeta", "running_mean", "running_var") + (("dresidual",) if has_res else ()):
        e = R.rel(got[k], want[k])
        if k == "dz":                            # case (a): dz is a difference of nearly equal terms; measure as the device test does
            e = float((np.abs(got[k] - want[k]) / b["dz_scale"]).max())
        assert e < TOL, (k, e)
    assert got["num_batches_tracked"] == want["num_batches_tracked"] == 8


@pytest.mark.parametrize("nbt", [0, 7])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_cumulative_average_over_two_calls(name, nbt):
    """momentum=None: f = 1 / num_batches_tracked after the increment, twice."""
    want = _torch_bn(name, None, nbt=nbt, calls=2)
    f, _ = _ref(name, None, nbt=nbt, calls=2)
    for k in ("running_mean", "running_var"):
        assert R.rel(f[k], want[k]) < TOL, k
    assert f["num_batches_tracked"] == want["num_batches_tracked"] == nbt + 2


def test_null_forms_of_the_reference():
    t = R.inputs("b")
    f = R.fwd(t["z"], None, None, None, False, R.EPS, 0.1, None, None, None)
    assert "running_mean" not in f and not f["undecidable"].any()
    np.testing.assert_allclose(f["y"].mean(0), 0.0, atol=1e-12)
    np.testing.assert_allclose((f["y"] ** 2).mean(0), 1.0, rtol=1e-4)          # eps
    b = R.bwd(t["dy"], None, t["z"], None, f["save_mean"], f["save_rstd"])
    np.testing.assert_allclose(b["dz"].sum(0), 0.0, atol=1e-12)                # a shift of z changes nothing: dz sums to zero


@pytest.mark.parametrize("gamma_key", ["gamma", "gamma_mixed"])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_inputs_are_qualified(name, gamma_key):
    """At most 1e-3 of a case's elements have a ReLU that fp32 cannot decide; the cases without a ReLU have none; the offsets are
    what the table says (channel means 50 and 3 standard deviations from zero)."""
    (B, H, W, C), relu, _, off = R.CASES[name]
    f, _ = _ref(name, 0.1, gamma_key)
    share = float(f["undecidable"].mean())
    print(f"case {name} {gamma_key}: undecidable share {share:.3g}")
    assert share <= 1e-3
    if not relu:
        assert share == 0.0
    if off:
        z = R.inputs(name)["z"].astype(np.float64)
        ratio = np.abs(z.mean(0)) / z.std(0)
        assert ratio.min() > 0.9 * off - 1.0 and ratio.max() < 1.1 * off + 1.0
