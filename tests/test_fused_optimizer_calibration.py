"""Host-only side of the fused SGD / RMSprop / Adagrad tests: where torch's OWN fp32 optimisers stand against the bounds that
tests/test_gpu_fused_optimizers.py holds the HIP kernels to, the options the fused classes refuse, and what define_optim returns for
CPU parameters."""
import types

import pytest
import torch

import fused_optim_cases as C


@pytest.mark.parametrize("kind", C.KINDS)
def test_torch_fp32_sits_well_inside_the_bounds(kind):
    """The calibration of the bounds, kept on record: torch's fp32 CPU optimiser against torch's float64 one on the inputs of the GPU
    comparison.  Measured on the CPU this was written on: parameters at 0.53 / 0.40 / 0.19 of their bound (SGD / RMSprop / Adagrad),
    state at 0.06 / 0.05 / 0.03.  Asserted at 0.6 and 0.1: the bounds are meant to leave an fp32 implementation that rounds
    differently (the GPU contracts a * b + c) about a factor of two, and they only do while torch's own rounding takes about half."""
    ref_params, ref_state = C.torch_run(kind)
    params, state = C.torch_run(kind, torch.float32)
    idle = (C.FROZEN, C.NEVER)
    pe = max(C.param_excess(p, r) for i, (p, r) in enumerate(zip(params, ref_params)) if i not in idle)
    se = max(C.state_excess(state[i], ref_state[i]) for i in state if i not in idle)
    print(f"torch fp32 {kind}: parameters at {pe:.3f} of their bound, state at {se:.3f} of its bound")
    assert 0.0 < pe <= 0.6 and 0.0 < se <= 0.1


def test_float64_rules_are_torchs():
    """The formulas the entry-point test evaluates in float64 (fused_optim_cases.update64) are torch's updates: five steps on one tensor
    agree with torch's float64 optimisers to float64 rounding."""
    init, grads = C.inputs()
    for kind in C.KINDS:
        ref_params, ref_state = C.torch_run(kind)
        p, s = init[0].double(), torch.zeros_like(init[0], dtype=torch.float64)
        for k in range(C.STEPS):
            p, s = C.update64(kind, p, grads[k][0].double(), s, C.LR, **C.HYPER[kind])
        torch.testing.assert_close(p, ref_params[0], rtol=1e-13, atol=1e-14)
        torch.testing.assert_close(s, ref_state[0], rtol=1e-13, atol=1e-14)


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("kind,option", [("SGD", dict(nesterov=True, momentum=0.9)), ("SGD", dict(dampening=0.1)), ("SGD", dict(maximize=True)),
                                         ("RMSprop", dict(centered=True)), ("RMSprop", dict(momentum=0.9)), ("RMSprop", dict(maximize=True)),
                                         ("RMSprop", dict(weight_decay=1e-3)), ("Adagrad", dict(lr_decay=1e-2)), ("Adagrad", dict(maximize=True)),
                                         ("Adagrad", dict(initial_accumulator_value=0.1)), ("Adagrad", dict(weight_decay=1e-3))],
                         ids=lambda v: v if isinstance(v, str) else next(iter(v)))
def test_unsupported_torch_options_are_refused_by_name(kind, option):
    """At construction, and when a file written by a torch optimiser that used the option is loaded."""
    name = next(iter(option))
    with pytest.raises(NotImplementedError, match=name):
        C.fused_class(kind)(_params(), lr=1e-2, **option)
    written = C.torch_class(kind)(_params(), lr=1e-2, **option).state_dict()
    opt = C.fused_class(kind)(_params(), lr=1e-2)
    with pytest.raises(NotImplementedError, match=name):
        opt.load_state_dict(written)


@pytest.mark.parametrize("kind", C.KINDS)
def test_one_group_only_and_torch_group_format(kind):
    ps = _params()
    with pytest.raises(NotImplementedError, match="ONE parameter group"):
        C.fused_class(kind)([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-4}], lr=1e-3)
    opt = C.fused_class(kind)(ps, lr=1e-2, **C.HYPER[kind])
    sd = opt.state_dict()
    assert sd["state"] == {} and sd["param_groups"][0]["params"] == [0, 1]           # no state before the first step
    # every hyper-parameter the fused class carries is one of torch's, at torch's value for the same construction
    theirs = C.torch_class(kind)(_params(), lr=1e-2, **C.HYPER[kind]).state_dict()["param_groups"][0]
    ours = sd["param_groups"][0]
    assert set(ours) <= set(theirs) and all(theirs[k] == v for k, v in ours.items())
    # a state dict loaded before the bucket exists waits and round-trips unchanged
    t = C.torch_class(kind)(_params(), lr=3e-3, **C.HYPER[kind])
    for p in t.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    t.step()
    opt.load_state_dict(t.state_dict())
    back = opt.state_dict()
    assert opt.param_groups[0]["lr"] == 3e-3 and sorted(back["state"]) == [0, 1]
    for i in (0, 1):
        assert torch.equal(back["state"][i][C.STATE_KEY[kind]], t.state_dict()["state"][i][C.STATE_KEY[kind]])


def test_define_optim_names():
    """CPU parameters: torch's own class for every name, as for Adam; an unknown name is refused."""
    from utils.training_utils import define_optim
    for name in ("Adam",) + C.KINDS:
        args = types.SimpleNamespace(OPTIMIZATION=types.SimpleNamespace(optimizer=name, learning_rate=1e-3))
        assert type(define_optim(args, _params())) is getattr(torch.optim, name)
    with pytest.raises(ValueError):
        define_optim(types.SimpleNamespace(OPTIMIZATION=types.SimpleNamespace(optimizer="LBFGS", learning_rate=1e-3)), _params())
