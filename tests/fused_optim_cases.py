"""Shared by the fused-optimiser tests (no fixtures, no tests): the three optimisers' float64 update rules, the inputs of the
class-level comparison with torch, torch's own float64 run over them (computed once per process) and the bounds.

The bounds are stated for these inputs (five steps at lr 1e-2, gradients of magnitude 0.1 .. 5):
    parameters   |err| <= 1e-6 |ref| + 1e-7
    state        |err| <= 1e-6 |ref| + 1e-6 max|ref|   per tensor
torch's own fp32 CPU optimisers sit at 0.53 / 0.40 / 0.19 of the parameter bound (SGD / RMSprop / Adagrad) and below 0.1 of the
state bound on them (tests/test_fused_optimizer_calibration.py re-measures that), which leaves the GPU's contracted multiply-adds
about a factor of two."""
import functools

import torch

KINDS = ("SGD", "RMSprop", "Adagrad")
LR = 1e-2
STEPS = 5
SHAPES = [(64, 3, 7, 7), (64,), (128, 64, 3, 3), (5,), (1, 16, 3, 3), (1,), (3,)]
FROZEN, NEVER = 2, 4            # positions (in the parameter list) of a requires_grad=False and of a never-differentiated parameter
# the reference's settings (utils/training_utils.py:26-47)
HYPER = {"SGD": dict(momentum=0.9, weight_decay=1e-3), "RMSprop": dict(alpha=0.99, eps=1e-8), "Adagrad": dict(eps=1e-10)}
STATE_KEY = {"SGD": "momentum_buffer", "RMSprop": "square_avg", "Adagrad": "sum"}
PARAM_RTOL, PARAM_ATOL, STATE_RTOL = 1e-6, 1e-7, 1e-6


def torch_class(kind):
    return getattr(torch.optim, kind)


def fused_class(kind):
    from e2ehip import optim
    return getattr(optim, "Fused" + kind)


def update64(kind, p, g, s, lr, **h):
    """One step of include/e2eslam.h's formulas on float64 tensors -> (p, state)."""
    if kind == "SGD":
        s = h["momentum"] * s + (g + h["weight_decay"] * p)
        return p - lr * s, s
    if kind == "RMSprop":
        s = h["alpha"] * s + (1.0 - h["alpha"]) * g * g
    else:
        s = s + g * g
    return p - lr * g / (s.sqrt() + h["eps"]), s


def sparse_randn(shape, scale, gen):
    """randn * scale with the small elements set to exactly 0 (the kernels' zero-gradient case), fp32."""
    g = torch.randn(*shape, generator=gen) * scale
    g[g.abs() < 0.05] = 0.0
    return g


@functools.lru_cache(maxsize=None)
def inputs():
    """(initial values of the 7 trained + 2 idle parameters, gradients[step][trained parameter]) in fp32; never modified."""
    gen = torch.Generator().manual_seed(20260)
    shapes = list(SHAPES)
    shapes.insert(FROZEN, (6, 2))
    shapes.insert(NEVER, (4,))
    init = tuple(torch.randn(*sh, generator=gen) for sh in shapes)
    grads = tuple(tuple(sparse_randn(sh, 0.1 + k, gen) for sh in SHAPES) for k in range(STEPS + 1))      # one spare step for the state-dict tests
    assert any(bool((g == 0).any()) for g in grads[0])
    return init, grads


def trained(params):
    return [p for i, p in enumerate(params) if i not in (FROZEN, NEVER)]


def make_params(device, dtype=torch.float32, values=None):
    init, _ = inputs()
    values = init if values is None else values
    return [torch.nn.Parameter(v.detach().to(device=device, dtype=dtype).clone(), requires_grad=i != FROZEN) for i, v in enumerate(values)]


def set_grads(params, k):
    """Install step k's gradients the way a backward pass does: a new tensor where there is none, in place where there is one."""
    _, grads = inputs()
    for p, g in zip(trained(params), grads[k]):
        g = g.to(device=p.device, dtype=p.dtype)
        if p.grad is None:
            p.grad = g.clone()
        else:
            p.grad.copy_(g)


def run(opt, params, steps):
    for k in steps:
        opt.zero_grad()
        set_grads(params, k)
        opt.step()


@functools.lru_cache(maxsize=None)
def torch_run(kind, dtype=torch.float64, steps=STEPS):
    """torch's own optimiser on the CPU -> (parameters, {parameter index: state tensor}) after `steps` steps."""
    params = make_params("cpu", dtype)
    opt = torch_class(kind)(params, lr=LR, **HYPER[kind])
    run(opt, params, range(steps))
    return [p.detach() for p in params], {i: opt.state[p][STATE_KEY[kind]] for i, p in enumerate(params) if STATE_KEY[kind] in opt.state.get(p, {})}


def param_excess(got, ref):
    """max |err| / bound over the elements: <= 1 holds the parameter bound."""
    ref = ref.detach().double()
    return float(((got.detach().cpu().double() - ref).abs() / (PARAM_RTOL * ref.abs() + PARAM_ATOL)).max())


def state_excess(got, ref):
    ref = ref.detach().double()
    return float(((got.detach().cpu().double() - ref).abs() / (STATE_RTOL * ref.abs() + STATE_RTOL * ref.abs().max())).max())


def check_against(kind, what, params, state, ref_params, ref_state):
    """Prints the figures, then asserts: idle parameters untouched and stateless, the others within the bounds."""
    init, _ = inputs()
    for i in (FROZEN, NEVER):
        assert torch.equal(params[i].detach().cpu(), init[i]) and i not in state, f"{kind}: idle parameter {i} moved or has state"
    pe = max(param_excess(p, r) for i, (p, r) in enumerate(zip(params, ref_params)) if i not in (FROZEN, NEVER))
    assert sorted(state) == sorted(i for i in ref_state if i not in (FROZEN, NEVER)) == [i for i in range(len(params)) if i not in (FROZEN, NEVER)]
    se = max(state_excess(state[i], ref_state[i]) for i in state)
    print(f"{kind} {what}: parameters at {pe:.3f} of their bound, state at {se:.3f} of its bound")
    assert pe <= 1.0 and se <= 1.0, (kind, what, pe, se)
    return pe, se
