"""A NetPlan with the stage-entry forward call (E2E_FWD_ENTRY_PAIR) and the fused head backward (E2E_HEAD_BWD_FUSED) on against the same plan with
both off -- the launches of the parent form: every activation, the disparity, and every parameter gradient must be equal BIT FOR BIT after a
forward, a backward and a forward_one(1); and a captured step graph replayed with the switches on must equal the eager run."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, H, W = 2, 64, 96


def _model():
    from depth_estimation.networks import DispResNet_Indoor
    torch.manual_seed(3)
    m = DispResNet_Indoor(18, False)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_var.uniform_(0.5, 1.5)
                mod.running_mean.normal_(0.0, 0.2)
                mod.weight.uniform_(0.8, 1.2)
                mod.bias.normal_(0.0, 0.2)
    m.to(DEV).eval()
    for name, q in m.named_parameters():
        if name.find("bn") != -1:
            q.requires_grad = False
    return m


def _run(on, monkeypatch, replay=False):
    """-> (activations after forward, gradients, activations after forward_one(1) on a second frame pair[, the same three from a replayed graph])"""
    from e2ehip.netplan import NetPlan, _BNAffine
    for name in ("E2E_FWD_ENTRY_PAIR", "E2E_HEAD_BWD_FUSED"):
        monkeypatch.setenv(name, "1" if on else "0")
    m = _model()
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, H, W, 3, generator=g).to(DEV)
    x2 = torch.rand(B, H, W, 3, generator=g).to(DEV)
    gd = torch.randn(B, 1, H, W, generator=g).to(DEV)
    plan = NetPlan(m, B, H, W, DEV, overlap=False)
    assert plan.entry_pair == on
    entries = [op for op in plan.ops if getattr(op, "entry", None) is not None]
    assert len(entries) == (3 if on else 0)                   # layer2.0, layer3.0, layer4.0
    assert sum(isinstance(op, _BNAffine) and op.fwd_in is not None for op in plan.ops) == len(entries)
    plan.refresh_layouts()

    def step():
        plan.forward()
        plan.backward()

    def state():
        return [op.out.t.clone() for op in plan.ops] + [plan.disp.t.clone()] + [op.scale.clone() for op in plan.ops if isinstance(op, _BNAffine)]

    def grads():
        return [plan.sink(q).clone() for q in plan.parameters()]

    def whole():
        plan.x.t.copy_(x)
        plan.disp.g.copy_(gd.reshape(plan.disp.g.shape))
        for q in plan.parameters():
            plan.sink(q).zero_()
        yield None                                            # the caller runs the step (eagerly or by replay)
        torch.cuda.synchronize()
        acts, gr = state(), grads()
        plan.x.t.copy_(x2)
        plan.forward_one(1)
        torch.cuda.synchronize()
        yield acts, gr, state()

    it = whole()
    next(it)
    step()
    eager = next(it)
    if not replay:
        plan.close()
        return eager
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        step()
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            step()
    it = whole()
    next(it)
    graph.replay()
    replayed = next(it)
    del graph
    plan.close()
    return eager, replayed


def _equal(a, b, what):
    for part, xs, ys in zip(("activations", "gradients", "activations after forward_one(1)"), a, b):
        assert len(xs) == len(ys) > 0
        for i, (p, q) in enumerate(zip(xs, ys)):
            assert torch.isfinite(p).all() and torch.equal(p, q), f"{what}: {part}[{i}] differ"


def test_plan_with_switches_on_equals_switches_off(monkeypatch):
    _equal(_run(True, monkeypatch), _run(False, monkeypatch), "switches on / off")


def test_replayed_step_graph_equals_the_eager_run(monkeypatch):
    eager, replayed = _run(True, monkeypatch, replay=True)
    _equal(eager, replayed, "eager / replayed")
