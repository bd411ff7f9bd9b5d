"""e2e_conv2d_bwd_pair_deferred (a layer's backward-data and backward-weight GEMMs as ONE launch) against the two separate calls it replaces:
every tile runs the arithmetic of its own launch, so input gradient, weight gradient and bias gradient must be equal BIT FOR BIT -- in both
orders of the two tile sets, on every layer shape of the network at the benchmark size, on small shapes, and on the shapes that fall back to
the two launch sequences."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# B, Cin(x), Cskip, up, H, W (input of the convolution at full resolution), Cout, k, stride, pad, reflect
NETWORK = [
    (2, 64, 0, 1, 120, 160, 64, 3, 1, 1, 0), (2, 64, 0, 1, 120, 160, 128, 3, 2, 1, 0), (2, 64, 0, 1, 120, 160, 128, 1, 2, 0, 0),
    (2, 128, 0, 1, 60, 80, 128, 3, 1, 1, 0), (2, 128, 0, 1, 60, 80, 256, 3, 2, 1, 0), (2, 128, 0, 1, 60, 80, 256, 1, 2, 0, 0),
    (2, 256, 0, 1, 30, 40, 256, 3, 1, 1, 0), (2, 256, 0, 1, 30, 40, 512, 3, 2, 1, 0), (2, 256, 0, 1, 30, 40, 512, 1, 2, 0, 0),
    (2, 512, 0, 1, 15, 20, 512, 3, 1, 1, 0), (2, 512, 0, 1, 15, 20, 256, 3, 1, 1, 1), (2, 256, 256, 2, 30, 40, 256, 3, 1, 1, 1),
    (2, 256, 0, 1, 30, 40, 128, 3, 1, 1, 1), (2, 128, 128, 2, 60, 80, 128, 3, 1, 1, 1), (2, 128, 0, 1, 60, 80, 64, 3, 1, 1, 1),
    (2, 64, 64, 2, 120, 160, 64, 3, 1, 1, 1), (2, 64, 0, 1, 120, 160, 32, 3, 1, 1, 1), (2, 32, 64, 2, 240, 320, 32, 3, 1, 1, 1),
    (2, 32, 0, 1, 240, 320, 16, 3, 1, 1, 1), (2, 16, 0, 2, 480, 640, 16, 3, 1, 1, 1),
]
SMALL = [   # the shapes of test_gpu_conv.CASES that have a backward-data GEMM
    (2, 64, 0, 1, 12, 20, 64, 3, 1, 1, 0), (2, 64, 0, 1, 12, 20, 128, 3, 2, 1, 0), (1, 64, 0, 1, 13, 9, 128, 1, 2, 0, 0),
    (2, 512, 0, 1, 2, 3, 256, 3, 1, 1, 1), (2, 256, 256, 2, 4, 6, 256, 3, 1, 1, 1), (1, 32, 64, 2, 16, 24, 32, 3, 1, 1, 1),
    (1, 32, 0, 1, 20, 36, 16, 3, 1, 1, 1), (1, 16, 0, 2, 24, 40, 16, 3, 1, 1, 1), (1, 128, 0, 1, 30, 40, 128, 3, 1, 1, 0),
    (2, 64, 0, 1, 30, 44, 128, 3, 2, 1, 0), (1, 128, 0, 1, 17, 23, 256, 3, 2, 1, 0), (2, 64, 0, 1, 16, 24, 128, 1, 2, 0, 0),
]
# one shape per kind of path that does not pair (the backward-data decompositions of the network are all paired or thin):
# backward-weight with 32-row tiles (Cout <= 32), the 16-channel backward-weight kernel, the thin patch kernels (both halves), 16-deep chunks
FALLBACK = [
    (2, 64, 0, 1, 40, 56, 32, 3, 1, 1, 0),      # backward-weight k_wgrad_gemm4<1, 4>
    (1, 64, 0, 1, 20, 36, 16, 3, 1, 1, 0),      # backward-weight k_wgrad_gemm16, backward-data 16 columns
    (1, 16, 0, 1, 24, 40, 16, 3, 1, 1, 1),      # backward-data k_conv3x3_thin + backward-weight thin patch kernel
    (2, 64, 0, 1, 10, 14, 80, 3, 1, 1, 0),      # Cout % 32 != 0: 16-deep chunks of the backward-data GEMM
]
SENTINEL = 64


def _inputs(spec, seed):
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = spec
    g = torch.Generator().manual_seed(seed)
    Cin = Cx + Cs
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    t = dict(spec=spec, Cin=Cin, Ho=Ho, Wo=Wo)
    t["da"] = torch.randn(B, Ho, Wo, Cout, generator=g).to(DEV)
    t["wb"] = torch.randn(k * k * Cout, (Cin + 3) // 4 * 4, generator=g).to(DEV)
    t["src0"] = torch.randn(B, H // up, W // up, Cx, generator=g).to(DEV)
    t["src1"] = torch.randn(B, H, W, Cs, generator=g).to(DEV) if Cs else None
    t["scale"] = (torch.rand(Cout, generator=g) + 0.5).to(DEV) if not pm else None
    t["bias"] = bool(pm)
    pp = p if pm else 0
    t["dx_shape"] = (B, H + 2 * pp, W + 2 * pp, Cin)
    t["x_in"] = torch.randn(t["dx_shape"], generator=g).to(DEV) if not pm else None
    t["pre"] = torch.randn(t["dx_shape"], generator=g).to(DEV) if not pm else None
    t["dx0"] = torch.randn(t["dx_shape"], generator=g).to(DEV)
    return t


def _run(t, how, mode="plain"):
    """how: 'separate' (the two entry points) or 0 / 1 (the pair entry, wgrad_first); mode: plain / acc / pre / relu / elu (fused forms)"""
    from e2ehip import _lib as L
    lib = L.load()
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = t["spec"]
    Cin, Ho, Wo = t["Cin"], t["Ho"], t["Wo"]
    n_dx = t["dx0"].numel()
    dx_buf = torch.full((n_dx + SENTINEL,), float("nan"), device=DEV)
    if mode == "acc":
        dx_buf[:n_dx] = t["dx0"].flatten()
    dx = dx_buf[:n_dx]
    acc = 1 if mode == "acc" else 0
    in_act = {"relu": 1, "elu": 2}.get(mode, 0)
    x_in = t["x_in"] if in_act else None
    pre = t["pre"] if mode == "pre" else None
    n_wsb = lib.e2e_conv2d_bwd_data_workspace_floats(B, t["dx_shape"][1], t["dx_shape"][2], Cin, k * k * Cout, s)
    wsb = torch.zeros(max(n_wsb, 1), device=DEV)
    wsw = torch.empty(lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, 1 if t["bias"] else 0), device=DEV)
    dw_buf = torch.full((Cout * Cin * k * k + SENTINEL,), float("nan"), device=DEV)
    db = torch.full((Cout,), float("nan"), device=DEV) if t["bias"] else None
    d = L.WgradReduceDesc()
    ld = t["wb"].shape[1]
    data_args = [L.ptr(t["da"]), L.ptr(t["wb"]), ld, L.ptr(dx), B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm]
    w_tail = [L.ptr(t["src0"]), L.ptr(t["src1"]), Cx, up, L.ptr(dw_buf), L.ptr(db), L.ptr(wsw)]
    if how == "separate":
        L.call("e2e_conv2d_bwd_data_fused", *data_args, acc, L.ptr(x_in), in_act, L.ptr(pre), L.ptr(wsb if n_wsb else None), L.stream())
        L.call("e2e_conv2d_bwd_weight_scaled_deferred", L.ptr(t["da"]), L.ptr(t["scale"]), *w_tail, B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, 0,
               0.0, 1.0, ctypes.byref(d), L.stream())
    else:
        L.call("e2e_conv2d_bwd_pair_deferred", *data_args, acc, L.ptr(x_in), in_act, L.ptr(pre), L.ptr(wsb if n_wsb else None), L.ptr(t["scale"]),
               *w_tail, 0, 0.0, 1.0, ctypes.byref(d), how, L.stream())
    arr = (L.WgradReduceDesc * 1)(d)
    total = lib.e2e_wgrad_reduce_batch_prepare(arr, 1)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.call("e2e_wgrad_reduce_batched", L.ptr(table), 1, total, L.stream())
    torch.cuda.synchronize()
    return dx_buf, dw_buf, db


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
                                         and torch.equal(torch.isnan(a), torch.isnan(b)))


def _check(spec, modes=("plain",), seed=1):
    t = _inputs(spec, seed)
    for mode in modes:
        ref = _run(t, "separate", mode)
        assert torch.isnan(ref[0][-SENTINEL:]).all() and torch.isnan(ref[1][-SENTINEL:]).all()
        assert not torch.isnan(ref[1][:-SENTINEL]).any()
        for order in (0, 1):
            out = _run(t, order, mode)
            for name, a, b in zip(("dx", "dW", "db"), out, ref):
                assert _same(a, b), f"{spec} {mode} order {order}: {name} differs from the separate launches"


@pytest.mark.parametrize("spec", NETWORK, ids=[f"net{i}" for i in range(len(NETWORK))])
def test_network_layers_bit_identical(spec):
    direct = spec[2] == 0 and spec[3] == 1 and not spec[10]
    _check(spec, ("plain", "acc", "pre", "relu", "elu") if direct else ("plain",))


@pytest.mark.parametrize("spec", SMALL, ids=[f"small{i}" for i in range(len(SMALL))])
def test_small_shapes_bit_identical(spec):
    direct = spec[2] == 0 and spec[3] == 1 and not spec[10]
    _check(spec, ("plain", "acc", "pre", "relu", "elu") if direct else ("plain",))


@pytest.mark.parametrize("spec", FALLBACK, ids=[f"fallback{i}" for i in range(len(FALLBACK))])
def test_fallback_shapes_bit_identical(spec):
    _check(spec, ("plain", "acc") if not spec[10] else ("plain",))


def test_run_to_run_bit_equality():
    for spec in (NETWORK[0], NETWORK[9], NETWORK[13]):
        t = _inputs(spec, 3)
        a, b = _run(t, 1), _run(t, 1)
        for x, y in zip(a, b):
            assert _same(x, y)


def _plan_grads(paired, monkeypatch, B=2, H=64, W=96):
    """One eager forward + backward of a one-stream NetPlan, then the same replayed from a captured graph: (eager, replayed) gradient buckets."""
    from e2ehip.netplan import NetPlan
    from depth_estimation.networks import DispResNet_Indoor
    monkeypatch.setenv("E2E_PAIRED_BWD", "1" if paired else "0")
    torch.manual_seed(3)
    m = DispResNet_Indoor(18, False)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_var.uniform_(0.5, 1.5)
                mod.weight.uniform_(0.8, 1.2)
    m.to(DEV).eval()
    for name, q in m.named_parameters():
        if name.find("bn") != -1:
            q.requires_grad = False
    g = torch.Generator().manual_seed(5)
    x = torch.rand(B, H, W, 3, generator=g).to(DEV)
    gd = torch.randn(B, 1, H, W, generator=g).to(DEV)
    plan = NetPlan(m, B, H, W, DEV, overlap=False)
    assert plan.paired == paired
    plan.refresh_layouts()
    plan.forward(x)
    plan.backward(gd)
    torch.cuda.synchronize()
    eager = [plan.sink(q).clone() for q in plan.parameters()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        plan.forward()
        plan.backward()
        s.synchronize()
        with torch.cuda.graph(graph, stream=s):
            plan.forward()
            plan.backward()
    for q in plan.parameters():
        plan.sink(q).zero_()
    plan.x.t.copy_(x)
    plan.disp.g.copy_(gd.reshape(plan.disp.g.shape))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [plan.sink(q).clone() for q in plan.parameters()]
    del graph
    plan.close()
    return eager, replayed


def test_plan_paired_and_separate_gradients_identical_eager_and_replayed(monkeypatch):
    e1, r1 = _plan_grads(True, monkeypatch)
    e0, r0 = _plan_grads(False, monkeypatch)
    assert len(e1) == len(e0) > 0
    for a, b, c, d in zip(e1, r1, e0, r0):
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(c, d)
