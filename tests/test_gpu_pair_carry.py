"""e2e_conv2d_bwd_pair_carry (a paired backward launch whose grid also runs slab reductions left by earlier backward-weight GEMMs),
e2e_conv2d_bwd_pair_is_one_launch and e2e_wgrad_reduce_batched_range against what they replace: every reduction item and every GEMM tile
does the arithmetic it does in its own launch, so all results must be equal BIT FOR BIT (torch.equal + equal NaN masks; NaN sentinels
behind every output buffer).

Carriers: the four shapes of tests/test_gpu_bwd_pair.py SMALL named in the issue, one per kind of layer.  Two of them -- the 1x1 stride-2
layer at 13 x 9 and the reflect + upsample + concat layer at 4 x 6 -- have output rows shorter than 8 pixels: the backward-weight half
takes the scalar-loader GEMM there, the two GEMMs do not pair (neither here nor before this entry point existed), and the carried range
runs as a launch of its own.  They stay as cases of the fallback; WIDE adds one shape of each of the two kinds that does pair (same
channels, 16 x 24 and 4 x 16), so that every kind is also covered on the one-launch path, and the query is checked against both groups."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64

# B, Cin(x), Cskip, up, H, W (input of the convolution at full resolution), Cout, k, stride, pad, reflect
CARRIERS = [(2, 64, 0, 1, 12, 20, 64, 3, 1, 1, 0), (2, 64, 0, 1, 12, 20, 128, 3, 2, 1, 0), (1, 64, 0, 1, 13, 9, 128, 1, 2, 0, 0),
            (2, 256, 256, 2, 4, 6, 256, 3, 1, 1, 1)]
WIDE = [(2, 64, 0, 1, 16, 24, 128, 1, 2, 0, 0), (2, 256, 256, 2, 4, 16, 256, 3, 1, 1, 1)]
ONE_LAUNCH = [CARRIERS[0], CARRIERS[1]] + WIDE
FALLBACK = [(2, 64, 0, 1, 40, 56, 32, 3, 1, 1, 0), (1, 64, 0, 1, 20, 36, 16, 3, 1, 1, 0), (1, 16, 0, 1, 24, 40, 16, 3, 1, 1, 1), (2, 64, 0, 1, 10, 14, 80, 3, 1, 1, 0)]
# the carried layers: spec, bias column, scale, accumulate, expected zl.  Quads (Cout x ceil(columns / 4)): 9216 = 144 x 64; 6960 = 27 x 256 + 48;
# 3504 = 54 x 64 + 48 -- the last work item of B and of C is partly empty
CARRIED = [((2, 64, 0, 1, 32, 40, 64, 3, 1, 1, 0), False, True, 0, 8),
           ((2, 64, 0, 1, 12, 20, 48, 3, 1, 1, 1), True, False, 1, 2),
           ((2, 32, 0, 1, 32, 40, 48, 3, 1, 1, 1), True, True, 0, 8)]


def _geom(spec):
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = spec
    return Cx + Cs, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
                                         and torch.equal(torch.isnan(a), torch.isnan(b)))


def _copy_desc(d):
    from e2ehip import _lib as L
    return L.WgradReduceDesc.from_buffer_copy(bytes(d))


# -- the carried layers: their backward-weight GEMMs run ONCE; every test reads the slabs, none writes them ----------------------------------
@functools.lru_cache(maxsize=None)
def _carried():
    from e2ehip import _lib as L
    lib = L.load()
    out = []
    for i, (spec, bias, scaled, acc, zl) in enumerate(CARRIED):
        B, Cx, Cs, up, H, W, Cout, k, s, p, pm = spec
        Cin, Ho, Wo = _geom(spec)
        g = torch.Generator().manual_seed(100 + i)
        da = torch.randn(B, Ho, Wo, Cout, generator=g).to(DEV)
        src0 = torch.randn(B, H, W, Cx, generator=g).to(DEV)
        scale = (torch.rand(Cout, generator=g) + 0.5).to(DEV) if scaled else None
        n_dw = Cout * Cin * k * k
        dw0, db0 = torch.randn(n_dw, generator=g).to(DEV), torch.randn(Cout, generator=g).to(DEV)      # what accumulate = 1 adds to
        slabs = torch.empty(lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, 1 if bias else 0), device=DEV)
        d = L.WgradReduceDesc()
        L.call("e2e_conv2d_bwd_weight_scaled_deferred", L.ptr(da), L.ptr(scale), L.ptr(src0), None, Cx, up, L.ptr(dw0), L.ptr(db0) if bias else None, L.ptr(slabs),
               B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, acc, 0.0, 1.0, ctypes.byref(d), L.stream())
        assert d.zl == zl and (d.S >= 8) == (zl == 8), f"carried layer {i}: zl {d.zl}, {d.S} slabs"
        assert bool(d.has_bias) == bias and bool(d.scale) == scaled and d.accumulate == acc
        out.append(dict(desc=d, slabs=slabs, scale=scale, n_dw=n_dw, Cout=Cout, bias=bias, acc=acc, dw0=dw0, db0=db0))
    torch.cuda.synchronize()
    quads = [c["Cout"] * ((c["desc"].KH * c["desc"].KW * c["desc"].Cin + c["desc"].has_bias + 3) // 4) for c in out]
    assert quads[0] % 64 == 0 and quads[1] % 256 not in (0, 64, 128, 192) and quads[2] % 64 != 0
    return out


class _Table:
    """A prepared device table over the carried layers with OUTPUT buffers of its own (NaN-prefilled, or the accumulate layers' start
    values; SENTINEL NaNs behind each) -- and, for the reference, slab copies of its own."""

    def __init__(self, copy_slabs=False):
        from e2ehip import _lib as L
        layers = _carried()
        self.keep, self.outs, descs = [], [], []
        for c in layers:
            dw = torch.full((c["n_dw"] + SENTINEL,), float("nan"), device=DEV)
            db = torch.full((c["Cout"] + SENTINEL,), float("nan"), device=DEV) if c["bias"] else None
            if c["acc"]:
                dw[:c["n_dw"]] = c["dw0"]
                if db is not None:
                    db[:c["Cout"]] = c["db0"]
            d = _copy_desc(c["desc"])
            d.dw, d.dbias = dw.data_ptr(), db.data_ptr() if db is not None else None
            if copy_slabs:
                self.keep.append(c["slabs"].clone())
                d.slabs = self.keep[-1].data_ptr()
            descs.append(d)
            self.outs.append((dw, db))
        self.n = len(descs)
        arr = (L.WgradReduceDesc * self.n)(*descs)
        self.total = L.load().e2e_wgrad_reduce_batch_prepare(arr, self.n)
        assert self.total > 0
        self.firsts = [d.first_item for d in arr] + [self.total]
        self.dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)

    def untouched(self, i):
        """layer i's outputs are what they were before any launch"""
        c, (dw, db) = _carried()[i], self.outs[i]
        if c["acc"]:
            return torch.equal(dw[:c["n_dw"]], c["dw0"]) and torch.isnan(dw[c["n_dw"]:]).all() and (db is None or torch.equal(db[:c["Cout"]], c["db0"]))
        return bool(torch.isnan(dw).all()) and (db is None or bool(torch.isnan(db).all()))


@functools.lru_cache(maxsize=None)
def _reference_table():
    """what ONE e2e_wgrad_reduce_batched launch writes from copies of the carried layers' slabs"""
    from e2ehip import _lib as L
    t = _Table(copy_slabs=True)
    L.call("e2e_wgrad_reduce_batched", L.ptr(t.dev), t.n, t.total, L.stream())
    torch.cuda.synchronize()
    for i, (dw, db) in enumerate(t.outs):
        n = _carried()[i]["n_dw"]
        assert not torch.isnan(dw[:n]).any() and torch.isnan(dw[n:]).all()
        assert db is None or (not torch.isnan(db[:-SENTINEL]).any() and torch.isnan(db[-SENTINEL:]).all())
    return t


def _layers_equal(t, which, msg):
    ref = _reference_table()
    for i in range(t.n):
        if i in which:
            for name, a, b in zip(("dW", "db"), t.outs[i], ref.outs[i]):
                assert _same(a, b), f"{msg}: {name} of carried layer {i} differs from e2e_wgrad_reduce_batched"
        else:
            assert t.untouched(i), f"{msg}: carried layer {i} lies outside the range and was written"


# -- the carrier --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _carrier_inputs(spec):
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = spec
    Cin, Ho, Wo = _geom(spec)
    g = torch.Generator().manual_seed(11)
    t = dict(spec=spec)
    t["da"] = torch.randn(B, Ho, Wo, Cout, generator=g).to(DEV)
    t["wb"] = torch.randn(k * k * Cout, (Cin + 3) // 4 * 4, generator=g).to(DEV)
    t["src0"] = torch.randn(B, H // up, W // up, Cx, generator=g).to(DEV)
    t["src1"] = torch.randn(B, H, W, Cs, generator=g).to(DEV) if Cs else None
    t["scale"] = (torch.rand(Cout, generator=g) + 0.5).to(DEV) if not pm else None
    pp = p if pm else 0
    t["dx_shape"] = (B, H + 2 * pp, W + 2 * pp, Cin)
    return t


def _run_carrier(spec, order, carry=None, expect_error=False):
    """The pair entry point on a carrier (carry None: e2e_conv2d_bwd_pair_deferred; else (table pointer, n, first item, items, place) for
    e2e_conv2d_bwd_pair_carry), then the carrier's own slab reduction: (dx, dW, db) with their sentinels."""
    from e2ehip import _lib as L
    lib = L.load()
    t = _carrier_inputs(spec)
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = spec
    Cin, Ho, Wo = _geom(spec)
    n_dx = B * t["dx_shape"][1] * t["dx_shape"][2] * Cin
    dx = torch.full((n_dx + SENTINEL,), float("nan"), device=DEV)
    n_wsb = lib.e2e_conv2d_bwd_data_workspace_floats(B, t["dx_shape"][1], t["dx_shape"][2], Cin, k * k * Cout, s)
    wsb = torch.zeros(max(n_wsb, 1), device=DEV)
    wsw = torch.empty(lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, 1 if pm else 0), device=DEV)
    dw = torch.full((Cout * Cin * k * k + SENTINEL,), float("nan"), device=DEV)
    db = torch.full((Cout + SENTINEL,), float("nan"), device=DEV) if pm else None
    d = L.WgradReduceDesc()
    args = [L.ptr(t["da"]), L.ptr(t["wb"]), t["wb"].shape[1], L.ptr(dx), B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, 0, None, 0, None,
            L.ptr(wsb if n_wsb else None), L.ptr(t["scale"]), L.ptr(t["src0"]), L.ptr(t["src1"]), Cx, up, L.ptr(dw), L.ptr(db), L.ptr(wsw), 0, 0.0, 1.0,
            ctypes.byref(d), order]
    if carry is None:
        L.call("e2e_conv2d_bwd_pair_deferred", *args, L.stream())
    elif expect_error:
        with pytest.raises(L.E2EError, match=r"failed \(-1\)"):
            L.call("e2e_conv2d_bwd_pair_carry", *args, *carry, L.stream())
        torch.cuda.synchronize()
        return dx, dw, db
    else:
        L.call("e2e_conv2d_bwd_pair_carry", *args, *carry, L.stream())
    arr = (L.WgradReduceDesc * 1)(d)
    total = lib.e2e_wgrad_reduce_batch_prepare(arr, 1)
    own = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.call("e2e_wgrad_reduce_batched", L.ptr(own), 1, total, L.stream())
    torch.cuda.synchronize()
    return dx, dw, db


@functools.lru_cache(maxsize=None)
def _carrier_reference(spec, order):
    ref = _run_carrier(spec, order)
    assert torch.isnan(ref[0][-SENTINEL:]).all() and torch.isnan(ref[1][-SENTINEL:]).all() and not torch.isnan(ref[1][:-SENTINEL]).any()
    return ref


def _carrier_equal(out, spec, order, msg):
    for name, a, b in zip(("dx", "dW", "db"), out, _carrier_reference(spec, order)):
        assert _same(a, b), f"{msg}: the carrier's {name} differs from e2e_conv2d_bwd_pair_deferred"


def _query(spec):
    from e2ehip import _lib as L
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = spec
    Cin, Ho, Wo = _geom(spec)
    pp = p if pm else 0
    n_wsb = L.load().e2e_conv2d_bwd_data_workspace_floats(B, H + 2 * pp, W + 2 * pp, Cin, k * k * Cout, s)
    return L.query("e2e_conv2d_bwd_pair_is_one_launch", ld_bwd=(Cin + 3) // 4 * 4, B=B, Hs=H, Ws=W, Cin=Cin, Cout=Cout, Ho=Ho, Wo=Wo, KH=k, KW=k, stride=s, pad=p,
                   pad_mode=pm, accumulate=0, in_act=0, has_pre_add=0, has_workspace=1 if n_wsb else 0, has_src1=1 if Cs else 0, C1=Cx, up=up, has_bias=1 if pm else 0)


# 1. carried reductions equal the batched launch; the carrier's own results equal the plain paired call
@pytest.mark.parametrize("place", (0, 1, 2))
@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("spec", CARRIERS + WIDE, ids=[f"carrier{i}" for i in range(len(CARRIERS))] + [f"wide{i}" for i in range(len(WIDE))])
def test_carried_reductions_equal_the_batched_launch(spec, order, place):
    from e2ehip import _lib as L
    t = _Table()
    out = _run_carrier(spec, order, (L.ptr(t.dev), t.n, 0, t.total, place))
    _layers_equal(t, {0, 1, 2}, f"{spec} order {order} place {place}")
    _carrier_equal(out, spec, order, f"{spec} order {order} place {place}")


# 2. a range inside the table touches its own layers only
@pytest.mark.parametrize("spec", (CARRIERS[0], CARRIERS[2]), ids=("one_launch", "two_launches"))
def test_sub_range_touches_only_its_layers(spec):
    from e2ehip import _lib as L
    t = _Table()
    out = _run_carrier(spec, 0, (L.ptr(t.dev), t.n, t.firsts[1], t.firsts[2] - t.firsts[1], 0))
    _layers_equal(t, {1}, f"{spec} middle layer")
    _carrier_equal(out, spec, 0, f"{spec} middle layer")


# 3. no carried items: the plain paired call (the table may be absent)
@pytest.mark.parametrize("order", (0, 1))
def test_no_carried_items_is_the_plain_pair_call(order):
    from e2ehip import _lib as L
    for spec in (CARRIERS[0], CARRIERS[3]):
        _carrier_equal(_run_carrier(spec, order, (None, 0, 0, 0, 1)), spec, order, f"{spec} without items")
    t = _Table()
    _carrier_equal(_run_carrier(CARRIERS[1], order, (L.ptr(t.dev), t.n, t.firsts[1], 0, 2)), CARRIERS[1], order, "empty range of a table")
    _layers_equal(t, set(), "empty range of a table")


# 4. a carrier whose GEMMs do not pair: the range runs as a launch of its own
@pytest.mark.parametrize("place", (0, 1, 2))
def test_fallback_carrier(place):
    from e2ehip import _lib as L
    spec = FALLBACK[0]
    t = _Table()
    out = _run_carrier(spec, 0, (L.ptr(t.dev), t.n, 0, t.total, place))
    _layers_equal(t, {0, 1, 2}, f"fallback carrier place {place}")
    _carrier_equal(out, spec, 0, f"fallback carrier place {place}")


# 5. the query (host only)
def test_query_one_launch():
    for spec in ONE_LAUNCH:
        assert _query(spec) == 1, f"{spec} runs as one k_conv_bwd_pair launch"
    for spec in FALLBACK + [CARRIERS[2], CARRIERS[3]]:
        assert _query(spec) == 0, f"{spec} runs as two launch sequences"
    B, Cx, Cs, up, H, W, Cout, k, s, p, pm = CARRIERS[0]
    from e2ehip import _lib as L
    assert L.load().e2e_conv2d_bwd_pair_is_one_launch(60, B, H, W, 64, 64, H, W, 3, 3, 1, 1, 0, 0, 0, 0, 1, 0, 64, 1, 0) == 0     # ld_bwd < Cin: refused


# 6. the range form of the batched reduction
def test_range_form_equals_the_batched_launch():
    from e2ehip import _lib as L
    t = _Table()
    L.call("e2e_wgrad_reduce_batched_range", L.ptr(t.dev), t.n, 0, t.total, L.stream())
    torch.cuda.synchronize()
    _layers_equal(t, {0, 1, 2}, "whole table")
    for cut in (t.firsts[1], t.firsts[1] + 3, t.firsts[2] - 1, 1, t.total - 1):      # on a layer boundary, inside the zl = 2 layer, inside the zl = 8 layers
        t = _Table()
        L.call("e2e_wgrad_reduce_batched_range", L.ptr(t.dev), t.n, cut, t.total - cut, L.stream())
        L.call("e2e_wgrad_reduce_batched_range", L.ptr(t.dev), t.n, 0, cut, L.stream())
        torch.cuda.synchronize()
        _layers_equal(t, {0, 1, 2}, f"ranges [0, {cut}) + [{cut}, {t.total})")
    t = _Table()
    L.call("e2e_wgrad_reduce_batched_range", L.ptr(t.dev), t.n, t.firsts[1], t.firsts[2] - t.firsts[1], L.stream())
    torch.cuda.synchronize()
    _layers_equal(t, {1}, "middle layer")
    for bad in ((None, 3, 0, 1), (L.ptr(t.dev), t.n, -1, 2), (L.ptr(t.dev), t.n, 0, 0), (L.ptr(t.dev), 0, 0, 1)):
        with pytest.raises(L.E2EError, match=r"failed \(-1\)"):
            L.call("e2e_wgrad_reduce_batched_range", *bad, L.stream())


# 7. the launch plan
class _Names:
    """stands in for e2ehip.profile.KernelTimer: records which entry points the plan calls"""

    def __init__(self):
        self.names = []

    def around(self, name, args, fn):
        self.names.append(name)
        return fn()


def _plan_run(carry, monkeypatch, B=2, H=64, W=96):
    """A one-stream NetPlan: the gradient bucket after the first eager pass, after a second one, replayed from a captured graph, and the
    bucket after backward_late_layers() alone (on a NaN-filled bucket) -- plus the entry points the second eager pass called."""
    from e2ehip import _lib as L
    from e2ehip.netplan import NetPlan
    from depth_estimation.networks import DispResNet_Indoor
    monkeypatch.setenv("E2E_PAIRED_BWD", "1")
    monkeypatch.setenv("E2E_CARRY_REDUCE", "1" if carry else "0")
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
    assert plan.carry == carry
    params = plan.parameters()

    def bucket():
        torch.cuda.synchronize()
        return [plan.sink(q).clone() for q in params]

    plan.refresh_layouts()
    plan.forward(x)
    plan.backward(gd)                                        # builds the two reduction tables
    first = bucket()
    rec = _Names()
    monkeypatch.setattr(L, "PROFILE_HOOK", [rec])
    plan.forward()
    plan.backward()
    monkeypatch.setattr(L, "PROFILE_HOOK", [None])
    second = bucket()
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
    for q in params:
        plan.sink(q).zero_()
    plan.x.t.copy_(x)
    plan.disp.g.copy_(gd.reshape(plan.disp.g.shape))
    graph.replay()
    replayed = bucket()
    del graph
    late_ids = set()
    for op in plan.ops[plan.split_index:]:
        for q in (getattr(op, "weight", None), getattr(op, "bias", None), *((op.bn.weight, op.bn.bias) if hasattr(op, "bn") else ())):
            if q is not None:
                late_ids.add(id(q))
    for q in params:
        plan.sink(q).fill_(float("nan"))
    plan.forward()
    plan.backward_late_layers()
    late_only = bucket()
    plan.backward_early_layers()
    final = bucket()
    is_late = [id(q) in late_ids for q in params]
    plan.close()
    return dict(first=first, second=second, replayed=replayed, late_only=late_only, final=final, is_late=is_late, names=rec.names)


def test_plan_carried_and_batched_gradients_identical(monkeypatch):
    c, b = _plan_run(True, monkeypatch), _plan_run(False, monkeypatch)
    # the carrying plan did carry, in both halves, and its left-overs went through the range form; the other plan ran today's launches
    assert c["names"].count("e2e_conv2d_bwd_pair_carry") >= 10 and c["names"].count("e2e_wgrad_reduce_batched_range") == 2
    assert "e2e_wgrad_reduce_batched" not in c["names"]
    assert b["names"].count("e2e_wgrad_reduce_batched") == 2 and "e2e_conv2d_bwd_pair_carry" not in b["names"] and "e2e_wgrad_reduce_batched_range" not in b["names"]
    assert len(c["first"]) == len(b["first"]) > 0 and any(c["is_late"]) and not all(c["is_late"])
    for i in range(len(c["first"])):
        ref = b["first"][i]
        assert not torch.isnan(ref).any()
        for run in (c, b):
            for key in ("first", "second", "replayed", "final"):
                assert torch.equal(run[key][i], ref), f"parameter {i}: {key} bucket (E2E_CARRY_REDUCE={int(run is c)}) differs"
            if run["is_late"][i]:
                assert torch.equal(run["late_only"][i], ref), f"late parameter {i} is not complete after backward_late_layers()"


# 8. argument errors: the library's error code, nothing launched
def test_argument_errors_launch_nothing():
    from e2ehip import _lib as L
    t = _Table()
    spec = CARRIERS[0]
    for carry in ((None, t.n, 0, 5, 0), (L.ptr(t.dev), 0, 0, 5, 0), (L.ptr(t.dev), t.n, 0, -1, 0), (L.ptr(t.dev), t.n, -2, 4, 0), (L.ptr(t.dev), t.n, 0, 5, 3)):
        dx, dw, db = _run_carrier(spec, 0, carry, expect_error=True)
        assert torch.isnan(dx).all() and torch.isnan(dw).all(), f"{carry[1:]}: a refused call wrote the carrier's outputs"
        _layers_equal(t, set(), f"refused call {carry[1:]}")
