"""e2e_conv2d_fwd_entry_pair (a stage entry's conv1, its 1x1 downsample convolution, the BatchNorm fold and the affine as ONE launch) against the
four calls it replaces -- e2e_conv2d_fwd (3x3 stride 2 + frozen-BN scale / shift + ReLU), e2e_conv2d_fwd (1x1 stride 2, plain), e2e_bn_fold,
e2e_affine_fwd -- in the same build: every tile runs the arithmetic of its own launch and the 1x1 part's epilogue evaluates the expressions
of the two small kernels, so conv1's output, z, the affine output and scale / shift / rstd must be equal BIT FOR BIT (torch.equal + equal NaN
masks; a NaN sentinel region behind every output).  Also against float64 (torch.nn.functional on the CPU) with the forward bound of
tests/test_gpu_conv.py: max |y - y64| / max |y64| < 2e-5."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
EPS = 1e-5

# B, Cin, Cout, H, W of the block input; the query's answer
SMALL = [
    ((2, 64, 128, 12, 20), 1),       # 6 x 10 output, one ragged row tile
    ((1, 64, 128, 13, 9), 1),        # odd sizes, 7 x 5 output
    ((2, 256, 512, 6, 8), 1),        # conv1 deep enough for split-K, the 1x1 branch unsplit
    ((1, 128, 256, 30, 40), 1),
    ((1, 64, 144, 12, 20), 1),       # a ragged column tile: columns past Cout in the second 128-wide tile
]
NETWORK = [((2, 64, 128, 120, 160), 1), ((2, 128, 256, 60, 80), 1), ((2, 256, 512, 30, 40), 1)]
REFUSED = [((2, 64, 80, 12, 20), 0)]       # Cout % 32 != 0 and below 128 columns: 64 x 64 tiles, the four launches


def _inputs(spec, seed=1):
    B, Cin, Cout, H, W = spec
    g = torch.Generator().manual_seed(seed)
    t = dict(spec=spec, Ho=(H - 1) // 2 + 1, Wo=(W - 1) // 2 + 1)
    t["x"] = torch.randn(B, H, W, Cin, generator=g)
    t["w1"] = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    t["wd"] = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    t["scale1"] = torch.rand(Cout, generator=g) + 0.5
    t["shift1"] = torch.randn(Cout, generator=g)
    t["gamma"] = torch.rand(Cout, generator=g) * 0.4 + 0.8
    t["beta"] = torch.randn(Cout, generator=g)
    t["mean"] = torch.randn(Cout, generator=g)
    t["var"] = torch.rand(Cout, generator=g) + 0.5
    t["dev"] = {k: v.to(DEV) for k, v in t.items() if torch.is_tensor(v)}
    return t


def _layouts(t):
    from e2ehip import _lib as L
    B, Cin, Cout, H, W = t["spec"]
    ld = (Cout + 3) // 4 * 4
    wf1, wfd = torch.zeros(9 * Cin, ld, device=DEV), torch.zeros(Cin, ld, device=DEV)
    L.call("e2e_conv_weight_layouts", L.ptr(t["dev"]["w1"]), Cout, Cin, 3, 3, L.ptr(wf1), ld, None, 0, L.stream())
    L.call("e2e_conv_weight_layouts", L.ptr(t["dev"]["wd"]), Cout, Cin, 1, 1, L.ptr(wfd), ld, None, 0, L.stream())
    return wf1, wfd, ld


def _buf(n):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV)


def _run(t, how, slot=None, nbatch=None):
    """how: 'separate' (the four entry points) or 'pair'.  slot: B = 1 launched on image `slot` of `nbatch`-image buffers.
    Returns the six output buffers (with their sentinel regions): out1, z, y, scale, shift, rstd."""
    from e2ehip import _lib as L
    lib = L.load()
    B, Cin, Cout, H, W = t["spec"]
    Ho, Wo, d = t["Ho"], t["Wo"], t["dev"]
    wf1, wfd, ld = _layouts(t)
    nb = B if slot is None else nbatch
    n_img = Ho * Wo * Cout
    out1, z, y = _buf(nb * n_img), _buf(nb * n_img), _buf(nb * n_img)
    sc, sh, rs = _buf(Cout), _buf(Cout), _buf(Cout)
    n_ws = lib.e2e_conv2d_splitk_workspace_floats(B * Ho * Wo, Cout, 9 * Cin)
    ws = torch.zeros(n_ws, device=DEV) if n_ws else None
    x = d["x"] if slot is None else torch.cat([torch.randn_like(d["x"])] * slot + [d["x"]] + [torch.randn_like(d["x"])] * (nbatch - slot - 1))
    at = (lambda b: L.ptr(b)) if slot is None else (lambda b: L.ptr(b[slot * n_img:]))
    xp = L.ptr(x) if slot is None else L.ptr(x[slot])
    st = L.stream()
    if how == "separate":
        L.call("e2e_conv2d_fwd", xp, None, Cin, 1, L.ptr(wf1), ld, L.ptr(d["scale1"]), L.ptr(d["shift1"]), None, at(out1), B, H, W, Cin, Cout, 3, 3, 2, 1, 0, 1,
               0.0, 1.0, L.ptr(ws), st)
        L.call("e2e_conv2d_fwd", xp, None, Cin, 1, L.ptr(wfd), ld, None, None, None, at(z), B, H, W, Cin, Cout, 1, 1, 2, 0, 0, 0, 0.0, 1.0, None, st)
        L.call("e2e_bn_fold", L.ptr(d["gamma"]), L.ptr(d["beta"]), L.ptr(d["mean"]), L.ptr(d["var"]), EPS, L.ptr(sc), L.ptr(sh), L.ptr(rs), Cout, st)
        zs = z if slot is None else z[slot * n_img:]
        L.call("e2e_affine_fwd", L.ptr(zs), L.ptr(sc), L.ptr(sh), None, 0, at(y), B * n_img, Cout, st)
    else:
        L.call("e2e_conv2d_fwd_entry_pair", x=xp, w1_fwd=L.ptr(wf1), ld1=ld, scale1=L.ptr(d["scale1"]), shift1=L.ptr(d["shift1"]), out1=at(out1), act1=1,
               workspace1=L.ptr(ws), wd_fwd=L.ptr(wfd), ldd=ld, gamma=L.ptr(d["gamma"]), beta=L.ptr(d["beta"]), running_mean=L.ptr(d["mean"]),
               running_var=L.ptr(d["var"]), eps=EPS, bn_scale=L.ptr(sc), bn_shift=L.ptr(sh), bn_rstd=L.ptr(rs), z=at(z), y=at(y), B=B, Hs=H, Ws=W, Cin=Cin,
               Cout=Cout, KH=3, KW=3, stride=2, pad=1, stream=st)
    torch.cuda.synchronize()
    return out1, z, y, sc, sh, rs


NAMES = ("conv1 output", "z", "affine output", "scale", "shift", "rstd")


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def _query(spec):
    from e2ehip import _lib as L
    B, Cin, Cout, H, W = spec
    n_ws = L.load().e2e_conv2d_splitk_workspace_floats(B * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1), Cout, 9 * Cin)
    ld = (Cout + 3) // 4 * 4
    return L.query("e2e_conv2d_fwd_entry_pair_is_one_launch", ld1=ld, ldd=ld, has_workspace1=1 if n_ws else 0, B=B, Hs=H, Ws=W, Cin=Cin, Cout=Cout, KH=3, KW=3,
                   stride=2, pad=1)


def _ref64(t):
    """float64 on the CPU: conv1 + scale / shift + ReLU, the 1x1 branch, the folded BatchNorm vectors, the affine -- NHWC like the kernels' outputs"""
    x = t["x"].double().permute(0, 3, 1, 2)
    o1 = F.relu(F.conv2d(x, t["w1"].double(), None, 2, 1) * t["scale1"].double().view(1, -1, 1, 1) + t["shift1"].double().view(1, -1, 1, 1))
    z = F.conv2d(x, t["wd"].double(), None, 2, 0)
    rstd = 1.0 / torch.sqrt(t["var"].double() + EPS)
    scale = t["gamma"].double() * rstd
    shift = t["beta"].double() - t["mean"].double() * scale
    y = z * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().flatten()
    return nhwc(o1), nhwc(z), nhwc(y), scale, shift, rstd


def _check(spec, expect_one_launch, with_ref64=True):
    t = _inputs(spec)
    assert _query(spec) == expect_one_launch, f"{spec}: the query's answer"
    ref = _run(t, "separate")
    out = _run(t, "pair")
    for name, a, b in zip(NAMES, out, ref):
        assert torch.isnan(b[-SENTINEL:]).all() and not torch.isnan(b[:-SENTINEL]).any(), f"{spec}: {name} of the separate launches"
        assert _same(a, b), f"{spec}: {name} differs from the separate launches"
    if with_ref64:
        for name, a, r in zip(NAMES, out, _ref64(t)):
            err = ((a[:-SENTINEL].double().cpu() - r).abs().max() / r.abs().max()).item()
            print(f"{spec} {name}: {err:.2e} of max |reference|")
            assert err < 2e-5, f"{spec}: {name} against float64: {err:.2e}"


@pytest.mark.parametrize("spec,one", SMALL, ids=[f"small{i}" for i in range(len(SMALL))])
def test_small_shapes_bit_identical(spec, one):
    _check(spec, one)


@pytest.mark.parametrize("spec,one", NETWORK, ids=[f"net{i}" for i in range(len(NETWORK))])
def test_network_shapes_bit_identical(spec, one):
    _check(spec, one)


@pytest.mark.parametrize("spec,one", REFUSED, ids=[f"refused{i}" for i in range(len(REFUSED))])
def test_refused_shape_same_results_through_the_fallback(spec, one):
    _check(spec, one)


@pytest.mark.parametrize("spec", [(1, 64, 128, 12, 20), (1, 256, 512, 6, 8)], ids=["unsplit", "splitk"])
def test_slot_form_leaves_the_other_image_untouched(spec):
    """B = 1 launched on image 1 of B = 2 buffers -- the launch arguments NetPlan.forward_one replays: image 1 equals the separate launches on the same
    slot and a whole-buffer B = 1 run, image 0 keeps its NaN fill."""
    t = _inputs(spec, seed=2)
    assert _query(spec) == 1
    n_img = t["Ho"] * t["Wo"] * spec[2]
    ref = _run(t, "separate", slot=1, nbatch=2)
    out = _run(t, "pair", slot=1, nbatch=2)
    whole = _run(t, "pair")
    for name, a, b, w in zip(NAMES, out, ref, whole):
        assert _same(a, b), f"{spec}: {name} differs from the separate launches"
    for name, a, w in zip(NAMES[:3], out[:3], whole[:3]):
        assert torch.isnan(a[:n_img]).all(), f"{spec}: {name} of image 0 was written"
        assert torch.equal(a[n_img:2 * n_img], w[:n_img]) and torch.isnan(a[2 * n_img:]).all()


def test_run_to_run_bit_equality():
    t = _inputs(NETWORK[2][0], seed=3)
    a, b = _run(t, "pair"), _run(t, "pair")
    for x, y in zip(a, b):
        assert _same(x, y)


def test_query_matches_the_kernels_launched():
    """The kernels a call launches, as the profiler records them: k_conv_fwd_pair alone (plus conv1's split-K epilogue) where the query says one
    launch, the two GEMMs + k_bn_fold + k_affine_fwd where it says fallback."""
    from torch.profiler import ProfilerActivity, profile
    for spec, one in (SMALL[0], SMALL[2], REFUSED[0]):
        t = _inputs(spec)
        _run(t, "pair")                                                      # (layouts and buffers once outside the recorded region's interest)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            _run(t, "pair")
        names = [e.name for e in prof.events() if e.name.startswith(("k_", "void k_"))]
        assert any("k_weight_layouts" in n for n in names), "the profiler recorded no kernel of the library"
        pair = sum("k_conv_fwd_pair" in n for n in names)
        small = sum(("k_bn_fold" in n) or ("k_affine_fwd" in n) for n in names)
        gemms = sum("k_conv_gemm" in n for n in names)
        assert _query(spec) == one
        assert (pair, small, gemms) == ((1, 0, 0) if one else (0, 2, 2)), f"{spec}: query {one}, launched {names}"


def test_refusals():
    from e2ehip import _lib as L
    t = _inputs((1, 64, 128, 12, 20))
    d = t["dev"]
    wf1, wfd, ld = _layouts(t)
    o = torch.empty(6 * 10 * 128, device=DEV)
    v = torch.empty(128, device=DEV)
    kw = dict(x=L.ptr(d["x"]), w1_fwd=L.ptr(wf1), ld1=ld, scale1=L.ptr(d["scale1"]), shift1=L.ptr(d["shift1"]), out1=L.ptr(o), act1=1, workspace1=None,
              wd_fwd=L.ptr(wfd), ldd=ld, gamma=L.ptr(d["gamma"]), beta=L.ptr(d["beta"]), running_mean=L.ptr(d["mean"]), running_var=L.ptr(d["var"]), eps=EPS,
              bn_scale=L.ptr(v), bn_shift=L.ptr(v), bn_rstd=L.ptr(v), z=L.ptr(o), y=L.ptr(o), B=1, Hs=12, Ws=20, Cin=64, Cout=128, KH=3, KW=3, stride=2, pad=1,
              stream=L.stream())
    for bad in (dict(x=None), dict(gamma=None), dict(y=None), dict(ldd=126), dict(stride=3), dict(KH=3, KW=3, pad=0)):
        with pytest.raises(L.E2EError):
            L.call("e2e_conv2d_fwd_entry_pair", **{**kw, **bad})
    torch.cuda.synchronize()
    assert L.query("e2e_conv2d_fwd_entry_pair_is_one_launch", ld1=126, ldd=ld, has_workspace1=0, B=1, Hs=12, Ws=20, Cin=64, Cout=128, KH=3, KW=3, stride=2, pad=1) == 0
