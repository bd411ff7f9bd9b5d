"""The five entry points of csrc/warp_photo_fused.hip -- the launch every refinement step makes -- called directly through the C ABI, against
the float64 composition that include/e2eslam.h promises for them (tests/lossgrad_contract_ref.py on top of tests/warp_contract_ref.py):

  A. e2e_warp_photo_lossgrad_workspace_floats: 0 for a non-positive size, else the header's formula;
  B. e2e_warp_photo_lossgrad: six shapes x both paddings x use_mask 0/1 x reg_kind 0/1/2 x three (w_photo, w_reg) pairs (w_photo = 0 and
     w_reg = 0 among them) x channels-last, contiguous and one-image-behind-the-batch frames; loss_out NULL;
  C. e2e_warp_photo_lossgrad_hostgeo: the B = 1 shapes, both paddings, mask 0/1, reg_kind 0/2, the geometry formed in float64 on the host;
  D. e2e_warp_photo_lossgrad_chain / _chain_flush: four steps with four different losses over the slot sets 6, 7, 0, 1, each loss arriving one
     launch late; more workgroups than slots at (3,49,161); the overflow flag tripped by values alone and cleared again;
  E. the calls the header rules out: E2EError before any launch, every output, the loss and the whole workspace as they were.

Every output is NaN-filled and followed by a 64-element sentinel; the workspace is allocated at exactly the size its query returns, plus a
sentinel.  After each call: every output fully written, nothing behind it touched, a second identical call bit-identical.  Bounds and
exclusions come from the references alone (tests/lossgrad_contract_ref.py states the rule); tests/test_lossgrad_contract_inputs.py proves
the excluded shares and the shapes' properties without a GPU.  profiles/lossgrad_contracts.txt holds the measured errors as fractions of
their bounds."""
import ctypes
import time

import pytest
import torch

import lossgrad_contract_ref as G
import warp_contract_ref as R
from warp_contract_ref import F64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
WORST = {}
LAYOUTS = {"same": 0, "differ": 0}                                    # nhwc against nchw, bit for bit: recorded, not asserted
W_CHAIN = R.G_LOSS[0]


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


@pytest.fixture(scope="module", autouse=True)
def _report():
    t0 = time.perf_counter()
    yield
    print()
    for section, name in sorted(WORST):
        ratio, e, bnd, what = WORST[section, name]
        print(f"lossgrad contracts {section} {name}: largest error / bound = {ratio:.3f} ({e:.2e} of {bnd:.2e} at {what})")
    print(f"lossgrad contracts: channels-last and contiguous frames bit-identical in {LAYOUTS['same']} of {LAYOUTS['same'] + LAYOUTS['differ']} calls")
    print(f"lossgrad contracts: module time {time.perf_counter() - t0:.1f} s")


def _nan(n):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=torch.float32)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _untouched(buf, what):
    assert torch.isnan(buf).all(), f"{what}: written although it was not asked for"


def _dev(t):
    return t.contiguous().to(DEV)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _check(section, what, dev, r64, bnd, keep=None):
    err = (dev.double().reshape(r64.shape) - r64).abs()
    if keep is not None:
        err = err[keep]
    e = float(err.max()) if err.numel() else 0.0
    ratio = e / bnd if bnd > 0 else (0.0 if e == 0 else float("inf"))
    key = (section, what.split(" | ")[-1].split(",")[0])
    if ratio >= WORST.get(key, (-1.0, ""))[0]:
        WORST[key] = (ratio, e, bnd, what)
    assert e <= bnd, f"{section} {what}: max|gpu - r64| = {e:.3e} > bound {bnd:.3e} ({ratio:.2f} x)"


def _operands(s, layout):
    """the scene on the device; frames channels-last, contiguous, or one image behind every batch element (batch stride 0)"""
    o = {k: _dev(s[k]) for k in ("depth", "d_src", "ri_t", "ri_s", "K", "invK", "T")}
    for k in ("src", "tgt"):
        if layout == "nhwc":
            o[k] = _nhwc(s[k].to(DEV))
        elif layout == "expand":
            o[k] = _dev(s[k][:1]).expand(s["B"], -1, -1, -1)
            assert o[k].stride(0) == 0
        else:
            o[k] = _dev(s[k])
    return o


def _geo12(s):
    """geometry12_host of the scene (B = 1): host memory"""
    return (ctypes.c_float * 12)(*[float(v) for v in G.geometry12(s, "host")[0]])


def _reg_ptrs(L, o, reg_kind):
    return (L.ptr(o["ri_t"]), L.ptr(o["ri_s"]), L.ptr(o["d_src"])) if reg_kind else (None, None, None)


def _lossgrad(L, o, shape, pad, use_mask, reg_kind, w, geo=None, want_loss=True, tag=""):
    """e2e_warp_photo_lossgrad (geo None) or _hostgeo, twice on fresh buffers: g_depth_tgt fully written, g_depth_src fully written with a
    regulariser and untouched without, loss_out written when given, every sentinel and the workspace's intact, the two calls bit-identical
    -> dict(g_dt, g_ds, loss) of CPU tensors"""
    B, H, W = shape
    N = B * H * W
    nws = L.query("e2e_warp_photo_lossgrad_workspace_floats", B, H, W)
    ss, ts = L.strides4(o["src"]), L.strides4(o["tgt"])
    runs = []
    for _ in range(2):
        b = dict(g_dt=_nan(N), g_ds=_nan(N), loss=_nan(2), ws=_nan(nws))
        tail = (use_mask, pad, reg_kind, *_reg_ptrs(L, o, reg_kind), w[0], w[1], L.ptr(b["loss"]) if want_loss else None, L.ptr(b["g_dt"]), L.ptr(b["g_ds"]), L.ptr(b["ws"]))
        if geo is None:
            L.call("e2e_warp_photo_lossgrad", L.ptr(o["depth"]), L.ptr(o["src"]), ss, L.ptr(o["tgt"]), ts, L.ptr(o["K"]), L.ptr(o["invK"]), L.ptr(o["T"]), *tail, B, H, W, L.stream())
        else:
            L.call("e2e_warp_photo_lossgrad_hostgeo", L.ptr(o["depth"]), L.ptr(o["src"]), ss, L.ptr(o["tgt"]), ts, ctypes.cast(geo, ctypes.c_void_p), *tail, H, W, L.stream())
        torch.cuda.synchronize()
        _written(b["g_dt"], N, f"{tag}: g_depth_tgt")
        _written(b["g_ds"], N, f"{tag}: g_depth_src") if reg_kind else _untouched(b["g_ds"], f"{tag}: g_depth_src (reg_kind 0)")
        _written(b["loss"], 2, f"{tag}: loss_out") if want_loss else _untouched(b["loss"], f"{tag}: loss_out")
        assert torch.isnan(b["ws"][nws:]).all(), f"{tag}: workspace written past the size its query returned"
        runs.append(b)
    for k in ("g_dt", "g_ds", "loss"):
        assert _same_bits(runs[0][k], runs[1][k]), f"{tag}: {k}: two identical calls differ"
    return {k: runs[0][k][:2 if k == "loss" else N].cpu() for k in ("g_dt", "g_ds", "loss")}


def _compare(section, tag, out, c, w, form):
    """loss_out[0], loss_out[1], g_depth_tgt and g_depth_src of one call against the float64 reference of case c"""
    _check(section, f"{tag} | loss_out[0]", out["loss"][0], c[F64]["loss"], G.loss_bound(c, form))
    if c["reg_kind"]:
        _check(section, f"{tag} | loss_out[1]", out["loss"][1], c[F64]["reg"], G.reg_bound(c))
    else:
        assert float(out["loss"][1]) == 0.0, f"{tag}: loss_out[1] = {float(out['loss'][1])} without a regulariser"
    _compare_grads(section, tag, out, c, w, form)


def _compare_grads(section, tag, out, c, w, form):
    t64, s64 = R.fused_grads(c, w, F64)
    _check(section, f"{tag} | g_depth_tgt", out["g_dt"], t64, G.grad_bound(c, w, form), G.grad_keep(c, w))
    if c["reg_kind"]:
        _check(section, f"{tag} | g_depth_src", out["g_ds"], s64, G.src_grad_bound(c, w), ~c["reg_excluded_s"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. the workspace query
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_workspace_query():
    L = _L()
    for B, H, W in G.LG_SHAPES + [(1, 480, 640)]:
        n = L.query("e2e_warp_photo_lossgrad_workspace_floats", B, H, W)
        assert n == (2 * B * -(-W // 32) * -(-H // 8) + 1) // 2 * 2 + 2 * 8 * 129 == G.workspace_floats(B, H, W)
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -3, 4), (1, 4, -3)):
        assert L.query("e2e_warp_photo_lossgrad_workspace_floats", *bad) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. e2e_warp_photo_lossgrad against float64
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", G.PADS, ids=lambda p: R.PAD_NAME[p])
@pytest.mark.parametrize("shape", G.LG_SHAPES, ids=str)
def test_lossgrad(shape, pad):
    """Each frame layout is compared with float64 on its own: channels-last frames select another template instantiation under border
    padding, and under FMA contraction the two need not round alike (how often they do is printed at teardown)."""
    L = _L()
    layouts = ("nhwc", "nchw") + (("expand",) if shape in G.EXPAND_SHAPES else ())
    ops = {lay: _operands(G.expanded_scene(*shape) if lay == "expand" else R.fused_scene(*shape), lay) for lay in layouts}
    for use_mask in G.MASKS:
        for reg_kind in G.REGS:
            first = {}
            for lay in layouts:
                c = G.lg_case(shape, pad, use_mask, reg_kind, lay == "expand")
                for w in R.G_LOSS:
                    tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} reg={reg_kind} w={w} {lay}"
                    out = _lossgrad(L, ops[lay], shape, pad, use_mask, reg_kind, w, tag=tag)
                    _compare("B", tag, out, c, w, "device")
                    if lay == "nhwc":
                        first[w] = out
                    elif lay == "nchw":
                        LAYOUTS["same" if all(_same_bits(out[k], first[w][k]) for k in ("g_dt", "loss")) else "differ"] += 1
                        if w == R.G_LOSS[0]:                          # loss_out NULL: the same gradients, no second launch
                            quiet = _lossgrad(L, ops[lay], shape, pad, use_mask, reg_kind, w, want_loss=False, tag=tag + " loss_out=NULL")
                            assert _same_bits(quiet["g_dt"], out["g_dt"]), f"{tag}: g_depth_tgt depends on loss_out"
                            assert not reg_kind or _same_bits(quiet["g_ds"], out["g_ds"]), f"{tag}: g_depth_src depends on loss_out"


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. e2e_warp_photo_lossgrad_hostgeo
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", G.PADS, ids=lambda p: R.PAD_NAME[p])
@pytest.mark.parametrize("shape", G.HOSTGEO_SHAPES, ids=str)
def test_lossgrad_hostgeo(shape, pad):
    L = _L()
    s = R.fused_scene(*shape)
    geo = _geo12(s)
    for lay in ("nhwc", "nchw"):
        o = _operands(s, lay)
        for _, _, use_mask, reg_kind in [c for c in G.HOSTGEO_CASES if c[:2] == (shape, pad)]:
            c = G.lg_case(shape, pad, use_mask, reg_kind)
            for w in R.G_LOSS:
                tag = f"{shape} {R.PAD_NAME[pad]} mask={use_mask} reg={reg_kind} w={w} {lay}"
                _compare("C", tag, _lossgrad(L, o, shape, pad, use_mask, reg_kind, w, geo=geo, tag=tag), c, w, "host")


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. the chained form and its flush
# ---------------------------------------------------------------------------------------------------------------------------------------
def _chain_step(L, o, shape, pad, use_mask, reg_kind, geo, cur, prev, loss_prev, ws, tag):
    """one chained launch on fresh gradient buffers -> (g_dt, g_ds), still on the device"""
    B, H, W = shape
    N = B * H * W
    g_dt, g_ds = _nan(N), _nan(N)
    mats = (None, None, None, ctypes.cast(geo, ctypes.c_void_p)) if geo is not None else (L.ptr(o["K"]), L.ptr(o["invK"]), L.ptr(o["T"]), None)
    L.call("e2e_warp_photo_lossgrad_chain", L.ptr(o["depth"]), L.ptr(o["src"]), L.strides4(o["src"]), L.ptr(o["tgt"]), L.strides4(o["tgt"]), *mats, use_mask, pad,
           reg_kind, *_reg_ptrs(L, o, reg_kind), W_CHAIN[0], W_CHAIN[1], cur, prev, L.ptr(loss_prev), L.ptr(g_dt), L.ptr(g_ds), L.ptr(ws), B, H, W, L.stream())
    torch.cuda.synchronize()
    _written(g_dt, N, f"{tag}: g_depth_tgt")
    _written(g_ds, N, f"{tag}: g_depth_src") if reg_kind else _untouched(g_ds, f"{tag}: g_depth_src (reg_kind 0)")
    return g_dt, g_ds


def _flush(L, ws, cur, reg_kind, loss, shape):
    L.call("e2e_warp_photo_lossgrad_chain_flush", L.ptr(ws), cur, reg_kind, L.ptr(loss), *shape, L.stream())
    torch.cuda.synchronize()


def _chain_area_clean(L, ws, shape, tag):
    nws = L.query("e2e_warp_photo_lossgrad_workspace_floats", *shape)
    assert nws == G.workspace_floats(*shape)
    assert torch.isnan(ws[nws:]).all(), f"{tag}: workspace written past the size its query returned"
    left = int((ws[G.chain_offset(*shape):nws].view(torch.int32) != 0).sum())
    assert left == 0, f"{tag}: {left} words of the slot sets are not zero after the flush"


def _zeroed_workspace(L, shape):
    nws = L.query("e2e_warp_photo_lossgrad_workspace_floats", *shape)
    ws = _nan(nws)
    ws[:nws] = 0                                                      # zero-filled once, as the header asks
    return ws


@pytest.mark.parametrize("reg_kind", G.REGS)
@pytest.mark.parametrize("shape,form", G.CHAIN_CASES, ids=str)
def test_chain(shape, form, reg_kind):
    """Four launches whose (padding, use_mask) run through all four combinations, so that every step has a loss of its own, over the slot
    sets 6, 7, 0, 1; at (3,49,161) 72 workgroups share the 64 slots.  Twice over the same workspace."""
    L = _L()
    s = R.fused_scene(*shape)
    lay = "nhwc" if form == "host" else "nchw"
    o = _operands(s, lay)
    geo = _geo12(s) if form == "host" else None
    ws = _zeroed_workspace(L, shape)
    passes = []
    for rep in range(2):
        losses = [_nan(2) for _ in G.CHAIN_STEPS]
        grads = []
        for k, ((pad, use_mask), (cur, prev)) in enumerate(zip(G.CHAIN_STEPS, G.CHAIN_SETS)):
            tag = f"{shape} {form} reg={reg_kind} step {k} ({R.PAD_NAME[pad]}, mask={use_mask}, set {cur} after {prev})"
            grads.append(_chain_step(L, o, shape, pad, use_mask, reg_kind, geo, cur, prev, losses[k - 1] if k else None, ws, tag))
            if k:
                _written(losses[k - 1], 2, f"{tag}: loss_prev_out")
            _untouched(losses[k], f"{tag}: the loss of the running step")
        _flush(L, ws, G.CHAIN_SETS[-1][0], reg_kind, losses[-1], shape)
        _written(losses[-1], 2, "flush: loss_out")
        _chain_area_clean(L, ws, shape, f"{shape} {form} reg={reg_kind} pass {rep}")
        passes.append((losses, grads))
    for k, (pad, use_mask) in enumerate(G.CHAIN_STEPS):
        tag = f"{shape} {form} reg={reg_kind} chain step {k} ({R.PAD_NAME[pad]}, mask={use_mask})"
        c = G.lg_case(shape, pad, use_mask, reg_kind)
        (losses, grads), (losses2, grads2) = passes
        assert _same_bits(losses[k], losses2[k]), f"{tag}: the second pass over the same workspace gives another loss"
        assert _same_bits(grads[k][0], grads2[k][0]) and _same_bits(grads[k][1], grads2[k][1]), f"{tag}: the second pass gives other gradients"
        classic = _lossgrad(L, o, shape, pad, use_mask, reg_kind, W_CHAIN, geo=geo, tag=tag + " classic")
        N = shape[0] * shape[1] * shape[2]
        assert _same_bits(grads[k][0][:N].cpu(), classic["g_dt"]), f"{tag}: g_depth_tgt differs from e2e_warp_photo_lossgrad's"
        assert not reg_kind or _same_bits(grads[k][1][:N].cpu(), classic["g_ds"]), f"{tag}: g_depth_src differs from e2e_warp_photo_lossgrad's"
        out = dict(loss=losses[k][:2].cpu(), g_dt=classic["g_dt"], g_ds=classic["g_ds"])
        _compare("D", tag, out, c, W_CHAIN, form)


@pytest.mark.parametrize("offset", G.OVERFLOW_OFFSETS)
def test_chain_overflow_flag(offset):
    """Per-workgroup sums above 2.6e8 / #workgroups, reached by finite values alone (far above; and every one within ten times the limit):
    both losses of that step are NaN, its gradients are those of e2e_warp_photo_lossgrad, and the next launch on the same workspace has a
    finite loss again, within its bound."""
    L = _L()
    shape, reg_kind, pad, use_mask = G.OVERFLOW_SHAPE, G.OVERFLOW_REG, 1, 1
    N = shape[0] * shape[1] * shape[2]
    over, plain = _operands(G.overflow_scene(offset), "nhwc"), _operands(R.fused_scene(*shape), "nhwc")
    ws = _zeroed_workspace(L, shape)
    loss_over, loss_plain = _nan(2), _nan(2)
    g_over = _chain_step(L, over, shape, pad, use_mask, reg_kind, None, 0, -1, None, ws, "overflow step")
    g_plain = _chain_step(L, plain, shape, pad, use_mask, reg_kind, None, 1, 0, loss_over, ws, "step after the overflow")
    _flush(L, ws, 1, reg_kind, loss_plain, shape)
    assert torch.isnan(loss_over).all(), f"losses of the overflowing step: {loss_over[:2].tolist()}"
    _written(loss_plain, 2, "the loss after the overflow")
    _chain_area_clean(L, ws, shape, "after the overflow")
    classic = _lossgrad(L, over, shape, pad, use_mask, reg_kind, W_CHAIN, tag="overflow inputs, classic")
    assert _same_bits(g_over[0][:N].cpu(), classic["g_dt"]) and _same_bits(g_over[1][:N].cpu(), classic["g_ds"]), "the overflow reached the gradients"
    assert torch.isfinite(classic["loss"]).all() and torch.isfinite(classic["g_dt"]).all()
    c = G.lg_case(shape, pad, use_mask, reg_kind)
    out = dict(loss=loss_plain[:2].cpu(), g_dt=g_plain[0][:N].cpu(), g_ds=g_plain[1][:N].cpu())
    _compare("D", "the step after the overflow", out, c, W_CHAIN, "device")


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. what the header rules out: an error before any launch, every output, the loss and the workspace as they were
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_everything_alone():
    L = _L()
    B, H, W = 2, 4, 6
    N = B * H * W
    st = L.stream()
    img = torch.rand(B, 3, H, W, device=DEV)
    s4, i_ = L.strides4(img), L.ptr(img)
    mats = torch.eye(4, device=DEV).repeat(B, 1, 1).contiguous()
    m_ = L.ptr(mats)
    plane = torch.rand(N, device=DEV) + 1
    r_ = L.ptr(plane)
    geo = (ctypes.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    g_ = ctypes.cast(geo, ctypes.c_void_p)
    outs = [_nan(N), _nan(N), _nan(2), _nan(2)]
    gt, gs, lo, lp = (L.ptr(o) for o in outs)
    nws = L.query("e2e_warp_photo_lossgrad_workspace_floats", B, H, W)
    ws = torch.rand(nws + SENTINEL, device=DEV)
    ws0 = ws.clone()
    w_ = L.ptr(ws)
    count = [0]

    def refused(name, *args):
        with pytest.raises(L.E2EError, match=name):
            L.call(name, *args)
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs) and _same_bits(ws, ws0), f"{name}: an output or the workspace changed although the call was refused"
        count[0] += 1

    def each_null(name, args, required):
        for k in required:
            refused(name, *[None if j == k else a for j, a in enumerate(args)])

    def each_value(name, args, at, bad):
        for k, values in zip(at, bad):
            for v in values:
                refused(name, *[v if j == k else a for j, a in enumerate(args)])

    dims = ((2, -1), (3, -1), (0, -1), (0, 1), (0, 1))                # padding_mode 2 and -1, reg_kind 3 and -1, B <= 0, H and W of 0 and 1
    a = [r_, i_, s4, i_, s4, m_, m_, m_, 1, 1, 2, r_, r_, r_, 1.0, 0.1, lo, gt, gs, w_, B, H, W, st]
    name = "e2e_warp_photo_lossgrad"
    each_null(name, a, (0, 1, 3, 5, 6, 7, 17, 19))
    each_null(name, a, (11, 12, 13, 18))                              # a regulariser buffer missing with reg_kind = 2
    each_value(name, a, (9, 10, 20, 21, 22), dims)
    a = [r_, i_, s4, i_, s4, g_, 1, 1, 2, r_, r_, r_, 1.0, 0.1, lo, gt, gs, w_, H, W, st]
    name = "e2e_warp_photo_lossgrad_hostgeo"
    each_null(name, a, (0, 1, 3, 5, 15, 17))                          # 5: geometry12_host
    each_null(name, a, (9, 10, 11, 16))
    each_value(name, a, (7, 8, 18, 19), dims[:2] + dims[3:])
    a = [r_, i_, s4, i_, s4, m_, m_, m_, None, 1, 1, 2, r_, r_, r_, 1.0, 0.1, 1, 0, lp, gt, gs, w_, B, H, W, st]
    name = "e2e_warp_photo_lossgrad_chain"
    each_null(name, a, (0, 1, 3, 5, 6, 7, 20, 22))                    # K, inv_K, T are required when no host geometry is given
    each_null(name, a, (12, 13, 14, 21))
    each_value(name, a, (10, 11, 23, 24, 25), dims)
    each_value(name, a, (17, 18), ((-1, 8, 0), (8,)))                 # set_cur of -1 and 8 and equal to set_prev; set_prev of 8
    each_null(name, a, (19,))                                         # set_prev >= 0 without loss_prev_out
    each_value(name, a, (8,), ((g_,),))                               # host geometry with B = 2
    a = [r_, i_, s4, i_, s4, None, None, None, g_, 1, 1, 2, r_, r_, r_, 1.0, 0.1, 1, 0, lp, gt, gs, w_, 1, H, W, st]
    each_null(name, a, (0, 1, 3, 20, 22))                             # the same with host geometry (B = 1)
    a = [w_, 1, 2, lo, B, H, W, st]
    name = "e2e_warp_photo_lossgrad_chain_flush"
    each_null(name, a, (0, 3))
    each_value(name, a, (1, 4, 5, 6), ((-1, 8),) + dims[2:])
    print(f"\nE: {count[0]} refused calls, every output and the workspace left as they were")
    assert count[0] == 83
