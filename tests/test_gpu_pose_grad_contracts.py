"""The entry points of csrc/pose_grad.hip (the adjoint of the ICP normal equations with respect to the sources and to the targets, the
pose gradients of transform_points and Project3D, their workspace queries), called by name, against the float64 / extended-precision
references of tests/slam_grad_contract_ref.py -- at the sizes at which the staging takes another path, which
tests/test_slam_grad_contract_inputs.py proves on the CPU that each case reaches:

  a. e2e_transform_points_bwd_t: one partial, the second stage's first and second trip, the clamp at PG_MAX_PARTS, the grid-stride loop;
  b. e2e_icp_normal_equations_bwd: the same sizes, indices outside [0, n_tgt), distances on the float32 edge of the threshold;
  c. e2e_icp_normal_equations_bwd_tgt: segments of 64 and 65 rows (thread / wave), more queued segments than waves, targets in the
     second and third tile of the scan, more than 256 tiles (the scan's carry), the grid-stride trips of count and fill;
  d. e2e_project3d_bwd_t: 64 / 65 / 256 partials and the stride, batched against unbatched bit for bit, the clamp branch.

Every output is NaN-filled (or holds a known prior under `accumulate`) and is followed by a 64-element sentinel; every workspace is
allocated at exactly the size its query returns plus a sentinel and is poisoned before EACH call; every call is made twice and must
give equal bits (the kernels use no float atomics).  Comparisons are against the CPU references only, except where a bitwise
cross-check between two calls is stated."""
import numpy as np
import pytest
import torch

import slam_grad_contract_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
POISON = -0x5A5A5A5A


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _nan(n, dtype=torch.float32):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _out(n, prior=None):
    """n float32 + sentinel: NaN, or the prior's values (accumulate) followed by a NaN sentinel"""
    buf = _nan(n)
    if prior is not None:
        buf[:n] = prior.reshape(-1).to(DEV)
    return buf


def _tail_intact(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"


def _written(buf, n, what):
    _tail_intact(buf, n, what)
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _ws_doubles(nbytes):
    """a float64 workspace of exactly nbytes, NaN-poisoned, plus a NaN sentinel"""
    assert nbytes > 0 and nbytes % 8 == 0
    return _nan(nbytes // 8, torch.float64), nbytes // 8


def _ws_ints(nbytes):
    assert nbytes > 0 and nbytes % 4 == 0
    return torch.full((nbytes // 4 + SENTINEL,), POISON, device=DEV, dtype=torch.int32), nbytes // 4


def _refused(L, name, outputs, **kw):
    with pytest.raises(L.E2EError, match=rf"{name} failed \(-1\)"):
        L.call(name, **kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outputs), f"{name}: an output changed although the call was refused"


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. e2e_transform_points_bwd_t
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(R.TP_SIZES), ids=lambda n: f"n{n}")
def test_transform_points_bwd_t_against_extended_precision_sums(n):
    L = _L()
    c = R.hip_constants()
    nbytes = L.query("e2e_transform_points_bwd_t_workspace_bytes")
    assert nbytes == c["PG_MAX_PARTS"] * 12 * 8
    case = R.transform_case(n)
    g, p = case["g"].to(DEV), case["points"].to(DEV)
    outs = []
    for _ in range(2):
        out = _nan(12, torch.float64)
        ws, nws = _ws_doubles(nbytes)
        L.call("e2e_transform_points_bwd_t", g=L.ptr(g), points=L.ptr(p), n=n, out12=L.ptr(out), workspace=L.ptr(ws), stream=L.stream())
        torch.cuda.synchronize()
        _written(out, 12, "out12")
        _tail_intact(ws, nws, "workspace")
        outs.append(out)
    assert _same_bits(*outs), f"n={n}: two calls differ"
    dev = outs[0][:12].cpu().numpy()
    err = np.abs(dev.astype(np.longdouble) - case["want"])
    ratio = float((err / case["scale"]).max())
    print(f"a n={n}: worst |err| / sum|terms| = {ratio:.2e} (bound {R.NE_BOUND})")
    assert (err <= R.NE_BOUND * case["scale"]).all(), f"n={n}: |err| / sum|terms| = {ratio:.2e} > {R.NE_BOUND}"


def test_transform_points_bwd_t_refusals():
    L = _L()
    case = R.transform_case(63)
    g, p = case["g"].to(DEV), case["points"].to(DEV)
    out = _nan(12, torch.float64)
    ws, _ = _ws_doubles(L.query("e2e_transform_points_bwd_t_workspace_bytes"))
    good = dict(g=L.ptr(g), points=L.ptr(p), n=63, out12=L.ptr(out), workspace=L.ptr(ws), stream=L.stream())
    for bad in (dict(g=None), dict(points=None), dict(out12=None), dict(workspace=None), dict(n=0), dict(n=-5)):
        _refused(L, "e2e_transform_points_bwd_t", (out, ws), **{**good, **bad})


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. e2e_icp_normal_equations_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
def _ne_bwd(L, dev, case, thresh, with_dists, accumulate):
    """-> g_src (n,3) on the host, after the sentinel check and the repeat"""
    n = case["n"]
    outs = []
    for _ in range(2):
        out = _out(n * 3, case["prior"] if accumulate else None)
        L.call("e2e_icp_normal_equations_bwd", src=L.ptr(dev["src"]), tgt=L.ptr(dev["tgt"]), tgt_normals=L.ptr(dev["nrm"]), n_tgt=case["nt"],
               idx=L.ptr(dev["idx"]), dists=L.ptr(dev["dists"]) if with_dists else None, dist_thresh=thresh, adj28=L.ptr(dev["adj"]), n=n,
               g_src=L.ptr(out), accumulate=accumulate, stream=L.stream())
        torch.cuda.synchronize()
        _written(out, n * 3, "g_src")
        outs.append(out)
    assert _same_bits(*outs), "two calls differ"
    return outs[0][:n * 3].cpu().reshape(n, 3)


@pytest.mark.parametrize("n", R.NEB_SIZES, ids=lambda n: f"n{n}")
def test_normal_equations_bwd_at_every_staging_size(n):
    L = _L()
    worst = 0.0
    for nt in R.NEB_TARGETS:
        case = R.ne_bwd_case(n, nt)
        dev = {k: case[k].to(DEV) for k in ("src", "tgt", "nrm", "idx", "dists", "adj")}       # tgt, nrm: exactly nt rows, no slack
        assert dev["tgt"].numel() == nt * 3 == dev["nrm"].numel()
        for what, thresh, with_dists, keep in (("keep all, dists NULL", -1.0, False, case["keep_all"]), ("keep all, dists given", -1.0, True, case["keep_all"]),
                                               ("threshold 0.25", 0.25, True, case["keep_thresh"])):
            ref = R.ne_bwd_reference(case, keep)
            for accumulate in (0, 1):
                tag = f"n={n} nt={nt} {what} accumulate={accumulate}"
                got = _ne_bwd(L, dev, case, thresh, with_dists, accumulate)
                # the rows that are not kept: exactly 0, or the prior's bits
                rest = got[~keep]
                assert _same_bits(rest, case["prior"][~keep]) if accumulate else not bool(rest.any()), f"{tag}: a row that is not kept changed"
                if not accumulate:                            # the kept set, exactly: every kept row's gradient is non-zero in the reference
                    assert torch.equal((got != 0).any(1), keep), f"{tag}: the kept set differs"
                want = ref + case["prior"].double() if accumulate else ref
                if bool(keep.any()):
                    e = float((got.double() - want).abs().max() / want.abs().max())
                    worst = max(worst, e)
                    assert e <= R.NEB_BOUND, f"{tag}: {e:.3e} of the largest entry > {R.NEB_BOUND}"
    print(f"b n={n}: worst rel {worst:.2e} (bound {R.NEB_BOUND})")


def test_normal_equations_bwd_refusals():
    L = _L()
    case = R.ne_bwd_case(63, 7)
    dev = {k: case[k].to(DEV) for k in ("src", "tgt", "nrm", "idx", "dists", "adj")}
    out = _nan(63 * 3)
    good = dict(src=L.ptr(dev["src"]), tgt=L.ptr(dev["tgt"]), tgt_normals=L.ptr(dev["nrm"]), n_tgt=7, idx=L.ptr(dev["idx"]), dists=L.ptr(dev["dists"]),
                dist_thresh=0.25, adj28=L.ptr(dev["adj"]), n=63, g_src=L.ptr(out), accumulate=0, stream=L.stream())
    for bad in (dict(src=None), dict(tgt=None), dict(tgt_normals=None), dict(idx=None), dict(adj28=None), dict(g_src=None), dict(n=0), dict(n_tgt=0),
                dict(dists=None), dict(dists=None, dist_thresh=0.0)):      # a non-negative threshold needs the distances
        _refused(L, "e2e_icp_normal_equations_bwd", (out,), **{**good, **bad})


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. e2e_icp_normal_equations_bwd_tgt
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_normal_equations_bwd_tgt_workspace_query():
    L = _L()
    q = lambda n, nt: L.query("e2e_icp_normal_equations_bwd_tgt_workspace_bytes", n, nt)
    for n, nt in ((1, 1), (63, 4096), (64, 4097), (70001, 9000), (4242, R.HUGE), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert q(n, nt) == R.tgt_workspace_bytes(n, nt), (n, nt)
    for n, nt in ((0, 5), (5, 0), (-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31), (2 ** 40, 2 ** 40)):
        assert q(n, nt) == 0, (n, nt)


def _ne_bwd_tgt(L, dev, case, accumulate, want_t=True, want_n=True, dists=True, thresh=R.TGT_THRESH):
    n, nt = case["n"], case["nt"]
    nbytes = L.query("e2e_icp_normal_equations_bwd_tgt_workspace_bytes", n, nt)
    assert nbytes == R.tgt_workspace_bytes(n, nt)
    runs = []
    for _ in range(2):
        ws, nws = _ws_ints(nbytes)
        outs = [_out(nt * 3, p if accumulate else None) if wanted else None for wanted, p in zip((want_t, want_n), case["prior"])]
        L.call("e2e_icp_normal_equations_bwd_tgt", src=L.ptr(dev["src"]), tgt=L.ptr(dev["tgt"]), tgt_normals=L.ptr(dev["nrm"]), n_tgt=nt,
               idx=L.ptr(dev["idx"]), dists=L.ptr(dev["dists"]) if dists else None, dist_thresh=thresh, adj28=L.ptr(dev["adj"]), n=n,
               g_tgt=L.ptr(outs[0]), g_tgt_normals=L.ptr(outs[1]), accumulate=accumulate, workspace=L.ptr(ws), stream=L.stream())
        torch.cuda.synchronize()
        assert bool((ws[nws:] == POISON).all()), "workspace: written past the size its query returned"
        for o, what in zip(outs, ("g_tgt", "g_tgt_normals")):
            if o is not None:
                _written(o, nt * 3, what)
        runs.append(outs)
    assert all(a is None or _same_bits(a, b) for a, b in zip(*runs)), "two calls differ"
    return [None if o is None else o[:nt * 3].reshape(nt, 3) for o in runs[0]]


@pytest.mark.parametrize("name", list(R.TGT_CASES))
def test_normal_equations_bwd_tgt_at_every_staging_edge(name):
    L = _L()
    case = R.tgt_case(name)
    dev = {k: case[k].to(DEV) for k in ("src", "tgt", "nrm", "idx", "dists", "adj")}
    unnamed = case["counts"] == 0
    worst = 0.0
    for accumulate in (0, 1):
        wants = R.tgt_want(case, accumulate)
        both = _ne_bwd_tgt(L, dev, case, accumulate)
        for what, got_d, (want, bound), prior in zip(("g_tgt", "g_tgt_normals"), both, wants, case["prior"]):
            got = got_d.cpu()
            tag = f"{name} accumulate={accumulate} {what}"
            rest = got[unnamed]                               # a target that no kept row names: exactly 0, or the prior's bits
            assert _same_bits(rest, prior[unnamed]) if accumulate else not bool(rest.any()), f"{tag}: a target that no kept row names changed"
            err = (got.double() - want).abs()
            over = err > bound
            ratio = float((err / bound.clamp(min=1e-300))[~unnamed].max())
            worst = max(worst, ratio)
            assert not bool(over.any()), (f"{tag}: {int(over.any(1).sum())} targets beyond 2^-24 |want| + 1e-12 S, the worst at {ratio:.2f} x the bound: "
                                          f"targets {torch.nonzero(over.any(1))[:8, 0].tolist()} with {case['counts'][over.any(1)][:8].tolist()} rows")
        # each output NULL in turn: the other one has the same bits
        only_t = _ne_bwd_tgt(L, dev, case, accumulate, want_n=False)
        only_n = _ne_bwd_tgt(L, dev, case, accumulate, want_t=False)
        assert only_t[1] is None and only_n[0] is None
        assert _same_bits(only_t[0], both[0]) and _same_bits(only_n[1], both[1]), f"{name} accumulate={accumulate}: an output depends on the other's presence"
    print(f"c {name}: n={case['n']} n_tgt={case['nt']}: worst |err| / (2^-24 |want| + 1e-12 S) = {worst:.3f}")


def test_normal_equations_bwd_tgt_negative_threshold_keeps_every_row_in_range():
    """dists NULL and a negative threshold: every row whose index is in range counts -- the lengths case's dropped distances come back."""
    L = _L()
    import slam_chain_grad_ref as C
    case = R.tgt_case("lengths")
    dev = {k: case[k].to(DEV) for k in ("src", "tgt", "nrm", "idx", "dists", "adj")}
    keep = (case["idx"] >= 0) & (case["idx"] < case["nt"])
    assert int(keep.sum()) > int(case["keep"].sum())
    g_t, g_n, S_t, S_n = C.ne_bwd_tgt_closed_form(case["src"], case["tgt"], case["nrm"], case["idx"], keep, case["adj"], with_scale=True)
    for dists in (False, True):
        got = _ne_bwd_tgt(L, dev, case, 0, dists=dists, thresh=-1.0)
        for o, want, S in zip(got, (g_t, g_n), (S_t, S_n)):
            assert bool(((o.cpu().double() - want).abs() <= 2.0 ** -24 * want.abs() + 1e-12 * S).all())


def test_normal_equations_bwd_tgt_refusals():
    L = _L()
    case = R.tgt_case("lengths")
    n, nt = case["n"], case["nt"]
    dev = {k: case[k].to(DEV) for k in ("src", "tgt", "nrm", "idx", "dists", "adj")}
    ws, _ = _ws_ints(R.tgt_workspace_bytes(n, nt))
    gt, gn = _nan(nt * 3), _nan(nt * 3)
    good = dict(src=L.ptr(dev["src"]), tgt=L.ptr(dev["tgt"]), tgt_normals=L.ptr(dev["nrm"]), n_tgt=nt, idx=L.ptr(dev["idx"]), dists=L.ptr(dev["dists"]),
                dist_thresh=0.25, adj28=L.ptr(dev["adj"]), n=n, g_tgt=L.ptr(gt), g_tgt_normals=L.ptr(gn), accumulate=0, workspace=L.ptr(ws),
                stream=L.stream())
    before = ws.clone()
    for bad in (dict(src=None), dict(tgt=None), dict(tgt_normals=None), dict(idx=None), dict(adj28=None), dict(workspace=None), dict(n=0), dict(n_tgt=0),
                dict(n=2 ** 31), dict(n_tgt=2 ** 31), dict(g_tgt=None, g_tgt_normals=None), dict(dists=None), dict(dists=None, dist_thresh=0.0)):
        _refused(L, "e2e_icp_normal_equations_bwd_tgt", (gt, gn), **{**good, **bad})
    assert torch.equal(ws, before)


# ---------------------------------------------------------------------------------------------------------------------------------------
# d. e2e_project3d_bwd_t
# ---------------------------------------------------------------------------------------------------------------------------------------
def _project3d_bwd_t(L, pts, K, T, Wg, Wz, shape):
    """-> g_T (B,4,4) on the device; inputs are device tensors, Wz None for g_z = NULL"""
    B, H, W = shape
    nbytes = L.query("e2e_project3d_bwd_t_workspace_bytes", B)
    assert nbytes == B * R.hip_constants()["PG_MAX_PARTS"] * 12 * 8
    outs = []
    for _ in range(2):
        out = _nan(B * 16)
        ws, nws = _ws_doubles(nbytes)
        L.call("e2e_project3d_bwd_t", points=L.ptr(pts), K=L.ptr(K), T=L.ptr(T), g_grid=L.ptr(Wg), g_z=L.ptr(Wz), g_T=L.ptr(out), workspace=L.ptr(ws),
               B=B, H=H, W=W, stream=L.stream())
        torch.cuda.synchronize()
        _written(out, B * 16, "g_T")
        _tail_intact(ws, nws, "workspace")
        outs.append(out)
    assert _same_bits(*outs), "two calls differ"
    return outs[0][:B * 16].reshape(B, 4, 4)


def _project_check(L, case, tag):
    B, H, W = case["shape"]
    dev = {k: case[k].to(DEV).contiguous() for k in ("pts", "K", "T", "Wg", "Wz")}
    figures = []
    for with_gz in (False, True):
        got = _project3d_bwd_t(L, dev["pts"], dev["K"], dev["T"], dev["Wg"], dev["Wz"] if with_gz else None, case["shape"])
        want = case["want"][with_gz]
        for b in range(B):
            e = float((got[b].cpu().double() - want[b]).abs().max() / want[b].abs().max())
            figures.append(e)
            print(f"d {tag} g_z {'given' if with_gz else 'NULL'} item {b}: rel {e:.3e} (bound {R.P3D_BOUND:.1e}), max|ref| {float(want[b].abs().max()):.3e}")
        if B > 1:                                             # a bitwise cross-check: item b of the batched call is the B = 1 call on that item
            for b in range(B):
                one = _project3d_bwd_t(L, dev["pts"][b:b + 1].contiguous(), dev["K"][b:b + 1].contiguous(), dev["T"][b:b + 1].contiguous(),
                                       dev["Wg"][b:b + 1].contiguous(), dev["Wz"][b:b + 1].contiguous() if with_gz else None, (1, H, W))
                assert _same_bits(one[0], got[b]), f"{tag}: item {b} of the batched call differs from the call on that item alone"
    assert R.P3D_BOUND <= 1e-4
    assert max(figures) <= R.P3D_BOUND, f"{tag}: {max(figures):.3e} > {R.P3D_BOUND:.1e}"


@pytest.mark.parametrize("shape", list(R.P3D_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_project3d_bwd_t_at_every_staging_size(shape):
    _project_check(_L(), R.project_case(shape), "x".join(map(str, shape)))


def test_project3d_bwd_t_clamp_branch():
    """A band of points below the clamp at 1e-3 (just above zero, and behind the camera): g_z does not reach them, the grid term does
    (tests/test_slam_grad_contract_inputs.py shows that the reference tells both apart at 100 times the bound)."""
    _project_check(_L(), R.clamp_case(), "clamp")


def test_project3d_bwd_t_refusals():
    L = _L()
    q = lambda B: L.query("e2e_project3d_bwd_t_workspace_bytes", B)
    assert q(0) == 0 == q(-3) and q(3) == 3 * q(1)
    case = R.project_case((1, 2, 2))
    dev = {k: case[k].to(DEV).contiguous() for k in ("pts", "K", "T", "Wg", "Wz")}
    out = _nan(16)
    ws, _ = _ws_doubles(q(1))
    good = dict(points=L.ptr(dev["pts"]), K=L.ptr(dev["K"]), T=L.ptr(dev["T"]), g_grid=L.ptr(dev["Wg"]), g_z=L.ptr(dev["Wz"]), g_T=L.ptr(out),
                workspace=L.ptr(ws), B=1, H=2, W=2, stream=L.stream())
    for bad in (dict(H=1), dict(W=1), dict(B=0), dict(B=65536), dict(points=None), dict(K=None), dict(T=None), dict(g_grid=None), dict(g_T=None),
                dict(workspace=None)):
        _refused(L, "e2e_project3d_bwd_t", (out, ws), **{**good, **bad})
