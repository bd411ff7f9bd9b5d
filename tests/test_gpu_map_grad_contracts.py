"""The entry points of csrc/pointfusion_grad.hip (the tape of one PointFusion map step and its adjoint, the normals' tape and adjoint,
the depth gradient of the fusion confidence) and of csrc/normal_maps_grad.hip (the adjoint of the normal map), called by name, at the
sizes at which their staging takes another path -- which tests/test_slam_grad_contract_inputs.py proves on the CPU from the sizes:

  a. the tape's row numbering (an ordered scan over blocks of CP_BLOCK pixels), exact: a short block, a full block, the first pixel of
     the next block, five blocks, 257 blocks (block 256 sums the counts before it in two trips) and 725 x 725 (1337 pixels behind the
     grid cap of the pixel passes), with holes at the block edges; read through e2e_pf_fuse_bwd and through e2e_pf_fuse_normals_bwd;
  b. rows dropped at the map's capacity;
  c. the values of one step against tests/pointfusion_grad_ref.py and tests/normal_grad_ref.py with those modules' own bounds;
  d. e2e_normal_maps_bwd and e2e_vertex_alpha_bwd behind their grid cap of 2048 workgroups, and batched.

The map step runs through FusionMap, as _one_step_gpu of tests/test_gpu_pointfusion_grad.py does, onto a previous map of a few hundred
points in view, so that most pixels are fresh.  The map's arrays, the tapes and every output are followed by a 64-element sentinel; the
tapes are allocated at exactly the size their queries return and poisoned before each call; outputs are NaN-filled or hold a known prior
under `accumulate`; every call is made twice and must give equal bits (gathers, no atomics).  Comparisons are against the CPU references
only, except where a cross-check between the tape and the forward append is stated."""
import functools

import pytest
import torch

import normal_grad_ref as N
import pointfusion_grad_ref as P
import slam_grad_contract_ref as R
from test_gpu_normal_grad import NORMAL_MAPS_BOUND, STEP_BOUND
from test_gpu_pointfusion_grad import ALPHA_BOUND, NAMES, ONE_STEP_BOUND, _one_step_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
ROW_WIDTH = {"points": 3, "normals": 3, "colors": 3, "ccounts": 1}


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _nan(n):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV)


def _out(shape, prior=None):
    """(buffer with a NaN sentinel, its view of `shape`): NaN-filled, or holding the prior"""
    n = 1
    for s in shape:
        n *= s
    buf = _nan(n)
    if prior is not None:
        buf[:n] = prior.float().reshape(-1).to(DEV)
    return buf, buf[:n].view(*shape)


def _tail_intact(buf, what):
    assert torch.isnan(buf[-SENTINEL:]).all(), f"{what}: written past the end"


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _poisoned_bytes(nbytes):
    assert nbytes > 0
    return torch.full((nbytes + SENTINEL,), 0xA5, device=DEV, dtype=torch.uint8)


class Step:
    """One map step of a case of slam_grad_contract_ref.map_case onto its previous map, with the capacity `cap` (default: room for
    every pixel): frame maps -> associate -> e2e_pf_fuse_tape (twice: equal bits) -> e2e_pf_fuse_normals_tape (twice) -> e2e_pf_fuse_append."""

    def __init__(self, case, cap=None):
        from e2ehip.fusionmap import FusionMap
        L = _L()
        self.case, self.H, self.W = case, case["H"], case["W"]
        H, W = self.H, self.W
        self.M0 = case["M"]
        self.cap = self.M0 + H * W if cap is None else cap
        fm = self.fm = FusionMap(self.cap, H, W, DEV)
        self.bufs = {}
        for name, width in ROW_WIDTH.items():                 # the map's arrays at exactly the capacity, then a sentinel
            buf = _nan(self.cap * width)
            buf[:self.cap * width] = 0
            self.bufs[name] = buf
            setattr(fm, name, buf[:self.cap * width].view(self.cap, 3) if width == 3 else buf[:self.cap])
        fm.load_state(*(case["prev"][k].to(DEV) for k in ("points", "normals", "colors", "ccounts")))
        self.rgb, self.depth = case["rgb"].to(DEV).contiguous(), case["depth"].to(DEV).contiguous()
        self.K, self.pose = case["K"].to(DEV).contiguous(), case["pose"].to(DEV).contiguous()
        with torch.no_grad():
            self.maps = maps = fm.frame_maps(self.depth, self.K, self.pose)
            fm.associate(maps, self.K, self.pose)
            tapes, ntapes = [], []
            for _ in range(2):
                tape = _poisoned_bytes(L.query("e2e_pf_fuse_tape_bytes", H, W))
                L.call("e2e_pf_fuse_tape", map_points=L.ptr(fm.points), map_colors=L.ptr(fm.colors), map_ccounts=L.ptr(fm.ccounts), M=self.M0,
                       map_capacity=self.cap, depth=L.ptr(self.depth), workspace=L.ptr(fm.ws), H=H, W=W, tape=L.ptr(tape), stream=L.stream())
                ntape = _poisoned_bytes(L.query("e2e_pf_fuse_normals_tape_bytes", H, W))
                L.call("e2e_pf_fuse_normals_tape", tape=L.ptr(tape), map_normals=L.ptr(fm.normals), M=self.M0, ntape=L.ptr(ntape), H=H, W=W,
                       stream=L.stream())
                tapes.append(tape)
                ntapes.append(ntape)
            torch.cuda.synchronize()
            assert torch.equal(tapes[0], tapes[1]) and torch.equal(ntapes[0], ntapes[1]), "two recordings of the same step differ"
            for t in tapes + ntapes:
                assert bool((t[-SENTINEL:] == 0xA5).all()), "a tape was written past the size its query returned"
            self.tape, self.ntape = tapes[0], ntapes[0]
            L.call("e2e_pf_fuse_append", map_points=L.ptr(fm.points), map_normals=L.ptr(fm.normals), map_colors=L.ptr(fm.colors),
                   map_ccounts=L.ptr(fm.ccounts), M=self.M0, map_capacity=self.cap, depth=L.ptr(self.depth), Vg=L.ptr(maps["Vg"]), Ng=L.ptr(maps["ng"]),
                   rgb=L.ptr(self.rgb), alpha=L.ptr(maps["alpha"]), workspace=L.ptr(fm.ws), H=H, W=W, new_count_out=L.ptr(fm._count), stream=L.stream())
            self.needed = int(fm._count.item())               # the size the append asked for
        self.M1 = min(self.needed, self.cap)
        fm.M = self.M1
        self.unique = fm.table("unique").cpu()
        for name, buf in self.bufs.items():
            _tail_intact(buf, f"map {name}")

    def fuse_bwd(self, g, want):
        """e2e_pf_fuse_bwd with the upstream gradients g {points, colors, ccounts: (M1, ...) or None} -> {name: tensor} for the outputs
        named in `want`, after the sentinel check and the repeat"""
        L = _L()
        H, W, M0 = self.H, self.W, self.M0
        shapes = {"g_Vg": (H, W, 3), "g_rgb": (H, W, 3), "g_alpha": (H, W), "g_prev_points": (M0, 3), "g_prev_colors": (M0, 3), "g_prev_ccounts": (M0,)}
        gd = {k: (None if v is None else v.float().to(DEV).contiguous()) for k, v in g.items()}
        runs = []
        for _ in range(2):
            outs = {k: _out(shapes[k]) if k in want else (None, None) for k in shapes}
            L.call("e2e_pf_fuse_bwd", tape=L.ptr(self.tape), Vg=L.ptr(self.maps["Vg"]), rgb=L.ptr(self.rgb), alpha=L.ptr(self.maps["alpha"]),
                   g_points=L.ptr(gd["points"]), g_colors=L.ptr(gd["colors"]), g_ccounts=L.ptr(gd["ccounts"]), ccounts_after=L.ptr(self.fm.ccounts),
                   M_before=M0, M_after=self.M1, H=H, W=W, stream=L.stream(), **{k: L.ptr(v[1]) for k, v in outs.items()})
            torch.cuda.synchronize()
            for k in want:
                _tail_intact(outs[k][0], k)
                assert not torch.isnan(outs[k][1]).any(), f"{k}: an element was not written"
            runs.append(outs)
        assert all(_same_bits(runs[0][k][1], runs[1][k][1]) for k in want), "two calls differ"
        return {k: runs[0][k][1] for k in want}

    def normals_bwd(self, gN, accumulate, want, priors=None):
        """e2e_pf_fuse_normals_bwd with the upstream gradient gN (M1,3) -> {name: tensor} for the outputs named in `want` (under
        `accumulate`, g_alpha and g_prev_ccounts start from their priors), after the sentinel check and the repeat"""
        L = _L()
        H, W, M0 = self.H, self.W, self.M0
        shapes = {"g_Ng": (H, W, 3), "g_prev_normals": (M0, 3), "g_alpha": (H, W), "g_prev_ccounts": (M0,)}
        gNd = gN.float().to(DEV).contiguous()
        runs = []
        for _ in range(2):
            outs = {k: _out(shapes[k], priors[k] if accumulate and k in ("g_alpha", "g_prev_ccounts") else None) if k in want else (None, None)
                    for k in shapes}
            L.call("e2e_pf_fuse_normals_bwd", tape=L.ptr(self.tape), ntape=L.ptr(self.ntape), Ng=L.ptr(self.maps["ng"]), alpha=L.ptr(self.maps["alpha"]),
                   g_normals=L.ptr(gNd), ccounts_after=L.ptr(self.fm.ccounts), M_before=M0, M_after=self.M1, accumulate=accumulate, H=H, W=W,
                   stream=L.stream(), **{k: L.ptr(v[1]) for k, v in outs.items()})
            torch.cuda.synchronize()
            for k in want:
                _tail_intact(outs[k][0], k)
                assert not torch.isnan(outs[k][1]).any(), f"{k}: an element was not written"
            runs.append(outs)
        assert all(_same_bits(runs[0][k][1], runs[1][k][1]) for k in want), "two calls differ"
        return {k: runs[0][k][1] for k in want}


@functools.lru_cache(maxsize=None)
def _step(shape, cap=None):
    return Step(R.map_case(*shape), cap)


def _numbering(st, cap=None):
    """what the tape numbered, read through e2e_pf_fuse_bwd with g_points[r] = (r + 1, 0, 0), against the CPU's numbering"""
    case, M0, M1 = st.case, st.M0, st.M1
    N_ = st.H * st.W
    rows, fresh = R.append_rows(case, st.unique, M0, cap)
    assert st.needed == M0 + fresh, f"the append asked for {st.needed} rows, the CPU counts {M0} + {fresh}"
    gP = torch.zeros(M1, 3)
    gP[:, 0] = torch.arange(1, M1 + 1, dtype=torch.float32)   # exact in float32: M1 < 2^24
    appended = rows >= 0
    fused = torch.zeros(N_, dtype=torch.bool)
    fused[st.unique[:, 1] * st.W + st.unique[:, 2]] = True
    winner = (st.unique[:, 0] + 1).float()[torch.argsort(st.unique[:, 1] * st.W + st.unique[:, 2])]       # the fused pixels' rows + 1, in pixel order
    by_points = st.fuse_bwd(dict(points=gP, colors=None, ccounts=None), ("g_Vg",))["g_Vg"]
    by_normals = st.normals_bwd(gP, 0, ("g_Ng",))["g_Ng"]                                                 # the normals' pixel pass reads the same tape
    for what, got in (("e2e_pf_fuse_bwd", by_points.cpu().reshape(N_, 3)), ("e2e_pf_fuse_normals_bwd", by_normals.cpu().reshape(N_, 3))):
        assert torch.equal(got[appended, 0], (rows[appended] + 1).float()), f"{what}: an appended pixel's row differs from the CPU's numbering"
        assert not bool(got[:, 1:].any()), what
        assert not bool(got[~appended & ~fused].any()), f"{what}: a pixel with zero depth, or one dropped at the capacity, received a gradient"
        assert bool((got[fused, 0] > 0).all()) and bool((got[fused, 0] <= winner).all()), what          # a fused pixel: a / (c + a) of its winner's
    # a cross-check between the tape and the forward append (not a reference): the appended row holds the pixel's vertex, bit for bit
    Vg = st.maps["Vg"][0].reshape(N_, 3)
    q = torch.nonzero(appended)[:, 0].to(DEV)
    assert _same_bits(st.fm.points[rows[appended].to(DEV)], Vg[q]), "map_points[row(q)] is not Vg[q]"
    return rows, fresh


# ---------------------------------------------------------------------------------------------------------------------------------------
# a. row numbering, exact
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.MAP_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_tape_numbers_the_appended_rows_as_the_forward_does(shape):
    st = _step(shape)
    rows, fresh = _numbering(st)
    assert st.M1 == st.M0 + fresh and 0 < st.unique.shape[0] <= st.M0 and fresh > st.H * st.W // 2        # fused, and mostly fresh
    edge = torch.tensor(st.case["edge_holes"])
    assert bool((rows[edge] == -1).all())
    print(f"a {shape}: M {st.M0} -> {st.M1}, {st.unique.shape[0]} fused, {fresh} appended, {st.H * st.W - int(st.case['valid'].sum())} holes")


# ---------------------------------------------------------------------------------------------------------------------------------------
# b. capacity
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.CAPACITY_CASES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_beyond_the_capacity_are_dropped(shape):
    k = R.CAPACITY_CASES[shape]
    case = R.map_case(*shape)
    cap = case["M"] + k
    st = _step(shape, cap)                                    # (checks the sentinels behind the map's arrays: nothing behind the capacity)
    rows, fresh = _numbering(st, cap)
    assert fresh > k and st.needed == case["M"] + fresh > cap and st.M1 == cap
    assert int((rows >= 0).sum()) == k and int(rows.max()) == cap - 1
    full = R.append_rows(case, st.unique, case["M"])[0]
    assert torch.equal(rows[rows >= 0], full[(full >= 0) & (full < cap)])                                 # the first k fresh pixels keep their rows
    print(f"b {shape}: capacity {cap}, {fresh} fresh pixels, {fresh - k} dropped")


# ---------------------------------------------------------------------------------------------------------------------------------------
# c. values of one step
# ---------------------------------------------------------------------------------------------------------------------------------------
def _rel(got, want):
    want = want.double().cpu()
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("shape", R.VALUE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_step_gradients_against_the_float64_step(shape):
    from e2ehip import ops
    L = _L()
    st = _step(shape)
    case, H, W = st.case, st.H, st.W
    up = {k: (lambda M, i=i, k=k: P.weights((M,) if k == "ccounts" else (M, 3), 10 + i)) for i, k in enumerate(NAMES)}
    got = st.fuse_bwd({k: up[k](st.M1) for k in NAMES}, ("g_Vg", "g_rgb", "g_alpha", "g_prev_points", "g_prev_colors", "g_prev_ccounts"))
    gbuf, gd = _out((H, W))
    L.call("e2e_vertex_maps_bwd", L.ptr(st.depth), L.ptr(st.K), L.ptr(st.pose), None, L.ptr(got["g_Vg"]), L.ptr(gd), 1, H, W, L.stream())
    L.call("e2e_vertex_alpha_bwd", depth=L.ptr(st.depth), K=L.ptr(st.K), alpha=L.ptr(st.maps["alpha"]), g_alpha=L.ptr(got["g_alpha"]),
           alpha_den=float(ops.fusion_alpha_den(st.fm.sigma)), g_depth=L.ptr(gd), accumulate=1, B=1, H=H, W=W, stream=L.stream())
    torch.cuda.synchronize()
    _tail_intact(gbuf, "g_depth")
    want = _one_step_reference(case["prev"], case["rgb"], case["depth"], case["K"], case["pose"], st.unique, up)
    for name, g, w in zip(ONE_STEP_BOUND, (gd, got["g_rgb"], got["g_prev_points"], got["g_prev_colors"], got["g_prev_ccounts"]), want):
        assert torch.isfinite(g).all(), f"{name}: an element was not written"
        e = _rel(g, w)
        print(f"c {shape} {name}: rel {e:.3e} (bound {ONE_STEP_BOUND[name]:.1e})")
        assert ONE_STEP_BOUND[name] <= 1e-4 and e <= ONE_STEP_BOUND[name], f"{name}: {e:.3e} > {ONE_STEP_BOUND[name]:.1e}"
    assert not bool(gd.cpu()[~case["valid"]].any())


@pytest.mark.parametrize("shape", R.VALUE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("accumulate", [0, 1])
def test_one_step_normals_gradients_against_the_closed_form(shape, accumulate):
    st = _step(shape)
    case, H, W, M0, M1 = st.case, st.H, st.W, st.M0, st.M1
    gN = P.weights((M1, 3), 50)
    shapes = {"g_Ng": (H, W, 3), "g_prev_normals": (M0, 3), "g_alpha": (H, W), "g_prev_ccounts": (M0,)}
    priors = {k: P.weights(shapes[k], 60 + i) for i, k in enumerate(STEP_BOUND)}
    got = st.normals_bwd(gN, accumulate, tuple(shapes), priors)
    frame = dict(ng=st.maps["ng"][0].cpu().double(), alpha=st.maps["alpha"][0].cpu().double(), valid=case["valid"])
    g_ng, g_alpha, g_prevN, g_prevcc = N.fuse_normals_bwd_closed_form({k: v.double() for k, v in case["prev"].items()}, frame, st.unique, gN)
    for k, w in (("g_Ng", g_ng), ("g_prev_normals", g_prevN), ("g_alpha", g_alpha), ("g_prev_ccounts", g_prevcc)):
        w = w + priors[k] if accumulate and k in ("g_alpha", "g_prev_ccounts") else w
        e = _rel(got[k], w)
        print(f"c {shape} normals {k} accumulate={accumulate}: rel {e:.3e} (bound {STEP_BOUND[k]:.1e})")
        assert STEP_BOUND[k] <= 1e-4 and e <= STEP_BOUND[k], f"{k}: {e:.3e} > {STEP_BOUND[k]:.1e}"
    assert not bool(got["g_Ng"].cpu()[~case["valid"]].any())


# ---------------------------------------------------------------------------------------------------------------------------------------
# d. e2e_normal_maps_bwd, e2e_vertex_alpha_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _normal_reference(shape, mode):
    return R.normal_maps_reference(R.normal_case(shape), mode)


def _hole_check(got, case, accumulate, what):
    hole = case["depth"] == 0
    g = got.cpu()
    assert _same_bits(g[hole], case["prior"].float()[hole]) if accumulate else not bool(g[hole].any()), f"{what}: a hole's element changed"


@pytest.mark.parametrize("shape", list(R.NORMAL_SHAPES), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["g_Nm", "g_Ng", "both"])
def test_normal_maps_bwd_behind_the_grid_cap(shape, mode):
    L = _L()
    B, H, W = shape
    case = R.normal_case(shape)
    dd, Kd, pd = case["depth"].to(DEV).contiguous(), case["K"].to(DEV)[None].repeat(B, 1, 1).contiguous(), case["poses"].to(DEV).contiguous()
    gn, gg = (case[k].float().to(DEV).contiguous() if mode in (k, "both") else None for k in ("g_Nm", "g_Ng"))
    ref = _normal_reference(shape, mode)
    assert torch.isfinite(ref).all()
    for accumulate in (0, 1):
        runs = []
        for _ in range(2):
            buf, out = _out((B, H, W), case["prior"] if accumulate else None)
            L.call("e2e_normal_maps_bwd", depth=L.ptr(dd), K=L.ptr(Kd), pose=L.ptr(pd), g_Nm=L.ptr(gn), g_Ng=L.ptr(gg), g_depth=L.ptr(out),
                   accumulate=accumulate, B=B, H=H, W=W, stream=L.stream())
            torch.cuda.synchronize()
            _tail_intact(buf, "g_depth")
            assert torch.isfinite(out).all(), "an element was not written"
            runs.append(out)
        assert _same_bits(*runs), "two calls differ"
        want = ref + case["prior"] if accumulate else ref
        e = _rel(runs[0], want)
        tail = _rel(runs[0].reshape(B, -1)[:, -1337:], want.reshape(B, -1)[:, -1337:]) if H * W > 1337 else e
        print(f"d normal maps {shape} {mode} accumulate={accumulate}: rel {e:.3e}, the last 1337 pixels alone {tail:.3e} (bound {NORMAL_MAPS_BOUND:.1e})")
        assert NORMAL_MAPS_BOUND <= 1e-4 and e <= NORMAL_MAPS_BOUND and tail <= NORMAL_MAPS_BOUND
        _hole_check(runs[0], case, accumulate, "e2e_normal_maps_bwd")


@pytest.mark.parametrize("shape", list(R.NORMAL_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_vertex_alpha_bwd_behind_the_grid_cap(shape):
    from e2ehip import ops
    L = _L()
    B, H, W = shape
    case = R.normal_case(shape)
    dd, Kd, pd = case["depth"].to(DEV).contiguous(), case["K"].to(DEV)[None].repeat(B, 1, 1).contiguous(), case["poses"].to(DEV).contiguous()
    alpha = ops.vertex_normal_maps(dd, Kd, pd)["alpha"].contiguous()          # the forward's alpha, read back
    den = ops.fusion_alpha_den(0.6)
    ref = R.alpha_bwd_reference(case, alpha.cpu(), float(torch.tensor(den, dtype=torch.float32)))
    ga = case["g_alpha"].float().to(DEV).contiguous()
    for accumulate in (0, 1):
        runs = []
        for _ in range(2):
            buf, out = _out((B, H, W), case["prior"] if accumulate else None)
            L.call("e2e_vertex_alpha_bwd", depth=L.ptr(dd), K=L.ptr(Kd), alpha=L.ptr(alpha), g_alpha=L.ptr(ga), alpha_den=float(den), g_depth=L.ptr(out),
                   accumulate=accumulate, B=B, H=H, W=W, stream=L.stream())
            torch.cuda.synchronize()
            _tail_intact(buf, "g_depth")
            assert torch.isfinite(out).all(), "an element was not written"
            runs.append(out)
        assert _same_bits(*runs), "two calls differ"
        want = ref + case["prior"] if accumulate else ref
        e = _rel(runs[0], want)
        tail = _rel(runs[0].reshape(B, -1)[:, -1337:], want.reshape(B, -1)[:, -1337:]) if H * W > 1337 else e
        print(f"d alpha {shape} accumulate={accumulate}: rel {e:.3e}, the last 1337 pixels alone {tail:.3e} (bound {ALPHA_BOUND:.1e})")
        assert ALPHA_BOUND <= 1e-4 and e <= ALPHA_BOUND and tail <= ALPHA_BOUND
        _hole_check(runs[0], case, accumulate, "e2e_vertex_alpha_bwd")


def test_tape_size_queries():
    L = _L()
    blocks = lambda n: -(-n // R.hip_constants()["CP_BLOCK"])
    for H, W in list(R.MAP_SHAPES) + [(1, 1), (480, 640)]:
        n = H * W
        assert L.query("e2e_pf_fuse_tape_bytes", H, W) == (64 + 4 * ((blocks(n) + 15) // 16 * 16) + 36 * n + 255) // 256 * 256
        assert L.query("e2e_pf_fuse_normals_tape_bytes", H, W) == (12 * n + 255) // 256 * 256
    for H, W in ((0, 5), (5, 0), (-1, 5)):
        assert L.query("e2e_pf_fuse_tape_bytes", H, W) == 0 == L.query("e2e_pf_fuse_normals_tape_bytes", H, W)
