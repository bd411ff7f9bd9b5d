"""The device entry points of the resident ICP odometry (csrc/icp.hip, and e2e_pf_active_subsample_dev of csrc/pointfusion.hip), called
directly, against the references of tests/icp_ref.py -- the contracts include/e2eslam.h states, not the kernels' formulas:

  A. e2e_icp_normal_equations: the 29 sums at every size at which the reduction takes another path (one partial, the 64-lane fold's
     first and second trip, the grid-stride loop), with and without a distance threshold;
  B. e2e_icp_state_init;
  C. e2e_icp_update from synthetic sums: the 6x6 solve on systems that make partial pivoting swap rows, the se(3) exponential over the
     whole range of angles and the pose composition, GradICP's damping / gate update, the stopped state, the trace cap;
  D. e2e_icp_reduce_update against e2e_icp_normal_equations + e2e_icp_update, bit for bit;
  E. e2e_icp_source_subsample;
  F. e2e_pf_active_subsample_dev against the oracle's active points;
  G. the argument combinations the header rules out: E2EError before any launch, outputs untouched.

Every output buffer is NaN-filled (integer buffers: a poison value) and followed by a sentinel; the workspace and the state vector are
allocated at exactly the size their queries return, also followed by a sentinel.  So each case also checks that what was meant to be
written was written and that nothing past any buffer's end was."""
import functools

import numpy as np
import pytest
import torch

import icp_ref
from oracle import pointfusion as opf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 64
POISON = -0x5A5A5A5A
LM = {"default": dict(lambda_max=2.0, B=1.0, B2=1.0, nu=200.0), "wide": dict(lambda_max=10.0, B=3.0, B2=0.5, nu=1.0)}


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _nan(n, dtype=torch.float32):
    return torch.full((n + SENTINEL,), float("nan"), device=DEV, dtype=dtype)


def _poison(n, dtype=torch.int64):
    return torch.full((n + SENTINEL,), POISON, device=DEV, dtype=dtype)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _written(buf, n, what):
    assert torch.isnan(buf[n:]).all(), f"{what}: written past the end"
    assert not torch.isnan(buf[:n]).any(), f"{what}: {int(torch.isnan(buf[:n]).sum())} of {n} elements not written"


def _untouched(*bufs):
    return all(b is None or bool(torch.isnan(b).all()) for b in bufs)


def _workspace():
    nbytes = _L().load().e2e_icp_workspace_bytes()
    assert nbytes % 8 == 0
    return _nan(nbytes // 8, torch.float64), nbytes // 8


def _rigid(seed):
    """a general rigid transform (float32, as prev_pose is): 0.7 rad about a skew axis, a translation of a metre or two"""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(3)
    return icp_ref.expm_twist(np.concatenate([rng.uniform(-2, 2, 3), w * (0.7 / np.linalg.norm(w))])).astype(np.float64).astype(np.float32)


class Odo:
    """the buffers of one odometry: state at exactly e2e_icp_state_doubles() float64, T32 / step32 / pose_out (4,4) float32, each NaN-filled
    and followed by a NaN sentinel"""

    def __init__(self, damp=None, prev=None, pose=True):
        L = _L()
        self.ns = L.load().e2e_icp_state_doubles()
        self.state, self.T32, self.step32 = _nan(self.ns, torch.float64), _nan(16), _nan(16)
        self.pose = _nan(16) if pose and prev is not None else None       # pose_out needs prev_pose
        self.prev = None if prev is None else torch.from_numpy(np.ascontiguousarray(prev, np.float32)).to(DEV)
        self.ws, self.nws = _workspace()
        if damp is not None:
            L.call("e2e_icp_state_init", L.ptr(self.state), L.ptr(self.T32), L.ptr(self.step32), L.ptr(self.prev), L.ptr(self.pose), float(damp), L.stream())

    def update(self, out29, mode, phase, lm=LM["default"]):
        L = _L()
        o = out29 if torch.is_tensor(out29) else torch.from_numpy(np.asarray(out29, np.float64)).to(DEV)
        L.call("e2e_icp_update", out29=L.ptr(o), state=L.ptr(self.state), T32=L.ptr(self.T32), step32=L.ptr(self.step32), prev_pose=L.ptr(self.prev),
               pose_out=L.ptr(self.pose), mode=mode, phase=phase, stream=L.stream(), **lm)
        torch.cuda.synchronize()

    def reduce_update(self, case, src, thresh, mode, phase, lm=LM["default"]):
        L = _L()
        L.call("e2e_icp_reduce_update", src=L.ptr(src), tgt=L.ptr(case["tgt"]), tgt_normals=L.ptr(case["nrm"]), idx=L.ptr(case["idx"]),
               dists=L.ptr(case["dists"]), dist_thresh=thresh, n=src.shape[0], workspace=L.ptr(self.ws), state=L.ptr(self.state), T32=L.ptr(self.T32),
               step32=L.ptr(self.step32), prev_pose=L.ptr(self.prev), pose_out=L.ptr(self.pose), mode=mode, phase=phase, stream=L.stream(), **lm)
        torch.cuda.synchronize()

    def host(self):
        """(state (ns,), T32, step32, pose_out or None) as numpy, after checking every sentinel"""
        torch.cuda.synchronize()
        for buf, n, what in ((self.state, self.ns, "state"), (self.T32, 16, "T32"), (self.step32, 16, "step32"), (self.pose, 16, "pose_out")):
            if buf is not None:
                _written(buf, n, what)
        assert torch.isnan(self.ws[self.nws:]).all(), "workspace: written past the size its query returned"
        return (self.state[:self.ns].cpu().numpy(), self.T32[:16].cpu().numpy().reshape(4, 4), self.step32[:16].cpu().numpy().reshape(4, 4),
                None if self.pose is None else self.pose[:16].cpu().numpy().reshape(4, 4))

    def same_bits(self, other):
        return all(a is None and b is None or _same_bits(a, b)
                   for a, b in ((self.state, other.state), (self.T32, other.T32), (self.step32, other.step32), (self.pose, other.pose)))

    def snapshot(self):
        return [None if b is None else b.clone() for b in (self.state, self.T32, self.step32, self.pose)]


def _one_ulp32(dev, ref64):
    """dev (float32) within one float32 ulp of the float64 value ref64"""
    return bool((np.abs(dev.astype(np.float64) - ref64) <= np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# A. e2e_icp_normal_equations
# ---------------------------------------------------------------------------------------------------------------------------------------
NE_SIZES = {1: "smallest", 5: "five points", 63: "partial wave", 256: "one partial", 257: "two partials", 16384: "64 partials: full wave, one trip",
            16385: "65 partials: second trip, lane 0 only", 19200: "75 partials: the product's size", 65536: "256 partials", 70001: "grid-stride, ragged"}
NE_TARGETS = (1, 7, 3000)
NE_BOUND = 1e-13               # x sum |terms|: float64 chains of <= ~32 additions are 36 x 2^-53 = 4e-15; the rest covers the order of the products
EDGE = np.float32(0.0625)      # dist_thresh 0.25 squared, exact in float32
SPECIAL = (EDGE, np.nextafter(EDGE, np.float32(0)), np.nextafter(EDGE, np.float32(1)), np.float32("nan"), np.float32("inf"))
SPECIAL_KEPT = (False, True, False, False, False)


def _ne_case(n, nt):
    rng = np.random.default_rng(1000 * nt + n)
    src, tgt = rng.uniform(-2, 2, (n, 3)).astype(np.float32), rng.uniform(-2, 2, (nt, 3)).astype(np.float32)
    nrm = rng.standard_normal((nt, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    idx = rng.integers(0, nt, n)
    idx[-1] = nt - 1
    if n > 1:
        idx[0] = 0
    if n > 3:
        idx[2] = idx[1]                                       # a repeat even among 3000 targets
    dists = rng.uniform(0, 0.125, n).astype(np.float32)       # about half below 0.0625
    where = {}
    for k, v in enumerate(SPECIAL):                           # the boundary values, at the head and (where there is room) in the last workgroup
        for pos in ((k,) if n < 10 else (k, n - 1 - k)):
            if pos < n:
                dists[pos] = v
                where[pos] = SPECIAL_KEPT[k]
    with np.errstate(invalid="ignore"):
        keep = dists < EDGE
    assert all(keep[p] == kept for p, kept in where.items())
    case = dict(n=n, src_h=src, tgt_h=tgt, nrm_h=nrm, idx_h=idx, keep=keep)
    for k, a in (("src", src), ("tgt", tgt), ("nrm", nrm), ("idx", idx.astype(np.int64)), ("dists", dists)):
        case[k] = torch.from_numpy(a).to(DEV)
    return case


def _normal_equations(case, thresh, with_dists=True):
    """-> (out29 as numpy, the second call's bits equal the first's)"""
    L = _L()
    outs = []
    for _ in range(2):
        out = _nan(29, torch.float64)
        ws, nws = _workspace()
        L.call("e2e_icp_normal_equations", L.ptr(case["src"]), L.ptr(case["tgt"]), L.ptr(case["nrm"]), L.ptr(case["idx"]),
               L.ptr(case["dists"]) if with_dists else None, thresh, case["n"], L.ptr(out), L.ptr(ws), L.stream())
        torch.cuda.synchronize()
        _written(out, 29, "out29")
        assert torch.isnan(ws[nws:]).all(), "workspace: written past the size its query returned"
        outs.append(out)
    return outs[0][:29].cpu().numpy(), _same_bits(outs[0], outs[1])


@pytest.mark.parametrize("n", list(NE_SIZES), ids=lambda n: f"n{n}")
def test_normal_equations_against_extended_precision_sums(n):
    worst = 0.0
    for nt in NE_TARGETS:
        case = _ne_case(n, nt)
        everything = np.ones(n, bool)
        for what, thresh, with_dists, keep in (("keep all, dists NULL", -1.0, False, everything), ("threshold 0.25", 0.25, True, case["keep"]),
                                               ("threshold 0", 0.0, True, ~everything)):
            ref, scale = icp_ref.normal_equations(case["src_h"], case["tgt_h"], case["nrm_h"], case["idx_h"], keep)
            dev, repeat = _normal_equations(case, thresh, with_dists)
            assert repeat, f"n={n} nt={nt} {what}: two calls differ"
            assert dev[27] == float(keep.sum()), f"n={n} nt={nt} {what}: {dev[27]} inliers, {keep.sum()} expected"
            err = np.abs(dev.astype(np.longdouble) - ref)
            if not keep.any():
                assert not dev.any(), f"n={n} nt={nt} {what}: sums of no inliers must be exactly 0"
                continue
            ratio = float((err / scale)[scale > 0].max())
            worst = max(worst, ratio)
            assert (err <= NE_BOUND * scale).all(), f"n={n} nt={nt} {what}: |err| / sum|terms| = {ratio:.2e} > {NE_BOUND}"
    print(f"A n={n}: worst |err| / sum|terms| = {worst:.2e} (bound {NE_BOUND})")


# ---------------------------------------------------------------------------------------------------------------------------------------
# B. e2e_icp_state_init
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_state_init_defines_everything():
    prev = _rigid(1)
    for pose in (True, False):
        o = Odo(damp=0.375, prev=prev if pose else None, pose=pose)
        st, T32, step32, pose_out = o.host()
        assert np.array_equal(st, icp_ref.initial_state(o.ns, 0.375)) and st[22] == st[26] == 0.375
        assert np.array_equal(T32, np.eye(4)) and np.array_equal(step32, np.eye(4))
        if pose:
            assert _same_bits(o.pose[:16], o.prev.reshape(-1))
    o = Odo(damp=1e-8, prev=prev, pose=False)                  # prev_pose given, pose_out NULL: accepted, nothing to write
    assert o.host()[0][22] == 1e-8


# ---------------------------------------------------------------------------------------------------------------------------------------
# C. e2e_icp_update
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(icp_ref.PIVOT_SEEDS)))
def test_update_solve_on_systems_that_swap_rows(k):
    """backward error (independent of the conditioning) and forward error (times the condition number the reference computes)"""
    A, b = icp_ref.pivoting_systems()[k]
    for lam in (0.0, 1e-8, 1.0):
        o = Odo(damp=lam)
        o.update(icp_ref.pack(A, b, 100, 1.0), 1, 0)
        xi = o.host()[0][16:22]
        Al = A + lam * np.eye(6)
        xi_ref = np.linalg.solve(Al, b)
        back = np.abs(Al @ xi - b).max() / (np.linalg.norm(Al, np.inf) * np.abs(xi).max() + np.abs(b).max())
        fwd = np.abs(xi - xi_ref).max() / (np.linalg.cond(Al) * np.abs(xi_ref).max())
        print(f"C solve {k} lambda={lam}: backward {back:.2e} (bound 1e-13), forward / cond {fwd:.2e} (bound 1e-12), cond {np.linalg.cond(Al):.1e}")
        assert back <= 1e-13 and fwd <= 1e-12


@pytest.mark.parametrize("th", icp_ref.ANGLES, ids=lambda t: f"w{t:g}")
def test_update_exponential_and_composition(th):
    """mode 0 with A = I: xi is the right-hand side, state T <- exp(xi) T against the true exponential, T32 its float32, pose_out = T prev_pose"""
    prev = _rigid(2)
    o = Odo(damp=0.0, prev=prev)
    o.update(icp_ref.pack(np.eye(6), np.concatenate([[0.3, -0.2, 0.5], _rigid(3)[:3, 3] * 0.2]), 100, 1.0), 0, 0)   # T_prev: not the identity
    worst = 0.0
    for _, xi in [c for c in icp_ref.sweep_twists(per_angle=8, seed=5) if c[0] == th]:
        T_prev = o.host()[0][:16].reshape(4, 4)
        o.update(icp_ref.pack(np.eye(6), xi, 100, 1.0), 0, 0)
        st, T32, _, pose = o.host()
        assert np.array_equal(st[16:22], xi)
        T = st[:16].reshape(4, 4)
        ref = icp_ref.expm_twist(xi) @ T_prev.astype(np.longdouble)
        scale = max(1.0, np.abs(xi[:3]).max(), np.abs(T_prev).max())
        err = float(np.abs(T - ref).max()) / scale
        worst = max(worst, err)
        assert err <= 2e-14, f"|w| = {th}: |T - expm(xi) T_prev| = {err:.2e} of max(1, |v|, |T_prev|)"
        assert np.array_equal(T32, T.astype(np.float32))
        assert _one_ulp32(pose, T @ prev.astype(np.float64))
    print(f"C exp |w|={th:g}: worst {worst:.2e} (bound 2e-14)")


def _gradicp_trials(name):
    """(err / cnt of phase 0, {trial: (cnt', err')}) -- sized so that each trial reaches its branch under the parameter set"""
    if name == "default":                                     # nu = 200, B2 = 1: exp overflows from delta < -3.55
        return 5.0, {"better": (100, 490.0), "worse": (100, 550.0), "equal": (100, 500.0), "overflow": (100, 100.0), "no_inliers": (0, 3.0)}
    return 2000.0, {"better": (100, 198000.0), "worse": (100, 210000.0), "equal": (100, 200000.0), "overflow": (100, 0.0), "no_inliers": (0, 1990.0)}


def _state_close(dev, ref, what):
    """1e-14 relative: the T block against its largest entry, every other element against itself"""
    tscale = max(1.0, np.abs(ref[:16]).max())
    assert (np.abs(dev[:16] - ref[:16]) <= 1e-14 * tscale).all(), f"{what}: T off by {np.abs(dev[:16] - ref[:16]).max() / tscale:.2e}"
    bad = np.abs(dev[16:] - ref[16:]) > 1e-14 * np.abs(ref[16:])
    assert not bad.any(), f"{what}: state{(np.nonzero(bad)[0] + 16).tolist()} = {dev[16:][bad]} expected {ref[16:][bad]}"
    return float(max(np.abs(dev[:16] - ref[:16]).max() / tscale, (np.abs(dev[16:] - ref[16:]) / np.maximum(np.abs(ref[16:]), 1e-300)).max()))


@pytest.mark.parametrize("trial", ["better", "worse", "equal", "overflow", "no_inliers"])
@pytest.mark.parametrize("name", list(LM))
def test_update_gradicp_phases(name, trial):
    lm, lmax = LM[name], LM[name]["lambda_max"]
    e0, trials = _gradicp_trials(name)
    prev, lam = _rigid(4), 1e-3
    o = Odo(damp=lam, prev=prev)
    A = 2.0 * np.eye(6)                                       # (2 + lambda) xi = b: one rounding on either side, so xi is not what is compared
    o.update(icp_ref.pack(A, [0.2, -0.4, 0.6, 0.3, 0.5, -0.2], 100, 1.0), 0, 0, lm)
    ref = o.host()
    T_before = ref[0][:16].copy()
    worst = 0.0
    steps = [(icp_ref.pack(A, [0.1, 0.3, -0.2, -0.12, 0.2, 0.16], 100, e0 * 100), 0), (icp_ref.pack(np.zeros((6, 6)), np.zeros(6), *trials[trial]), 1)]
    for out29, phase in steps:
        ref = icp_ref.lm_step(ref[0], out29, 1, phase, T32=ref[1], step32=ref[2], prev_pose=prev, pose_out=ref[3], **lm)
        o.update(out29, 1, phase, lm)
        st, T32, step32, pose = o.host()
        worst = max(worst, _state_close(st, ref[0], f"{name}/{trial} phase {phase}"))
        assert (np.abs(step32 - ref[2]) <= 1e-14 * np.abs(ref[2])).all() and (np.abs(T32 - ref[1]) <= 1e-14 * np.abs(ref[1])).all()
        assert np.array_equal(T32, st[:16].reshape(4, 4).astype(np.float32))
        assert _one_ulp32(pose, st[:16].reshape(4, 4) @ prev.astype(np.float64)) and _one_ulp32(pose, ref[0][:16].reshape(4, 4) @ prev.astype(np.float64))
        assert st[25] == 1 + phase and np.isfinite(st).all()
        if phase == 0:
            assert st[23] == e0 and np.array_equal(st[:16], T_before) and st[22] == lam
    # the trial reaches the branch it is named after (conditions on the inputs, from the reference)
    cnt, err = trials[trial]
    delta = err / max(cnt, 1) - e0
    factor, moved = st[22] / lam, np.abs(st[:16] - T_before).max()
    if trial == "better":
        assert lm["nu"] * delta < -19.9 and moved > 0.01
    elif trial == "worse":
        assert lm["nu"] * delta > 60 and moved <= 1e-14 * np.abs(T_before).max() and abs(factor - lmax) <= 1e-14 * lmax
    elif trial == "equal":
        assert delta == 0 and abs(factor - (1 / lmax + (lmax - 1 / lmax) / (1 + lm["B"]))) <= 1e-14 * factor
    elif trial == "overflow":
        assert -lm["B2"] * lm["nu"] * delta > 710 and st[22] == lam * (1.0 / lmax)
    else:
        assert cnt == 0 and delta == err - e0
    print(f"C gradicp {name}/{trial}: worst relative difference to lm_step {worst:.2e} (bound 1e-14); gate step moved T by {moved:.2e}, lambda x {factor:.6g}")


def test_update_stops_for_good_below_six_inliers():
    prev = _rigid(6)
    o = Odo(damp=1e-6, prev=prev)
    good = icp_ref.pack(2.0 * np.eye(6), [0.1, 0.3, -0.2, -0.12, 0.2, 0.16], 100, 7.0)
    o.update(good, 0, 0)
    o.update(good, 1, 0)                                      # step32 is now a real trial step
    before = o.host()
    assert not np.array_equal(before[2], np.eye(4))
    o.update(icp_ref.pack(2.0 * np.eye(6), np.ones(6), 5, 7.0), 1, 0)
    st, T32, step32, pose = o.host()
    assert st[24] == 1.0 and np.array_equal(step32, np.eye(4))
    assert np.array_equal(st[:16], before[0][:16]) and np.array_equal(T32, before[1]) and np.array_equal(pose, before[3]) and st[25] == before[0][25]
    ref = icp_ref.lm_step(before[0], icp_ref.pack(2.0 * np.eye(6), np.ones(6), 5, 7.0), 1, 0, T32=before[1], step32=before[2], pose_out=before[3])
    assert np.array_equal(st, ref[0])
    snap = o.snapshot()
    for i in range(10):
        mode, phase = ((0, 0), (1, 0), (1, 1))[i % 3]
        o.update(good, mode, phase)
    assert all(_same_bits(a, b) for a, b in zip(snap, o.snapshot()))
    o.host()


def test_update_trace_holds_the_first_64_iterations():
    o = Odo(damp=0.0)
    xi = np.array([1e-3, -2e-3, 1e-3, 2e-3, 1e-3, -1e-3])
    for k in range(70):
        o.update(icp_ref.pack(np.eye(6), xi, 100 + k, 0.5 * k), 0, 0)
    st = o.host()[0]                                          # (checks the sentinel after the state: pair 64 would land on it)
    assert st[25] == 70 and o.ns == 32 + 2 * 64
    assert np.array_equal(st[32::2], 100.0 + np.arange(64)) and np.array_equal(st[33::2], 0.5 * np.arange(64))
    ref = icp_ref.expm_twist(70 * xi)                         # 70 equal steps commute
    assert np.abs(st[:16].reshape(4, 4) - ref).max() <= 70 * 2e-14


# ---------------------------------------------------------------------------------------------------------------------------------------
# D. e2e_icp_reduce_update = e2e_icp_normal_equations + e2e_icp_update, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cloud_case(n):
    """sources a few centimetres off their targets (a solvable, well-conditioned system) plus a second cloud for the trial step"""
    rng = np.random.default_rng(n)
    nt = 3000
    tgt = rng.uniform(-2, 2, (nt, 3)).astype(np.float32)
    nrm = rng.standard_normal((nt, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    idx = rng.integers(0, nt, n)
    src = (tgt[idx] + 0.05 * rng.standard_normal((n, 3))).astype(np.float32)
    nxt = (src + 0.01 * rng.standard_normal((n, 3))).astype(np.float32)
    dists = rng.uniform(0, 0.08, n).astype(np.float32)        # four in five below 0.0625
    return {k: torch.from_numpy(a).to(DEV) for k, a in (("src", src), ("nxt", nxt), ("tgt", tgt), ("nrm", nrm), ("idx", idx.astype(np.int64)), ("dists", dists))}


@pytest.mark.parametrize("mode,phase", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("n", [5, 256, 16385, 19200, 70001], ids=lambda n: f"n{n}")
def test_reduce_update_is_bit_identical_to_the_two_calls(n, mode, phase):
    L = _L()
    case = _cloud_case(n)
    prev = _rigid(7)
    thresh = 0.25 if mode == 1 else -1.0
    two, one = Odo(damp=1e-6, prev=prev), Odo(damp=1e-6, prev=prev)
    out = _nan(29, torch.float64)
    for ph in range(phase + 1):
        src = case["nxt"] if ph == 1 else case["src"]
        L.call("e2e_icp_normal_equations", L.ptr(src), L.ptr(case["tgt"]), L.ptr(case["nrm"]), L.ptr(case["idx"]), L.ptr(case["dists"]), thresh, n,
               L.ptr(out), L.ptr(two.ws), L.stream())
        two.update(out, mode, ph)
        one.reduce_update(case, src, thresh, mode, ph)
    st = two.host()[0]
    one.host()
    _written(out, 29, "out29")
    assert st[24] == (1.0 if n < 6 else 0.0) and st[25] == (0 if (mode == 1 and phase == 0) or n < 6 else 1)      # the update did what the case is about
    assert one.same_bits(two), "e2e_icp_reduce_update differs from e2e_icp_normal_equations + e2e_icp_update"


# ---------------------------------------------------------------------------------------------------------------------------------------
# E. e2e_icp_source_subsample
# ---------------------------------------------------------------------------------------------------------------------------------------
def _subsample(Vg, depth, ds, status):
    L = _L()
    H, W = depth.shape
    n = -(-H // ds) * -(-W // ds)
    src = _nan(n * 3)
    L.call("e2e_icp_source_subsample", L.ptr(Vg), L.ptr(depth), H, W, ds, L.ptr(src), L.ptr(status), L.stream())
    torch.cuda.synchronize()
    _written(src, n * 3, "src")
    assert _same_bits(src[:n * 3], Vg[::ds, ::ds].reshape(-1)), f"({H}, {W}, {ds}): src is not Vg[::ds, ::ds]"
    assert (status[1:] == POISON).all(), "status: written past the word"
    return int(status[0])


@pytest.mark.parametrize("H,W,ds", [(7, 10, 4), (9, 9, 3), (5, 6, 1), (3, 50, 8), (60, 80, 4)])
def test_source_subsample_and_its_status_word(H, W, ds):
    g = torch.Generator().manual_seed(H * W + ds)
    Vg = torch.randn(H, W, 3, generator=g).to(DEV)
    depth = (torch.rand(H, W, generator=g) + 0.5).to(DEV)
    status = _poison(1, torch.int32)
    status[0] = 0
    assert _subsample(Vg, depth, ds, status) == 0
    hs, wl = (H - 1) // ds * ds, (W - 1) // ds * ds               # the last selected row and column
    if ds > 1:
        hole = depth.clone()
        hole[min(1, H - 1), 1] = 0.0                                # under no selected pixel
        if wl + 1 < W:
            hole[hs, wl + 1] = 0.0
        assert _subsample(Vg, hole, ds, status) == 0
    hole = depth.clone()
    hole[hs, wl] = 0.0                                              # under the last selected pixel
    assert _subsample(Vg, hole, ds, status) == 1
    assert _subsample(Vg, depth, ds, status) == 1                   # sticky: a clean frame does not lower it
    status[0] = 0
    hole = depth.clone()
    hole[0, 0] = 0.0
    assert _subsample(Vg, hole, ds, status) == 1


# ---------------------------------------------------------------------------------------------------------------------------------------
# F. e2e_pf_active_subsample_dev
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _active_case():
    """one 24 x 32 frame as the map (capacity 4096: four count blocks), associated with the next view 0.3 m on; the rows above the live
    count hold copies of active points, which nothing may read"""
    from e2ehip.fusionmap import FusionMap
    from e2ehip.synthetic import make_sequence
    L = _L()
    H, W = 24, 32
    colors, depths, K, poses = make_sequence(2, H, W, seed=3, step=0.3, noise=0.0, scene="corner")
    colors, depths, K, poses = colors[0], depths[0, ..., 0], K[0, 0], poses[0]
    st, _ = opf.pointfusion_step(opf.empty_state(), colors[0], depths[0], K, poses[0])
    active = opf.find_active_map_points(st["points"], K, poses[1], H, W)[:, 0]
    M, P = st["points"].shape[0], active.shape[0]
    assert 0 < P < M and M + P <= 4096
    fm = FusionMap(4096, H, W, DEV)
    fm.load_state(st["points"].to(DEV), st["normals"].to(DEV), st["colors"].to(DEV), st["ccounts"].to(DEV))
    for arr, key in ((fm.points, "points"), (fm.normals, "normals"), (fm.ccounts, "ccounts")):
        arr[M:M + P] = st[key][active].to(DEV)
    Kd, pose = K.to(DEV).contiguous(), poses[1].to(DEV).contiguous()
    maps = fm.frame_maps(depths[1].to(DEV), Kd, pose)
    L.call("e2e_pf_associate_dev", map_points=L.ptr(fm.points), map_normals=L.ptr(fm.normals), map_ccounts=L.ptr(fm.ccounts), map_count_dev=L.ptr(fm.count),
           K=L.ptr(Kd), pose=L.ptr(pose), Vg=L.ptr(maps["Vg"]), Ng=L.ptr(maps["ng"]), dist_th=fm.dist_th, dot_th=fm.dot_th, workspace=L.ptr(fm.ws),
           map_capacity=fm.cap, H=H, W=W, stream=L.stream())
    torch.cuda.synchronize()
    return fm, active, P


def _active_subsample(fm, ds, tcap, tcount):
    L = _L()
    tgt, tgt_n = _nan(tcap * 3), _nan(tcap * 3)
    L.call("e2e_pf_active_subsample_dev", map_points=L.ptr(fm.points), map_normals=L.ptr(fm.normals), map_count_dev=L.ptr(fm.count), map_capacity=fm.cap,
           workspace=L.ptr(fm.ws), H=fm.H, W=fm.W, dsratio=ds, tgt=L.ptr(tgt), tgt_normals=L.ptr(tgt_n), tgt_count_dev=L.ptr(tcount), tgt_capacity=tcap,
           stream=L.stream())
    torch.cuda.synchronize()
    assert (tcount[3:] == POISON).all(), "tgt_count_dev: written past its three words"
    return tgt, tgt_n


def test_active_subsample_reference_has_ragged_counts():
    _, _, P = _active_case()
    assert sum(P % ds != 0 for ds in (1, 3, 4, 7)) >= 2


@pytest.mark.parametrize("ds", [1, 3, 4, 7])
def test_active_subsample_against_the_oracle(ds):
    fm, active, P = _active_case()
    sel = active[::ds].to(DEV)
    T = -(-P // ds)
    assert sel.numel() == T
    tcount = _poison(3)
    tcount[:3] = 0
    for tcap in (T, T + 5):                                   # exactly enough, and more than enough: rows beyond the count stay unwritten
        tgt, tgt_n = _active_subsample(fm, ds, tcap, tcount)
        assert tcount[:3].tolist() == [T, P, 0]
        for buf, rows, what in ((tgt, fm.points, "tgt"), (tgt_n, fm.normals, "tgt_normals")):
            assert _same_bits(buf[:T * 3], rows[sel].reshape(-1)), f"{what}: not the active map rows [::{ds}]"
            assert torch.isnan(buf[T * 3:]).all(), f"{what}: written beyond the target count"
    # one row too few: flag, clamped count, nothing past the end; the flag then stays
    tgt, tgt_n = _active_subsample(fm, ds, T - 1, tcount)
    assert tcount[:3].tolist() == [T - 1, P, 1]
    for buf, rows in ((tgt, fm.points), (tgt_n, fm.normals)):
        assert _same_bits(buf[:(T - 1) * 3], rows[sel[:T - 1]].reshape(-1)) and torch.isnan(buf[(T - 1) * 3:]).all()
    _active_subsample(fm, ds, T, tcount)
    assert tcount[:3].tolist() == [T, P, 1]


# ---------------------------------------------------------------------------------------------------------------------------------------
# G. what the header rules out: an error before any launch, every output as it was
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_outputs_alone():
    L = _L()
    E = L.E2EError
    case = _ne_case(63, 7)
    src, tgt, nrm, idx, dists = (L.ptr(case[k]) for k in ("src", "tgt", "nrm", "idx", "dists"))
    st = L.stream()
    o = Odo(prev=_rigid(8))                                   # never initialised: all NaN
    state, T32, step32, prev, pose, ws = (L.ptr(t) for t in (o.state, o.T32, o.step32, o.prev, o.pose, o.ws))
    out = _nan(29, torch.float64)
    out29 = L.ptr(out)
    lm = (2.0, 1.0, 1.0, 200.0)

    def refused(name, *args):
        with pytest.raises(E, match=name):
            L.call(name, *args)
        torch.cuda.synchronize()
        assert _untouched(o.state, o.T32, o.step32, o.pose, o.ws, out), f"{name}: an output changed although the call was refused"

    # null pointers
    refused("e2e_icp_normal_equations", src, tgt, nrm, idx, dists, -1.0, 63, None, ws, st)
    refused("e2e_icp_update", None, state, T32, step32, prev, pose, 0, 0, *lm, st)
    for args in ((None, T32, step32), (state, None, step32), (state, T32, None)):
        refused("e2e_icp_state_init", *args, prev, pose, 1e-8, st)
        refused("e2e_icp_update", out29, *args, prev, pose, 0, 0, *lm, st)
        refused("e2e_icp_reduce_update", src, tgt, nrm, idx, dists, -1.0, 63, ws, *args, prev, pose, 0, 0, *lm, st)
    # pose_out without prev_pose
    refused("e2e_icp_state_init", state, T32, step32, None, pose, 1e-8, st)
    refused("e2e_icp_update", out29, state, T32, step32, None, pose, 0, 0, *lm, st)
    refused("e2e_icp_reduce_update", src, tgt, nrm, idx, dists, -1.0, 63, ws, state, T32, step32, None, pose, 0, 0, *lm, st)
    # n = 0
    refused("e2e_icp_normal_equations", src, tgt, nrm, idx, dists, -1.0, 0, out29, ws, st)
    refused("e2e_icp_reduce_update", src, tgt, nrm, idx, dists, -1.0, 0, ws, state, T32, step32, prev, pose, 0, 0, *lm, st)
    # a threshold without distances
    for thresh in (0.0, 0.25):
        refused("e2e_icp_normal_equations", src, tgt, nrm, idx, None, thresh, 63, out29, ws, st)
        refused("e2e_icp_reduce_update", src, tgt, nrm, idx, None, thresh, 63, ws, state, T32, step32, prev, pose, 0, 0, *lm, st)
    # (mode, phase)
    for mode, phase in ((0, 1), (2, 0), (1, 2), (-1, 0)):
        refused("e2e_icp_update", out29, state, T32, step32, prev, pose, mode, phase, *lm, st)
        refused("e2e_icp_reduce_update", src, tgt, nrm, idx, dists, -1.0, 63, ws, state, T32, step32, prev, pose, mode, phase, *lm, st)
    # dsratio = 0, tgt_capacity = 0
    Vg, depth, sub, status = torch.ones(4, 4, 3, device=DEV), torch.ones(4, 4, device=DEV), _nan(48), _poison(1, torch.int32)
    with pytest.raises(E, match="e2e_icp_source_subsample"):
        L.call("e2e_icp_source_subsample", L.ptr(Vg), L.ptr(depth), 4, 4, 0, L.ptr(sub), L.ptr(status), st)
    fm, _, P = _active_case()
    tgt_o, tgt_n, tcount = _nan(3 * P), _nan(3 * P), _poison(3)
    for ds, tcap in ((0, P), (4, 0)):
        with pytest.raises(E, match="e2e_pf_active_subsample_dev"):
            L.call("e2e_pf_active_subsample_dev", map_points=L.ptr(fm.points), map_normals=L.ptr(fm.normals), map_count_dev=L.ptr(fm.count),
                   map_capacity=fm.cap, workspace=L.ptr(fm.ws), H=fm.H, W=fm.W, dsratio=ds, tgt=L.ptr(tgt_o), tgt_normals=L.ptr(tgt_n),
                   tgt_count_dev=L.ptr(tcount), tgt_capacity=tcap, stream=st)
    torch.cuda.synchronize()
    assert _untouched(sub, tgt_o, tgt_n) and (status == POISON).all() and (tcount == POISON).all()
