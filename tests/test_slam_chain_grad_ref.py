"""Pins tests/slam_chain_grad_ref.py, the float64 reference of the chain gradient that tests/test_gpu_slam_chain_grad.py compares the
GPU with: the closed forms of the target-side adjoint of one ICP reduction (include/e2eslam.h, e2e_icp_normal_equations_bwd_tgt) are
what autograd finds by walking icp_grad_ref.sums, and the chain's depth gradient is the derivative of the chain with every discrete
choice held fixed (float64 central differences).  CPU only.

The chain: the three-frame "corner" sequence at 24x32.  A first run searches freely and takes its tables from the float32 oracle
(oracle.pointfusion for the active and unique tables and the map's normals; oracle.icp cross-checks the poses); every later
evaluation is forced to the same lists.

Measured here: closed forms vs autograd 0 (g_tgt) / 2.3e-16 (g_tgt_normals), relative to the largest entry; poses vs oracle.icp at most
7.6e-8; central differences 4.9e-9 (icp) / 6.6e-9 (gradicp) of the frame's largest gradient entry; the chain moves the depth gradient
of frames 0 / 1 / 2 by 0.65 / 0.71 / 0.53 of their largest entry against the rule that holds the map and the poses constant."""
import functools

import pytest
import torch

import icp_grad_ref as I
import pointfusion_grad_ref as P
import slam_chain_grad_ref as C
from oracle import icp as oicp
from oracle import pointfusion as opf

H, W, DS, DAMP = 24, 32, 4, 1e-3
MODES = {"icp": dict(mode="icp"), "gradicp": dict(mode="gradicp", nu=200.0)}


def _rel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the closed forms of the target-side adjoint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(7, 5), (333, 40), (4099, 3)])
def test_closed_forms_are_the_autograd_of_the_sums(n, m):
    g = torch.Generator().manual_seed(100 * n + m)
    src, tgt = torch.rand(n, 3, generator=g, dtype=torch.float64), torch.rand(m, 3, generator=g, dtype=torch.float64)
    nrm = torch.nn.functional.normalize(torch.randn(m, 3, generator=g, dtype=torch.float64), dim=1)
    idx = torch.randint(0, m, (n,), generator=g)
    keep = torch.rand(n, generator=g) < 0.5
    adj = torch.randn(28, generator=g, dtype=torch.float64)
    t64, n64 = tgt.clone().requires_grad_(True), nrm.clone().requires_grad_(True)
    AtA, Atb, err = I.sums(src, t64, n64, idx, keep)
    packed = torch.stack([AtA[r, c] for r in range(6) for c in range(r, 6)])
    want = torch.autograd.grad((adj[:21] * packed).sum() + (adj[21:27] * Atb).sum() + adj[27] * err, [t64, n64])
    got = C.ne_bwd_tgt_closed_form(src, tgt, nrm, idx, keep, adj)
    for name, a, b in zip(("g_tgt", "g_tgt_normals"), got, want):
        e = _rel(a, b)
        print(f"{name} (n={n}, m={m}): {e:.2e}, max |ref| {float(b.abs().max()):.3e}")
        # float64 sums of up to 4099 / 3 terms of one sign pattern: n eps / 2 = 4.6e-13 is the worst case for any order of summation
        assert e <= 1e-12
    named = torch.zeros(m, dtype=torch.bool)
    named[idx[keep]] = True
    assert all(float(a[~named].abs().max() if (~named).any() else 0.0) == 0.0 for a in got)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def _sequence():
    from e2ehip.synthetic import make_sequence
    colors, depths, K, poses = make_sequence(3, H, W, seed=3, step=0.02, noise=0.0, scene="corner")
    return colors[0], depths[0, ..., 0], K[0, 0], poses[0]


@functools.lru_cache(maxsize=None)
def _free_run(mode):
    """The chain with free searches: per frame the float64 localisation against the float32 oracle's map, then the oracle's map step
    with that pose.  -> steps (the discrete choices), the oracle's final state, the poses (float32), oracle.icp's poses."""
    rgbs, depths, K, poses_gt = _sequence()
    kw = dict(numiters=20, damp=DAMP, **MODES[mode])
    state, steps, poses, oracle_poses = opf.empty_state(), [], [poses_gt[0]], [poses_gt[0].double()]
    state, tab = opf.pointfusion_step(state, rgbs[0], depths[0], K, poses[0])
    steps.append(dict(unique=tab["unique"], sel=None, records=None, normals=None))
    for f in (1, 2):
        sel = opf.find_active_map_points(state["points"], K, poses[-1], H, W)[::DS, 0]
        pose64, recs = C.localise(state["points"].double(), state["normals"], depths[f].double(), K, poses[-1], sel, None, DS, **kw)
        assert len(recs) == 20 and recs[0]["idx"].numel() == 48
        oracle_poses.append(torch.from_numpy(oicp.frame_to_model(state["points"], state["normals"], depths[f], K, poses[-1], dsratio=DS, **kw)[0]))
        normals = state["normals"]
        poses.append(pose64.float())
        state, tab = opf.pointfusion_step(state, rgbs[f], depths[f], K, poses[-1])
        assert tab["unique"].shape[0] > 0
        steps.append(dict(unique=tab["unique"], sel=sel, records=recs, normals=normals))
    return steps, state, poses, oracle_poses


def _gradients(mode, steps, chain_rule=True):
    rgbs, depths, K, poses_gt = _sequence()
    d64 = [d.double().requires_grad_(True) for d in depths]
    kw = dict(numiters=20, damp=DAMP, **MODES[mode])
    state, poses = C.chain([c.double() for c in rgbs], d64, K, poses_gt[0], steps, DS, **kw)
    if not chain_rule:
        # the rule without the chain: the map is a constant of the localisation, prev_pose and the map step's pose are constants
        state, poses, pts = P.empty_state(), [poses_gt[0].double()], None
        for f in range(3):
            if f:
                pose, _ = C.localise(pts.detach(), steps[f]["normals"], d64[f], K, poses[-1].detach(), steps[f]["sel"], steps[f]["records"], DS, **kw)
                poses.append(pose)
            state = P.step(state, rgbs[f].double(), d64[f], K, poses[-1].detach(), steps[f]["unique"])
            pts = state["points"]
    return state, poses, torch.autograd.grad(C.scalar(state, poses), d64)


@pytest.mark.parametrize("mode", list(MODES))
def test_chain_reference_gradient_is_the_central_difference(mode):
    rgbs, depths, K, poses_gt = _sequence()
    steps, st32, poses32, oracle_poses = _free_run(mode)
    state, poses, grads = _gradients(mode, steps)
    for k in ("points", "colors", "ccounts"):
        e = _rel(st32[k], state[k].detach())
        print(f"{k} vs the float32 oracle: {e:.2e}")
        assert e <= 1e-6                                                 # float32 arithmetic on values of order 1: a few ulp
    for f in (1, 2):
        e = _rel(oracle_poses[f], poses[f].detach())
        print(f"pose {f} vs oracle.icp: {e:.2e}")
        assert e <= 1e-5                                                 # twenty iterations on float32 clouds against float64 ones
    kw = dict(numiters=20, damp=DAMP, **MODES[mode])
    c64, d64 = [c.double() for c in rgbs], [d.double() for d in depths]

    def value(f, idx, delta):
        d = [t.clone() for t in d64]
        d[f][idx] += delta
        return float(C.scalar(*C.chain(c64, d, K, poses_gt[0], steps, DS, **kw)))

    # per frame: two pixels the odometry uses as sources (multiples of DS; frame 0 has none), two it does not, a corner
    h, worst = 1e-6, 0.0
    for f in range(3):
        for idx in [(4, 8), (16, 20), (5, 9), (13, 2), (H - 1, W - 1)]:
            fd = (value(f, idx, h) - value(f, idx, -h)) / (2 * h)
            worst = max(worst, abs(fd - float(grads[f][idx])) / float(grads[f].abs().max()))
    print(f"central differences ({mode}): {worst:.2e}")
    # h = 1e-6 on a float64 scalar of some 1e4 terms of order 1 that passes through forty 6x6 solves: its rounding, about 1e-12, over
    # 2h is 5e-7 absolute against gradients whose largest entry is of order 10 to 100
    assert worst <= 1e-6
    # the chain is not a small correction of the rule that holds the map and the poses constant
    _, _, flat = _gradients(mode, steps, chain_rule=False)
    moved = [float((a - b).abs().max() / a.abs().max()) for a, b in zip(grads, flat)]
    print(f"share of the depth gradient the chain adds ({mode}):", [f"{m:.2f}" for m in moved])
    assert all(m > 0.1 for m in moved)
