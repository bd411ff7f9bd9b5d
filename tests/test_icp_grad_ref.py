"""Pins tests/icp_grad_ref.py, the float64 restatement of the ICP / GradICP loop that the GPU adjoint (tests/test_gpu_pose_grad.py) is
compared with: it computes what oracle/icp.py computes, its autograd gradient is the derivative of that computation with the neighbour
lists held fixed (central differences), and on the test scenes every nearest neighbour wins by a margin that float32 searches cannot
overturn.  CPU only.

Unconverged runs (1, 2, 3 iterations) on purpose: at convergence the gradient does not depend on the path, so only these exercise the
adjoints of the damping update and of the gate."""
import numpy as np
import pytest
import torch

import icp_grad_ref as R
from oracle import icp as oicp

DAMP = 1e-3
THRESH = 0.012
MODES = {"icp": dict(mode="icp"), "gradicp-nu200": dict(mode="gradicp", nu=200.0), "gradicp-nu2e4": dict(mode="gradicp", nu=2e4)}
CASES = [(7, 8, None), (150, 12, None), (333, 12, None), (333, 12, THRESH)]


def _loss_grad(src, tgt, tgt_n, C, **kw):
    s = src.double().requires_grad_(True)
    T, recs = R.icp(s, tgt, tgt_n, **kw)
    (g,) = torch.autograd.grad((C * T[:3]).sum(), s)
    return T.detach(), recs, g


@pytest.mark.parametrize("n,grid,thresh", CASES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("numiters", [1, 2, 3])
def test_restatement_matches_oracle_and_central_differences(n, grid, thresh, mode, numiters):
    tgt, tgt_n, src = R.scene(n, grid)
    kw = dict(numiters=numiters, damp=DAMP, dist_thresh=thresh, **MODES[mode])
    T_or, tr_or = oicp.point_to_plane_icp(src, tgt, tgt_n, **kw)
    T32, recs32 = R.icp(src.double(), tgt, tgt_n, round32=True, **kw)
    assert len(recs32) == len(tr_or) == numiters and [r["cnt"] for r in recs32] == [c for c, _ in tr_or]
    err = float((T32 - torch.from_numpy(T_or)).abs().max())
    print(f"restatement vs oracle: {err:.2e}")
    assert err <= 1e-8

    C = R.weights((3, 4))
    T, recs, g = _loss_grad(src, tgt, tgt_n, C, **kw)
    margin, gap = min(r["margin"] for r in recs), min(r["gap"] for r in recs)
    print(f"neighbour margin {margin:.2f}, threshold gap {gap:.2e}, inliers {[r['cnt'] for r in recs]}")
    assert margin >= 1.5
    # float32 clouds and poses move a distance by ~1e-7 m (6e-8 x 0.6 m coordinates, poses within 1e-7), 1e-5 of the 12 mm threshold:
    # ten times that gap and every path classifies every source alike
    assert gap >= 1e-4
    if thresh is not None:
        assert 6 <= recs[0]["cnt"] < n // 2 and all(r["cnt"] == n for r in recs[1:])      # the keep mask bites, then lets everything in

    # central differences over every coordinate, neighbour lists and keep masks forced, as one batched call
    h = 1e-6
    E = torch.eye(3 * n, dtype=torch.float64).reshape(3 * n, n, 3) * h
    base = src.double()
    Tp, _ = R.icp(base + E, tgt, tgt_n, forced=recs, **kw)
    Tm, _ = R.icp(base - E, tgt, tgt_n, forced=recs, **kw)
    fd = ((C * (Tp - Tm)[:, :3]).sum((-1, -2)) / (2 * h)).reshape(n, 3)
    rel = float((fd - g).abs().max() / g.abs().max())
    print(f"|grad| max {float(g.abs().max()):.3f}, central differences rel {rel:.2e}")
    assert rel <= (1e-4 if n == 7 else 1e-7)


def test_modes_differ_when_unconverged_and_agree_when_converged():
    """The path matters only before convergence: after 3 iterations icp's and gradicp's gradients differ by percents, after 20 they agree."""
    tgt, tgt_n, src = R.scene(333, 12)
    C = R.weights((3, 4))
    g = {(m, k): _loss_grad(src, tgt, tgt_n, C, numiters=k, damp=DAMP, **MODES[m])[2] for m in ("icp", "gradicp-nu200") for k in (3, 20)}
    d3 = float((g["icp", 3] - g["gradicp-nu200", 3]).abs().max() / g["icp", 3].abs().max())
    d20 = float((g["icp", 20] - g["gradicp-nu200", 20]).abs().max() / g["icp", 20].abs().max())
    print(f"icp vs gradicp gradient: 3 iterations {d3:.2e}, 20 iterations {d20:.2e}")
    assert d3 > 1e-2 and d20 < 1e-4
