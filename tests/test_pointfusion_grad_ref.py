"""Pins tests/pointfusion_grad_ref.py, the float64 restatement of the PointFusion map step that the GPU adjoint
(tests/test_gpu_pointfusion_grad.py) is compared with: over a 3-frame chain it computes what oracle.pointfusion.pointfusion_step
computes, its autograd gradient is the one autograd finds by walking the float32 oracle itself, and it is the derivative of the
computation with the association held fixed (float64 central differences).  CPU only.

Measured here (24x32 / 48x64), largest absolute difference over the largest entry of the float64 tensor:
  values vs the float32 oracle       points 1.7e-7 / 1.9e-7, colors 1.6e-7 / 1.5e-7, ccounts 5.5e-7 / 5.6e-7
  gradients vs the oracle's autograd d/d depth 3.2e-6 / 5.2e-6, d/d rgb 3.0e-7 / 3.9e-7 (the largest of the three frames)
  gradients vs central differences   d/d depth 3.1e-9 / 8.3e-9, d/d rgb 3.5e-9 / 2.5e-9"""
import functools

import pytest
import torch

import pointfusion_grad_ref as R
from oracle import pointfusion as opf

SHAPES = [(24, 32), (48, 64)]


@functools.lru_cache(maxsize=None)
def _oracle_chain(H, W):
    """The float32 oracle over the three frames, with its own autograd gradient of R.scalar wrt every depth and colour."""
    rgbs, depths, K, poses = R.sequence(H, W)
    d32 = [d.clone().requires_grad_(True) for d in depths]
    c32 = [c.clone().requires_grad_(True) for c in rgbs]
    state, uniques, counts = opf.empty_state(), [], []
    for f in range(3):
        M = state["points"].shape[0]
        state, tab = opf.pointfusion_step(state, c32[f], d32[f], K, poses[f])
        uniques.append(tab["unique"])
        counts.append((tab["unique"].shape[0], state["points"].shape[0] - M, int((depths[f] == 0).sum()), tab["similar"].shape[0]))
    s = sum((R.weights(tuple(state[k].shape), i).float() * state[k]).sum() for i, k in enumerate(("points", "colors", "ccounts")))
    grads = torch.autograd.grad(s, d32 + c32)
    return {k: v.detach() for k, v in state.items()}, uniques, counts, grads[:3], grads[3:]


def _reference(H, W, uniques):
    rgbs, depths, K, poses = R.sequence(H, W)
    d64 = [d.double().requires_grad_(True) for d in depths]
    c64 = [c.double().requires_grad_(True) for c in rgbs]
    state = R.chain(c64, d64, K, poses, uniques)
    grads = torch.autograd.grad(R.scalar(state), d64 + c64)
    return state, grads[:3], grads[3:]


def _rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_matches_the_oracle_and_its_autograd(H, W):
    st32, uniques, counts, gd32, gc32 = _oracle_chain(H, W)
    print("per step (matched, appended, invalid, similar):", counts)
    if (H, W) == (24, 32):
        assert counts[2][:3] == (659, 91, 18)
    else:
        assert counts[2][0] == 2779 and counts[2][3] == 2826             # several map points contend for one pixel
    assert uniques[0].shape[0] == 0 and all(c[0] > 0 and c[1] > 0 and c[2] == 18 for c in counts[1:])
    st64, gd64, gc64 = _reference(H, W, uniques)
    for k in ("points", "colors", "ccounts"):
        assert st64[k].shape == st32[k].shape
        e = _rel(st32[k], st64[k].detach())
        print(f"{k}: {e:.2e}")
        assert e <= 1e-6                                                 # float32 arithmetic on values of order 1: a few ulp
    for f in range(3):
        ed, ec = _rel(gd32[f], gd64[f]), _rel(gc32[f], gc64[f])
        print(f"frame {f}: d/d depth {ed:.2e}, d/d rgb {ec:.2e}; max |g| {float(gd64[f].abs().max()):.3e} / {float(gc64[f].abs().max()):.3e}")
        assert float(gd64[f].abs().max()) > 0 and float(gc64[f].abs().max()) > 0       # every frame is reached
        assert float(gd64[f][2:5, 3:9].abs().max()) == 0.0                            # the hole gets nothing
        # the float32 walk takes the difference of nearby positions after scaling them: 5e-6 measured; 1e-4 is the project's ceiling for
        # float32 against float64
        assert ed <= 1e-4 and ec <= 1e-4


@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_gradient_is_the_central_difference(H, W):
    _, uniques, _, _, _ = _oracle_chain(H, W)
    rgbs, depths, K, poses = R.sequence(H, W)
    _, gd64, gc64 = _reference(H, W, uniques)
    d64, c64 = [d.double() for d in depths], [c.double() for c in rgbs]

    def value(f, which, idx, delta):
        d, c = [t.clone() for t in d64], [t.clone() for t in c64]
        (d if which == "d" else c)[f][idx] += delta
        return float(R.scalar(R.chain(c, d, K, poses, uniques)))

    # per frame: a fused pixel, an appended one (frames 1, 2), pixels next to the hole and in the corners, and colour entries of each
    fused = [set(map(tuple, u[:, 1:].tolist())) for u in uniques]
    h = 1e-6
    worst_d = worst_c = 0.0
    for f in range(3):
        valid = [(y, x) for y in range(H) for x in range(W) if depths[f, y, x] != 0]
        picks = [p for p in valid if p in fused[f]][:: max(1, len(fused[f]) // 3)][:3]
        picks += [p for p in valid if p not in fused[f]][::37][:3] + [(1, 3), (5, 9), (H - 1, W - 1)]
        assert len(picks) >= 6
        for (y, x) in picks:
            fd = (value(f, "d", (y, x), h) - value(f, "d", (y, x), -h)) / (2 * h)
            worst_d = max(worst_d, abs(fd - float(gd64[f][y, x])) / float(gd64[f].abs().max()))
            ch = (y + x) % 3
            fc = (value(f, "c", (y, x, ch), h) - value(f, "c", (y, x, ch), -h)) / (2 * h)
            worst_c = max(worst_c, abs(fc - float(gc64[f][y, x, ch])) / float(gc64[f].abs().max()))
    print(f"central differences: d/d depth {worst_d:.2e}, d/d rgb {worst_c:.2e}")
    # h = 1e-6 on a float64 sum of some 1e4 terms of order 1: its rounding, about 1e-13, over 2h is 5e-8 absolute against gradients whose
    # largest entry is about 3 -> 2e-8; the rgb dependence is linear and the depth's curvature term h^2 f''' / 6 is far below that
    assert worst_d <= 1e-7 and worst_c <= 1e-7
