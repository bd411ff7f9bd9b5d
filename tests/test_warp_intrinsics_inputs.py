"""Host-only proof of what tests/warp_intrinsics_ref.py claims: the closed form of include/e2eslam.h equals float64 autograd of the oracle
composition, the rows and columns that must be zero are zero, every admitted case has an empty exclusion set, the float32 reference stays
inside its own bound, the operator references stay clear of the z clamp, and the CPU self-calibration run that the GPU test is compared
with reduces the loss and the focal error."""
import pytest
import torch

import warp_geo_ref as G
import warp_intrinsics_ref as I
import warp_window_ref as Wr
from warp_contract_ref import F32, F64


@pytest.mark.parametrize("shape,pad,use_mask", I.PAIR_CASES, ids=str)
def test_closed_form_equals_float64_autograd(shape, pad, use_mask):
    """measured: <= 1e-15 of the largest entry on the thirteen cases; 1e-12 is asked for"""
    c = I.pair_case(shape, pad, use_mask)
    assert not c["grad_excluded"].any(), "a pose case whose exclusion set is not empty"
    for got, which in zip(I.closed_form(c), I.MATRICES):
        want = c[F64][which]
        top = float(want.abs().max())
        e = float((got - want).abs().max())
        assert top > 0 and e <= 1e-12 * top, f"{which}: {e:.3e} of {top:.3e}"
        assert float(got[:, 3].abs().max()) == 0.0 and float(want[:, 3].abs().max()) == 0.0, f"{which}: row 3 is not zero"
    for r in (c[F64], c[F32]):
        assert float(r["g_invK"][:, :, 3].abs().max()) == 0.0, "g_inv_K: column 3 is not zero"
    # with K and inv_K as leaves the other gradients are those of the pose module's composition
    import warp_pose_ref as P
    p = P.pose_case(shape, pad, use_mask)
    assert torch.equal(c[F64]["g_T"], p[F64]["g_T"]) and torch.equal(c[F32]["g_T"], p[F32]["g_T"])


def test_the_float32_reference_stays_inside_its_bound_and_the_measured_figures():
    worst = {w: 0.0 for w in I.MATRICES}
    for k in I.PAIR_CASES:
        c = I.pair_case(*k)
        for w in I.MATRICES:
            e = float((c[F32][w].double() - c[F64][w]).abs().max())
            assert e <= I.bound("pair", c, w), (k, w)
            worst[w] = max(worst[w], I.rel_error(c, w))
    print(f"\nfloat32 autograd against float64, relative to the largest entry: K {worst['g_K']:.2e}, inv_K {worst['g_invK']:.2e}")
    assert 0 < worst["g_K"] < 1e-4 and 0 < worst["g_invK"] < 1e-4


def test_zero_and_expanded_cases():
    z = I.pair_case(*I.ZERO_CASE)
    for dt in (F64, F32):
        assert float(z[dt]["g_K"].abs().max()) == 0.0 and float(z[dt]["g_invK"].abs().max()) == 0.0
    e = I.pair_case(*I.EXPANDED_CASE, expanded=True)
    assert not e["grad_excluded"].any(), "the expanded case is not admitted"
    assert e[F64]["g_K"].shape == (4, 4) and e[F64]["g_invK"].shape == (4, 4)
    got = [m.sum(0) for m in I.closed_form(e)]                       # one matrix behind both batch elements gets the sum
    for g, w in zip(got, I.MATRICES):
        assert float((g - e[F64][w]).abs().max()) <= 1e-12 * float(e[F64][w].abs().max())


def test_window_cases_are_admitted_and_s2_is_the_sum_over_the_sources():
    assert {c[3] for c in I.WINDOW_CASES} == set(I.MODES) and len(I.WINDOW_CASES) == len(set(I.WINDOW_CASES))
    for k in I.WINDOW_CASES:
        c = I.window_case(*k)
        assert not c["grad_excluded"].any(), f"{k}: exclusion set not empty"
        for w in I.MATRICES:
            assert float((c[F32][w].double() - c[F64][w]).abs().max()) <= I.bound("window", c, w), (k, w)
            assert float(c[F64][w][:, 3].abs().max()) == 0.0
    # flags off, S = 2: the loss is the mean of the two sources' maps, so the gradient is half the sum of the one-source gradients
    shape, pad, mask = (2, 9, 33), 1, 1
    both = I.window_case(shape, pad, mask, (2, 0, 0))[F64]
    s2, Kl, iKl, base = I._window_maps(shape, pad, mask, F64)
    for k, w in enumerate(I.MATRICES):
        per = [torch.autograd.grad(base["rep"][:, s].mean(), (Kl, iKl), retain_graph=True)[k] for s in range(2)]
        assert float((both[w] - (per[0] + per[1]) / 2).abs().max()) <= 1e-12 * float(both[w].abs().max())


def test_geo_cases():
    adm = [k for k in I.GEO_CASES if I.geo_case(*k)["admitted"]]
    print(f"\n{len(adm)} of {len(I.GEO_CASES)} geometric cases admitted on this machine")
    assert {k for k in I.GEO_CASES if k[0] == (1, 3, 5)} <= set(adm), "every case of (1,3,5) is admitted whatever the machine"
    assert any(k[0][0] == 2 and k[3][0] == 2 for k in adm), "no admitted case with B = 2 and S = 2"
    for k in adm:
        c = I.geo_case(*k)
        for w in I.MATRICES:
            assert float((c[F32][w].double() - c[F64][w]).abs().max()) <= I.bound("geo", c, w), (k, w)
    # modes outside warp_geo_ref.MODES go through the same admission rule
    assert set(I.MODES) - set(G.MODES) == {(1, 0, 0)} and set(I.MODES) - set(Wr.MODES) == {(1, 0, 0)}


@pytest.mark.parametrize("shape", I.OP_SHAPES, ids=str)
def test_operator_references(shape):
    c = I.operator_case(*shape)
    for dt in (F64, F32):
        assert float(c[dt]["c2"].min()) > 0.1, "a projected point near the clamp of z_out"
        assert float(c[dt]["g_K"][:, 3].abs().max()) == 0.0 and float(c[dt]["g_invK"][:, 3].abs().max()) == 0.0
        assert float(c[dt]["g_invK"][:, :, 3].abs().max()) == 0.0
        assert not torch.equal(c[dt]["g_K"], c[dt]["g_K_z"])
    # the closed forms of the header
    B, H, W = shape
    from oracle import warp_loss as wl
    s = c["scene"]
    Q = torch.matmul(c["g_cam"][:, :3].double(), (s["depth"].double().view(B, 1, H * W) * wl.pixel_grid(B, H, W, F64)).transpose(1, 2))
    assert float((Q - c[F64]["g_invK"][:, :3, :3]).abs().max()) <= 1e-12 * float(Q.abs().max())


def test_cpu_self_calibration_reduces_the_loss_and_the_focal_error():
    RECOVERY = I.RECOVERY
    s, src, tgt = I.recovery_scene()
    f, trace = I.cpu_learn_intrinsics(s["depth"], src, tgt, s["K"], s["T"], RECOVERY["steps"], RECOVERY["lr"], RECOVERY["init"])
    err0 = max(abs(RECOVERY["init"][0] - 1), abs(RECOVERY["init"][1] - 1))
    err1 = max(abs(float(f[0]) - 1), abs(float(f[1]) - 1))
    print(f"\nCPU self-calibration: loss {trace[0]:.5f} -> {trace[-1]:.5f}, focal error {err0:.4f} -> {err1:.4f}, factors {f.tolist()}")
    assert trace[-1] < 0.7 * trace[0] and err1 < 0.7 * err0
    Ke, inv = I.intrinsics_from_factors(s["K"], f)
    assert float((torch.matmul(Ke, inv) - torch.eye(4)).abs().max()) < 1e-5
