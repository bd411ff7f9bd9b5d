"""tests/icp_ref.py, the references of tests/test_gpu_icp_contracts.py, checked on the host -- and the two Python restatements of the
se(3) exponential (e2ehip.icp.se3_exp, oracle.icp.se3_exp; csrc/icp.hip's icp_se3_exp is the third, checked on the GPU) against the
true exponential over the whole range of angles (CPU only)."""
import numpy as np
import pytest

import icp_ref

SE3_BOUND = 2e-14


def test_expm_twist_matches_scipy():
    """50 random twists against scipy.linalg.expm at 1e-14 (max abs over the 16 entries).  scipy's float64 Pade result is itself only that
    good for |w| < 2.5 (there its rotation block is orthogonal to 6e-15; from |w| = 3 up R R^T - I reaches 1e-13 .. 2.8e-13 and the
    difference to the series 4e-14 .. 1.2e-13, measured over 200 twists per unit of |w|), so the twists of THIS comparison have
    |w| <= 2.5; the test below covers |w| up to 10 with identities that need no second implementation."""
    from scipy.linalg import expm
    rng = np.random.default_rng(1)
    for _ in range(50):
        w = rng.standard_normal(3)
        xi = np.concatenate([rng.uniform(-5, 5, 3), w * (rng.uniform(0, 2.5) / np.linalg.norm(w))])
        E = icp_ref.expm_twist(xi)
        assert E.dtype == np.longdouble
        assert np.abs(E.astype(np.float64) - expm(icp_ref.twist_matrix(xi, np.float64))).max() <= 1e-14
    assert np.array_equal(icp_ref.expm_twist(np.zeros(6)), np.eye(4))


def test_expm_twist_is_a_group_exponential_up_to_ten_radians():
    """what only the true exponential satisfies, in extended precision (eps 1.1e-19; 1e-16 leaves room for |v| = 5 and 6 squarings):
    exp(xi) exp(-xi) = I, exp(xi) = exp(xi / 2)^2 (halving is exact in binary), the rotation block orthogonal with determinant 1 and rotating
    about w by |w| (trace = 1 + 2 cos |w|), the translation along a pure screw axis (v parallel to w) equal to v."""
    rng = np.random.default_rng(2)
    I4 = np.eye(4, dtype=np.longdouble)
    for _ in range(50):
        w, th = rng.standard_normal(3), rng.uniform(0, 10)
        xi = np.concatenate([rng.uniform(-5, 5, 3), w * (th / np.linalg.norm(w))])
        E, h = icp_ref.expm_twist(xi), icp_ref.expm_twist(xi / 2)
        assert np.abs(E @ icp_ref.expm_twist(-xi) - I4).max() < 1e-16
        assert np.abs(h @ h - E).max() < 1e-16
        R = E[:3, :3]
        assert np.abs(R @ R.T - I4[:3, :3]).max() < 1e-16 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-14
        assert abs(float(np.trace(R)) - (1 + 2 * np.cos(np.linalg.norm(xi[3:])))) < 4e-15      # |w| itself is a float64 here: 2 ulp(10)
        assert np.abs(R @ xi[3:].astype(np.longdouble) - xi[3:]).max() < 1e-16
        screw = np.concatenate([xi[3:] * 0.25, xi[3:]])                      # exactly parallel
        assert np.abs(icp_ref.expm_twist(screw)[:3, 3] - screw[:3]).max() < 1e-16 and np.array_equal(E[3], I4[3])


def lu_row_swaps(A):
    """number of row exchanges of a plain LU with partial pivoting (first largest |entry| of the column, as LAPACK's idamax)"""
    A = np.array(A, np.float64)
    swaps = 0
    for k in range(len(A) - 1):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        if p != k:
            A[[k, p]] = A[[p, k]]
            swaps += 1
        A[k + 1:] -= np.outer(A[k + 1:, k] / A[k, k], A[k])
    return swaps


def test_pivoting_systems_swap_rows_and_stay_well_conditioned():
    systems = icp_ref.pivoting_systems()
    assert len(systems) >= 4
    assert lu_row_swaps(np.diag([3.0, 2.0, 1.0]) + 0.1) == 0 and lu_row_swaps(np.array([[1.0, 2.0], [3.0, 4.0]])) == 1
    for A, b in systems:
        assert A.shape == (6, 6) and b.shape == (6,) and np.array_equal(A, A.T) and np.linalg.eigvalsh(A).min() > 0
        for lam in (0.0, 1e-8, 1.0):                      # the dampings the GPU test adds
            Al = A + lam * np.eye(6)
            assert lu_row_swaps(Al) >= 2 and np.linalg.cond(Al) < 1e5


def test_normal_equations_reference_on_a_hand_case():
    """two points, one dropped by keep: the sums of the remaining one, written out"""
    src = np.array([[1.0, 2.0, 3.0], [9.0, 9.0, 9.0]], np.float32)
    tgt = np.array([[0.0, 0.0, 0.0], [1.5, 2.0, 2.0]], np.float32)
    nrm = np.array([[1.0, 0.0, 0.0], [0.0, 0.6, 0.8]], np.float32)
    sums, scales = icp_ref.normal_equations(src, tgt, nrm, [1, 0], [True, False])
    n = nrm[1].astype(np.float64)
    a = np.array([n[0], n[1], n[2], 2 * n[2] - 3 * n[1], 3 * n[0] - 1 * n[2], 1 * n[1] - 2 * n[0]])
    b = n[1] * 0.0 + n[2] * -1.0
    A, Atb, cnt, err = icp_ref.unpack(sums)
    np.testing.assert_allclose(A, np.outer(a, a), rtol=0, atol=1e-15)
    np.testing.assert_allclose(Atb, a * b, rtol=0, atol=1e-15)
    assert cnt == 1 and abs(err - b * b) < 1e-15
    assert (scales >= np.abs(sums)).all() and abs(float(scales[8]) - n[1] * (2 * n[2] + 3 * n[1])) < 1e-15
    assert np.array_equal(icp_ref.pack(A, Atb, cnt, err), sums.astype(np.float64))
    zero, zscale = icp_ref.normal_equations(src, tgt, nrm, [1, 0], [False, False])
    assert not zero.any() and not zscale.any()


def test_lm_step_follows_the_header():
    """the reference of e2e_icp_update on a case small enough to follow: A = I, no damping"""
    st0 = icp_ref.initial_state(160, 0.0)
    xi = np.array([0.1, 0.0, 0.0, 0.0, 0.0, 0.0])
    st, T32, step32, pose = icp_ref.lm_step(st0, icp_ref.pack(np.eye(6), xi, 100, 2.0), 0, 0, prev_pose=np.eye(4, dtype=np.float32))
    assert np.array_equal(st[16:22], xi) and st[25] == 1 and (st[32], st[33]) == (100, 2.0)
    assert abs(st[3] - 0.1) < 1e-16 and T32.dtype == np.float32 and np.array_equal(pose, T32) and step32 is None
    # gradicp: phase 0 leaves T, phase 1 with an unchanged error halves the step
    st, _, step32, _ = icp_ref.lm_step(st0, icp_ref.pack(np.eye(6), xi, 100, 2.0), 1, 0)
    assert st[25] == 0 and st[23] == 0.02 and np.array_equal(st[:16], st0[:16]) and step32[0, 3] == np.float32(0.1)
    st[22] = 1.0
    st2, _, _, _ = icp_ref.lm_step(st, icp_ref.pack(np.zeros((6, 6)), np.zeros(6), 50, 1.0), 1, 1, lambda_max=2.0, B=1.0)
    assert abs(st2[3] - 0.05) < 1e-16 and st2[25] == 1 and abs(st2[22] - (0.5 + 1.5 / 2)) < 1e-16
    # fewer than 6 inliers: stopped for good
    st3, _, step32, _ = icp_ref.lm_step(st0, icp_ref.pack(np.eye(6), xi, 5, 2.0), 0, 0)
    assert st3[24] == 1 and np.array_equal(step32, np.eye(4)) and np.array_equal(st3[:16], st0[:16])
    st4, _, _, _ = icp_ref.lm_step(st3, icp_ref.pack(np.eye(6), xi, 100, 2.0), 0, 0)
    assert np.array_equal(st4, st3)


@pytest.mark.parametrize("which", ["e2ehip", "oracle"])
def test_se3_exp_restatements_match_the_true_exponential(which):
    """max |se3_exp(xi) - expm(twist(xi))| over the 16 entries <= 2e-14 max(1, |v|_inf), 200 directions per angle.  With the former
    closed form from 1e-8 up this measured 6.8e-9 at |w| = 1e-8, 5.5e-11 at 1e-6 and 3.2e-13 at 1e-4; with the series below 1e-2 the worst
    is 2.4e-16 below the cut-over and 2.6e-15 just above it (|w| = 1.01e-2, closed form)."""
    if which == "e2ehip":
        from e2ehip.icp import se3_exp
    else:
        from oracle.icp import se3_exp
    worst = {}
    for th, xi in icp_ref.sweep_twists():
        err = float(np.abs(se3_exp(xi) - icp_ref.expm_twist(xi)).max()) / max(1.0, np.abs(xi[:3]).max())
        worst[th] = max(worst.get(th, 0.0), err)
    print({th: f"{e:.1e}" for th, e in worst.items()})
    bad = {th: e for th, e in worst.items() if not e <= SE3_BOUND}
    assert not bad, bad
