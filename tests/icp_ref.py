"""Test references for the ICP odometry's entry points (no fixtures; tests/test_icp_ref.py checks them on the host and
tests/test_gpu_icp_contracts.py compares the kernels of csrc/icp.hip with them).

Plain numpy, written from the contracts include/e2eslam.h states -- not from oracle/icp.py and not from the kernels' formulas: the se(3)
exponential is the matrix exponential of the 4x4 twist (no Rodrigues formula), the 29 sums are extended-precision sums of the products
as the header writes them, the solve is numpy's."""
import numpy as np

LD = np.longdouble
STATE_T, STATE_XI, STATE_LAMBDA, STATE_ERR0, STATE_STOPPED, STATE_ITERS, STATE_DAMP, STATE_TRACE, TRACE_SLOTS = 0, 16, 22, 23, 24, 25, 26, 32, 64


def twist_matrix(xi, dtype=LD):
    """xi = (v, omega) -> the 4x4 element of se(3): [[hat(omega), v], [0, 0]]"""
    v, w = [dtype(x) for x in xi[:3]], [dtype(x) for x in xi[3:]]
    M = np.zeros((4, 4), dtype)
    M[0, 1], M[0, 2], M[1, 2] = -w[2], w[1], -w[0]
    M[1, 0], M[2, 0], M[2, 1] = w[2], -w[1], w[0]
    M[:3, 3] = v
    return M


def expm_twist(xi):
    """exp of the 4x4 twist of xi in np.longdouble: scale by 2^-s until max|M| <= 0.25, 40 Taylor terms, square s times.
    (max|M| <= 0.25 bounds the 4x4 matrix's norm by 1: term 40 is below 1 / 40! ~ 1e-48 of the first.)"""
    M = twist_matrix(xi)
    s = 0
    while np.abs(M).max() > LD(0.25):
        M = M / LD(2)
        s += 1
    E, term = np.eye(4, dtype=LD), np.eye(4, dtype=LD)
    for k in range(1, 41):
        term = term @ M / LD(k)
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def normal_equations(src, tgt, nrm, idx, keep):
    """The 29 numbers of e2e_icp_normal_equations over the sources with keep[i], in np.longdouble: (sums, scales), both (29,).
    scales[k] is the sum of the absolute values of the terms of sums[k], the terms taken at the level the contract writes them:
    a cross-product component s_p n_q - s_q n_p counts |s_p n_q| + |s_q n_p|, the residual n . (t - s) counts sum_k |n_k (t_k - s_k)|,
    and a product of two such factors counts the product of their absolute sums.  A float64 evaluation of the contract's expressions
    in any order has an error of a few ulp of THIS number per addition level, whatever cancels inside a factor or between points."""
    keep = np.asarray(keep, bool)
    idx = np.asarray(idx)[keep]
    s = np.asarray(src, np.float32)[keep].astype(LD)
    t = np.asarray(tgt, np.float32)[idx].astype(LD)
    n = np.asarray(nrm, np.float32)[idx].astype(LD)
    a = np.concatenate([n, np.cross(s, n)], 1)                                                  # (m, 6)
    a_abs = np.concatenate([np.abs(n), np.abs(s[:, [1, 2, 0]] * n[:, [2, 0, 1]]) + np.abs(s[:, [2, 0, 1]] * n[:, [1, 2, 0]])], 1)
    b = (n * (t - s)).sum(1)
    b_abs = np.abs(n * (t - s)).sum(1)
    sums, scales = np.zeros(29, LD), np.zeros(29, LD)
    k = 0
    for r in range(6):
        for c in range(r, 6):
            sums[k], scales[k] = (a[:, r] * a[:, c]).sum(), (a_abs[:, r] * a_abs[:, c]).sum()
            k += 1
    for r in range(6):
        sums[21 + r], scales[21 + r] = (a[:, r] * b).sum(), (a_abs[:, r] * b_abs).sum()
    sums[27] = scales[27] = LD(len(s))
    sums[28], scales[28] = (b * b).sum(), (b_abs * b_abs).sum()
    return sums, scales


def unpack(out29):
    """-> (A^T A (6,6), A^T b (6,), count, sum r^2), float64"""
    v = np.asarray(out29, np.float64)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = v[:21]
    return A + np.triu(A, 1).T, v[21:27].copy(), float(v[27]), float(v[28])


def pack(A, b, cnt, err):
    """out29 from a symmetric 6x6 matrix, a right-hand side, an inlier count and a residual sum"""
    return np.concatenate([np.asarray(A, np.float64)[np.triu_indices(6)], np.asarray(b, np.float64), [float(cnt), float(err)]])


def initial_state(n, damp):
    st = np.zeros(n)
    st[STATE_T:STATE_T + 16] = np.eye(4).reshape(-1)
    st[STATE_LAMBDA] = st[STATE_DAMP] = damp
    return st


def lm_step(state, out29, mode, phase, lambda_max=2.0, B=1.0, B2=1.0, nu=200.0, T32=None, step32=None, prev_pose=None, pose_out=None):
    """One e2e_icp_update as include/e2eslam.h states it, on a float64 state vector.  Returns new (state, T32, step32, pose_out);
    what the contract leaves alone is returned as given (None stays None)."""
    st = np.array(state, np.float64)
    T32, step32, pose_out = (None if x is None else np.array(x, np.float32) for x in (T32, step32, pose_out))
    if st[STATE_STOPPED] != 0:
        return st, T32, step32, pose_out
    A, b, cnt, err = unpack(out29)

    def advance(xi):
        T = (expm_twist(xi) @ st[STATE_T:STATE_T + 16].reshape(4, 4).astype(LD))
        st[STATE_T:STATE_T + 16] = T.astype(np.float64).reshape(-1)
        st[STATE_ITERS] += 1
        pose = None if prev_pose is None else (T.astype(np.float64) @ np.asarray(prev_pose, np.float64)).astype(np.float32)
        return T.astype(np.float64).astype(np.float32), pose

    if phase == 0:
        if cnt < 6:
            st[STATE_STOPPED] = 1.0
            return st, T32, np.eye(4, dtype=np.float32), pose_out
        xi = np.linalg.solve(A + st[STATE_LAMBDA] * np.eye(6), b)
        st[STATE_XI:STATE_XI + 6] = xi
        it = int(st[STATE_ITERS])
        if it < TRACE_SLOTS:
            st[STATE_TRACE + 2 * it], st[STATE_TRACE + 2 * it + 1] = cnt, err
        if mode == 0:
            T32, pose_out = advance(xi)
        else:
            st[STATE_ERR0] = err / max(cnt, 1.0)
            step32 = expm_twist(xi).astype(np.float64).astype(np.float32)
    else:
        delta = err / max(cnt, 1.0) - st[STATE_ERR0]
        with np.errstate(over="ignore"):
            st[STATE_LAMBDA] *= 1.0 / lambda_max + (lambda_max - 1.0 / lambda_max) / (1.0 + B * np.exp(-B2 * nu * delta))
        gate = 1.0 / (1.0 + np.exp(np.clip(nu * delta, -60.0, 60.0)))
        T32, pose_out = advance(gate * st[STATE_XI:STATE_XI + 6])
    return st, T32, step32, pose_out


# the angles at which a restatement can go wrong: 0, both sides of the former small-angle cut (1e-8) where 1 - cos(th) and th - sin(th)
# cancel completely, both sides of the series cut-over (1e-2), past pi and past 2 pi
ANGLES = (0, 1e-12, 9.9e-9, 1e-8, 1.0001e-8, 1e-6, 1e-4, 1e-3, 9.99e-3, 1e-2, 1.01e-2, 0.1, 1, 3.1, 6.2, 10)


def sweep_twists(per_angle=200, vmax=5.0, seed=0):
    """[(|w|, xi)]: per_angle random directions for each angle of ANGLES, |v| uniform in [0, vmax]"""
    rng = np.random.default_rng(seed)
    out = []
    for th in ANGLES:
        for _ in range(per_angle):
            d, v = rng.standard_normal(3), rng.standard_normal(3)
            out.append((th, np.concatenate([v * (rng.uniform(0, vmax) / np.linalg.norm(v)), d * (th / np.linalg.norm(d))])))
    return out


PIVOT_SEEDS = (0, 2, 3, 4, 9, 21)         # 2 to 4 row exchanges at condition numbers 2.8e3 .. 4.1e4, with 0, 1e-8 or 1 added to the diagonal


def pivoting_systems():
    """[(A, b)]: 6x6 symmetric positive definite A = M^T M whose LU with partial pivoting exchanges rows (a diagonally dominant A^T A,
    as the odometry scenes of the suite give, never does), and right-hand sides.  M: random 8x6 with column scales 0.2 .. 8 -- the
    large entries sit in the LAST rows and columns -- and a multiple of the last column added to the first, so the first column's
    largest entry is not on the diagonal either.  The seeds are chosen so that every system swaps at least 2 rows at a condition
    number below 1e5 (tests/test_icp_ref.py asserts both)."""
    out = []
    for seed in PIVOT_SEEDS:
        rng = np.random.default_rng(1000 + seed)
        M = rng.standard_normal((8, 6)) * np.array([0.2, 0.5, 1.0, 2.0, 4.0, 8.0])
        M[:, 0] += rng.uniform(0.05, 0.2) * M[:, 5]
        out.append((M.T @ M, rng.standard_normal(6) * 10.0))
    return out
