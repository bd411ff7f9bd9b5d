"""float64 torch restatement of the host-driven ICP / GradICP loop (oracle/icp.py, e2ehip/icp.py) that autograd can walk: the reference
for the odometry's adjoint.  TEST INFRASTRUCTURE ONLY.

Same arithmetic as oracle.icp.point_to_plane_icp -- brute-force nearest neighbours, (A^T A + lambda I) xi = A^T b by torch.linalg.solve,
the twist exponential with the series below an angle of 1e-2, GradICP's logistic damping update and gate -- with the differentiation rule
of include/e2eslam.h: neighbour indices, keep masks and inlier counts are constants, targets are constants, the clipped part of the gate
has zero derivative.  Every function takes leading batch dimensions on `src` (with forced neighbour lists), so central differences over
all coordinates are one batched call."""
import numpy as np
import torch

TWIST = (0.008, -0.006, 0.005, 0.012, -0.009, 0.007)


def hat(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def se3_exp(xi):
    """xi (...,6) = (v, omega) -> (...,4,4); the coefficient branches of oracle.icp.se3_exp."""
    v, w = xi[..., :3], xi[..., 3:]
    t2 = (w * w).sum(-1)
    small = t2 < 1e-4
    a_s, b_s, c_s = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0), 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0), 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0)
    t2c = t2.clamp(min=1e-12)                         # keeps the unused closed forms (and their derivatives) finite at tiny angles
    th = t2c.sqrt()
    a_l, b_l, c_l = torch.sin(th) / th, (1.0 - torch.cos(th)) / t2c, (th - torch.sin(th)) / (t2c * th)
    a, b, c2 = (torch.where(small, s, l)[..., None, None] for s, l in ((a_s, a_l), (b_s, b_l), (c_s, c_l)))
    W = hat(w)
    W2 = W @ W
    eye = torch.eye(3, dtype=xi.dtype)
    R, V = eye + a * W + b * W2, eye + b * W + c2 * W2
    top = torch.cat([R, (V @ v[..., None])], -1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=xi.dtype).expand(*xi.shape[:-1], 1, 4)
    return torch.cat([top, bottom], -2)


def search(cur, tgt, dist_thresh):
    """Brute force in float64.  -> idx (n,), keep (n,) bool, margin = min second-nearest / nearest squared distance, and the smallest
    relative gap |d - thresh| / thresh of any point to the threshold (inf without one)."""
    d2 = ((cur[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
    two, ids = torch.topk(d2, 2, dim=1, largest=False)
    margin = float((two[:, 1] / two[:, 0].clamp(min=1e-300)).min())
    if dist_thresh is None:
        return ids[:, 0], torch.ones(cur.shape[0], dtype=torch.bool), margin, float("inf")
    d = two[:, 0].sqrt()
    return ids[:, 0], two[:, 0] < float(dist_thresh) ** 2, margin, float(((d - dist_thresh).abs() / dist_thresh).min())


def sums(cur, tgt, tgt_n, idx, keep):
    """-> AtA (...,6,6), Atb (...,6), err (...) over the kept rows; cur (...,n,3)."""
    s, t, n = cur[..., keep, :], tgt[idx[keep]], tgt_n[idx[keep]]
    A = torch.cat([n.expand_as(s), torch.cross(s, n.expand_as(s), dim=-1)], -1)
    b = (n * (t - s)).sum(-1)
    return A.mT @ A, (A.mT @ b[..., None])[..., 0], (b * b).sum(-1)


def icp(src, tgt, tgt_n, numiters=20, damp=1e-8, dist_thresh=None, mode="icp", lambda_max=2.0, B=1.0, B2=1.0, nu=200.0, forced=None,
        round32=False):
    """src (...,n,3) float64 (may require grad), tgt / tgt_n (m,3) -> T (...,4,4) float64 and the per-iteration records
    [dict(idx, keep, cnt, margin, gap [, idx2, keep2, cnt2])].  forced: records of an earlier call whose neighbour lists and keep masks
    are used instead of searching (required when src has batch dimensions).  round32: round the moved clouds to float32 as the oracle
    does (values only; the rounding is passed straight through)."""
    tgt, tgt_n = tgt.double(), tgt_n.double()
    batch = src.shape[:-2]
    T = torch.eye(4, dtype=torch.float64).expand(*batch, 4, 4)
    lam = torch.full(batch, float(damp), dtype=torch.float64)
    eye6 = torch.eye(6, dtype=torch.float64)
    recs = []

    def move(p, M):
        q = p @ M[..., :3, :3].mT + M[..., None, :3, 3]
        return q + (q.float().double() - q).detach() if round32 else q

    def find(p, k, second):
        if forced is not None:
            r = forced[k]
            return (r["idx2"], r["keep2"], 0.0, 0.0) if second else (r["idx"], r["keep"], r["margin"], r["gap"])
        return search(p.detach(), tgt, dist_thresh)

    for k in range(numiters):
        if forced is not None and k >= len(forced):
            break
        cur = move(src, T)
        idx, keep, margin, gap = find(cur, k, False)
        cnt = int(keep.sum())
        if cnt < 6:
            break
        AtA, Atb, err = sums(cur, tgt, tgt_n, idx, keep)
        xi = torch.linalg.solve(AtA + lam[..., None, None] * eye6, Atb)
        rec = dict(idx=idx, keep=keep, cnt=cnt, margin=margin, gap=gap)
        if mode == "gradicp":
            nxt = move(cur, se3_exp(xi))
            idx2, keep2, m2, g2 = find(nxt, k, True)
            cnt2 = int(keep2.sum())
            _, _, err2 = sums(nxt, tgt, tgt_n, idx2, keep2)
            delta = err2 / max(cnt2, 1) - err / max(cnt, 1)
            lam = lam * (1.0 / lambda_max + (lambda_max - 1.0 / lambda_max) / (1.0 + B * torch.exp(-B2 * nu * delta)))
            gate = 1.0 / (1.0 + torch.exp(torch.clamp(nu * delta, -60, 60)))
            step = se3_exp(gate[..., None] * xi)
            rec.update(idx2=idx2, keep2=keep2, cnt2=cnt2)
            if forced is None:
                rec.update(margin=min(margin, m2), gap=min(gap, g2))
        else:
            step = se3_exp(xi)
        T = step @ T
        recs.append(rec)
    return T, recs


def scene(n_src, grid=12, seed=7):
    """Three orthogonal jittered grid x grid planes (spacing 0.05, +-5 mm in-plane jitter) with their plane normals as the target;
    the source is n_src target points moved by TWIST plus +-2 mm noise.  float32 tensors (tgt, tgt_n, src)."""
    g = torch.Generator().manual_seed(seed)
    c = (torch.arange(grid, dtype=torch.float64) + 0.5) * 0.05
    u, v = torch.meshgrid(c, c, indexing="ij")
    pts, nrm = [], []
    for axis in range(3):
        uv = torch.stack([u.reshape(-1), v.reshape(-1)], 1) + (torch.rand(grid * grid, 2, generator=g, dtype=torch.float64) - 0.5) * 0.01
        p = torch.zeros(grid * grid, 3, dtype=torch.float64)
        p[:, [a for a in range(3) if a != axis]] = uv
        n = torch.zeros(grid * grid, 3, dtype=torch.float64)
        n[:, axis] = 1.0
        pts.append(p)
        nrm.append(n)
    tgt, tgt_n = torch.cat(pts).float(), torch.cat(nrm).float()
    pick = torch.randperm(tgt.shape[0], generator=g)[:n_src]
    M = se3_exp(torch.tensor(TWIST, dtype=torch.float64))
    src = tgt[pick].double() @ M[:3, :3].T + M[:3, 3] + (torch.rand(n_src, 3, generator=g, dtype=torch.float64) - 0.5) * 0.004
    return tgt, tgt_n, src.float()


def weights(shape, seed=1):
    """Fixed weights C of the scalar sum(C . T[:3]) whose gradient the tests compare."""
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape))
