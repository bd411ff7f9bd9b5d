"""float64 torch restatement of the whole SLAM chain frame 0 -> {localise, fuse} x (L - 1) that autograd can walk: the reference for
the chain gradient (PointFusion(chain_gradient=True): the map and the previous pose are variables of the localisation, the pose is a
variable of the map step).  TEST INFRASTRUCTURE ONLY.

It composes tests/icp_grad_ref.py (icp) and tests/pointfusion_grad_ref.py (frame_maps, step), which keep the graph through a float64
pose, tgt and tgt_n that require grad.  Every discrete choice of the run it is compared with is GIVEN, per frame, in `steps[f]`:
    unique   the map step's table (rows [n, h, w]; empty for the step onto the empty map)
    sel      the rows of the map the localisation used as targets (active[::dsratio, 0]);            frames >= 1
    records  the neighbour lists and keep masks of every search, in the form icp(..., forced=...) takes  (None: search freely)
    normals  the map's normals before the step (M,3): constants, nothing differentiates them
With a free search on either side the comparison would be one of tie-breaks: the fused map has points at equal distances."""
import numpy as np
import torch

import icp_grad_ref as I
import pointfusion_grad_ref as P


def ne_bwd_tgt_closed_form(src, tgt, tgt_n, idx, keep, adj, with_scale=False):
    """The target-side adjoint of one ICP reduction as include/e2eslam.h states it, float64: adj (28,) in out29's order
    -> g_tgt, g_tgt_normals (m,3).  With U the upper-triangular unpacking of adj[:21], M = U + U^T, A_i = [n, s x n], b_i = n.(t - s):
    Abar_i = M A_i + b_i gbar, bbar_i = gbar.A_i + 2 ebar b_i; row j: sum over kept i with idx[i] == j of bbar_i n_j, and of
    bbar_i (t_j - s_i) + Abar_i[0:3] + Abar_i[3:6] x s_i.
    with_scale: also S_tgt, S_tgt_normals (m,3), per element the sum of the absolute values of the terms that were added (one term per
    kept row), the scale a bound on the summation error is stated against."""
    src, tgt, tgt_n, adj = src.double(), tgt.double(), tgt_n.double(), adj.double()
    U = torch.zeros(6, 6, dtype=torch.float64)
    k = 0
    for r in range(6):
        for c in range(r, 6):
            U[r, c] = adj[k]
            k += 1
    M, gbar, ebar = U + U.T, adj[21:27], adj[27]
    s, j = src[keep], idx[keep]
    t, n = tgt[j], tgt_n[j]
    A = torch.cat([n, torch.cross(s, n, dim=-1)], -1)
    b = (n * (t - s)).sum(-1)
    Abar = A @ M.T + b[:, None] * gbar
    bbar = A @ gbar + 2.0 * ebar * b
    rows_t, rows_n = bbar[:, None] * n, bbar[:, None] * (t - s) + Abar[:, :3] + torch.cross(Abar[:, 3:], s, dim=-1)
    g_tgt = torch.zeros_like(tgt).index_add_(0, j, rows_t)
    g_n = torch.zeros_like(tgt_n).index_add_(0, j, rows_n)
    if with_scale:
        return g_tgt, g_n, torch.zeros_like(tgt).index_add_(0, j, rows_t.abs()), torch.zeros_like(tgt_n).index_add_(0, j, rows_n.abs())
    return g_tgt, g_n


def forced_records(iterations, dist_thresh=None):
    """Trace.iterations of a recorded e2ehip.icp run -> the records icp(..., forced=...) takes (CPU tensors)."""
    def keep(d):
        d = d.cpu()
        return torch.ones(d.shape[0], dtype=torch.bool) if dist_thresh is None else d < np.float32(dist_thresh) * np.float32(dist_thresh)

    recs = []
    for it in iterations:
        r = dict(idx=it["idx"].cpu(), keep=keep(it["dists"]), cnt=it["cnt"], margin=0.0, gap=0.0)
        if "idx2" in it:
            r.update(idx2=it["idx2"].cpu(), keep2=keep(it["dists2"]), cnt2=it["cnt2"])
        recs.append(r)
    return recs


def source_mask(valid, dsratio):
    sub = torch.zeros_like(valid)
    sub[::dsratio, ::dsratio] = True
    return valid & sub


def localise(points, normals, depth, K, prev_pose, sel, records, dsratio=4, **icp_kw):
    """PointFusion._localize in float64: the live frame placed with prev_pose, every dsratio-th valid pixel as the source, the map rows
    `sel` as targets.  points (M,3), prev_pose (4,4), depth (H,W) may require grad.  -> pose = T . prev_pose (4,4), the records."""
    Vg, _, valid = P.frame_maps(depth, K, prev_pose)
    src = Vg[source_mask(valid, dsratio)]
    T, recs = I.icp(src, points[sel], normals.double()[sel], forced=records, **icp_kw)
    return T @ prev_pose.double(), recs


def chain(rgbs, depths, K, pose0, steps, dsratio=4, sigma=0.6, **icp_kw):
    """rgbs[f] (H,W,3), depths[f] (H,W) float64; pose0: the first frame's pose (a constant); steps: see the module's docstring.
    -> the final map state (points, colors, ccounts) and the list of poses, one graph."""
    state, poses = P.empty_state(), []
    for f, (rgb, depth, st) in enumerate(zip(rgbs, depths, steps)):
        if f == 0:
            pose = pose0.double()
        else:
            pose, _ = localise(state["points"], st["normals"], depth, K, poses[-1], st["sel"], st["records"], dsratio, **icp_kw)
        state = P.step(state, rgb, depth, K, pose, st["unique"], sigma)
        poses.append(pose)
    return state, poses


def pose_weights(f):
    """Fixed weights of frame f's term sum(w . pose_f[:3]) of the scalar the tests differentiate."""
    return P.weights((3, 4), 10 + f)


def scalar(state, poses, cloud=True):
    """pointfusion_grad_ref.scalar(final cloud) + sum_f sum(pose_weights(f) . pose_f[:3])."""
    s = sum((pose_weights(f) * p[:3]).sum() for f, p in enumerate(poses))
    return s + P.scalar(state) if cloud else s
