"""float64 torch restatement of the normals' side of the SLAM chain that autograd can walk: the normal maps of
oracle.pointfusion.vertex_normal_maps (forward differences of the vertex map, cross product, normalisation, rotation), the fuse
expression of fuse_with_map with its normals row, and the chain frame 0 -> {localise, fuse} x (L - 1) in which the localisation reads
the map's normals out of the same graph.  The reference for e2e_normal_maps_bwd, e2e_pf_fuse_normals_bwd and
PointFusion(normal_gradient=True).  TEST INFRASTRUCTURE ONLY.

It extends tests/pointfusion_grad_ref.py (whose constants and rule it keeps: the unique tables are GIVEN, the validity mask, the
append order and the intrinsics are constants, the inverse intrinsics are the float32 ones, widened) and tests/slam_chain_grad_ref.py
(every discrete choice of the run is GIVEN in `steps[f]`; its `normals` entry is not read here: the normals are the state's own).

The closed forms of include/e2eslam.h are restated in plain tensor code next to the functions autograd walks:
normal_maps_bwd_closed_form (the scatter form), normal_maps_bwd_gather (the form the kernel takes: pixel j collects its three
contributors), fuse_normals_bwd_closed_form, pose_term_closed_form."""
import torch

import pointfusion_grad_ref as P
import slam_chain_grad_ref as C
from oracle import pointfusion as opf

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# the normal maps
# ---------------------------------------------------------------------------------------------------------------------
def _rays(K, H, W):
    Ki = opf.intrinsics_inverse(K.float()).double()
    hs, ws = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    return torch.stack([Ki[0, 0] * ws + Ki[0, 2], Ki[1, 1] * hs + Ki[1, 2], torch.ones(H, W, dtype=F64)], -1)


def _cross(a, b):
    """a x b with every product rounded on its own, as the oracle writes it: a fused multiply-add would leave a x a != 0."""
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _differences(V):
    """dh = V[h,w+1] - V[h,w] (0 in the last column), dv = V[h+1,w] - V[h,w] (0 in the last row): the zeros are constants."""
    H, W, _ = V.shape
    dh = torch.cat([V[:, 1:] - V[:, :-1], torch.zeros(H, 1, 3, dtype=F64)], 1)
    dv = torch.cat([V[1:] - V[:-1], torch.zeros(1, W, 3, dtype=F64)], 0)
    return dh, dv


def frame_normal_maps(depth, K, pose):
    """depth (H,W) float64 (may require grad); K (4,4); pose (4,4) (may require grad) -> n, ng (H,W,3) float64, valid (H,W) bool.
    n = (c / where(|c| == 0, 1, |c|)) vf with c = dh x dv; ng = R n.  The where is taken on the squared sum, before the root: the
    root of 0 has no derivative and autograd would return NaN through the branch that is not taken."""
    H, W = depth.shape
    valid = depth.detach() != 0
    vf = valid.to(F64)[..., None]
    V = _rays(K, H, W) * depth[..., None] * vf
    dh, dv = _differences(V)
    c = _cross(dh, dv)
    sq = (c * c).sum(-1, keepdim=True)
    nrm = torch.sqrt(torch.where(sq == 0, torch.ones_like(sq), sq))
    n = c / nrm * vf
    ng = n @ pose.double()[:3, :3].T
    return n, ng, valid


def _cross_adjoints(depth, K, pose, g_n, g_ng):
    """Per pixel g_dh, g_dv (H,W,3) of the rule in include/e2eslam.h; 0 for the difference the forward holds at the constant 0."""
    H, W = depth.shape
    vf = (depth != 0).to(F64)[..., None]
    V = _rays(K, H, W) * depth[..., None] * vf
    dh, dv = _differences(V)
    c = _cross(dh, dv)
    nrm = torch.sqrt((c * c).sum(-1, keepdim=True))
    gn = torch.zeros(H, W, 3, dtype=F64)
    if g_n is not None:
        gn = gn + g_n
    if g_ng is not None:
        gn = gn + g_ng @ pose.double()[:3, :3]              # R^T g_ng
    gn = gn * vf
    zero = nrm == 0
    safe = torch.where(zero, torch.ones_like(nrm), nrm)
    nh = c / safe
    gc = torch.where(zero, gn, (gn - nh * (nh * gn).sum(-1, keepdim=True)) / safe)
    g_dh, g_dv = _cross(dv, gc), _cross(gc, dh)
    g_dh[:, W - 1] = 0
    g_dv[H - 1] = 0
    return g_dh, g_dv, zero[..., 0]


def normal_maps_bwd_closed_form(depth, K, pose, g_n=None, g_ng=None):
    """d/d depth of sum(g_n . n) + sum(g_ng . ng), the scatter form: pixel p sends -(g_dh + g_dv) to V_p, g_dh to V_{h,w+1}, g_dv to
    V_{h+1,w}; g_depth = vf r . gV.  float64 tensors; -> (H,W)."""
    depth = depth.detach().double()
    H, W = depth.shape
    g_dh, g_dv, _ = _cross_adjoints(depth, K, pose.detach(), g_n, g_ng)
    gV = -(g_dh + g_dv)
    gV[:, 1:] += g_dh[:, :-1]
    gV[1:] += g_dv[:-1]
    return (_rays(K, H, W) * gV).sum(-1) * (depth != 0).to(F64)


def normal_maps_bwd_gather(depth, K, pose, g_n=None, g_ng=None):
    """The same as the kernel takes it: the thread of pixel j = (h,w) collects j itself, (h,w-1) whose right neighbour it is and
    (h-1,w) whose lower neighbour it is, each recomputed from its own three depths and its gn (seven depths, three gn per pixel)."""
    depth = depth.detach().double()
    H, W = depth.shape
    R = pose.detach().double()[:3, :3]
    rays = _rays(K, H, W)

    def vertex(h, w):
        return rays[h, w] * depth[h, w]                      # 0 for an invalid pixel

    def contributor(h, w):
        z = torch.zeros(3, dtype=F64)
        if depth[h, w] == 0:
            return z, z
        dh = vertex(h, w + 1) - vertex(h, w) if w + 1 < W else z
        dv = vertex(h + 1, w) - vertex(h, w) if h + 1 < H else z
        gn = z.clone()
        if g_n is not None:
            gn = gn + g_n[h, w]
        if g_ng is not None:
            gn = gn + R.T @ g_ng[h, w]
        c = _cross(dh, dv)
        nrm = torch.sqrt((c * c).sum())
        gc = gn if nrm == 0 else (gn - (c / nrm) * ((c / nrm) * gn).sum()) / nrm
        return (_cross(dv, gc) if w + 1 < W else z), (_cross(gc, dh) if h + 1 < H else z)

    out = torch.zeros(H, W, dtype=F64)
    for h in range(H):
        for w in range(W):
            if depth[h, w] == 0:
                continue
            a, b = contributor(h, w)
            gV = -(a + b)
            if w > 0:
                gV = gV + contributor(h, w - 1)[0]
            if h > 0:
                gV = gV + contributor(h - 1, w)[1]
            out[h, w] = (rays[h, w] * gV).sum()
    return out


def pose_term_closed_form(n, g_ng):
    """ng = R n: d/dR of sum(g_ng . ng) = sum_p g_ng[p] n_p^T (3,3); nothing reaches the translation or the bottom row."""
    return g_ng.reshape(-1, 3).T @ n.reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the map step with its normals row
# ---------------------------------------------------------------------------------------------------------------------
def empty_state():
    return dict(P.empty_state(), normals=torch.zeros(0, 3, dtype=F64))


ROWS = (("points", "Vg"), ("normals", "ng"), ("colors", "rgb"))


def fuse(state, frame, unique):
    """pointfusion_grad_ref.fuse with the normals row: N' = (c N + a ng[q]) / where(c + a == 0, 1, c + a), not renormalised.
    frame: dict Vg, ng, rgb (H,W,3), alpha (H,W), valid (H,W) bool."""
    M = state["points"].shape[0]
    valid, alpha = frame["valid"], frame["alpha"]
    new_mask = valid.clone()
    if M > 0 and unique.shape[0] > 0:
        n, h, w = unique[:, 0], unique[:, 1], unique[:, 2]
        assert n.unique().numel() == n.numel() and (h * valid.shape[1] + w).unique().numel() == n.numel()    # one row, one pixel
        c = state["ccounts"]
        fa = torch.zeros(M, dtype=F64).index_put((n,), alpha[h, w])
        cn = c + fa
        den = torch.where(cn == 0, torch.ones_like(cn), cn)
        out = {"ccounts": cn}
        for name, src in ROWS:
            f = torch.zeros(M, 3, dtype=F64).index_put((n,), frame[src][h, w])
            out[name] = (c[:, None] * state[name] + fa[:, None] * f) / den[:, None]
        new_mask[h, w] = False
    else:
        out = dict(state)
    new = {name: torch.cat([out[name], frame[src][new_mask]], 0) for name, src in ROWS}
    new["ccounts"] = torch.cat([out["ccounts"], alpha[new_mask]], 0)
    return new


def frame(rgb, depth, K, pose, sigma=0.6):
    Vg, alpha, valid = P.frame_maps(depth, K, pose, sigma)
    _, ng, _ = frame_normal_maps(depth, K, pose)
    return dict(Vg=Vg, ng=ng, rgb=rgb, alpha=alpha, valid=valid)


def step(state, rgb, depth, K, pose, unique, sigma=0.6):
    return fuse(state, frame(rgb, depth, K, pose, sigma), unique)


def fuse_normals_bwd_closed_form(state, frame, unique, gN):
    """The normals' rule of include/e2eslam.h for one step: state (before the step), the frame's ng / alpha / valid, the unique table,
    gN (M_after,3) -> g_ng (H,W,3), g_alpha (H,W), g_prev_normals (M,3), g_prev_ccounts (M): the normals' contributions only."""
    M = state["normals"].shape[0]
    ng, alpha, valid = frame["ng"].detach(), frame["alpha"].detach(), frame["valid"]
    N0, c0 = state["normals"].detach(), state["ccounts"].detach()
    g_ng, g_alpha = torch.zeros_like(ng), torch.zeros_like(alpha)
    g_prevN, g_prevcc = gN[:M].clone(), torch.zeros(M, dtype=F64)
    new_mask = valid.clone()
    if M > 0 and unique.shape[0] > 0:
        n, h, w = unique[:, 0], unique[:, 1], unique[:, 2]
        g_prevN[c0 == 0] = 0                                  # a zero-confidence row in a step where anything matched
        u, v, N, a, c = gN[n], ng[h, w], N0[n], alpha[h, w], c0[n]
        s = c + a
        z = s == 0
        den = torch.where(z, torch.ones_like(s), s)
        D = (u * (v - N)).sum(-1)
        wf, wm = torch.where(z, torch.zeros_like(s), a / den), torch.where(z, torch.zeros_like(s), c / den)
        g_ng[h, w] = wf[:, None] * u
        g_prevN[n] = wm[:, None] * u
        g_alpha[h, w] = torch.where(z, (u * v).sum(-1), wm * (D / den))
        g_prevcc[n] = torch.where(z, (u * N).sum(-1), -wf * (D / den))
        new_mask[h, w] = False
    g_ng[new_mask] = gN[M:]
    return g_ng, g_alpha, g_prevN, g_prevcc


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def chain(rgbs, depths, K, pose0, steps, dsratio=4, sigma=0.6, **icp_kw):
    """slam_chain_grad_ref.chain with the normals in the graph: the state carries them, the localisation of frame f reads the state's
    normals (steps[f]["normals"] is not used), the map step fuses them with a pose that is a variable (ng = R n).
    -> the final state (points, normals, colors, ccounts) and the list of poses, one graph."""
    state, poses = empty_state(), []
    for f, (rgb, depth, st) in enumerate(zip(rgbs, depths, steps)):
        if f == 0:
            pose = pose0.double()
        else:
            pose, _ = C.localise(state["points"], state["normals"], depth, K, poses[-1], st["sel"], st["records"], dsratio, **icp_kw)
        state = step(state, rgb, depth, K, pose, st["unique"], sigma)
        poses.append(pose)
    return state, poses


def degenerate_frame():
    """5x7 depth with every case of the rule at nrm == 0: (1,2) is valid with invalid right and lower neighbours (dh = dv = -V), the
    last row and the last column (one difference is the constant 0), the bottom-right corner (both), and one more invalid pixel (3,4).
    -> depth (5,7) float32, the (h,w) of the valid pixels with nrm == 0."""
    g = torch.Generator().manual_seed(57)
    depth = 1.5 + torch.rand(5, 7, generator=g)
    depth[1, 3] = depth[2, 2] = 0
    depth[3, 4] = 0
    zero = [(1, 2)] + [(4, w) for w in range(7)] + [(h, 6) for h in range(4)]
    return depth, zero
