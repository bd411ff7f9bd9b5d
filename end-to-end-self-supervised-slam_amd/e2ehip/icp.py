"""Frame-to-model ICP odometry (gradslam's "icp" / "gradicp" odometry providers).

Per Gauss-Newton iteration the GPU transforms the source cloud, finds exact nearest neighbours in the active map
points and folds the N x 6 point-to-plane system into 29 numbers (csrc/icp.hip); the 6x6 solve and the se(3)
exponential are float64 on the host (one 232-byte copy per iteration; odometry runs once per keyframe, not per
refinement step)."""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import ops


def _so3_hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)


def se3_exp(xi):
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = np.linalg.norm(w)
    W = _so3_hat(w)
    t2 = th * th
    # below 1e-2 the closed forms lose what 1 - cos(th) and th - sin(th) cancel (all of b and c2 at th ~ 1e-8); the series, cut after
    # th^4, is then exact to th^6 / 5040 < 2e-16
    if th < 1e-2:
        a, b, c2 = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0), 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0), 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0)
    else:
        a, b, c2 = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)
    R, V = np.eye(3) + a * W + b * W @ W, np.eye(3) + b * W + c2 * W @ W       # R = I + a W + b W^2 ; V = I + b W + c2 W^2
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


def _unpack(v):
    AtA = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            AtA[r, c] = AtA[c, r] = v[k]
            k += 1
    return AtA, v[21:27], int(round(v[27])), float(v[28])


def se3_exp_bwd(xi, Tbar):
    """Adjoint of se3_exp: Tbar (4,4) (its top three rows count) -> xibar (6,), float64, same branch as the forward."""
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    t2 = float(w @ w)
    th = np.sqrt(t2)
    W = _so3_hat(w)
    W2 = W @ W
    if th < 1e-2:                                                              # the series and its derivatives with respect to th^2
        b, c2 = 0.5 - t2 / 24.0 * (1.0 - t2 / 30.0), 1.0 / 6.0 - t2 / 120.0 * (1.0 - t2 / 42.0)
        a = 1.0 - t2 / 6.0 * (1.0 - t2 / 20.0)
        da, db, dc = -1.0 / 6.0 + t2 / 60.0, -1.0 / 24.0 + t2 / 360.0, -1.0 / 120.0 + t2 / 2520.0
    else:
        sn, cs = np.sin(th), np.cos(th)
        a, b, c2 = sn / th, (1.0 - cs) / t2, (th - sn) / (t2 * th)
        # d/d(th^2) = (d/dth) / (2 th)
        da = (th * cs - sn) / t2 / (2.0 * th)
        db = (th * sn - 2.0 * (1.0 - cs)) / (t2 * th) / (2.0 * th)
        dc = ((1.0 - cs) * th - 3.0 * (th - sn)) / (t2 * t2) / (2.0 * th)
    V = np.eye(3) + b * W + c2 * W2
    Rb, tb = np.asarray(Tbar[:3, :3], np.float64), np.asarray(Tbar[:3, 3], np.float64)
    Vb = np.outer(tb, v)
    ab, bb, cb = np.sum(Rb * W), np.sum(Rb * W2) + np.sum(Vb * W), np.sum(Vb * W2)
    Wb = a * Rb + b * (Rb @ W.T + W.T @ Rb) + b * Vb + c2 * (Vb @ W.T + W.T @ Vb)
    wb = np.array([Wb[2, 1] - Wb[1, 2], Wb[0, 2] - Wb[2, 0], Wb[1, 0] - Wb[0, 1]]) + 2.0 * w * (ab * da + bb * db + cb * dc)
    return np.concatenate([V.T @ tb, wb])


def _reduce(cur, tgt, tgt_n, dist_thresh, out, ws, index=None):
    d, idx = ops.knn1(cur, index if index is not None else tgt)
    L.call("e2e_icp_normal_equations", L.ptr(cur), L.ptr(tgt), L.ptr(tgt_n), L.ptr(idx), L.ptr(d),
           -1.0 if dist_thresh is None else float(dist_thresh), cur.shape[0], L.ptr(out), L.ptr(ws), L.stream())
    return _unpack(out.cpu().numpy()) + (idx, d)


class Trace(list):
    """[(inliers, sum r^2)] per iteration, as ever; a differentiable run also keeps, in `iterations`, what its backward walks: per
    iteration a dict with T (the transform the step started from), xi, lam, AtA, Atb, cnt, err, idx and dists of the search (device), and
    for gradicp idx2 / dists2 / cnt2 / err2 of the trial step, delta and y (the gated twist)."""
    iterations = ()


def _icp_loop(src, tgt, tgt_n, numiters, damp, dist_thresh, mode, lambda_max, B, B2, nu, record=False):
    dev = src.device
    out = torch.empty(29, device=dev, dtype=torch.float64)
    ws = torch.empty(L.load().e2e_icp_workspace_bytes(), device=dev, dtype=torch.uint8)
    T = np.eye(4)
    lam = float(damp)
    trace = Trace()
    recs = []
    index = ops.KnnIndex(tgt, src.shape[0])               # the target cloud is fixed: one grid for all iterations
    for _ in range(numiters):
        cur = ops.transform_points(src, torch.from_numpy(T).float().to(dev))
        AtA, Atb, cnt, err, idx, d = _reduce(cur, tgt, tgt_n, dist_thresh, out, ws, index)
        if cnt < 6:
            break
        xi = np.linalg.solve(AtA + lam * np.eye(6), Atb)
        step = se3_exp(xi)
        rec = dict(T=T, xi=xi, lam=lam, AtA=AtA, Atb=Atb.copy(), cnt=cnt, err=err, idx=idx, dists=d, y=xi) if record else None
        if mode == "gradicp":
            nxt = ops.transform_points(cur, torch.from_numpy(step).float().to(dev))
            _, _, cnt2, err2, idx2, d2 = _reduce(nxt, tgt, tgt_n, dist_thresh, out, ws, index)
            delta = (err2 / max(cnt2, 1)) - (err / max(cnt, 1))
            lam = lam * (1.0 / lambda_max + (lambda_max - 1.0 / lambda_max) / (1.0 + B * np.exp(-B2 * nu * delta)))
            y = xi / (1.0 + np.exp(np.clip(nu * delta, -60, 60)))
            step = se3_exp(y)
            if record:
                rec.update(idx2=idx2, dists2=d2, cnt2=cnt2, err2=err2, delta=delta, y=y)
        T = step @ T
        trace.append((cnt, err))
        if record:
            recs.append(rec)
    trace.iterations = recs
    return T, trace


def _icp_backward(src, tgt, tgt_n, recs, Tbar, dist_thresh, mode, lambda_max, B, B2, nu, want_tgt=False, want_tgt_n=False):
    """The iterations in reverse (the rule of include/e2eslam.h: searches, keep masks and counts fixed).  Tbar (4,4) float64: the
    adjoint of the final transform.  -> d/d src (n,3) fp32, and d/d tgt, d/d tgt_n (m,3) fp32 where wanted (None otherwise): the
    targets are not moved by the running transform, so every reduction of every iteration adds into the same pair."""
    dev, n, st = src.device, src.shape[0], L.stream()
    thresh = -1.0 if dist_thresh is None else float(dist_thresh)
    g_src = torch.zeros_like(src)
    g_tgt = torch.zeros_like(tgt) if want_tgt else None
    g_tgt_n = torch.zeros_like(tgt_n) if want_tgt_n else None
    tgt_ws = None
    if want_tgt or want_tgt_n:
        tgt_ws = torch.empty(L.query("e2e_icp_normal_equations_bwd_tgt_workspace_bytes", n, tgt.shape[0]), device=dev, dtype=torch.uint8)
    cur, nxt, g_cur, g_nxt, tmp = (torch.empty_like(src) for _ in range(5))
    lambar = 0.0
    Tbar = np.array(Tbar, np.float64)

    def ne_bwd(pts, idx, d, adj, g, accumulate):
        adj = torch.from_numpy(adj).to(dev)
        L.call("e2e_icp_normal_equations_bwd", src=L.ptr(pts), tgt=L.ptr(tgt), tgt_normals=L.ptr(tgt_n), n_tgt=tgt.shape[0], idx=L.ptr(idx),
               dists=L.ptr(d), dist_thresh=thresh, adj28=L.ptr(adj), n=n, g_src=L.ptr(g), accumulate=int(accumulate), stream=st)
        if tgt_ws is not None:
            L.call("e2e_icp_normal_equations_bwd_tgt", src=L.ptr(pts), tgt=L.ptr(tgt), tgt_normals=L.ptr(tgt_n), n_tgt=tgt.shape[0], idx=L.ptr(idx),
                   dists=L.ptr(d), dist_thresh=thresh, adj28=L.ptr(adj), n=n, g_tgt=L.ptr(g_tgt), g_tgt_normals=L.ptr(g_tgt_n), accumulate=1,
                   workspace=L.ptr(tgt_ws), stream=st)

    def dT(g, pts):
        full = np.zeros((4, 4))
        full[:3] = ops.transform_points_bwd_T(g, pts).cpu().numpy()
        return full

    for rec in reversed(recs):
        Tk, xi, y, lam_k = rec["T"], rec["xi"], rec["y"], rec["lam"]
        T32 = torch.from_numpy(Tk).float().to(dev)
        L.call("e2e_transform_points", L.ptr(src), L.ptr(T32), L.ptr(cur), n, 0, st)
        S = se3_exp(y)
        ybar = se3_exp_bwd(y, Tbar @ Tk.T)
        Tbar = S.T @ Tbar
        errbar, have_cur = 0.0, False
        if mode == "gradicp":
            delta, cnt, cnt2 = rec["delta"], rec["cnt"], rec["cnt2"]
            z = nu * delta
            gate = 1.0 / (1.0 + np.exp(np.clip(z, -60, 60)))
            xibar = gate * ybar
            dgate = -nu * gate * (1.0 - gate) if -60.0 < z < 60.0 else 0.0         # the clipped region has zero derivative
            e = B * np.exp(-B2 * nu * delta)
            q = 1.0 / lambda_max + (lambda_max - 1.0 / lambda_max) / (1.0 + e)
            dq = (lambda_max - 1.0 / lambda_max) * e * B2 * nu / (1.0 + e) ** 2
            deltabar = float(ybar @ xi) * dgate + lambar * lam_k * dq
            lambar = lambar * q
            err2bar, errbar = deltabar / max(cnt2, 1), -deltabar / max(cnt, 1)
            if err2bar != 0.0:
                step32 = torch.from_numpy(se3_exp(xi)).float().to(dev)
                L.call("e2e_transform_points", L.ptr(cur), L.ptr(step32), L.ptr(nxt), n, 0, st)
                adj = np.zeros(28)
                adj[27] = err2bar
                ne_bwd(nxt, rec["idx2"], rec["dists2"], adj, g_nxt, 0)
                L.call("e2e_transform_points", L.ptr(g_nxt), L.ptr(step32), L.ptr(g_cur), n, 1, st)
                xibar = xibar + se3_exp_bwd(xi, dT(g_nxt, cur))
                have_cur = True
        else:
            xibar = ybar
        gbar = np.linalg.solve((rec["AtA"] + lam_k * np.eye(6)).T, xibar)
        Gbar = -np.outer(gbar, xi)
        lambar += float(np.trace(Gbar))
        adj = np.zeros(28)
        k = 0
        for r in range(6):
            for c in range(r, 6):
                adj[k] = Gbar[r, c] if r == c else Gbar[r, c] + Gbar[c, r]
                k += 1
        adj[21:27], adj[27] = gbar, errbar
        ne_bwd(cur, rec["idx"], rec["dists"], adj, g_cur, have_cur)
        Tbar = Tbar + dT(g_cur, src)
        L.call("e2e_transform_points", L.ptr(g_cur), L.ptr(T32), L.ptr(tmp), n, 1, st)
        g_src += tmp
    return g_src, g_tgt, g_tgt_n


class _DifferentiableICP(torch.autograd.Function):
    """forward: the launch sequence and host arithmetic of _icp_loop (values bit-identical to the plain call), recording each iteration;
    backward: _icp_backward, plus T^T gbar for prev_pose.  Output: T (4,4) float64, or with prev_pose the pose fl32(T . prev_pose).
    tgt, tgt_n and prev_pose get a gradient only when they require one (point_to_plane_icp detaches them unless target_gradient)."""

    @staticmethod
    def forward(ctx, src, tgt, tgt_n, prev_pose, cfg, holder):
        T, trace = _icp_loop(src, tgt.detach(), tgt_n.detach(), record=True, **cfg)
        holder.append(trace)
        ctx.save_for_backward(src, tgt, tgt_n)
        ctx.recs, ctx.cfg = trace.iterations, cfg
        ctx.prev = None if prev_pose is None else prev_pose.detach().double().cpu().numpy()
        ctx.T = T
        if prev_pose is None:
            return torch.from_numpy(T).to(src.device)
        return torch.from_numpy(T @ ctx.prev).float().to(src.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        src, tgt, tgt_n = ctx.saved_tensors
        Tbar = g.double().cpu().numpy()
        g_prev = None
        if ctx.prev is not None:
            if ctx.needs_input_grad[3]:
                g_prev = torch.from_numpy(ctx.T.T @ Tbar).float().to(g.device)
            Tbar = Tbar @ ctx.prev.T
        c = ctx.cfg
        g_src, g_tgt, g_tgt_n = _icp_backward(src, tgt, tgt_n, ctx.recs, Tbar, c["dist_thresh"], c["mode"], c["lambda_max"], c["B"], c["B2"], c["nu"],
                                              want_tgt=ctx.needs_input_grad[1], want_tgt_n=ctx.needs_input_grad[2])
        return g_src if ctx.needs_input_grad[0] else None, g_tgt, g_tgt_n, g_prev, None, None


def point_to_plane_icp(src, tgt, tgt_n, numiters=20, damp=1e-8, dist_thresh=None, mode="icp", lambda_max=2.0, B=1.0, B2=1.0, nu=200.0,
                       prev_pose=None, target_gradient=False):
    """src (Ns,3), tgt / tgt_n (Nt,3) device tensors -> 4x4 float64 numpy transform aligning src to tgt, plus a trace.
    When src requires grad (and grad mode is on) the transform is a (4,4) float64 DEVICE tensor of the same values that carries the
    gradient to src (the adjoint stated in include/e2eslam.h; targets are constants), and the trace holds the recorded iterations
    (Trace.iterations).  prev_pose (4,4): return the pose fl32(T . prev_pose) as a float32 device tensor instead of T.
    target_gradient: tgt, tgt_n and prev_pose are variables too (the chain gradient): the call is differentiable when any of the four
    requires grad, and the result carries the gradient to each that does.  The values do not depend on the switch."""
    if mode not in ("icp", "gradicp"):
        raise ValueError(f"unknown odometry mode {mode}")
    cfg = dict(numiters=numiters, damp=damp, dist_thresh=dist_thresh, mode=mode, lambda_max=lambda_max, B=B, B2=B2, nu=nu)
    if not target_gradient:
        tgt, tgt_n, prev_pose = tgt.detach(), tgt_n.detach(), None if prev_pose is None else prev_pose.detach()
    differentiable = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (src, tgt, tgt_n, prev_pose))
    src, tgt, tgt_n = (L.dev(t, n).contiguous() for t, n in ((src, "src"), (tgt, "tgt"), (tgt_n, "tgt_normals")))
    if differentiable:
        holder = []
        out = _DifferentiableICP.apply(src, tgt, tgt_n, prev_pose, cfg, holder)
        return out, holder[0]
    with torch.no_grad():
        T, trace = _icp_loop(src, tgt, tgt_n, **cfg)
    if prev_pose is not None:
        return torch.from_numpy(T @ prev_pose.detach().double().cpu().numpy()).float().to(src.device), trace
    return T, trace


def frame_to_model(fmap, depth, K, prev_pose, dsratio=4, map_tensors=None, prev_pose_gradient=False, **kw):
    """PointFusion._localize: pose of the live frame (depth (H,W)) given the resident map `fmap` (e2ehip.FusionMap)
    and the previous frame's pose.  Returns a (4,4) float32 device tensor and the iteration trace.  When depth requires grad (and grad
    mode is on) the pose carries the gradient to the depth: through the source points only -- by default the map and prev_pose are
    constants.  The chain gradient: map_tensors = (points, normals), the caller's graph-bearing tensors whose VALUES are the resident
    rows, make the targets variables; prev_pose_gradient keeps prev_pose attached (it places the source cloud, Vg = prev_pose . V, and
    it is the right factor of pose = fl32(T . prev_pose)).  Values and trace do not depend on either."""
    H, W = fmap.H, fmap.W
    if fmap.M == 0:
        raise ValueError("frame-to-model odometry needs a non-empty map")
    if map_tensors is not None:
        map_points, map_normals = map_tensors
        assert map_points.shape == (fmap.M, 3) and map_normals.shape == (fmap.M, 3), "map_tensors must stand for the resident rows"
    K = K.detach()
    if not prev_pose_gradient:
        prev_pose = prev_pose.detach()
    variables = [depth, prev_pose] + (list(map_tensors) if map_tensors is not None else [])
    differentiable = torch.is_grad_enabled() and any(t.requires_grad for t in variables)
    chain = map_tensors is not None or prev_pose_gradient
    with torch.set_grad_enabled(differentiable):
        maps = fmap.frame_maps(depth, K, prev_pose)
        prev_pose_var, prev_pose = prev_pose, prev_pose.detach()          # the association takes it as a constant
        sub = torch.zeros(H, W, dtype=torch.bool, device=depth.device)
        sub[::dsratio, ::dsratio] = True
        keep = maps["valid"][0] & sub
        src = ops.select_rows(maps["Vg"][0].reshape(-1, 3), keep.reshape(-1)) if differentiable else maps["Vg"][0][keep]
        fmap.associate(maps, K, prev_pose)
        sel = fmap.table("active")[::dsratio, 0]
        if sel.numel() < 6 or src.shape[0] < 6:
            raise RuntimeError("too few points for frame-to-model ICP (no overlap between the live frame and the map)")
        if map_tensors is not None:
            tgt, tgt_n = map_points.index_select(0, sel), map_normals.index_select(0, sel)
        else:
            tgt, tgt_n = fmap.points[sel].detach(), fmap.normals[sel].detach()
        pose, trace = point_to_plane_icp(src, tgt, tgt_n, prev_pose=prev_pose_var, target_gradient=chain, **kw)
    return pose, trace


class ResidentOdometry:
    """PointFusion._localize for the driver's resident map WITHOUT a host round trip: source / target selection, the nearest-neighbour
    index over the targets and the `numiters` Gauss-Newton (icp) or Levenberg-Marquardt (gradicp) iterations are a fixed sequence of
    launches over buffers allocated once -- sizes that depend on the map (live points, active points, targets) are device data -- so a
    keyframe's odometry can sit inside the captured map-update graph (RefineStepPlan.update_map(odometry=...)).  Same arithmetic as
    frame_to_model / point_to_plane_icp above (which remain for ad-hoc clouds and as the cross-check) with the 6x6 solve, the se(3)
    exponential and the damping update in the e2e_icp_update kernel instead of numpy.

    Requires a live frame whose selected pixels all have depth (network predictions 1 / disp do); a hole raises `status`, read by
    check() together with the target-capacity overflow flag wherever the host synchronises anyway."""

    def __init__(self, fmap, dsratio=4, numiters=20, mode="gradicp", damp=1e-8, dist_thresh=None, lambda_max=2.0, B=1.0, B2=1.0, nu=200.0,
                 target_capacity=None, grid_cells=256):
        if mode not in ("icp", "gradicp"):
            raise ValueError(f"unknown odometry mode {mode}")
        self.map, self.ds, self.numiters, self.mode = fmap, int(dsratio), int(numiters), mode
        self.damp, self.dist_thresh = float(damp), dist_thresh
        self.lm = dict(lambda_max=float(lambda_max), B=float(B), B2=float(B2), nu=float(nu))
        H, W, dev = fmap.H, fmap.W, fmap.device
        self.n_src = ((H + self.ds - 1) // self.ds) * ((W + self.ds - 1) // self.ds)
        # active points are map points that project into ONE frame: a few per pixel at most
        self.tcap = int(target_capacity or min(fmap.cap, 8 * H * W) // self.ds + 1)
        f = dict(device=dev, dtype=torch.float32)
        lib = L.load()
        self.Vg, self.Ng = torch.empty(1, H, W, 3, **f), torch.empty(1, H, W, 3, **f)
        self.alpha = torch.empty(1, H, W, **f)
        self.src, self.cur, self.nxt = (torch.empty(self.n_src, 3, **f) for _ in range(3))
        self.tgt, self.tgt_n = torch.empty(self.tcap, 3, **f), torch.empty(self.tcap, 3, **f)
        self.tcount = torch.zeros(3, device=dev, dtype=torch.int64)
        self.status = torch.zeros(1, device=dev, dtype=torch.int32)
        # a coarse grid: 19 200 queries of a sparse target set, decimetres away while the pose is still wrong (e2e_knn1_index_*_res)
        self.cells = int(grid_cells)
        self.index = torch.empty(lib.e2e_knn1_index_capacity_bytes_res(self.n_src, self.tcap, self.cells), device=dev, dtype=torch.uint8)
        self.d = torch.empty(self.n_src, **f)
        self.idx = torch.empty(self.n_src, device=dev, dtype=torch.int64)
        self.out29 = torch.empty(29, device=dev, dtype=torch.float64)
        self.ws = torch.empty(lib.e2e_icp_workspace_bytes(), device=dev, dtype=torch.uint8)
        self.state = torch.zeros(lib.e2e_icp_state_doubles(), device=dev, dtype=torch.float64)
        self.T32, self.step32 = torch.eye(4, **f), torch.eye(4, **f)
        self.pose = torch.eye(4, **f)                       # the result: live pose (4,4), rewritten by every run()
        from .ops import fusion_alpha_den
        self._alpha_den = float(fusion_alpha_den(fmap.sigma))

    def _search_reduce_update(self, pts, st, warm, phase, prev_pose):
        # every search after the first of a keyframe starts from the previous search's neighbours (same source points, moved by one small
        # step; same targets): a real target point's distance bounds the ball from the start -- exact for any candidate
        L.call("e2e_knn1_index_query_dev_res", p1=L.ptr(pts), n1=self.n_src, ref_points=L.ptr(self.tgt) if warm else None,
               warm_idx=L.ptr(self.idx) if warm else None, n2_capacity=self.tcap, max_queries=self.n_src, index=L.ptr(self.index),
               cells_per_axis=self.cells, dists=L.ptr(self.d), idx=L.ptr(self.idx), stream=st)
        L.call("e2e_icp_reduce_update", src=L.ptr(pts), tgt=L.ptr(self.tgt), tgt_normals=L.ptr(self.tgt_n), idx=L.ptr(self.idx), dists=L.ptr(self.d),
               dist_thresh=-1.0 if self.dist_thresh is None else float(self.dist_thresh), n=self.n_src, workspace=L.ptr(self.ws), state=L.ptr(self.state),
               T32=L.ptr(self.T32), step32=L.ptr(self.step32), prev_pose=L.ptr(prev_pose), pose_out=L.ptr(self.pose),
               mode=1 if self.mode == "gradicp" else 0, phase=phase, stream=st, **self.lm)

    def run(self, depth, K, prev_pose):
        """depth (H,W) of the live frame, K (4,4), prev_pose (4,4): contiguous device tensors (resident buffers when this is captured).
        Leaves the estimated live pose in self.pose and returns it.  No host synchronisation, no allocation."""
        m, st = self.map, L.stream()
        H, W = m.H, m.W
        for n, t in (("depth", depth), ("K", K), ("prev_pose", prev_pose)):
            if not L.dev(t, n).is_contiguous():
                raise ValueError(f"ResidentOdometry.run: {n} must be contiguous")
        # the live frame placed with the PREVIOUS pose (initial guess), and the map points active in that view
        L.call("e2e_vertex_normal_maps", depth=L.ptr(depth), K=L.ptr(K), pose=L.ptr(prev_pose), alpha_den=self._alpha_den, V=None, Nm=None,
               Vg=L.ptr(self.Vg), Ng=L.ptr(self.Ng), alpha=L.ptr(self.alpha), B=1, H=H, W=W, stream=st)
        L.call("e2e_pf_associate_dev", map_points=L.ptr(m.points), map_normals=L.ptr(m.normals), map_ccounts=L.ptr(m.ccounts), map_count_dev=L.ptr(m.count),
               K=L.ptr(K), pose=L.ptr(prev_pose), Vg=L.ptr(self.Vg), Ng=L.ptr(self.Ng), dist_th=m.dist_th, dot_th=m.dot_th, workspace=L.ptr(m.ws),
               map_capacity=m.cap, H=H, W=W, stream=st)
        L.call("e2e_pf_active_subsample_dev", map_points=L.ptr(m.points), map_normals=L.ptr(m.normals), map_count_dev=L.ptr(m.count), map_capacity=m.cap,
               workspace=L.ptr(m.ws), H=H, W=W, dsratio=self.ds, tgt=L.ptr(self.tgt), tgt_normals=L.ptr(self.tgt_n), tgt_count_dev=L.ptr(self.tcount),
               tgt_capacity=self.tcap, stream=st)
        L.call("e2e_icp_source_subsample", L.ptr(self.Vg), L.ptr(depth), H, W, self.ds, L.ptr(self.src), L.ptr(self.status), st)
        L.call("e2e_knn1_index_build_dev_res", L.ptr(self.tgt), L.ptr(self.tcount), self.tcap, self.n_src, L.ptr(self.index), self.cells, st)
        L.call("e2e_icp_state_init", L.ptr(self.state), L.ptr(self.T32), L.ptr(self.step32), L.ptr(prev_pose), L.ptr(self.pose), self.damp, st)
        for it in range(self.numiters):
            L.call("e2e_transform_points", L.ptr(self.src), L.ptr(self.T32), L.ptr(self.cur), self.n_src, 0, st)
            self._search_reduce_update(self.cur, st, it > 0, 0, prev_pose)
            if self.mode == "gradicp":
                L.call("e2e_transform_points", L.ptr(self.cur), L.ptr(self.step32), L.ptr(self.nxt), self.n_src, 0, st)
                self._search_reduce_update(self.nxt, st, True, 1, prev_pose)
        m._assoc_M = None
        return self.pose

    def check(self):
        """Host read (one sync) of the two error flags of all runs so far; raises if either fired.  Returns (iterations done by the last run,
        its trace [(inliers, sum r^2)], targets, active points)."""
        st, tc, status = self.state.cpu(), self.tcount.cpu(), int(self.status.item())
        if status:
            raise RuntimeError("resident odometry: a selected pixel of the live frame had no depth (use icp.frame_to_model for depth maps with holes)")
        if int(tc[2]):
            raise RuntimeError(f"resident odometry: more than {self.tcap} target points; raise target_capacity")
        it = int(st[25])
        return it, [(int(st[32 + 2 * k]), float(st[33 + 2 * k])) for k in range(min(it, 64))], int(tc[0]), int(tc[1])
