"""torch.autograd glue over the C ABI (include/e2eslam.h).  Device memory, streams and autograd
bookkeeping come from PyTorch-ROCm; every computation below is a hand-written HIP kernel."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

PADDING = {"zeros": 0, "border": 1}


def _padding(mode):
    if mode not in PADDING:
        raise ValueError(f"padding_mode '{mode}' is not supported by the HIP path (zeros | border)")
    return PADDING[mode]


def _mat(t, name, B):
    t = L.dev(t, name)
    if t.shape != (B, 4, 4):
        raise ValueError(f"{name}: expected shape ({B},4,4), got {tuple(t.shape)}")
    return t.contiguous()


# ---------------------------------------------------------------------------------------------
class _Backproject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, inv_K):
        B, _, H, W = depth.shape
        d = L.dev(depth, "depth").contiguous()
        ik = _mat(inv_K, "inv_K", B)
        out = torch.empty(B, 4, H * W, device=d.device, dtype=torch.float32)
        L.call("e2e_backproject_fwd", L.ptr(d), L.ptr(ik), L.ptr(out), B, H, W, L.stream())
        ctx.save_for_backward(ik, d if ctx.needs_input_grad[1] else None)       # the depth only for the gradient wrt inv_K
        ctx.dims = (B, H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ik, d = ctx.saved_tensors
        B, H, W = ctx.dims
        g = g.contiguous()
        gd = gik = None
        if ctx.needs_input_grad[0]:
            gd = torch.empty(B, 1, H, W, device=g.device, dtype=torch.float32)
            L.call("e2e_backproject_bwd", L.ptr(g), L.ptr(ik), L.ptr(gd), B, H, W, L.stream())
        if ctx.needs_input_grad[1]:          # inv_K is a parameter (self-calibration): sum g_cam[r] depth pix_j
            gik = torch.empty(B, 4, 4, device=g.device, dtype=torch.float32)
            ws = torch.empty(L.query("e2e_backproject_bwd_invk_workspace_bytes", B), device=g.device, dtype=torch.uint8)
            L.call("e2e_backproject_bwd_invk", g_cam=L.ptr(g), depth=L.ptr(d), g_inv_K=L.ptr(gik), workspace=L.ptr(ws), B=B, H=H, W=W, stream=L.stream())
        return gd, gik


def backproject(depth, inv_K):
    """BackprojectDepth.forward -- view_synthesis.py:34-40."""
    if depth.dim() != 4 or depth.shape[1] != 1:
        raise ValueError(f"depth: expected (B,1,H,W), got {tuple(depth.shape)}")
    return _Backproject.apply(depth, inv_K)


class _Project3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, K, T, H, W, geometric):
        B = points.shape[0]
        p = L.dev(points, "points").contiguous()
        K, T = _mat(K, "K", B), _mat(T, "T", B)
        grid = torch.empty(B, H, W, 2, device=p.device, dtype=torch.float32)
        valid = torch.empty(B, 1, H, W, device=p.device, dtype=torch.float32)
        z = torch.empty(B, 1, H, W, device=p.device, dtype=torch.float32) if geometric else None
        L.call("e2e_project3d_fwd", L.ptr(p), L.ptr(K), L.ptr(T), L.ptr(grid), L.ptr(valid), L.ptr(z), B, H, W, L.stream())
        ctx.save_for_backward(p, K, T)
        ctx.dims = (B, H, W)
        ctx.mark_non_differentiable(valid)
        if geometric:
            return grid, z, valid
        return grid, valid

    @staticmethod
    @once_differentiable
    def backward(ctx, g_grid, *rest):
        p, K, T = ctx.saved_tensors
        B, H, W = ctx.dims
        g_z = rest[0] if len(rest) == 2 else None
        g_grid = (g_grid if g_grid is not None else torch.zeros(B, H, W, 2, device=p.device)).contiguous()
        g_z = g_z.contiguous() if g_z is not None else None
        gp = gK = gT = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty_like(p)
            L.call("e2e_project3d_bwd", L.ptr(p), L.ptr(K), L.ptr(T), L.ptr(g_grid), L.ptr(g_z), L.ptr(gp), B, H, W, L.stream())
        if ctx.needs_input_grad[2]:          # the pose carries a graph (differentiable odometry, e2ehip.icp): d/dT through P = (K T)[:3]
            gT = torch.empty_like(T)
            ws = torch.empty(L.load().e2e_project3d_bwd_t_workspace_bytes(B), device=p.device, dtype=torch.uint8)
            L.call("e2e_project3d_bwd_t", points=L.ptr(p), K=L.ptr(K), T=L.ptr(T), g_grid=L.ptr(g_grid), g_z=L.ptr(g_z), g_T=L.ptr(gT),
                   workspace=L.ptr(ws), B=B, H=H, W=W, stream=L.stream())
        if ctx.needs_input_grad[1]:          # K is a parameter (self-calibration): d/dK through the same P, g_K[:3] = Pbar T^T
            gK = torch.empty_like(K)
            ws = torch.empty(L.query("e2e_project3d_bwd_k_workspace_bytes", B), device=p.device, dtype=torch.uint8)
            L.call("e2e_project3d_bwd_k", points=L.ptr(p), K=L.ptr(K), T=L.ptr(T), g_grid=L.ptr(g_grid), g_z=L.ptr(g_z), g_K=L.ptr(gK),
                   workspace=L.ptr(ws), B=B, H=H, W=W, stream=L.stream())
        return gp, gK, gT, None, None, None


def project3d(points, K, T, height, width, geometric=False):
    """Project3D.forward -- view_synthesis.py:54-78."""
    if points.dim() != 3 or points.shape[1] != 4 or points.shape[2] != height * width:
        raise ValueError(f"points: expected (B,4,{height * width}), got {tuple(points.shape)}")
    return _Project3D.apply(points, K, T, height, width, bool(geometric))


class _GridSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, inp, grid, pad, align):
        B, C, Hi, Wi = inp.shape
        _, Ho, Wo, _ = grid.shape
        inp = L.dev(inp, "input")
        grid = L.dev(grid, "grid").contiguous()
        out = torch.empty(B, C, Ho, Wo, device=inp.device, dtype=torch.float32)
        L.call("e2e_grid_sample_fwd", input=L.ptr(inp), in_strides=L.strides4(inp), grid=L.ptr(grid), out=L.ptr(out), B=B, C=C, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo,
               padding_mode=pad, align_corners=int(align), stream=L.stream())
        ctx.save_for_backward(inp, grid)
        ctx.cfg = (pad, int(align))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        inp, grid = ctx.saved_tensors
        pad, align = ctx.cfg
        B, C, Hi, Wi = inp.shape
        _, Ho, Wo, _ = grid.shape
        g = g.contiguous()
        gg = torch.empty_like(grid)
        common = dict(input=L.ptr(inp), in_strides=L.strides4(inp), grid=L.ptr(grid), g_out=L.ptr(g), g_grid=L.ptr(gg), B=B, C=C, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo,
                      padding_mode=pad, align_corners=align, stream=L.stream())
        if ctx.needs_input_grad[0]:      # gradient wrt the sampled image: a scatter -- fixed-point integer accumulation, bitwise reproducible
            gi = torch.empty(B, C, Hi, Wi, device=g.device, dtype=torch.float32)
            fx = torch.empty(B * C * Hi * Wi + 1, device=g.device, dtype=torch.int64)      # + the poison word (non-finite / out-of-range contributions)
            L.call("e2e_grid_sample_bwd_exact", g_input_fixed=L.ptr(fx), g_input=L.ptr(gi), **common)
            return gi, gg, None, None
        L.call("e2e_grid_sample_bwd", g_input=None, **common)
        return None, gg, None, None


def grid_sample(input, grid, mode="bilinear", padding_mode="zeros", align_corners=False):
    """F.grid_sample as the reference calls it (online_adaption.py:431-439,450-453)."""
    if mode != "bilinear":
        raise ValueError("only bilinear sampling is on the reference's path")
    if input.dim() != 4 or grid.dim() != 4 or grid.shape[-1] != 2 or grid.shape[0] != input.shape[0]:
        raise ValueError(f"grid_sample: bad shapes input {tuple(input.shape)} grid {tuple(grid.shape)}")
    return _GridSample.apply(input, grid, _padding(padding_mode), bool(align_corners))


class _Photometric(torch.autograd.Function):
    """returns (ssim (B,C,H,W), pmap (B,1,H,W)); either may be unused by the caller."""

    @staticmethod
    def forward(ctx, x, y, want_ssim, want_pmap):
        B, C, H, W = x.shape
        x, y = L.dev(x, "prediction"), L.dev(y, "target")
        ssim = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32) if want_ssim else None
        pmap = torch.empty(B, 1, H, W, device=x.device, dtype=torch.float32) if want_pmap else None
        L.call("e2e_photometric_fwd", x=L.ptr(x), xs=L.strides4(x), y=L.ptr(y), ys=L.strides4(y), ssim_out=L.ptr(ssim), pmap_out=L.ptr(pmap), B=B, C=C, H=H, W=W,
               stream=L.stream())
        ctx.save_for_backward(x, y)
        return ssim, pmap

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ssim, g_pmap):
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        g_ssim = g_ssim.contiguous() if g_ssim is not None else None
        g_pmap = g_pmap.contiguous() if g_pmap is not None else None
        gx = gy = None
        if g_ssim is None and g_pmap is None:
            return None, None, None, None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
            L.call("e2e_photometric_bwd", x=L.ptr(x), xs=L.strides4(x), y=L.ptr(y), ys=L.strides4(y), g_pmap=L.ptr(g_pmap), g_ssim=L.ptr(g_ssim), g_x=L.ptr(gx),
                   B=B, C=C, H=H, W=W, stream=L.stream())
        if ctx.needs_input_grad[1]:
            gy = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
            L.call("e2e_photometric_bwd", x=L.ptr(y), xs=L.strides4(y), y=L.ptr(x), ys=L.strides4(x), g_pmap=L.ptr(g_pmap), g_ssim=L.ptr(g_ssim), g_x=L.ptr(gy),
                   B=B, C=C, H=H, W=W, stream=L.stream())       # gradient wrt the target: the operands swapped
        return gx, gy, None, None


def _check_pair(x, y):
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"expected two (B,C,H,W) tensors of equal shape, got {tuple(x.shape)} / {tuple(y.shape)}")


def ssim(x, y):
    """SSIM.forward -- losses.py:23-37."""
    _check_pair(x, y)
    return _Photometric.apply(x, y, True, False)[0]


def photometric(prediction, target):
    """photometric_loss -- losses.py:97-117 (0.85 mean_c SSIM + 0.15 mean_c L1)."""
    _check_pair(prediction, target)
    return _Photometric.apply(prediction, target, False, True)[1]


# ---------------------------------------------------------------------------------------------
def _check_warp_inputs(fn, depth_tgt, srcs, tgt, K, inv_K, n_poses=None, intrinsics_grad=False):
    """What warp_photometric and warp_photometric_window (`fn`) refuse alike: intrinsics that require grad without intrinsics_grad=True, a
    depth_tgt that is not (B,1,H,W), for the window (n_poses given) anything but 1 or 2 sources and as many poses, frames that are not
    (B,3,H,W).  Returns (B, H, W)."""
    if torch.is_grad_enabled() and not intrinsics_grad:
        for n, t in (("K", K), ("inv_K", inv_K)):
            if torch.is_tensor(t) and t.requires_grad:
                raise NotImplementedError(f"{fn}: {n} requires grad, and the fused kernels have no gradient with respect to the intrinsics")
    if depth_tgt.dim() != 4 or depth_tgt.shape[1] != 1:
        raise ValueError(f"depth_tgt: expected (B,1,H,W), got {tuple(depth_tgt.shape)}")
    B, _, H, W = depth_tgt.shape
    if n_poses is not None and (len(srcs) not in (1, 2) or n_poses != len(srcs)):
        raise ValueError(f"{fn}: expected 1 or 2 source frames and as many poses, got {len(srcs)} and {n_poses}")
    for n, t in [("source_frame", s) for s in srcs] + [("target_frame", tgt)]:
        if tuple(t.shape) != (B, 3, H, W):
            raise ValueError(f"{n}: expected ({B},3,{H},{W}), got {tuple(t.shape)}")
    return B, H, W


class _WarpPhotometric(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_tgt, depth_src, init_tgt, init_src, src, tgt, K, inv_K, T, pad, use_mask, reg_kind, want_pmap):
        B, _, H, W = depth_tgt.shape
        dt = L.dev(depth_tgt, "depth_tgt").contiguous()
        src, tgt = L.dev(src, "source_frame"), L.dev(tgt, "target_frame")
        K, inv_K, T = _mat(K, "K", B), _mat(inv_K, "inv_K", B), _mat(T, "T", B)
        ds = it = is_ = None
        if reg_kind:
            ds = L.dev(depth_src, "depth_src").contiguous()
            it, is_ = L.dev(init_tgt, "init_tgt").contiguous(), L.dev(init_src, "init_src").contiguous()
        dev = dt.device
        synth = torch.empty(B, 3, H, W, device=dev, dtype=torch.float32)
        valid = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
        pmap = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32) if want_pmap else None
        loss = torch.zeros(2, device=dev, dtype=torch.float32)
        ws = torch.empty(L.load().e2e_warp_photo_workspace_floats(B, H, W), device=dev, dtype=torch.float32)
        L.call("e2e_warp_photo_fwd", depth_tgt=L.ptr(dt), src=L.ptr(src), src_strides=L.strides4(src), tgt=L.ptr(tgt), tgt_strides=L.strides4(tgt), K=L.ptr(K),
               inv_K=L.ptr(inv_K), T=L.ptr(T), synth=L.ptr(synth), valid=L.ptr(valid), pmap=L.ptr(pmap), use_mask=int(use_mask), padding_mode=pad,
               reg_kind=reg_kind, reg_init_tgt=L.ptr(it), reg_init_src=L.ptr(is_), depth_src=L.ptr(ds), loss_out=L.ptr(loss), workspace=L.ptr(ws),
               B=B, H=H, W=W, stream=L.stream())
        ctx.save_for_backward(dt, ds, it, is_, src, tgt, K, inv_K, T, synth, valid)
        ctx.cfg = (pad, int(use_mask), reg_kind, B, H, W)
        ctx.mark_non_differentiable(synth, valid)
        if pmap is not None:
            ctx.mark_non_differentiable(pmap)
        return loss[0], loss[1], synth, valid, pmap

    @staticmethod
    @once_differentiable
    def backward(ctx, g0, g1, *_):
        dt, ds, it, is_, src, tgt, K, inv_K, T, synth, valid = ctx.saved_tensors
        pad, use_mask, reg_kind, B, H, W = ctx.cfg
        z = torch.zeros((), device=dt.device)
        gl = torch.stack([g0 if g0 is not None else z, g1 if g1 is not None else z]).contiguous()
        gdt = torch.empty(B, 1, H, W, device=dt.device, dtype=torch.float32)
        gds = torch.empty(B, 1, H, W, device=dt.device, dtype=torch.float32) if reg_kind else None
        common = dict(depth_tgt=L.ptr(dt), src=L.ptr(src), src_strides=L.strides4(src), tgt=L.ptr(tgt), tgt_strides=L.strides4(tgt), K=L.ptr(K),
                      inv_K=L.ptr(inv_K), T=L.ptr(T), synth=L.ptr(synth), valid=L.ptr(valid), use_mask=use_mask, padding_mode=pad, reg_kind=reg_kind,
                      reg_init_tgt=L.ptr(it), reg_init_src=L.ptr(is_), depth_src=L.ptr(ds), g_loss=L.ptr(gl), g_depth_tgt=L.ptr(gdt),
                      g_depth_src=L.ptr(gds), B=B, H=H, W=W, stream=L.stream())
        gT = gK = giK = None
        if ctx.needs_input_grad[8]:          # the pose carries a graph (differentiable odometry, e2ehip.icp): the same kernel also sums d/dT
            gT = torch.empty(B, 4, 4, device=dt.device, dtype=torch.float32)
        if ctx.needs_input_grad[6] or ctx.needs_input_grad[7]:      # an intrinsic is a parameter (intrinsics_grad=True): 9 sums more, both gradients
            gK, giK = (torch.empty(B, 4, 4, device=dt.device, dtype=torch.float32) for _ in range(2))
            ws = torch.empty(L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", B, H, W), device=dt.device, dtype=torch.uint8)
            L.call("e2e_warp_photo_bwd_intrinsics", g_T=L.ptr(gT), g_K=L.ptr(gK), g_inv_K=L.ptr(giK), workspace=L.ptr(ws), **common)
        elif gT is not None:
            ws = torch.empty(L.load().e2e_warp_photo_bwd_pose_workspace_bytes(B, H, W), device=dt.device, dtype=torch.uint8)
            L.call("e2e_warp_photo_bwd_pose", g_T=L.ptr(gT), workspace=L.ptr(ws), **common)
        else:
            L.call("e2e_warp_photo_bwd", **common)
        return (gdt, gds) + (None,) * 4 + (gK if ctx.needs_input_grad[6] else None, giK if ctx.needs_input_grad[7] else None, gT) + (None,) * 4


def warp_photometric(depth_tgt, src, tgt, K, inv_K, T, padding_mode="border", use_mask=True,
                     depth_src=None, init_tgt=None, init_src=None, reg_kind=None, want_pmap=False, intrinsics_grad=False):
    """Fused image-space part of one refinement step (2 launches forward, 1 backward; 2 backward when T requires grad).

    depth_tgt (B,1,H,W); src/tgt (B,3,H,W) views (NHWC memory welcome); K, inv_K, T (B,4,4).
    reg_kind None | "l1" | "l2" adds mean-reg(init_tgt, depth_tgt) + mean-reg(init_src, depth_src).
    Returns dict(photometric, reg, synth, valid, pmap).

    Differentiated: depth_tgt, depth_src (through the regulariser only) and T (e2e_warp_photo_bwd_pose; the gradient has the shape of
    the T that was passed, so a pose expanded over the batch gets the sum).  The frames, init_tgt / init_src and the outputs synth, valid
    and pmap are constants.  K and inv_K are constants too: one that requires grad raises NotImplementedError -- unless
    intrinsics_grad=True (self-calibration): then the backward is e2e_warp_photo_bwd_intrinsics whenever K or inv_K requires grad, and
    K.grad / inv_K.grad have the shape of what was passed (a (4,4) matrix expanded over the batch gets the sum).  K and inv_K are
    independent inputs: the gradient of each is taken with the other held fixed.  With neither requiring grad the launches are the same
    as without the keyword.
    reference: online_adaption.py:412-455, :544-564, :482-511, :612-623."""
    B, H, W = _check_warp_inputs("warp_photometric", depth_tgt, [src], tgt, K, inv_K, intrinsics_grad=bool(intrinsics_grad))
    rk = {None: 0, "l1": 1, "l2": 2}.get(reg_kind, -1)
    if rk < 0:
        raise ValueError("please specify a correct norm")          # losses.py:146
    if rk:
        for n, t in (("depth_src", depth_src), ("init_tgt", init_tgt), ("init_src", init_src)):
            if t is None or tuple(t.shape) != (B, 1, H, W):
                raise ValueError(f"{n}: expected ({B},1,{H},{W})")
    p, r, synth, valid, pmap = _WarpPhotometric.apply(depth_tgt, depth_src, init_tgt, init_src, src, tgt, K, inv_K, T,
                                                      _padding(padding_mode), bool(use_mask), rk, bool(want_pmap))
    return {"photometric": p, "reg": r, "synth": synth, "valid": valid, "pmap": pmap}


TERM_AUTO_MASKING, TERM_MIN_REPROJECTION = 2, 4                # E2E_TERM_* of include/e2eslam.h


class _WarpPhotometricWindow(torch.autograd.Function):
    """the window (e2e_warp_photo_window_fwd / _bwd), or -- with geo_min_valid and one depth per source -- the window with the
    geometric-consistency term (e2e_warp_photo_geo_fwd / _bwd); geo_min_valid None: dsrc0 / dsrc1 are None, and so are the outputs geo and count.
    groups = G (not None, with the geometric term only): the batch is G scale groups and the term is reduced and gated per group
    (e2e_warp_photo_geo_groups_fwd / _bwd); geo and count are then (S G,), indexed [s G + g]"""

    @staticmethod
    def forward(ctx, depth_tgt, dsrc0, dsrc1, src0, src1, tgt, K, inv_K, T0, T1, tie_noise, pad, use_mask, terms, geo_min_valid, want_pmap,
                groups):
        B, _, H, W = depth_tgt.shape
        S = 1 if src1 is None else 2
        geo = geo_min_valid is not None
        G = 1 if groups is None else groups
        name = "e2e_warp_photo_geo" if geo else "e2e_warp_photo_window"
        entry = name if groups is None else "e2e_warp_photo_geo_groups"
        dt = L.dev(depth_tgt, "depth_tgt").contiguous()
        ds0 = L.dev(dsrc0, "depth_src").contiguous() if geo else None
        ds1 = L.dev(dsrc1, "depth_src").contiguous() if geo and S == 2 else None
        src0, tgt = L.dev(src0, "source_frame"), L.dev(tgt, "target_frame")
        if S == 2:
            src1 = L.dev(src1, "source_frame")
            if src1.stride() != src0.stride():                 # one stride set serves both sources: a copy of the second in the first's layout
                if 0 in src0.stride():
                    src0 = src0.contiguous()
                src1 = torch.empty_strided(src0.shape, src0.stride(), device=src0.device, dtype=torch.float32).copy_(src1)
        K, inv_K = _mat(K, "K", B), _mat(inv_K, "inv_K", B)
        T = torch.stack([_mat(t, "T", B) for t in ((T0, T1) if S == 2 else (T0,))])
        noise = L.dev(tie_noise, "tie_noise").contiguous() if tie_noise is not None else None
        dev = dt.device
        synth = torch.empty(S, B, 3, H, W, device=dev, dtype=torch.float32)
        valid = torch.empty(S, B, 1, H, W, device=dev, dtype=torch.float32)
        select = torch.empty(B, 1, H, W, device=dev, dtype=torch.int32)
        pmap = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32) if want_pmap else None
        count = torch.empty(S * G, device=dev, dtype=torch.int32) if geo else None
        loss = torch.zeros(1 + S * G if geo else 1, device=dev, dtype=torch.float32)
        ws = torch.empty(L.query(name + "_workspace_floats", S, B, H, W), device=dev, dtype=torch.float32)
        more = dict(depth_src0=L.ptr(ds0), depth_src1=L.ptr(ds1), geo_count=L.ptr(count), geo_min_valid=geo_min_valid) if geo else {}
        if groups is not None:
            more["groups"] = groups
        L.call(entry + "_fwd", depth_tgt=L.ptr(dt), src0=L.ptr(src0), src1=L.ptr(src1), src_strides=L.strides4(src0), tgt=L.ptr(tgt),
               tgt_strides=L.strides4(tgt), K=L.ptr(K), inv_K=L.ptr(inv_K), T=L.ptr(T), tie_noise=L.ptr(noise), synth=L.ptr(synth), valid=L.ptr(valid),
               select=L.ptr(select), pmap=L.ptr(pmap), use_mask=int(use_mask), padding_mode=pad, terms=terms, loss_out=L.ptr(loss),
               workspace=L.ptr(ws), S=S, B=B, H=H, W=W, stream=L.stream(), **more)
        ctx.save_for_backward(dt, ds0, ds1, src0, src1, tgt, K, inv_K, T, synth, valid, select, count)
        ctx.cfg = (pad, int(use_mask), terms, geo_min_valid, S, B, H, W, groups)
        ctx.mark_non_differentiable(*(t for t in (synth, valid, select, count, pmap) if t is not None))
        return loss[0], (loss[1:] if geo else None), synth, valid, select, count, pmap

    @staticmethod
    @once_differentiable
    def backward(ctx, g0, g1, *_):
        dt, ds0, ds1, src0, src1, tgt, K, inv_K, T, synth, valid, select, count = ctx.saved_tensors
        pad, use_mask, terms, geo_min_valid, S, B, H, W, groups = ctx.cfg
        geo = geo_min_valid is not None
        name = "e2e_warp_photo_geo" if geo else "e2e_warp_photo_window"
        dev = dt.device
        gl = (g0 if g0 is not None else torch.zeros((), device=dev)).reshape(1)
        if geo:
            gl = torch.cat([gl, g1 if g1 is not None else torch.zeros(S * (groups or 1), device=dev)])
        gl = gl.contiguous()
        gdt = torch.empty(B, 1, H, W, device=dev, dtype=torch.float32)
        gds = torch.empty(S, B, 1, H, W, device=dev, dtype=torch.float32) if geo else None
        gT = gK = giK = ws = None
        if ctx.needs_input_grad[8] or (S == 2 and ctx.needs_input_grad[9]):      # a pose carries a graph: the same launch also sums d/dT
            gT = torch.empty(S, B, 4, 4, device=dev, dtype=torch.float32)
        more = dict(depth_src0=L.ptr(ds0), depth_src1=L.ptr(ds1), geo_count=L.ptr(count), geo_min_valid=geo_min_valid,
                    g_depth_src=L.ptr(gds)) if geo else {}
        entry = name + "_bwd"
        if groups is not None:                                  # the grouped pair has no intrinsics form: warp_photometric_multiscale refuses K / inv_K
            more["groups"] = groups
        if ctx.needs_input_grad[6] or ctx.needs_input_grad[7]:  # an intrinsic is a parameter (intrinsics_grad=True): both gradients, summed over the sources
            entry = name + "_bwd_intrinsics"
            gK, giK = (torch.empty(B, 4, 4, device=dev, dtype=torch.float32) for _ in range(2))
            more.update(g_K=L.ptr(gK), g_inv_K=L.ptr(giK))
        if geo or gT is not None or gK is not None:            # the float64 sums; the geometric form's depth scatter always needs its scratch
            ws = torch.empty(L.query(entry + "_workspace_bytes", S, B, H, W), device=dev, dtype=torch.uint8)
        if groups is not None:
            entry = "e2e_warp_photo_geo_groups_bwd"             # the geo pair's workspace at the stacked batch
        L.call(entry, depth_tgt=L.ptr(dt), src0=L.ptr(src0), src1=L.ptr(src1), src_strides=L.strides4(src0), tgt=L.ptr(tgt),
               tgt_strides=L.strides4(tgt), K=L.ptr(K), inv_K=L.ptr(inv_K), T=L.ptr(T), synth=L.ptr(synth), valid=L.ptr(valid), select=L.ptr(select),
               use_mask=use_mask, padding_mode=pad, terms=terms, g_loss=L.ptr(gl), g_depth_tgt=L.ptr(gdt), g_T=L.ptr(gT), workspace=L.ptr(ws),
               S=S, B=B, H=H, W=W, stream=L.stream(), **more)
        g_T0 = gT[0] if gT is not None and ctx.needs_input_grad[8] else None
        g_T1 = gT[1] if gT is not None and S == 2 and ctx.needs_input_grad[9] else None
        return (gdt, gds[0] if geo else None, gds[1] if geo and S == 2 else None) + (None,) * 3 + \
            (gK if ctx.needs_input_grad[6] else None, giK if ctx.needs_input_grad[7] else None, g_T0, g_T1) + (None,) * 7


def warp_photometric_window(depth_tgt, srcs, tgt, K, inv_K, Ts, padding_mode="border", use_mask=True, min_reprojection=False,
                            auto_masking=False, tie_noise=None, want_pmap=False, geometric=False, depth_srcs=None, geo_min_valid=10000,
                            intrinsics_grad=False):
    """The fused pair over a window of one or two source frames with the candidate / minimum logic of train_depth.py:621-662
    (e2e_warp_photo_window_fwd / _bwd: 2 launches forward, 1 backward; 2 backward when a pose requires grad).

    geometric=True (LOSS.geometric, train_depth.py:558-576) takes e2e_warp_photo_geo_fwd / _bwd instead: the source images are then sampled
    with align_corners=True as the reference does under that flag, depth_srcs -- one (B,1,H,W) depth per source -- are sampled on the same grid,
    and the dict gains geometric (S,): per source sum(diff valid) / n if n > geo_min_valid else 0, differentiable, and geo_count (S,) int32:
    n, the valid projections of each source.  The depth of every source is then differentiated too.

    depth_tgt (B,1,H,W); srcs: 1 or 2 (B,3,H,W) views, tgt likewise (NHWC memory welcome; sources whose strides differ cost one copy of
    the second); K, inv_K (B,4,4); Ts: one (B,4,4) pose per source.  auto_masking puts the identity maps photometric(src m, tgt m) before
    the reprojection maps; min_reprojection keeps one candidate per source instead of their mean, and with both tie_noise (B,S,H,W) --
    None: nothing -- is added to the identity maps.  Returns dict(photometric, synth (S,B,3,H,W), valid (S,B,1,H,W), select (B,1,H,W) int32:
    the index of the first minimal candidate, pmap (B,1,H,W): the minimum, when asked for).

    Differentiated: depth_tgt and every T (the gradient has the shape of the T that was passed, so a pose expanded over the batch gets the
    sum).  Frames, masks, tie_noise and the other outputs are constants; K or inv_K requiring grad raises NotImplementedError unless
    intrinsics_grad=True: then the backward is e2e_warp_photo_window_bwd_intrinsics / e2e_warp_photo_geo_bwd_intrinsics whenever one of them
    requires grad, and K.grad / inv_K.grad (the sum over the sources) have the shape of what was passed."""
    srcs, Ts = list(srcs), list(Ts)
    S = len(srcs)
    B, H, W = _check_warp_inputs("warp_photometric_window", depth_tgt, srcs, tgt, K, inv_K, n_poses=len(Ts), intrinsics_grad=bool(intrinsics_grad))
    if tie_noise is not None and tuple(tie_noise.shape) != (B, S, H, W):
        raise ValueError(f"tie_noise: expected ({B},{S},{H},{W}), got {tuple(tie_noise.shape)}")
    terms = (TERM_AUTO_MASKING if auto_masking else 0) | (TERM_MIN_REPROJECTION if min_reprojection else 0)
    if geometric:
        depth_srcs = list(depth_srcs) if depth_srcs is not None else []
        if len(depth_srcs) != S or any(tuple(t.shape) != (B, 1, H, W) for t in depth_srcs):
            raise ValueError(f"warp_photometric_window: geometric=True needs depth_srcs, one ({B},1,{H},{W}) depth per source")
        if int(geo_min_valid) < 0:
            raise ValueError(f"geo_min_valid: {geo_min_valid} is negative")
        geo_min_valid = int(geo_min_valid)
    else:
        depth_srcs, geo_min_valid = [None, None], None
    p, geo, synth, valid, select, count, pmap = _WarpPhotometricWindow.apply(
        depth_tgt, depth_srcs[0], depth_srcs[1] if S == 2 else None, srcs[0], srcs[1] if S == 2 else None, tgt, K, inv_K, Ts[0],
        Ts[1] if S == 2 else None, tie_noise, _padding(padding_mode), bool(use_mask), terms, geo_min_valid, bool(want_pmap), None)
    out = {"photometric": p, "synth": synth, "valid": valid, "select": select, "pmap": pmap}
    if geometric:
        out.update(geometric=geo, geo_count=count)
    return out


# ---------------------------------------------------------------------------------------------
# RGB-D unprojection, rigid transforms, nearest neighbours
# ---------------------------------------------------------------------------------------------
def fusion_alpha_den(sigma, eps=1e-7):
    """2 sigma^2 + eps evaluated in double, rounded to fp32 when passed (gradslam get_alpha)."""
    return 2.0 * (float(sigma) ** 2) + eps


class _VertexMaps(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, K, pose, alpha_den, alpha_grad=False, normal_grad=False):
        B, H, W = depth.shape
        d = L.dev(depth, "depth").contiguous()
        K, pose = _mat(K, "intrinsics", B), _mat(pose, "poses", B)
        f = dict(device=d.device, dtype=torch.float32)
        V, Nm, Vg, Ng = (torch.empty(B, H, W, 3, **f) for _ in range(4))
        alpha = torch.empty(B, H, W, **f)
        L.call("e2e_vertex_normal_maps", depth=L.ptr(d), K=L.ptr(K), pose=L.ptr(pose), alpha_den=float(alpha_den), V=L.ptr(V), Nm=L.ptr(Nm), Vg=L.ptr(Vg),
               Ng=L.ptr(Ng), alpha=L.ptr(alpha), B=B, H=H, W=W, stream=L.stream())
        ctx.alpha_den = float(alpha_den) if alpha_grad else None
        ctx.normal_grad = bool(normal_grad)
        saved = (d, K, pose, alpha) if alpha_grad else (d, K, pose)
        if ctx.needs_input_grad[2]:                       # the pose is a variable (the chain gradient): its adjoint needs V
            saved = saved + (V,)
            if normal_grad:                               # ... and Ng = R n needs n
                saved = saved + (Nm,)
        ctx.save_for_backward(*saved)
        fixed = () if normal_grad else (Nm, Ng)
        if alpha_grad:
            ctx.mark_non_differentiable(*fixed)
        else:
            ctx.mark_non_differentiable(*fixed, alpha)
        if alpha_grad or normal_grad:
            ctx.set_materialize_grads(False)              # a map step that only moves confidences sends no g_Vg
        return V, Nm, Vg, Ng, alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, gV, gN, gVg, gNg, ga):
        d, K, pose = ctx.saved_tensors[:3]
        B, H, W = d.shape
        if ctx.alpha_den is None:
            ga = None
        if not ctx.normal_grad:
            gN = gNg = None
        if gV is None and gVg is None and ga is None and gN is None and gNg is None:
            return None, None, None, None, None, None
        gd = torch.empty_like(d)
        g_pose = None
        written = gV is not None or gVg is not None
        if written:
            gV = gV.contiguous() if gV is not None else None
            gVg = gVg.contiguous() if gVg is not None else None
            L.call("e2e_vertex_maps_bwd", L.ptr(d), L.ptr(K), L.ptr(pose), L.ptr(gV), L.ptr(gVg), L.ptr(gd), B, H, W, L.stream())
        if gN is not None or gNg is not None:
            gN = gN.contiguous() if gN is not None else None
            gNg = gNg.contiguous() if gNg is not None else None
        if ctx.needs_input_grad[2]:
            # Vg = (R V + t) on the valid pixels: g_pose[b][:3] = [sum g_Vg V^T | sum g_Vg]; alpha does not see the pose
            g_pose = torch.zeros(B, 4, 4, device=d.device, dtype=torch.float32)
            if gVg is not None:
                V = ctx.saved_tensors[-2 if ctx.normal_grad else -1]
                gm = (gVg * (d != 0)[..., None]).reshape(B, H * W, 3)
                for b in range(B):
                    g_pose[b, :3] = transform_points_bwd_T(gm[b], V[b].reshape(H * W, 3)).float()
            if gNg is not None:
                # Ng = R n: g_pose[b][:3,:3] += sum g_Ng n^T (n is 0 on the invalid pixels); the fourth column of that call is no gradient
                Nm = ctx.saved_tensors[-1]
                for b in range(B):
                    g_pose[b, :3, :3] += transform_points_bwd_T(gNg[b].reshape(H * W, 3), Nm[b].reshape(H * W, 3))[:, :3].float()
        if ga is not None:
            L.call("e2e_vertex_alpha_bwd", depth=L.ptr(d), K=L.ptr(K), alpha=L.ptr(ctx.saved_tensors[3]), g_alpha=L.ptr(ga.contiguous()),
                   alpha_den=ctx.alpha_den, g_depth=L.ptr(gd), accumulate=int(written), B=B, H=H, W=W, stream=L.stream())
            written = True
        if gN is not None or gNg is not None:
            L.call("e2e_normal_maps_bwd", depth=L.ptr(d), K=L.ptr(K), pose=L.ptr(pose), g_Nm=L.ptr(gN), g_Ng=L.ptr(gNg), g_depth=L.ptr(gd),
                   accumulate=int(written), B=B, H=H, W=W, stream=L.stream())
        return gd, None, g_pose, None, None, None


def vertex_normal_maps(depth, K, pose, sigma=0.6, alpha_grad=False, normal_grad=False):
    """depth (B,H,W), K/pose (B,4,4) -> dict V, n, Vg, ng (B,H,W,3), alpha (B,H,W), valid (B,H,W) bool.
    gradslam RGBDImages maps; differentiable wrt depth through V and Vg, and -- with alpha_grad=True only --
    through the fusion confidence alpha (e2e_vertex_alpha_bwd).  A pose that requires grad gets its gradient through Vg
    (e2e_transform_points_bwd_t per batch item; bottom row 0).  The normals are differentiated with normal_grad=True only: n and ng
    then carry the gradient to the depth (e2e_normal_maps_bwd, into the same g_depth) and ng to the rotation of such a pose; off,
    they are constants and the values are the same bits."""
    if depth.dim() != 3:
        raise ValueError(f"depth: expected (B,H,W), got {tuple(depth.shape)}")
    V, Nm, Vg, Ng, alpha = _VertexMaps.apply(depth, K, pose, fusion_alpha_den(sigma), bool(alpha_grad), bool(normal_grad))
    return {"V": V, "n": Nm, "Vg": Vg, "ng": Ng, "alpha": alpha, "valid": depth.detach() != 0}


class _TransformPoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, T):
        p = L.dev(points, "points").contiguous()
        T = L.dev(T, "transform").contiguous()
        out = torch.empty_like(p)
        L.call("e2e_transform_points", L.ptr(p), L.ptr(T), L.ptr(out), p.shape[0], 0, L.stream())
        ctx.save_for_backward(T, p if ctx.needs_input_grad[1] else None)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        T, p = ctx.saved_tensors
        g = g.contiguous()
        gp = gT = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty_like(g)
            L.call("e2e_transform_points", L.ptr(g), L.ptr(T), L.ptr(gp), g.shape[0], 1, L.stream())
        if ctx.needs_input_grad[1]:
            gT = torch.zeros(4, 4, device=g.device, dtype=torch.float32)
            gT[:3] = transform_points_bwd_T(g, p).float()
        return gp, gT


def transform_points_bwd_T(g, points):
    """g, points (n,3) -> (3,4) float64 device tensor [sum_i g_i p_i^T | sum_i g_i]: the top rows of d/dT of sum(g . (R p + t))."""
    out = torch.empty(3, 4, device=g.device, dtype=torch.float64)
    ws = torch.empty(L.load().e2e_transform_points_bwd_t_workspace_bytes(), device=g.device, dtype=torch.uint8)
    L.call("e2e_transform_points_bwd_t", L.ptr(g), L.ptr(points), g.shape[0], L.ptr(out), L.ptr(ws), L.stream())
    return out


def transform_points(points, T):
    """gradslam.geometry.geometryutils.transform_pointcloud: (N,3), (4,4) -> (N,3)."""
    if not torch.is_tensor(points) or not torch.is_tensor(T):
        raise TypeError("Expected torch.Tensor inputs")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"pointcloud must have shape (N,3), got {tuple(points.shape)}")
    if tuple(T.shape) != (4, 4):
        raise ValueError(f"transform must have shape (4,4), got {tuple(T.shape)}")
    if points.shape[0] == 0:
        return points.clone()
    return _TransformPoints.apply(points, T)


KNN_ALGORITHMS = {"auto": 0, "brute": 1, "grid": 2}


class _SelectRows(torch.autograd.Function):
    """x[mask] for a (N, C) tensor and a (N,) bool mask.  Same values as boolean indexing; the backward writes the
    incoming rows back with index_copy_ (the indices are unique) instead of ATen's accumulate path, which sorts the
    index list on every call (2 rocPRIM merge passes + indexing_backward: ~180 us per refinement step at 480x640)."""

    @staticmethod
    def forward(ctx, x, mask):
        idx = torch.nonzero(mask, as_tuple=False).reshape(-1)
        ctx.save_for_backward(idx)
        ctx.shape = x.shape
        return x.index_select(0, idx)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        return torch.zeros(ctx.shape, dtype=g.dtype, device=g.device).index_copy_(0, idx, g.contiguous()), None


def select_rows(x, mask):
    if x.dim() != 2 or mask.shape != x.shape[:1] or mask.dtype != torch.bool:
        raise ValueError("select_rows expects x (N, C) and a bool mask (N,)")
    return _SelectRows.apply(x, mask)


class _Knn1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, algorithm):
        a, b = L.dev(p1, "p1").contiguous(), L.dev(p2, "p2").contiguous()
        n1, n2 = a.shape[0], b.shape[0]
        d = torch.empty(n1, device=a.device, dtype=torch.float32)
        idx = torch.empty(n1, device=a.device, dtype=torch.int64)
        ws = torch.empty(L.load().e2e_knn1_workspace_bytes(n1, n2), device=a.device, dtype=torch.uint8)
        L.call("e2e_knn1_fwd", L.ptr(a), n1, L.ptr(b), n2, L.ptr(d), L.ptr(idx), L.ptr(ws), algorithm, L.stream())
        ctx.save_for_backward(a, b, idx)
        ctx.mark_non_differentiable(idx)
        return d, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, gd, _gi):
        a, b, idx = ctx.saved_tensors
        gd = gd.contiguous()
        gp = gq = None
        if ctx.needs_input_grad[0]:
            gp = torch.empty_like(a)
            L.call("e2e_knn1_bwd", L.ptr(gd), L.ptr(a), L.ptr(b), L.ptr(idx), a.shape[0], L.ptr(gp), L.stream())
        if ctx.needs_input_grad[1]:          # the reference cloud is differentiable (ChamferDistance's reverse term): reproducible scatter
            gq = torch.empty_like(b)
            fx = torch.empty(3 * b.shape[0] + 1, device=b.device, dtype=torch.int64)
            L.call("e2e_knn1_bwd_ref", L.ptr(gd), L.ptr(a), L.ptr(b), L.ptr(idx), a.shape[0], b.shape[0], L.ptr(fx), L.ptr(gq), L.stream())
        return gp, gq, None


class KnnIndex:
    """Uniform-grid index over a fixed reference cloud: built once, queried many times with results identical to
    knn1(p1, ref).  The reference tensor must not change while the index is in use (FusionMap drops its index whenever
    the map is updated)."""

    def __init__(self, ref, max_queries):
        ref = L.dev(ref, "ref")
        if ref.dim() != 2 or ref.shape[1] != 3 or ref.shape[0] == 0 or ref.requires_grad:
            raise ValueError("KnnIndex: reference cloud must be a detached, non-empty (P,3) tensor")
        self.ref = ref.contiguous()
        self.n2, self.max_queries = self.ref.shape[0], int(max_queries)
        self.ws = torch.empty(L.load().e2e_knn1_workspace_bytes(self.max_queries, self.n2), device=ref.device, dtype=torch.uint8)
        L.call("e2e_knn1_index_build", L.ptr(self.ref), self.n2, self.max_queries, L.ptr(self.ws), L.stream())

    resident = False

    def query(self, p1, n1, dists, idx, stream, row_len=0, warm=None):
        L.call("e2e_knn1_index_query", L.ptr(p1), int(n1), self.n2, self.max_queries, L.ptr(self.ws), L.ptr(dists), L.ptr(idx), stream)


class _Knn1Indexed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, index):
        a = L.dev(p1, "p1").contiguous()
        n1 = a.shape[0]
        d = torch.empty(n1, device=a.device, dtype=torch.float32)
        idx = torch.empty(n1, device=a.device, dtype=torch.int64)
        index.query(a, n1, d, idx, L.stream())
        ctx.save_for_backward(a, index.ref, idx)
        ctx.mark_non_differentiable(idx)
        return d, idx

    @staticmethod
    @once_differentiable
    def backward(ctx, gd, _gi):
        a, b, idx = ctx.saved_tensors
        gp = torch.empty_like(a)
        L.call("e2e_knn1_bwd", L.ptr(gd.contiguous()), L.ptr(a), L.ptr(b), L.ptr(idx), a.shape[0], L.ptr(gp), L.stream())
        return gp, None


def knn1(p1, p2, algorithm="auto"):
    """p2 may be a KnnIndex (prebuilt grid over the reference cloud).  algorithm: "auto" | "brute" | "grid" (identical results).  K=1 nearest neighbour of every row of p1 (P1,3) among p2 (P2,3): (squared dists (P1,), idx (P1,) int64).
    Differentiable wrt p1 (d/dp1 = 2 g (p1 - p2[idx])) and -- plain tensors only, not a prebuilt index -- wrt p2 (the scatter of the
    negative, as chamferdist's knn_points; the online path detaches p2, online_adaption.py:643)."""
    if isinstance(p2, KnnIndex) or getattr(p2, "resident", False):       # a prebuilt index (e2ehip.fusionmap.ResidentKnnIndex over the map)
        if p1.dim() != 2 or p1.shape[1] != 3 or p1.shape[0] == 0:
            raise ValueError(f"p1: expected non-empty (P,3), got {tuple(p1.shape)}")
        if p1.shape[0] > p2.max_queries:
            raise ValueError(f"knn1: {p1.shape[0]} queries exceed the {p2.max_queries} the index was built for")
        return _Knn1Indexed.apply(p1, p2)
    for n, t in (("p1", p1), ("p2", p2)):
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{n}: expected (P,3), got {tuple(t.shape)}")
    if p1.shape[0] == 0 or p2.shape[0] == 0:
        raise ValueError("knn1: empty point cloud")
    return _Knn1.apply(p1, p2, KNN_ALGORITHMS[algorithm])


# ---------------------------------------------------------------------------------------------
# median scaling chain, regulariser, metrics
# ---------------------------------------------------------------------------------------------
def median_lower(x):
    """torch.median(x) over all elements (lower median) -> 0-dim device tensor."""
    x = L.dev(x, "x").contiguous()
    out = torch.empty((), device=x.device, dtype=torch.float32)
    ws = torch.empty(L.load().e2e_median_workspace_bytes(), device=x.device, dtype=torch.uint8)
    L.call("e2e_median_lower", L.ptr(x), x.numel(), L.ptr(out), L.ptr(ws), L.stream())
    return out


class _DepthScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, median_gt, elements):
        d = L.dev(disp, "disp").contiguous()
        mg = L.dev(median_gt, "median_gt").reshape(1).contiguous()
        ctx.elements = elements
        n = d.numel()
        delta, depth = torch.empty_like(d), torch.empty_like(d)
        md = torch.empty(1, device=d.device, dtype=torch.float32)
        ratio = torch.empty(1, device=d.device, dtype=torch.float32)
        ws = torch.empty(L.load().e2e_depth_scale_workspace_bytes(), device=d.device, dtype=torch.uint8)
        L.call("e2e_depth_scale_fwd", L.ptr(d), L.ptr(mg), L.ptr(delta), L.ptr(depth), L.ptr(md), L.ptr(ratio), L.ptr(ws), n, L.stream())
        ctx.save_for_backward(delta, mg, md, ws)
        ratio = ratio.reshape(())
        ctx.mark_non_differentiable(delta, ratio)
        return depth, delta, ratio

    @staticmethod
    @once_differentiable
    def backward(ctx, g_depth, _gd, _gr):
        delta, mg, md, ws = ctx.saved_tensors
        g = g_depth.contiguous()
        g_disp = torch.empty_like(delta)
        el = ctx.elements
        L.call("e2e_depth_scale_bwd_at", L.ptr(g), L.ptr(delta), L.ptr(mg), L.ptr(md), L.ptr(el), 0 if el is None else int(el.numel()), L.ptr(g_disp),
               L.ptr(ws), delta.numel(), L.stream())
        return g_disp, None, None


def depth_from_disp_median_scaled(disp, median_gt, median_elements=None):
    """disp (F,1,H,W) of the keyframe pair -> (depth = (median_gt / median(1/disp)) / disp, unscaled 1/disp, ratio).
    The ratio stays inside the autograd graph exactly as in online_adaption.py:292-298 (the in-place `*= ratio`): its gradient is shared
    by the elements that hold the median value, as torch.median(x) differentiates.  median_elements (device int32 indices): name those
    elements instead (parity tests: the choice among near-tied values belongs to the evaluation, e2e_depth_scale_bwd_at)."""
    if median_elements is not None and (median_elements.dtype != torch.int32 or not median_elements.is_cuda):
        raise TypeError("median_elements: a device int32 tensor of flat indices")
    return _DepthScale.apply(disp, median_gt, median_elements)


class _FixedScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, scale):
        d = L.dev(disp, "disp").contiguous()
        depth = torch.empty_like(d)
        L.call("e2e_depth_fixed_scale_fwd", L.ptr(d), float(scale), None, L.ptr(depth), d.numel(), L.stream())
        ctx.save_for_backward(d)
        ctx.scale = float(scale)
        return depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        gd = torch.empty_like(d)
        L.call("e2e_depth_fixed_scale_bwd", L.ptr(g.contiguous()), L.ptr(d), ctx.scale, L.ptr(gd), d.numel(), L.stream())
        return gd, None


def depth_from_disp_fixed_scale(disp, scale=1.0):
    """depth = (1 / disp) * scale (train_depth.py:331, :343-345: the development harness scales by the constant
    ABLATION.scaling_depth instead of the median ratio); scale 1.0 is the plain `1 / disp`."""
    return _FixedScale.apply(disp, scale)


class _RangeDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, min_depth, max_depth, scale):
        d = L.dev(disp, "disp").contiguous()
        depth = torch.empty_like(d)
        ctx.cfg = (float(min_depth), float(max_depth), float(scale))
        L.call("e2e_disp_range_depth_fwd", L.ptr(d), *ctx.cfg, L.ptr(depth), d.numel(), L.stream())
        ctx.save_for_backward(d)
        return depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        gd = torch.empty_like(d)
        L.call("e2e_disp_range_depth_bwd", L.ptr(g.contiguous()), L.ptr(d), *ctx.cfg, L.ptr(gd), d.numel(), L.stream())
        return gd, None, None, None


def depth_from_disp_range(disp, min_depth, max_depth, scale=1.0):
    """depth = scale / (1 / max_depth + (1 / min_depth - 1 / max_depth) * disp): convert_disp_to_depth of the monodepth2 branch
    (training_utils.py:106-118, train_depth.py:297-299) on a sigmoid disparity in [0, 1], times the constant depth scale of
    train_depth.py:302-312 (scale 1.0: the plain conversion); one kernel each way."""
    return _RangeDepth.apply(disp, min_depth, max_depth, scale)


PYRAMID_SCALES = 4                    # disp0 .. disp3 of e2e_disp_pyramid_depth_fwd / _bwd


def _pyramid_args(ds):
    """disp0 .. disp3 and h0, w0 .. h3, w3 of the pyramid entry points: the given scales in the first slots, the rest absent"""
    pad = PYRAMID_SCALES - len(ds)
    sizes = [n for d in ds for n in d.shape[2:]] + [0] * (2 * pad)
    return [L.ptr(d) for d in ds] + [None] * pad + sizes


class _DispPyramidDepth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, size, min_depth, max_depth, scale, *disps):
        ds = [L.dev(d, "disp").contiguous() for d in disps]
        B, (H, W) = ds[0].shape[0], size
        ctx.cfg = (B, H, W, float(min_depth), float(max_depth), float(scale))
        depth = torch.empty(len(ds), B, 1, H, W, device=ds[0].device, dtype=torch.float32)
        L.call("e2e_disp_pyramid_depth_fwd", *_pyramid_args(ds), *ctx.cfg, L.ptr(depth), L.stream())
        ctx.save_for_backward(*ds)
        return depth

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ds = ctx.saved_tensors
        gds = [torch.empty_like(d) for d in ds]
        L.call("e2e_disp_pyramid_depth_bwd", L.ptr(g.contiguous()), *_pyramid_args(ds), *ctx.cfg,
               *([L.ptr(t) for t in gds] + [None] * (PYRAMID_SCALES - len(gds))), L.stream())
        return (None,) * 4 + tuple(gds)


def disp_pyramid_depth(disps, size, min_depth, max_depth, scale=1.0):
    """The monodepth2 disparity pyramid at full resolution: every (B,1,h_s,w_s) disparity of `disps` (1 to 4 scales, finest first)
    upsampled bilinearly to size = (H, W) as F.interpolate(align_corners=False) does and converted to depth as depth_from_disp_range
    does -> (S,B,1,H,W).  One launch forward (e2e_disp_pyramid_depth_fwd), one backward (e2e_disp_pyramid_depth_bwd: a gather, no
    atomics), a gradient to every disparity; a scale that already has the full size comes out bit-equal to depth_from_disp_range."""
    disps = list(disps)
    if not 1 <= len(disps) <= PYRAMID_SCALES:
        raise ValueError(f"disps: expected 1 to {PYRAMID_SCALES} scales, got {len(disps)}")
    H, W = (int(n) for n in size)
    for s, d in enumerate(disps):
        if not torch.is_tensor(d) or d.dim() != 4 or d.shape[1] != 1:
            raise ValueError(f"disps[{s}]: expected (B,1,h,w), got {tuple(d.shape) if torch.is_tensor(d) else type(d).__name__}")
        if d.shape[0] != disps[0].shape[0]:
            raise ValueError(f"disps[{s}]: expected ({disps[0].shape[0]},1,h,w), got {tuple(d.shape)}")
        if not (1 <= d.shape[2] <= H and 1 <= d.shape[3] <= W):
            raise ValueError(f"disps[{s}]: {d.shape[2]} x {d.shape[3]} does not fit the full size {H} x {W} (the pyramid only upsamples)")
    if not 0 < float(min_depth) < float(max_depth):
        raise ValueError(f"expected 0 < min_depth < max_depth, got {min_depth} and {max_depth}")
    return _DispPyramidDepth.apply((H, W), min_depth, max_depth, scale, *disps)


class MissingDispSrcs(ValueError, TypeError):
    """warp_photometric_multiscale(geometric=True) without disp_srcs: an argument the call requires is absent, which Python reports as a
    TypeError, and an unusable value of the keyword pair, which this package reports as a ValueError; callers may catch either"""


def warp_photometric_multiscale(disps, srcs, tgt, K, inv_K, Ts, min_depth, max_depth, scale=1.0, padding_mode="border", use_mask=True,
                                min_reprojection=False, auto_masking=False, tie_noise=None, geometric=False, disp_srcs=None,
                                geo_min_valid=10000):
    """monodepth2's multi-scale image-space loss: every scale's disparity is brought to the size of the frames and converted to depth
    (disp_pyramid_depth), the S scales are stacked along the batch, and ONE fused pair warps and compares them all at full resolution:
    warp_photometric for one source and no flags, warp_photometric_window otherwise.  The pair's mean over the stacked batch is
    sum_s loss_s / S.

    disps: 1 to 4 (B,1,h_s,w_s) disparities; srcs: 1 or 2 (B,3,H,W) views and tgt likewise; K, inv_K (B,4,4); Ts: one (B,4,4) pose per
    source; tie_noise (B,len(srcs),H,W) or None, the same draw for every scale.  With B = 1 the frames are read in place by every scale
    (a batch stride of 0); with a larger batch they are copied once per scale, as the kernels address the batch by one stride.
    Returns dict(photometric, photometric_per_scale (S,) detached, depth (S,B,1,H,W)).  Differentiated: every disparity and every T
    (stacked S times, so a pose with a graph gets the sum over the scales through e2e_warp_photo_bwd_pose / the window's backward).

    geometric=True adds the geometric-consistency term PER SCALE, as monodepth2's loss loop would take LOSS.geometric: disp_srcs holds one
    list of disparities per source frame, each with the scales and shapes of `disps`; every source's pyramid goes through
    disp_pyramid_depth exactly as the target's does, and ONE pair, e2e_warp_photo_geo_groups_fwd / _bwd with groups = len(disps), warps
    every scale and reduces and gates the term per scale (n_{s,g} > geo_min_valid; the reference's 10000).  As under
    warp_photometric_window(geometric=True) the source images are then sampled with align_corners=True.  The pyramids are one
    disp_pyramid_depth call each rather than one call over target and sources stacked along the batch: each call's (G,B,1,H,W) result
    IS the contiguous stacked batch the pair reads, whereas one stacked call would hand the pair strided slices and cost a copy of
    every full-resolution depth (and of its gradient) per step, more than the len(srcs) small launches each way it saves.  The dict gains
    geometric (len(srcs),) = mean_g G_{s,g}, differentiable; geometric_per_scale (G, len(srcs)), detached; geo_count (G, len(srcs)) int32.
    Differentiated then: every target disparity, every source disparity and every T, through one autograd node for the pair.  K or inv_K
    requiring grad raises NotImplementedError (the grouped pair has no intrinsics form)."""
    srcs, Ts = list(srcs), list(Ts)
    B, _, H, W = tgt.shape if torch.is_tensor(tgt) and tgt.dim() == 4 else (0, 0, 0, 0)
    if B == 0 or tgt.shape[1] != 3:
        raise ValueError(f"target_frame: expected (B,3,H,W), got {tuple(tgt.shape) if torch.is_tensor(tgt) else type(tgt).__name__}")
    if len(srcs) not in (1, 2) or len(Ts) != len(srcs):
        raise ValueError(f"warp_photometric_multiscale: expected 1 or 2 source frames and as many poses, got {len(srcs)} and {len(Ts)}")
    if geometric:
        if disp_srcs is None:
            raise MissingDispSrcs("warp_photometric_multiscale: geometric=True needs disp_srcs, one list of disparities per source frame "
                                  "with the scales and shapes of disps")
        disps = list(disps)
        disp_srcs = [list(p) for p in disp_srcs]
        if len(disp_srcs) != len(srcs) or any(len(p) != len(disps) or any(not torch.is_tensor(d) or not torch.is_tensor(t) or d.shape != t.shape
                                                                         for d, t in zip(p, disps)) for p in disp_srcs):
            raise ValueError("warp_photometric_multiscale: geometric=True needs disp_srcs, one list of disparities per source frame with "
                             "the scales and shapes of disps")
        if int(geo_min_valid) < 0:
            raise ValueError(f"geo_min_valid: {geo_min_valid} is negative")
    depth = disp_pyramid_depth(disps, (H, W), min_depth, max_depth, scale)
    S = depth.shape[0]
    if depth.shape[1] != B:
        raise ValueError(f"disps: batch {depth.shape[1]} against frames of batch {B}")
    if B == 1:
        frames = lambda t: t.expand(S, -1, -1, -1)
    else:
        frames = lambda t: t.repeat(S, 1, 1, 1)
    mats = lambda t: t.unsqueeze(0).expand(S, -1, -1, -1).reshape(S * B, 4, 4)
    stacked = depth.view(S * B, 1, H, W)
    if geometric:
        n = len(srcs)
        fs, ft = [frames(s) for s in srcs], frames(tgt)
        _check_warp_inputs("warp_photometric_multiscale", stacked, fs, ft, K, inv_K, n_poses=n)
        if tie_noise is not None and tuple(tie_noise.shape) != (B, n, H, W):
            raise ValueError(f"tie_noise: expected ({B},{n},{H},{W}), got {tuple(tie_noise.shape)}")
        dsrc = [disp_pyramid_depth(p, (H, W), min_depth, max_depth, scale).view(S * B, 1, H, W) for p in disp_srcs]
        noise = tie_noise.repeat(S, 1, 1, 1) if tie_noise is not None else None
        terms = (TERM_AUTO_MASKING if auto_masking else 0) | (TERM_MIN_REPROJECTION if min_reprojection else 0)
        p, geo, _synth, _valid, _select, count, pmap = _WarpPhotometricWindow.apply(
            stacked, dsrc[0], dsrc[1] if n == 2 else None, fs[0], fs[1] if n == 2 else None, ft, mats(K), mats(inv_K), mats(Ts[0]),
            mats(Ts[1]) if n == 2 else None, noise, _padding(padding_mode), bool(use_mask), terms, int(geo_min_valid), True, S)
        per = geo.view(n, S)                                     # [s G + g]
        return {"photometric": p, "photometric_per_scale": pmap.view(S, -1).mean(1), "depth": depth, "geometric": per.mean(1),
                "geometric_per_scale": per.detach().t(), "geo_count": count.view(n, S).t()}
    if len(srcs) == 1 and not (min_reprojection or auto_masking):
        out = warp_photometric(stacked, frames(srcs[0]), frames(tgt), mats(K), mats(inv_K), mats(Ts[0]), padding_mode=padding_mode,
                               use_mask=use_mask, want_pmap=True)
    else:
        noise = tie_noise.repeat(S, 1, 1, 1) if tie_noise is not None else None
        out = warp_photometric_window(stacked, [frames(s) for s in srcs], frames(tgt), mats(K), mats(inv_K), [mats(T) for T in Ts],
                                      padding_mode=padding_mode, use_mask=use_mask, min_reprojection=min_reprojection,
                                      auto_masking=auto_masking, tie_noise=noise, want_pmap=True)
    return {"photometric": out["photometric"], "photometric_per_scale": out["pmap"].view(S, -1).mean(1), "depth": depth}


class _MeanDiff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, kind):
        a, b = L.dev(a, "initial_depth").contiguous(), L.dev(b, "refined_depth").contiguous()
        out = torch.empty(1, device=a.device, dtype=torch.float32)
        ws = torch.empty(L.load().e2e_reduce_workspace_floats(), device=a.device, dtype=torch.float32)
        L.call("e2e_mean_diff_fwd", L.ptr(a), L.ptr(b), a.numel(), kind, L.ptr(out), L.ptr(ws), L.stream())
        ctx.save_for_backward(a, b)
        ctx.kind = kind
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        gb = torch.empty_like(b)
        L.call("e2e_mean_diff_bwd", L.ptr(a), L.ptr(b), L.ptr(g.reshape(1).contiguous()), a.numel(), ctx.kind, L.ptr(gb), L.stream())
        return None, gb, None


def mean_diff(initial, refined, kind):
    """mean |initial - refined| ("l1") or mean (initial - refined)^2 ("l2"); gradient flows to `refined` only
    (the initial depth is a detached clone: online_adaption.py:284-285)."""
    k = {"l1": 1, "l2": 2}.get(kind)
    if k is None:
        raise ValueError("please specify a correct norm")
    if initial.shape != refined.shape:
        raise ValueError("shape mismatch")
    if initial.requires_grad:
        raise NotImplementedError("gradient wrt the initial depth is not on the reference path")
    return _MeanDiff.apply(initial, refined, k)


def depth_metrics(gt, pred, mask_zero_gt):
    """-> (7,) device tensor: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 (losses.py:162-201)."""
    gt, pred = L.dev(gt, "gt").contiguous(), L.dev(pred, "pred").contiguous()
    if gt.numel() != pred.numel():
        raise ValueError("gt and pred must have the same number of elements")
    out = torch.empty(7, device=gt.device, dtype=torch.float32)
    ws = torch.empty(L.load().e2e_reduce_workspace_floats(), device=gt.device, dtype=torch.float32)
    L.call("e2e_depth_metrics", L.ptr(gt), L.ptr(pred), gt.numel(), int(bool(mask_zero_gt)), L.ptr(out), L.ptr(ws), L.stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# off-by-default losses (csrc/aux_losses.hip): each Function computes the loss AND the gradient for a unit upstream
# gradient in its forward launch; backward only scales the stored gradient by the incoming scalar.
# ---------------------------------------------------------------------------------------------------------------------
def _aux_ws(dev):
    return torch.empty(L.load().e2e_aux_workspace_floats(), device=dev, dtype=torch.float32)


class _Smoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, disp, img):
        d = L.dev(disp, "disp").contiguous()
        im = L.dev(img, "img")
        B, C, H, W = im.shape
        if tuple(d.shape) != (B, 1, H, W):
            raise ValueError(f"disp {tuple(d.shape)} does not match img {tuple(im.shape)}")
        out = torch.empty(2, device=d.device, dtype=torch.float32)
        g = torch.empty_like(d) if ctx.needs_input_grad[0] else None
        L.call("e2e_smoothness_lossgrad", disp=L.ptr(d), img=L.ptr(im), img_strides=L.strides4(im), B=B, C=C, H=H, W=W, loss_out=L.ptr(out), g_disp=L.ptr(g),
               workspace=L.ptr(_aux_ws(d.device)), stream=L.stream())
        ctx.save_for_backward(g)
        return out[0] + out[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        (g,) = ctx.saved_tensors
        return (g * go if g is not None else None), None


def smoothness(disp, img):
    """loss/losses.py:119-132: mean_x(|dx disp| exp(-mean_c |dx img|)) + mean_y(...); gradient w.r.t. disp only."""
    return _Smoothness.apply(disp, img)


class _DispPyramidSmoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, weights, want_grad, *disps):
        ds = [L.dev(d, "disp").contiguous() for d in disps]
        im = L.dev(img, "img")
        B, _, H, W = im.shape
        pad = [None] * (PYRAMID_SCALES - len(ds))
        sizes = _pyramid_args(ds)[PYRAMID_SCALES:]
        out = torch.empty(PYRAMID_SCALES + 1, device=im.device, dtype=torch.float32)
        gds = [torch.empty_like(d) for d in ds] if want_grad else []
        ws = torch.empty(L.query("e2e_disp_pyramid_smoothness_workspace_floats", *sizes, B), device=im.device, dtype=torch.float32)
        L.call("e2e_disp_pyramid_smoothness_lossgrad", *([L.ptr(d) for d in ds] + pad), *sizes, L.ptr(im), L.strides4(im), B, H, W,
               *(list(weights) + [0.0] * len(pad)), L.ptr(out), *([L.ptr(g) for g in gds] + [None] * (PYRAMID_SCALES - len(gds))),
               L.ptr(ws), L.stream())
        ctx.save_for_backward(*gds)
        return out                                                  # loss_out[5]: the graph is used through its last element only

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        gds, needs = ctx.saved_tensors, ctx.needs_input_grad[3:]
        if not gds:
            return (None,) * (3 + len(needs))
        return (None,) * 3 + tuple(g * go[PYRAMID_SCALES] if need else None for g, need in zip(gds, needs))


def disp_pyramid_smoothness(disps, img, weights=None):
    """monodepth2's edge-aware smoothness on every scale of the disparity pyramid: for each (B,1,h_s,w_s) disparity of `disps` (1 to 4
    scales, finest first) the smoothness (loss/losses.py:119-132) of its mean-normalised form against img (B,3,H,W, any strides, a
    constant) box-averaged to that scale's resolution -- F.avg_pool2d(img, (H / h_s, W / w_s)), so h_s must divide H and w_s W, and
    both be >= 2 -- weighted by weights[s] (default 1 each) and summed.  One entry-point call (two launches whatever the number of
    scales, e2e_disp_pyramid_smoothness_lossgrad) computes the loss and, where a disparity needs one, every gradient; the backward only
    scales them.  Returns dict(smoothness = the weighted sum (0-dim, carries the graph), smoothness_per_scale (S,) detached, unweighted)."""
    disps = list(disps)
    if not 1 <= len(disps) <= PYRAMID_SCALES:
        raise ValueError(f"disps: expected 1 to {PYRAMID_SCALES} scales, got {len(disps)}")
    if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"img: expected (B,3,H,W), got {tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}")
    B, _, H, W = img.shape
    for s, d in enumerate(disps):
        if not torch.is_tensor(d) or d.dim() != 4 or d.shape[1] != 1:
            raise ValueError(f"disps[{s}]: expected (B,1,h,w), got {tuple(d.shape) if torch.is_tensor(d) else type(d).__name__}")
        if d.shape[0] != B:
            raise ValueError(f"disps[{s}]: expected ({B},1,h,w) to go with img {tuple(img.shape)}, got {tuple(d.shape)}")
        h, w = d.shape[2:]
        if not (1 <= h <= H and 1 <= w <= W):
            raise ValueError(f"disps[{s}]: {h} x {w} does not fit the image {H} x {W}")
        if h < 2 or w < 2:
            raise ValueError(f"disps[{s}]: {h} x {w}: the smoothness needs at least 2 x 2 (an axis of one pixel has no edge)")
        if H % h or W % w:
            raise ValueError(f"disps[{s}]: {h} x {w} does not divide the image {H} x {W} (the colour pyramid is a box mean over whole blocks)")
    weights = [1.0] * len(disps) if weights is None else [float(v) for v in weights]
    if len(weights) != len(disps):
        raise ValueError(f"weights: expected one per scale ({len(disps)}), got {len(weights)}")
    want_grad = torch.is_grad_enabled() and any(d.requires_grad for d in disps)
    out = _DispPyramidSmoothness.apply(img, weights, want_grad, *disps)
    return {"smoothness": out[PYRAMID_SCALES], "smoothness_per_scale": out.detach()[:len(disps)]}


class _GeomConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wd, idp, mask):
        a, b = L.dev(wd, "warped_depth").contiguous(), L.dev(idp, "interpolated_depth").contiguous()
        if a.shape != b.shape:
            raise ValueError("warped / interpolated depth shapes differ")
        m = L.dev(mask, "valid_mask").expand_as(a).to(torch.float32).contiguous()
        stats = torch.empty(3, device=a.device, dtype=torch.float32)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        ga = torch.empty_like(a) if need else None
        gb = torch.empty_like(a) if need else None
        L.call("e2e_geometric_consistency_lossgrad", L.ptr(a), L.ptr(b), L.ptr(m), a.numel(), L.ptr(stats), L.ptr(ga), L.ptr(gb),
               L.ptr(_aux_ws(a.device)), L.stream())
        ctx.save_for_backward(ga, gb)
        return stats[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        ga, gb = ctx.saved_tensors
        return (ga * go if ga is not None else None), (gb * go if gb is not None else None), None


def geometric_consistency(warped_depth, interpolated_depth, valid_mask):
    """loss/losses.py:84-95; the `mask.sum() > 10000` gate is evaluated on the device (no host sync)."""
    return _GeomConsistency.apply(warped_depth, interpolated_depth, valid_mask)


class _MaskedL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, mask):
        p = L.dev(pred, "prediction").squeeze().contiguous()
        g = L.dev(gt, "sparse_groundtruth").squeeze().to(torch.float32).contiguous()
        m = L.dev(mask, "sparse_mask").squeeze().to(torch.float32).contiguous()
        if not (p.shape == g.shape == m.shape):
            raise ValueError("prediction / ground truth / mask shapes differ after squeeze()")
        out = torch.empty(1, device=p.device, dtype=torch.float32)
        gp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        L.call("e2e_masked_l1_lossgrad", L.ptr(p), L.ptr(g), L.ptr(m), p.numel(), L.ptr(out), L.ptr(gp), L.ptr(_aux_ws(p.device)), L.stream())
        ctx.save_for_backward(gp)
        ctx.shape = pred.shape
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        (gp,) = ctx.saved_tensors
        return ((gp * go).reshape(ctx.shape) if gp is not None else None), None, None


def masked_l1(prediction, sparse_groundtruth, sparse_mask):
    """loss/losses.py:151-160 depth_gt_loss."""
    return _MaskedL1.apply(prediction, sparse_groundtruth, sparse_mask)


class _MinReprojection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, errors):
        e = L.dev(errors, "errors").contiguous()
        B, C, H, W = e.shape
        out = torch.empty(1, device=e.device, dtype=torch.float32)
        ge = torch.empty_like(e) if ctx.needs_input_grad[0] else None
        L.call("e2e_min_reprojection_lossgrad", L.ptr(e), B, C, H, W, L.ptr(out), L.ptr(ge), L.ptr(_aux_ws(e.device)), L.stream())
        ctx.save_for_backward(ge)
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        (ge,) = ctx.saved_tensors
        return ge * go if ge is not None else None


def min_reprojection(errors):
    """train_depth.py:657-661: torch.min over the stacked per-source (and identity) error maps, then the mean."""
    if errors.dim() != 4:
        raise ValueError("errors must be (B, C, H, W)")
    return _MinReprojection.apply(errors)


class _DispBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pair):
        d = L.dev(pair, "disp pair").contiguous()
        if d.dim() != 4 or d.shape[0] != 2 or d.shape[1] != 1:
            raise ValueError("process_disparity expects the (2,1,H,W) disparities of [img, flip(img)]")
        H, W = d.shape[2], d.shape[3]
        out = torch.empty(1, 1, H, W, device=d.device, dtype=torch.float32)
        L.call("e2e_disp_blend_fwd", L.ptr(d), H, W, L.ptr(out), L.stream())
        ctx.hw = (H, W)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        H, W = ctx.hw
        g = go.contiguous()
        gd = torch.empty(2, 1, H, W, device=g.device, dtype=torch.float32)
        L.call("e2e_disp_blend_bwd", L.ptr(g), H, W, L.ptr(gd), L.stream())
        return gd


def process_disparity(disp_pair):
    """train_depth.py:224-237 (dual-disparity post-processing)."""
    return _DispBlend.apply(disp_pair)


# ---------------------------------------------------------------------------------------------------------------------
# helpers of train_depth.py's operator-by-operator loss assembly
# ---------------------------------------------------------------------------------------------------------------------
class _MaskMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        x = L.dev(x, "image")
        B, C, H, W = x.shape
        m = L.dev(mask, "valid_mask").reshape(B, 1, H, W).contiguous()
        out = torch.empty(B, C, H, W, device=x.device, dtype=torch.float32)
        L.call("e2e_mask_mul", L.ptr(x), L.strides4(x), L.ptr(m), B, C, H, W, L.ptr(out), L.stream())
        ctx.save_for_backward(m)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (m,) = ctx.saved_tensors
        g = g.contiguous()
        B, C, H, W = g.shape
        gx = torch.empty_like(g)
        L.call("e2e_mask_mul", L.ptr(g), L.strides4(g), L.ptr(m), B, C, H, W, L.ptr(gx), L.stream())
        return gx, None


def mask_mul(x, mask):
    """x (B,C,H,W) * mask (B,1,H,W) -- `prediction * valid_mask` of train_depth.py:713-714; the mask carries no gradient."""
    return _MaskMul.apply(x, mask)


class _ChannelMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = L.dev(x, "maps").contiguous()
        B, C, H, W = x.shape
        out = torch.empty(B, 1, H, W, device=x.device, dtype=torch.float32)
        L.call("e2e_channel_mean", L.ptr(x), B, C, H, W, 0, L.ptr(out), L.stream())
        ctx.C = C
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        B, _, H, W = g.shape
        gx = torch.empty(B, ctx.C, H, W, device=g.device, dtype=torch.float32)
        L.call("e2e_channel_mean", L.ptr(g), B, ctx.C, H, W, 1, L.ptr(gx), L.stream())
        return gx


def channel_mean(x):
    """x.mean(1, keepdim=True) of stacked photometric maps (train_depth.py:630)."""
    if x.dim() != 4:
        raise ValueError("channel_mean expects (B,C,H,W)")
    return x if x.shape[1] == 1 else _ChannelMean.apply(x)


class _MeanNormalize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d):
        d = L.dev(d, "disp").contiguous()
        B, C, H, W = d.shape
        out = torch.empty_like(d)
        ws = torch.empty(B * C * 130, device=d.device, dtype=torch.float32)
        L.call("e2e_mean_normalize", L.ptr(d), None, B * C, H, W, L.ptr(out), L.ptr(ws), L.stream())
        ctx.save_for_backward(d)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (d,) = ctx.saved_tensors
        B, C, H, W = d.shape
        gd = torch.empty_like(d)
        ws = torch.empty(B * C * 130, device=d.device, dtype=torch.float32)
        L.call("e2e_mean_normalize", L.ptr(d), L.ptr(g.contiguous()), B * C, H, W, L.ptr(gd), L.ptr(ws), L.stream())
        return gd


def mean_normalize(disp):
    """disp / (disp.mean(2, True).mean(3, True) + 1e-7) (train_depth.py:768-770)."""
    if disp.dim() != 4:
        raise ValueError("mean_normalize expects (B,C,H,W)")
    return _MeanNormalize.apply(disp)
