"""Pre-planned (allocation-free, hipGraph-capturable) launches of the fused refinement kernels.

`WarpPhotoPlan` owns every intermediate buffer of the image-space part of one refinement step, so a
step is exactly: e2e_warp_photo_fwd (+ its 1-block reduction) and e2e_warp_photo_bwd (or
e2e_warp_photo_bwd_pose, which also returns the gradient with respect to T, or e2e_warp_photo_bwd_intrinsics,
which returns the gradients with respect to K and inv_K as well) -- no
allocator traffic, no host synchronisation.  The build's driver and bench.py use it; the autograd
form for ad-hoc use is ops.warp_photometric."""
import ctypes

import torch

from . import _lib as L
from .ops import _padding


class WarpPhotoPlan:
    def __init__(self, B, H, W, device, padding_mode="border", use_mask=True, reg_kind="l2"):
        self.B, self.H, self.W = B, H, W
        self.pad = _padding(padding_mode)
        self.use_mask = int(bool(use_mask))
        self.reg = {None: 0, "l1": 1, "l2": 2}[reg_kind]
        f = dict(device=device, dtype=torch.float32)
        self.synth = torch.empty(B, 3, H, W, **f)
        self.valid = torch.empty(B, 1, H, W, **f)
        self.loss = torch.zeros(2, **f)            # [photometric mean, regulariser sum of means]
        self.g_loss = torch.ones(2, **f)           # upstream gradients of the two scalars
        self.g_depth_tgt = torch.empty(B, 1, H, W, **f)
        self.g_depth_src = torch.empty(B, 1, H, W, **f)
        self.ws = torch.empty(L.load().e2e_warp_photo_workspace_floats(B, H, W), **f)
        self.g_T = self.ws_pose = None             # backward(pose=True): the gradient wrt T and its float64 partial sums
        self.g_K = self.g_inv_K = self.ws_intrinsics = None        # backward(intrinsics=True): the gradients wrt K, inv_K and their sums

    def bind(self, depth_tgt, depth_src, init_tgt, init_src, src, tgt, K, inv_K, T):
        """Fix the input tensors (they may be rewritten in place between steps)."""
        B, H, W = self.B, self.H, self.W
        for n, t, shp in (("depth_tgt", depth_tgt, (B, 1, H, W)), ("src", src, (B, 3, H, W)), ("tgt", tgt, (B, 3, H, W)),
                          ("K", K, (B, 4, 4)), ("inv_K", inv_K, (B, 4, 4)), ("T", T, (B, 4, 4))):
            L.dev(t, n)
            if tuple(t.shape) != shp:
                raise ValueError(f"{n}: expected {shp}, got {tuple(t.shape)}")
        if self.reg:
            for n, t in (("depth_src", depth_src), ("init_tgt", init_tgt), ("init_src", init_src)):
                L.dev(t, n)
                if tuple(t.shape) != (B, 1, H, W) or not t.is_contiguous():
                    raise ValueError(f"{n}: expected contiguous {(B, 1, H, W)}")
        if not (depth_tgt.is_contiguous() and K.is_contiguous() and inv_K.is_contiguous() and T.is_contiguous()):
            raise ValueError("depth_tgt / K / inv_K / T must be contiguous")
        self.t = (depth_tgt, depth_src, init_tgt, init_src, src, tgt, K, inv_K, T)
        return self

    def _operands(self):
        """What every launch form of the step shares, under the parameter names of include/e2eslam.h: the bound tensors, the flags, the
        sizes and the stream.  Each call passes it as `geom` (L.bind takes what the prototype declares) and names only what differs."""
        dt, ds, it, is_, src, tgt, K, iK, T = self.t
        reg = self.reg
        return dict(depth_tgt=L.ptr(dt), src=L.ptr(src), src_strides=L.strides4(src), tgt=L.ptr(tgt), tgt_strides=L.strides4(tgt), K=L.ptr(K),
                    inv_K=L.ptr(iK), T=L.ptr(T), use_mask=self.use_mask, padding_mode=self.pad, reg_kind=reg, reg_init_tgt=L.ptr(it) if reg else None,
                    reg_init_src=L.ptr(is_) if reg else None, depth_src=L.ptr(ds) if reg else None, B=self.B, H=self.H, W=self.W, stream=L.stream())

    def forward(self, pmap=None):
        L.call("e2e_warp_photo_fwd", geom=self._operands(), synth=L.ptr(self.synth), valid=L.ptr(self.valid), pmap=L.ptr(pmap), loss_out=L.ptr(self.loss),
               workspace=L.ptr(self.ws))
        return self.loss

    def _pose_buffers(self):
        if self.g_T is None:
            dev = self.synth.device
            self.g_T = torch.empty(self.B, 4, 4, device=dev, dtype=torch.float32)
            self.ws_pose = torch.empty(L.load().e2e_warp_photo_bwd_pose_workspace_bytes(self.B, self.H, self.W), device=dev, dtype=torch.uint8)

    def _intrinsics_buffers(self):
        if self.g_K is None:
            dev = self.synth.device
            self.g_K, self.g_inv_K = (torch.empty(self.B, 4, 4, device=dev, dtype=torch.float32) for _ in range(2))
            self.ws_intrinsics = torch.empty(L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", self.B, self.H, self.W), device=dev, dtype=torch.uint8)

    def backward(self, pose=False, intrinsics=False):
        """-> (g_depth_tgt, g_depth_src); with pose=True (e2e_warp_photo_bwd_pose) -> (g_depth_tgt, g_depth_src, g_T), g_T (B,4,4) the
        gradient of g_loss[0] * photometric with respect to the bound T.  With intrinsics=True (e2e_warp_photo_bwd_intrinsics) the tuple
        ends with g_K, g_inv_K (B,4,4), the gradients with respect to the bound K and inv_K: (g_depth_tgt, g_depth_src[, g_T], g_K,
        g_inv_K).  Each output and its workspace are allocated once, by the first call that asks for it -- make that call before
        capturing a graph."""
        outputs = dict(synth=L.ptr(self.synth), valid=L.ptr(self.valid), g_loss=L.ptr(self.g_loss), g_depth_tgt=L.ptr(self.g_depth_tgt),
                       g_depth_src=L.ptr(self.g_depth_src) if self.reg else None)
        if intrinsics:
            self._intrinsics_buffers()
            if pose:
                self._pose_buffers()
            L.call("e2e_warp_photo_bwd_intrinsics", geom=self._operands(), g_T=L.ptr(self.g_T) if pose else None, g_K=L.ptr(self.g_K),
                   g_inv_K=L.ptr(self.g_inv_K), workspace=L.ptr(self.ws_intrinsics), **outputs)
            return (self.g_depth_tgt, self.g_depth_src) + ((self.g_T,) if pose else ()) + (self.g_K, self.g_inv_K)
        if not pose:
            L.call("e2e_warp_photo_bwd", geom=self._operands(), **outputs)
            return self.g_depth_tgt, self.g_depth_src
        self._pose_buffers()
        L.call("e2e_warp_photo_bwd_pose", geom=self._operands(), g_T=L.ptr(self.g_T), workspace=L.ptr(self.ws_pose), **outputs)
        return self.g_depth_tgt, self.g_depth_src, self.g_T


class LossGradPlan(WarpPhotoPlan):
    """One launch per step: e2e_warp_photo_lossgrad (loss and d/d depth together)."""

    def __init__(self, B, H, W, device, padding_mode="border", use_mask=True, reg_kind="l2", w_photo=1.0, w_reg=1e-2):
        super().__init__(B, H, W, device, padding_mode, use_mask, reg_kind)
        self.w_photo, self.w_reg = float(w_photo), float(w_reg)
        # zero-initialised ONCE: the tail of the workspace is the arrival ticket, which the kernel re-arms itself
        self.ws = torch.zeros(L.load().e2e_warp_photo_lossgrad_workspace_floats(B, H, W), device=device, dtype=torch.float32)

    def set_host_geometry(self, K, inv_K, T):
        """Give the pair's geometry as HOST (CPU) 4x4 tensors: the 12 numbers of c = d * M [x,y,1] + p4 then travel as
        kernel arguments (B = 1).  Call again whenever the pair changes; None switches back to the device matrices."""
        if K is None:
            self._geo = None
            return self
        if self.B != 1:
            raise ValueError("host geometry is per keyframe pair (B = 1)")
        K, inv_K, T = (t.detach().double().cpu().reshape(4, 4) for t in (K, inv_K, T))
        P = (K @ T)[:3]
        M = P[:, :3] @ inv_K[:3, :3]
        self._geo = (ctypes.c_float * 12)(*[float(v) for v in M.reshape(-1)], *[float(v) for v in P[:, 3]])
        return self

    def step_chain(self, set_cur, set_prev=-1, loss_prev=None):
        """One kernel for the whole step: the loss sums go to slot set `set_cur` (0..7) and the previous chained launch's
        set `set_prev` is finalised into `loss_prev` (a 2-float tensor).  Finish the last step with flush_chain().
        -> (g_depth_tgt, g_depth_src)."""
        geo = getattr(self, "_geo", None)
        matrices = dict(geometry12_host=None) if geo is None else dict(K=None, inv_K=None, T=None, geometry12_host=ctypes.cast(geo, ctypes.c_void_p))
        L.call("e2e_warp_photo_lossgrad_chain", geom=self._operands(), w_photo=self.w_photo, w_reg=self.w_reg, set_cur=int(set_cur), set_prev=int(set_prev),
               loss_prev_out=L.ptr(loss_prev) if set_prev >= 0 else None, g_depth_tgt=L.ptr(self.g_depth_tgt),
               g_depth_src=L.ptr(self.g_depth_src) if self.reg else None, workspace=L.ptr(self.ws), **matrices)
        return self.g_depth_tgt, self.g_depth_src

    def flush_chain(self, set_last, loss_out):
        L.call("e2e_warp_photo_lossgrad_chain_flush", L.ptr(self.ws), int(set_last), self.reg, L.ptr(loss_out), self.B, self.H, self.W, L.stream())
        return loss_out

    def step(self, want_loss=True):
        """-> (loss[2], g_depth_tgt, g_depth_src); gradients are of w_photo*loss[0] + w_reg*loss[1].
        want_loss=False launches the main kernel only (no second-stage reduction of the loss)."""
        outputs = dict(w_photo=self.w_photo, w_reg=self.w_reg, loss_out=L.ptr(self.loss) if want_loss else None, g_depth_tgt=L.ptr(self.g_depth_tgt),
                       g_depth_src=L.ptr(self.g_depth_src) if self.reg else None, workspace=L.ptr(self.ws))
        if getattr(self, "_geo", None) is not None:
            L.call("e2e_warp_photo_lossgrad_hostgeo", geom=self._operands(), geometry12_host=ctypes.cast(self._geo, ctypes.c_void_p), **outputs)
        else:
            L.call("e2e_warp_photo_lossgrad", geom=self._operands(), **outputs)
        return self.loss, self.g_depth_tgt, self.g_depth_src


TERM_GEOMETRIC, TERM_AUTO_MASKING, TERM_MIN_REPROJECTION = 1, 2, 4          # E2E_TERM_* (include/e2eslam.h)


class TermsLossGradPlan(LossGradPlan):
    """LossGradPlan with the loss terms the recommended configuration leaves off (LOSS.geometric, auto_masking, min_reprojection,
    smoothness): e2e_warp_photo_terms_lossgrad (+ e2e_smoothness_norm_lossgrad) when a flag is set, e2e_warp_photo_lossgrad -- the
    parent's very launch -- when none is.  Every launch argument is constant, so a step captures into a graph like the default one.

    loss5 = [photometric mean after the per-pixel minimum, regulariser, geometric term, smoothness term, #valid projections]
    (all unweighted); .loss stays the two-value (photometric, regulariser) row of the parent, a view of loss5."""

    def __init__(self, B, H, W, device, padding_mode="border", use_mask=True, reg_kind="l2", w_photo=1.0, w_reg=1e-2,
                 geometric=False, smoothness=False, auto_masking=False, min_reprojection=False, w_geometric=0.5, w_smoothness=1e-3):
        super().__init__(B, H, W, device, padding_mode, use_mask, reg_kind, w_photo, w_reg)
        self.geometric, self.smoothness = bool(geometric), bool(smoothness)
        self.terms = (TERM_GEOMETRIC if geometric else 0) | (TERM_AUTO_MASKING if auto_masking else 0) | (TERM_MIN_REPROJECTION if min_reprojection else 0)
        self.flagged = bool(self.terms) or self.smoothness
        self.w_geometric = float(w_geometric) if geometric else 0.0
        self.w_smoothness = float(w_smoothness) if smoothness else 0.0
        if not self.flagged:
            return
        if B != 1:
            raise ValueError("the flagged loss terms are planned per keyframe pair (B = 1)")
        f = dict(device=device, dtype=torch.float32)
        lib = L.load()
        self.loss5 = torch.zeros(5, **f)
        self.loss = self.loss5[0:2]
        # "Break tie's" (online_adaption.py:498): the plane exists only where the reference adds it; refreshed by the caller per step
        self.noise = torch.zeros(1, 1, H, W, **f) if (auto_masking and min_reprojection) else None
        self.ws_terms = torch.empty(lib.e2e_warp_photo_terms_lossgrad_workspace_floats(B, H, W), **f)
        self.ws_smooth = torch.empty(lib.e2e_smoothness_norm_lossgrad_workspace_floats(H, W), **f) if self.smoothness else None

    @property
    def writes_g_depth_src(self):
        return bool(self.reg) or self.geometric

    def bind(self, depth_tgt, depth_src, init_tgt, init_src, src, tgt, K, inv_K, T):
        super().bind(depth_tgt, depth_src, init_tgt, init_src, src, tgt, K, inv_K, T)
        if self.geometric:
            L.dev(depth_src, "depth_src")
            if tuple(depth_src.shape) != (self.B, 1, self.H, self.W) or not depth_src.is_contiguous():
                raise ValueError(f"depth_src: expected contiguous {(self.B, 1, self.H, self.W)}")
        return self

    def step(self, want_loss=True):
        """-> (loss[2], g_depth_tgt, g_depth_src); gradients are of w_photo*loss5[0] + w_reg*loss5[1] + w_geometric*loss5[2].
        The smoothness term is a function of the DISPARITY: see smoothness_step."""
        if not self.flagged:
            return super().step(want_loss)
        need_src = self.writes_g_depth_src
        L.call("e2e_warp_photo_terms_lossgrad", geom=self._operands(), depth_src=L.ptr(self.t[1]) if need_src else None, terms=self.terms,
               tie_noise=L.ptr(self.noise), w_photo=self.w_photo, w_reg=self.w_reg, w_geometric=self.w_geometric, loss_out=L.ptr(self.loss5),
               g_depth_tgt=L.ptr(self.g_depth_tgt), g_depth_src=L.ptr(self.g_depth_src) if need_src else None, workspace=L.ptr(self.ws_terms))
        return self.loss, self.g_depth_tgt, self.g_depth_src

    def smoothness_step(self, disp_src, g_disp_src):
        """loss5[3] = smoothness of disp_src / (mean + 1e-7) against the edges of the TARGET frame (online_adaption.py:600-610, sic);
        g_disp_src (H*W floats, already holding the other terms' gradient) += w_smoothness * its gradient."""
        if not self.smoothness:
            return
        tgt = self.t[5]
        L.call("e2e_smoothness_norm_lossgrad", L.ptr(disp_src), L.ptr(tgt), L.strides4(tgt), self.w_smoothness, L.ptr(self.loss5[3:4]),
               L.ptr(g_disp_src), L.ptr(self.ws_smooth), self.H, self.W, L.stream())

    def weighted_extra(self):
        """w_geometric * geometric + w_smoothness * smoothness as a device scalar (0 when no flag is set): what the driver's `loss`
        column adds to photometric + regulariser [+ 3-D]."""
        if not self.flagged:
            return torch.zeros((), device=self.ws.device)
        return self.w_geometric * self.loss5[2] + self.w_smoothness * self.loss5[3]
