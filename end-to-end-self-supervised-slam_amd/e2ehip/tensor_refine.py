"""Drivers D4/D6 of the reference reduced to their optimisation cores, on the fused kernels:

* `refine_depth_tensor` -- "OFT", train_depth_OFT.py:279-282: the depth map itself is the parameter
  (`define_optim(args, [inputs[("depth", 1, 0)]])`), refined with the same warp + photometric (+ regulariser) loss.
* `learn_depth_scale`   -- absolute_scale.py:207-240: a `ScaleLayer` (one scalar) or `Conv1x1(1, 1, bias=True)` (scale +
  offset) on top of a fixed depth prediction, trained through the same loss.

* `learn_intrinsics`    -- self-calibration: four factors on fx, fy, cx, cy of K, trained through the same loss with depth and pose fixed
  (the reference's scale_by_f / normalize_intrinsics / utils/pretrained_focal.py exist because the focal length may not match the data).

The first two run one `e2e_warp_photo_lossgrad` launch + one fused Adam launch per step; nothing else touches the GPU.  The third runs
the fused forward / backward pair with the gradient with respect to the intrinsics, torch's autograd on the 4x4 matrices, and fused Adam."""
import torch

from . import _lib as L
from . import ops
from .fused import LossGradPlan
from .optim import FusedAdam


def _plan(depth, depth_src, init_tgt, init_src, src, tgt, K, T, padding_mode, use_mask, reg_kind, w_reg):
    B, _, H, W = depth.shape
    plan = LossGradPlan(B, H, W, depth.device, padding_mode, use_mask, reg_kind, 1.0, w_reg)
    plan.bind(depth, depth_src, init_tgt, init_src, src, tgt, K.contiguous(), torch.linalg.pinv(K).contiguous(), T.contiguous())
    return plan


def refine_depth_tensor(depth_tgt, src, tgt, K, T, steps=3, lr=1e-3, padding_mode="border", use_mask=True,
                        depth_src=None, reg_kind=None, w_reg=1e-2):
    """depth_tgt (B,1,H,W) is refined IN A COPY by Adam on the photometric loss of warping `src` (B,3,H,W view) into the
    target view with depth_tgt, K (B,4,4), T (B,4,4).  With reg_kind "l1"/"l2" and depth_src, the regulariser of
    online_adaption.py:612-623 pulls both maps to their initial values.  Returns (refined depth, [loss per step])."""
    d = L.dev(depth_tgt, "depth_tgt").detach().clone().contiguous()
    p = torch.nn.Parameter(d)
    if reg_kind is not None and depth_src is None:
        raise ValueError("the depth regulariser needs depth_src")
    ds = L.dev(depth_src, "depth_src").detach().clone().contiguous() if reg_kind else None
    it, is_ = (d.clone(), ds.clone()) if reg_kind else (None, None)
    opt = FusedAdam([p], lr=lr)
    trace = []
    plan = None
    for _ in range(steps):
        if plan is None or plan.t[0].data_ptr() != p.data.data_ptr():   # FusedAdam re-homes the parameter at its first step
            plan = _plan(p.data, ds, it, is_, src, tgt, K, T, padding_mode, use_mask, reg_kind, w_reg)
        loss, g_tgt, _ = plan.step()
        trace.append(loss.clone())
        opt.zero_grad()
        if p.grad is None:
            p.grad = g_tgt.clone()
        else:
            p.grad.copy_(g_tgt)
        opt.step()
    return p.data.clone(), [float(v[0]) for v in torch.stack(trace).cpu()]


class ScaleLayer(torch.nn.Module):
    """depth_estimation/networks.py:207-215."""

    def __init__(self, init_value=0.5):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor([init_value]))

    def forward(self, x):
        return x * self.scale


def learn_depth_scale(depth_pred, src, tgt, K, T, steps=50, lr=1e-2, init_value=0.5, affine=False, padding_mode="border", use_mask=True,
                      init_bias=0.0):
    """Learn depth = w * depth_pred (+ b) through the photometric loss (absolute_scale.py:207-240; `affine` = the
    Conv1x1(1, 1, bias=True) variant, whose bias torch initialises at random: pass it as init_bias).  The depth network is frozen
    (its parameters are not in train_params, :223-224), so its prediction is an input.  Returns (w, b, [loss per step]).
    d loss / d w = <g, depth_pred>, d loss / d b = sum(g) with g = the fused kernel's d loss / d depth."""
    base = L.dev(depth_pred, "depth_pred").detach().contiguous()
    w = torch.nn.Parameter(torch.full((1,), float(init_value), device=base.device))
    b = torch.nn.Parameter(torch.full((1,), float(init_bias), device=base.device))
    params = [w, b] if affine else [w]
    opt = FusedAdam(params, lr=lr)
    cur = torch.empty_like(base)
    plan = _plan(cur, None, None, None, src, tgt, K, T, padding_mode, use_mask, None, 0.0)
    trace = []
    for _ in range(steps):
        torch.add(b.data if affine else torch.zeros_like(b.data), base * w.data, out=cur)
        loss, g, _ = plan.step()
        trace.append(loss.clone())
        opt.zero_grad()
        gw, gb = (g * base).sum().reshape(1), g.sum().reshape(1)
        for prm, gr in ((w, gw), (b, gb)) if affine else ((w, gw),):
            if prm.grad is None:
                prm.grad = gr.clone()
            else:
                prm.grad.copy_(gr)
        opt.step()
    return float(w.data), float(b.data), [float(v[0]) for v in torch.stack(trace).cpu()]


def intrinsics_from_factors(K, factors):
    """K (B,4,4), a zero-skew pinhole matrix; factors (4,) on fx, fy, cx, cy -> (K_eff, inv_K_eff), both (B,4,4): the scaled matrix and its
    closed-form inverse, built with torch on the 4x4 so that autograd carries d/d factors (any device)."""
    fx, fy, cx, cy = factors[0] * K[:, 0, 0], factors[1] * K[:, 1, 1], factors[2] * K[:, 0, 2], factors[3] * K[:, 1, 2]
    z, o = torch.zeros_like(fx), torch.ones_like(fx)
    K_eff = torch.stack([fx, z, cx, z, z, fy, cy, z, z, z, o, z, z, z, z, o], -1).view(-1, 4, 4)
    inv = torch.stack([1 / fx, z, -cx / fx, z, z, 1 / fy, -cy / fy, z, z, z, o, z, z, z, z, o], -1).view(-1, 4, 4)
    return K_eff, inv


def _require_pinhole(K):
    if K.dim() != 3 or tuple(K.shape[1:]) != (4, 4):
        raise ValueError(f"K: expected (B,4,4), got {tuple(K.shape)}")
    Kc = K.detach().cpu()
    rest = Kc.clone()
    rest[:, 0, 0] = rest[:, 1, 1] = rest[:, 0, 2] = rest[:, 1, 2] = 0
    rest[:, 2, 2] -= 1
    rest[:, 3, 3] -= 1
    if bool(rest.ne(0).any()) or bool((Kc[:, 0, 0] == 0).any()) or bool((Kc[:, 1, 1] == 0).any()) or not bool(torch.isfinite(Kc).all()):
        raise ValueError("learn_intrinsics: K must be a zero-skew pinhole matrix [[fx,0,cx,0],[0,fy,cy,0],[0,0,1,0],[0,0,0,1]] with fx, fy != 0")


def learn_intrinsics(depth_tgt, src, tgt, K, T, steps, lr, padding_mode="border", use_mask=True, init=(1, 1, 1, 1)):
    """Self-calibration through the photometric loss: four factors on fx, fy, cx, cy of the zero-skew pinhole K (B,4,4; anything else raises
    ValueError) are trained by FusedAdam through ops.warp_photometric(intrinsics_grad=True) -- K_eff and its closed-form inverse are
    rebuilt from the factors every step (intrinsics_from_factors), the fused backward returns dL/dK_eff and dL/d inv_K_eff, and torch
    carries both onto the factors.  Depth (B,1,H,W) and pose (B,4,4) are fixed.  Returns (factors (4,) on the CPU, K_eff (B,4,4) at those
    factors, [loss per step])."""
    if len(init) != 4:
        raise ValueError("init: four factors, on fx, fy, cx, cy")
    d = L.dev(depth_tgt, "depth_tgt").detach().contiguous()
    K = L.dev(K, "K").detach()
    _require_pinhole(K)
    T = L.dev(T, "T").detach().contiguous()
    f = torch.nn.Parameter(torch.tensor([float(v) for v in init], device=d.device))
    opt = FusedAdam([f], lr=lr)
    trace = []
    for _ in range(steps):
        K_eff, inv_eff = intrinsics_from_factors(K, f)
        loss = ops.warp_photometric(d, src, tgt, K_eff, inv_eff, T, padding_mode=padding_mode, use_mask=use_mask, intrinsics_grad=True)["photometric"]
        g, = torch.autograd.grad(loss, f)
        trace.append(loss.detach().clone())
        opt.zero_grad()
        if f.grad is None:
            f.grad = g.clone()
        else:
            f.grad.copy_(g)
        opt.step()
    with torch.no_grad():
        K_eff = intrinsics_from_factors(K, f.data)[0].clone()
    return f.data.detach().cpu().clone(), K_eff, ([float(v) for v in torch.stack(trace).cpu()] if trace else [])


def scale_grid_search(depth_pred, src, tgt, K, T, grid, steps=3, lr=1e-2, affine=True, padding_mode="border", use_mask=True, init_bias=0.0):
    """The outer loop of absolute_scale.py:268-405: for every initial value of SCALE_GRID_SEARCH.grid a FRESH scale layer and a fresh
    optimiser (`scale_layer_init(init_depth_scale)`, :207-240, :273) are trained for OPTIMIZATION.refinement_steps steps on the same
    batch.  Returns one record per grid value: {"init", "w", "b", "losses"} -- what the reference prints as "Trainable param after
    training" for each experiment."""
    out = []
    for init in grid:
        w, b, trace = learn_depth_scale(depth_pred, src, tgt, K, T, steps=steps, lr=lr, init_value=float(init), affine=affine,
                                        padding_mode=padding_mode, use_mask=use_mask, init_bias=init_bias)
        out.append({"init": float(init), "w": w, "b": b, "losses": trace})
    return out
