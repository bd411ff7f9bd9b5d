"""float64 torch restatement of the PointFusion map step (oracle/pointfusion.py: vertex and alpha maps, the fuse expression of
fuse_with_map, the append) that autograd can walk: the reference for the map step's adjoint (csrc/pointfusion_grad.hip).
TEST INFRASTRUCTURE ONLY.

The differentiation rule of include/e2eslam.h: every step's `unique` table (rows [n, h, w]: map row n wins pixel (h, w)) is GIVEN, the
validity mask, the append order, the poses and the intrinsics are constants, the normals are left out (nothing differentiates them and
nothing here reads them).  The constants are the float32 ones of the oracle, widened: the inverse intrinsics as
oracle.pointfusion.intrinsics_inverse rounds them, alpha's denominator 2 sigma^2 + 1e-7 rounded to float32."""
import numpy as np
import torch

from oracle import pointfusion as opf

F64 = torch.float64


def frame_maps(depth, K, pose, sigma=0.6):
    """depth (H,W) float64 (may require grad); K, pose (4,4) -> Vg (H,W,3), alpha (H,W) float64, valid (H,W) bool."""
    H, W = depth.shape
    Ki = opf.intrinsics_inverse(K.float()).double()
    hs, ws = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    valid = depth.detach() != 0
    vf = valid.to(F64)
    V = torch.stack([(Ki[0, 0] * ws + Ki[0, 2]) * depth, (Ki[1, 1] * hs + Ki[1, 2]) * depth, depth], -1) * vf[..., None]
    P = pose.double()
    Vg = (V @ P[:3, :3].T + P[:3, 3]) * vf[..., None]
    den = float(np.float32(2 * (sigma ** 2) + 1e-7))
    alpha = torch.exp(-(V * V).sum(-1) / den)
    return Vg, alpha, valid


def empty_state():
    return {"points": torch.zeros(0, 3, dtype=F64), "colors": torch.zeros(0, 3, dtype=F64), "ccounts": torch.zeros(0, dtype=F64)}


def fuse(state, Vg, rgb, alpha, valid, unique):
    """fuse_with_map without the normals.  Every map row goes through X' = (c X + a X_f) / where(c + a == 0, 1, c + a) when anything
    matched (a = 0, X_f = 0 for a row that won no pixel); then the valid pixels that matched nothing are appended in row-major order."""
    M = state["points"].shape[0]
    new_mask = valid.clone()
    if M > 0 and unique.shape[0] > 0:
        n, h, w = unique[:, 0], unique[:, 1], unique[:, 2]
        assert n.unique().numel() == n.numel() and (h * valid.shape[1] + w).unique().numel() == n.numel()    # one row, one pixel
        c = state["ccounts"]
        fa = torch.zeros(M, dtype=F64).index_put((n,), alpha[h, w])
        cn = c + fa
        den = torch.where(cn == 0, torch.ones_like(cn), cn)
        out = {"ccounts": cn}
        for name, src in (("points", Vg), ("colors", rgb)):
            f = torch.zeros(M, 3, dtype=F64).index_put((n,), src[h, w])
            out[name] = (c[:, None] * state[name] + fa[:, None] * f) / den[:, None]
        new_mask[h, w] = False
    else:
        out = dict(state)
    return {"points": torch.cat([out["points"], Vg[new_mask]], 0), "colors": torch.cat([out["colors"], rgb[new_mask]], 0),
            "ccounts": torch.cat([out["ccounts"], alpha[new_mask]], 0)}


def step(state, rgb, depth, K, pose, unique, sigma=0.6):
    Vg, alpha, valid = frame_maps(depth, K, pose, sigma)
    return fuse(state, Vg, rgb, alpha, valid, unique)


def chain(rgbs, depths, K, poses, uniques, sigma=0.6, state=None):
    """rgbs[f] (H,W,3), depths[f] (H,W) float64; uniques[f]: the table of step f (an empty one for a step onto an empty map)."""
    state = empty_state() if state is None else state
    for rgb, depth, pose, unique in zip(rgbs, depths, poses, uniques):
        state = step(state, rgb, depth, K, pose, unique, sigma)
    return state


def weights(shape, seed):
    """Fixed upstream gradients of order 1: float64 holding float32 values, so that a float32 side multiplies by the same numbers."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32).double()


def scalar(state, seed=0):
    """sum(wP . points) + sum(wC . colors) + sum(wcc . ccounts): one scalar that sends a different gradient into every output entry."""
    return sum((weights(tuple(state[k].shape), seed + i) * state[k]).sum() for i, k in enumerate(("points", "colors", "ccounts")))


def sequence(H, W, L=3, seed=5):
    """e2ehip.synthetic.make_sequence(L, H, W, seed) with a rectangular hole in every depth map: fused, appended and invalid pixels in
    one frame.  -> rgbs (L,H,W,3), depths (L,H,W), K (4,4), poses (L,4,4), float32."""
    from e2ehip.synthetic import make_sequence
    colors, depths, K, poses = make_sequence(L, H, W, seed=seed)
    depths = depths[0, ..., 0].clone()
    depths[:, 2:5, 3:9] = 0
    return colors[0], depths, K[0, 0], poses[0]
