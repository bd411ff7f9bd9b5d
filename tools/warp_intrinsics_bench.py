#!/usr/bin/env python3
"""Time of the image-space part of one step when the camera intrinsics carry a graph (self-calibration), 480 x 640, B = 1:

    alone, on the buffers of one forward: e2e_warp_photo_bwd_intrinsics next to e2e_warp_photo_bwd_pose and e2e_warp_photo_bwd
        (what the gradient with respect to K and inv_K adds: a second pass over the tiles for the 9 sums Q, and one final kernel);
    (a) chain   ops.backproject -> project3d -> grid_sample -> two mask_mul -> photometric -> mean, forward + backward, with the gradient
                for the depth, K, inv_K and T;
    (b) fused   ops.warp_photometric(intrinsics_grad=True), forward + backward, the same four gradients;
    and (b) for the window of two sources and for its geometric form, ops.warp_photometric_window(intrinsics_grad=True), each next to the
    same call with the intrinsics detached.

    python tools/warp_intrinsics_bench.py [--height 480 --width 640 --reps 20 --warmup 5]

Each figure is the median of `reps` single calls, each between two device events, the arms of a comparison taking turns.  One JSON line.
Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from warp_pose_bench import medians_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from e2ehip import _lib as L
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    L.load()
    if not torch.cuda.is_available():
        raise SystemExit("warp_intrinsics_bench: no GPU (the kernels have no CPU path)")
    dev, B, H, W = "cuda:0", 1, a.height, a.width
    colors, depths, K, poses = make_sequence(3, H, W, seed=7)
    src, tgt, src2 = (colors[:, i].to(dev).permute(0, 3, 1, 2) for i in (0, 1, 2))  # NCHW views of NHWC memory, as the driver passes them
    depth = depths[:, 1, ..., 0].reshape(B, 1, H, W).contiguous().to(dev)
    dsrcs = [depths[:, i, ..., 0].reshape(B, 1, H, W).contiguous().to(dev) for i in (0, 2)]
    K0 = K[:, 0].contiguous().to(dev)
    iK0 = torch.linalg.inv(K0)
    T0, T2 = ((torch.linalg.inv(poses[:, i]) @ poses[:, 1]).contiguous().to(dev) for i in (0, 2))
    leaves = lambda: (depth.clone().requires_grad_(), K0.clone().requires_grad_(), iK0.clone().requires_grad_(), T0.clone().requires_grad_())

    def chain():
        d, Kl, iKl, T = leaves()
        grid, valid = ops.project3d(ops.backproject(d, iKl), Kl, T, H, W)
        synth = ops.grid_sample(src, grid, padding_mode="border", align_corners=False)
        ops.photometric(ops.mask_mul(synth, valid), ops.mask_mul(tgt, valid)).mean().backward()
        return Kl.grad, iKl.grad

    def fused():
        d, Kl, iKl, T = leaves()
        ops.warp_photometric(d, src, tgt, Kl, iKl, T, padding_mode="border", use_mask=True, intrinsics_grad=True)["photometric"].backward()
        return Kl.grad, iKl.grad

    def window(geometric, intrinsics):
        def run():
            d, Kl, iKl, T = leaves()
            Tb = T2.clone().requires_grad_()
            more = dict(geometric=True, depth_srcs=dsrcs, geo_min_valid=0) if geometric else {}
            out = ops.warp_photometric_window(d, [src, src2], tgt, Kl if intrinsics else K0, iKl if intrinsics else iK0, [T, Tb], padding_mode="border",
                                              use_mask=True, min_reprojection=True, auto_masking=True, intrinsics_grad=True, **more)
            (out["photometric"] + out["geometric"].sum() if geometric else out["photometric"]).backward()
        return run

    (gK_c, giK_c), (gK_f, giK_f) = chain(), fused()
    rec = {"B": B, "H": H, "W": W, "reps": a.reps, "chain_vs_fused_rel_g_K": float((gK_c - gK_f).abs().max() / gK_f.abs().max()),
           "chain_vs_fused_rel_g_inv_K": float((giK_c - giK_f).abs().max() / giK_f.abs().max())}
    arms = {"chain_fwd_bwd": chain, "fused_fwd_bwd": fused, "window_pose_fwd_bwd": window(False, False), "window_intrinsics_fwd_bwd": window(False, True),
            "geo_pose_fwd_bwd": window(True, False), "geo_intrinsics_fwd_bwd": window(True, True)}
    for k, (med, best) in medians_us(arms, a.reps, a.warmup).items():
        rec[k + "_us_median"], rec[k + "_us_min"] = med, best

    # the three backward entry points alone, on the buffers of one forward
    f = dict(device=dev, dtype=torch.float32)
    synth, valid, loss = torch.empty(B, 3, H, W, **f), torch.empty(B, 1, H, W, **f), torch.zeros(2, **f)
    ws = torch.empty(L.query("e2e_warp_photo_workspace_floats", B, H, W), **f)
    geom = dict(depth_tgt=L.ptr(depth), src=L.ptr(src), src_strides=L.strides4(src), tgt=L.ptr(tgt), tgt_strides=L.strides4(tgt), K=L.ptr(K0),
                inv_K=L.ptr(iK0), T=L.ptr(T0), use_mask=1, padding_mode=1, reg_kind=0, reg_init_tgt=None, reg_init_src=None, depth_src=None,
                B=B, H=H, W=W, stream=L.stream())
    L.call("e2e_warp_photo_fwd", geom=geom, synth=L.ptr(synth), valid=L.ptr(valid), pmap=None, loss_out=L.ptr(loss), workspace=L.ptr(ws))
    g_loss, g_dt = torch.ones(2, **f), torch.empty(B, 1, H, W, **f)
    g_T, g_K, g_iK = (torch.empty(B, 4, 4, **f) for _ in range(3))
    ws_pose = torch.empty(L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W), device=dev, dtype=torch.uint8)
    ws_intr = torch.empty(L.query("e2e_warp_photo_bwd_intrinsics_workspace_bytes", B, H, W), device=dev, dtype=torch.uint8)
    outputs = dict(synth=L.ptr(synth), valid=L.ptr(valid), g_loss=L.ptr(g_loss), g_depth_tgt=L.ptr(g_dt), g_depth_src=None)
    alone = {"bwd": lambda: L.call("e2e_warp_photo_bwd", geom=geom, **outputs),
             "bwd_pose": lambda: L.call("e2e_warp_photo_bwd_pose", geom=geom, g_T=L.ptr(g_T), workspace=L.ptr(ws_pose), **outputs),
             "bwd_intrinsics": lambda: L.call("e2e_warp_photo_bwd_intrinsics", geom=geom, g_T=L.ptr(g_T), g_K=L.ptr(g_K), g_inv_K=L.ptr(g_iK),
                                              workspace=L.ptr(ws_intr), **outputs)}
    for k, (med, best) in medians_us(alone, a.reps, a.warmup).items():
        rec[k + "_us_median"], rec[k + "_us_min"] = med, best
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
