#!/usr/bin/env python3
"""Time of the image-space part of one training step when the relative pose T carries a graph (DATA.use_gt_pose: False), 480 x 640, B = 1:

    (a) chain   the operator chain that fused_losses=False takes: ops.backproject -> project3d -> grid_sample -> two mask_mul ->
                photometric -> min_reprojection (the mean), forward + backward, with the gradient for the depth and for T;
    (b) fused   ops.warp_photometric, forward + backward, the same two gradients (e2e_warp_photo_fwd + e2e_warp_photo_bwd_pose);
    and, alone, e2e_warp_photo_bwd_pose next to e2e_warp_photo_bwd on the same buffers (what the pose gradient adds to the launch).

    python tools/warp_pose_bench.py [--height 480 --width 640 --reps 20 --warmup 5]

Each figure is the median of `reps` single calls, each between two device events, the arms of a comparison taking turns (a call here is
tens to hundreds of microseconds, and (a), (b) include their host-side autograd work, which is part of what the step pays).  One JSON
line.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))


def medians_us(fns, reps, warmup):
    """{name: (median, fastest)} of `reps` single calls of every function, the functions taking turns (so that a drift of the machine
    meets all of them alike), each call between two device events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t[k].append(a.elapsed_time(b) * 1e3)
    return {k: (round(statistics.median(v), 1), round(min(v), 1)) for k, v in t.items()}


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
        raise SystemExit("warp_pose_bench: no GPU (the kernels have no CPU path)")
    dev, B, H, W = "cuda:0", 1, a.height, a.width
    colors, depths, K, poses = make_sequence(2, H, W, seed=7)
    src, tgt = (colors[:, i].to(dev).permute(0, 3, 1, 2) for i in (0, 1))          # NCHW views of NHWC memory, as the driver passes them
    depth = depths[:, 1, ..., 0].reshape(B, 1, H, W).contiguous().to(dev)
    K = K[:, 0].contiguous().to(dev)
    inv_K = torch.linalg.inv(K)
    T0 = (torch.linalg.inv(poses[:, 0]) @ poses[:, 1]).contiguous().to(dev)

    def chain():
        d, T = depth.clone().requires_grad_(), T0.clone().requires_grad_()
        grid, valid = ops.project3d(ops.backproject(d, inv_K), K, T, H, W)
        synth = ops.grid_sample(src, grid, padding_mode="border", align_corners=False)
        ops.min_reprojection(ops.photometric(ops.mask_mul(synth, valid), ops.mask_mul(tgt, valid))).backward()
        return d.grad, T.grad

    def fused():
        d, T = depth.clone().requires_grad_(), T0.clone().requires_grad_()
        ops.warp_photometric(d, src, tgt, K, inv_K, T, padding_mode="border", use_mask=True)["photometric"].backward()
        return d.grad, T.grad

    (_, gT_c), (_, gT_f) = chain(), fused()
    rec = {"B": B, "H": H, "W": W, "reps": a.reps, "chain_vs_fused_rel_g_T": float((gT_c - gT_f).abs().max() / gT_f.abs().max())}
    for k, (med, best) in medians_us({"chain_fwd_bwd": chain, "fused_fwd_bwd": fused}, a.reps, a.warmup).items():
        rec[k + "_us_median"], rec[k + "_us_min"] = med, best

    # the two backward entry points alone, on the buffers of one forward
    f = dict(device=dev, dtype=torch.float32)
    synth, valid, loss = torch.empty(B, 3, H, W, **f), torch.empty(B, 1, H, W, **f), torch.zeros(2, **f)
    ws = torch.empty(L.query("e2e_warp_photo_workspace_floats", B, H, W), **f)
    geom = dict(depth_tgt=L.ptr(depth), src=L.ptr(src), src_strides=L.strides4(src), tgt=L.ptr(tgt), tgt_strides=L.strides4(tgt), K=L.ptr(K),
                inv_K=L.ptr(inv_K), T=L.ptr(T0), use_mask=1, padding_mode=1, reg_kind=0, reg_init_tgt=None, reg_init_src=None, depth_src=None,
                B=B, H=H, W=W, stream=L.stream())
    L.call("e2e_warp_photo_fwd", geom=geom, synth=L.ptr(synth), valid=L.ptr(valid), pmap=None, loss_out=L.ptr(loss), workspace=L.ptr(ws))
    g_loss, g_dt, g_T = torch.ones(2, **f), torch.empty(B, 1, H, W, **f), torch.empty(B, 4, 4, **f)
    ws_pose = torch.empty(L.query("e2e_warp_photo_bwd_pose_workspace_bytes", B, H, W), device=dev, dtype=torch.uint8)
    outputs = dict(synth=L.ptr(synth), valid=L.ptr(valid), g_loss=L.ptr(g_loss), g_depth_tgt=L.ptr(g_dt), g_depth_src=None)
    alone = {"bwd": lambda: L.call("e2e_warp_photo_bwd", geom=geom, **outputs),
             "bwd_pose": lambda: L.call("e2e_warp_photo_bwd_pose", geom=geom, g_T=L.ptr(g_T), workspace=L.ptr(ws_pose), **outputs)}
    for k, (med, best) in medians_us(alone, a.reps, a.warmup).items():
        rec[k + "_us_median"], rec[k + "_us_min"] = med, best
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
