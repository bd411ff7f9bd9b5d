#!/usr/bin/env python3
"""Time of the image-space part of one training step with LOSS.geometric, 480 x 640, B = 1, every relative pose carrying a graph, for S = 1
(DATA.frames: [0, -1]) and S = 2 source frames ([0, -1, 1]), without and with LOSS.min_reprojection + LOSS.auto_masking:

    (a) chain   the operator chain that fused_losses=False takes -- per source ops.backproject -> project3d(geometric) -> grid_sample of the
                image (align_corners=True) and of the source depth (False) -> two mask_mul -> photometric -> geometric_consistency, and for
                auto-masking mask_mul -> photometric again; then cat / channel_mean / the tie-break plane and min_reprojection, plus
                mean_s G_s x 0.5 -- forward + backward, with the gradient for the depth, every source depth and every pose;
    (b) fused   ops.warp_photometric_window(geometric=True), forward + backward, the same gradients (e2e_warp_photo_geo_fwd + _bwd).

    python tools/warp_geo_bench.py [--height 480 --width 640 --reps 20 --warmup 5 --runs 3]

Each figure is the median of `reps` single calls, each between two device events, the two arms taking turns (both include their host-side
autograd work, which is part of what the step pays); `runs` repetitions of the whole measurement.  One JSON line per row and run.  The
synthetic sequence projects more than 10000 valid pixels per source at this size, so the reference's gate is open in both arms (the line
says so).  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from warp_pose_bench import medians_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    from e2ehip import _lib as L
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    L.load()
    if not torch.cuda.is_available():
        raise SystemExit("warp_geo_bench: no GPU (the kernels have no CPU path)")
    dev, B, H, W = "cuda:0", 1, a.height, a.width
    colors, depths, K, poses = make_sequence(3, H, W, seed=7)
    colors = colors.to(dev)
    srcs = [colors[:, i].permute(0, 3, 1, 2) for i in (0, 2)]                      # NCHW views of NHWC memory, as the driver passes them
    tgt = colors[:, 1].permute(0, 3, 1, 2)
    depth = depths[:, 1, ..., 0].reshape(B, 1, H, W).contiguous().to(dev)
    # the source depths 2 % off the scene's, one each way: on the exact depths wd - id is rounding noise on every plane of the scene, its sign --
    # hence g_depth_src -- would be decided by rounding, and the two arms could not be compared
    dsrc0 = [(depths[:, i, ..., 0].reshape(B, 1, H, W) * f).contiguous().to(dev) for i, f in ((0, 1.02), (2, 0.98))]
    K = K[:, 0].contiguous().to(dev)
    inv_K = torch.linalg.inv(K)
    T0 = [(torch.linalg.inv(poses[:, i]) @ poses[:, 1]).contiguous().to(dev) for i in (0, 2)]
    weight = 0.5                                                                   # LOSS.geometric_weight

    def leaves(S):
        return depth.clone().requires_grad_(), [x.clone().requires_grad_() for x in dsrc0[:S]], [T.clone().requires_grad_() for T in T0[:S]]

    def chain(S, flags, noise):
        d, dss, Ts = leaves(S)
        maps, autos, geos = [], [], []
        for src, ds, T in zip(srcs, dss, Ts):
            grid, wd, valid = ops.project3d(ops.backproject(d, inv_K), K, T, H, W, geometric=True)
            synth = ops.grid_sample(src, grid, padding_mode="border", align_corners=True)
            idp = ops.grid_sample(ds, grid, padding_mode="border", align_corners=False)
            y = ops.mask_mul(tgt, valid)
            maps.append(ops.photometric(ops.mask_mul(synth, valid), y))
            if flags:
                autos.append(ops.photometric(ops.mask_mul(src, valid), ops.mask_mul(tgt, valid)))
            geos.append(ops.geometric_consistency(wd, idp, valid))
        photo = torch.cat(maps, 1) if S > 1 else maps[0]
        if flags:
            ident = (torch.cat(autos, 1) if S > 1 else autos[0]) + noise
            photo = torch.cat((ident, photo), 1)
        elif S > 1:
            photo = ops.channel_mean(photo)
        geo = torch.stack(geos, 0)
        (ops.min_reprojection(photo) + geo.mean() * weight).backward()
        return d.grad, [x.grad for x in dss], [T.grad for T in Ts], geo.detach()

    def fused(S, flags, noise):
        d, dss, Ts = leaves(S)
        out = ops.warp_photometric_window(d, srcs[:S], tgt, K, inv_K, Ts, padding_mode="border", use_mask=True, min_reprojection=flags,
                                          auto_masking=flags, tie_noise=noise if flags else None, geometric=True, depth_srcs=dss)
        (out["photometric"] + out["geometric"].mean() * weight).backward()
        return d.grad, [x.grad for x in dss], [T.grad for T in Ts], out["geometric"].detach(), out["geo_count"]

    def rel(xs, ys):
        top = max(float(y.abs().max()) for y in ys)
        return max(float((x - y).abs().max()) for x, y in zip(xs, ys)) / top if top > 0 else 0.0

    for S in (1, 2):
        noise = torch.randn(B, S, H, W, device=dev) * 0.00001
        for flags in (False, True):
            c, f = chain(S, flags, noise), fused(S, flags, noise)
            rec0 = {"S": S, "min_reprojection": flags, "auto_masking": flags, "B": B, "H": H, "W": W, "reps": a.reps, "geo_count": f[4].tolist(),
                    "gate_open": bool((f[4] > 10000).all()), "G_chain": [round(float(x), 6) for x in c[3]], "G_fused": [round(float(x), 6) for x in f[3]],
                    "chain_vs_fused_rel_g_depth_src": rel(c[1], f[1]), "chain_vs_fused_rel_g_T": rel(c[2], f[2])}
            for run in range(a.runs):
                rec = dict(rec0, run=run)
                t = medians_us({"chain_fwd_bwd": lambda: chain(S, flags, noise), "fused_fwd_bwd": lambda: fused(S, flags, noise)}, a.reps, a.warmup)
                for k, (med, best) in t.items():
                    rec[k + "_us_median"], rec[k + "_us_min"] = med, best
                rec["fused_over_chain"] = round(t["fused_fwd_bwd"][0] / t["chain_fwd_bwd"][0], 3)
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
