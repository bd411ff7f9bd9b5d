#!/usr/bin/env python3
"""Time of one PointFusion map step at camera resolution against a large map: FusionMap.step, FusionMap.step_differentiable (forward:
the same kernels + the tape + the copy-out of the live rows) and its backward (e2e_pf_fuse_bwd + the vertex / alpha backward).

    python tools/map_grad_bench.py [--height 480 --width 640 --frames 5 --reps 20 --warmup 5] [--normals]

--normals adds a leg with the normals' gradient (step_differentiable(normal_gradient=True): the normals tape in the forward,
e2e_pf_fuse_normals_bwd and e2e_normal_maps_bwd in the backward, an upstream gradient on the normals as well) and times
e2e_normal_maps_bwd alone.

The map: `frames - 1` views of the synthetic scene from cameras turned so that no two overlap (every pixel appended: about
(frames - 1) x H x W rows), plus the first view again from the front; the timed step then fuses a slightly moved front view into it.
Device events around each part, the map state restored before every repetition (outside the timed region); medians are printed as
one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))


def yaw(deg, T):
    a = math.radians(deg)
    R = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1.0, 0], [-math.sin(a), 0, math.cos(a)]])
    out = T.clone()
    out[:3, :3] = R @ T[:3, :3]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--normals", action="store_true", help="also time the step with the normals' gradient, and e2e_normal_maps_bwd alone")
    a = ap.parse_args()
    from e2ehip.fusionmap import FusionMap
    from e2ehip.synthetic import make_sequence
    dev, H, W = "cuda:0", a.height, a.width
    colors, depths, K, poses = make_sequence(2, H, W, seed=5, step=0.02)
    rgb0, d0, rgb1, d1 = (t.to(dev).contiguous() for t in (colors[0, 0], depths[0, 0, ..., 0], colors[0, 1], depths[0, 1, ..., 0]))
    K, p0, p1 = K[0, 0].to(dev), poses[0, 0], poses[0, 1].to(dev)
    fm = FusionMap((a.frames + 2) * H * W, H, W, dev)
    for i in range(1, a.frames):                                           # views that share nothing: turned by 360 / frames degrees each
        fm.step(rgb0, d0, K, yaw(360.0 * i / a.frames, p0).to(dev))
    fm.step(rgb0, d0, K, p0.to(dev))
    M0 = fm.M
    base = [t.clone() for t in fm.live()]

    def restore():
        fm.load_state(*base)

    def timed(fn):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        out = fn(ev)
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), out

    def plain(ev):
        ev[0].record()
        fm.step(rgb1, d1, K, p1)
        ev[1].record()
        ev[2].record()
        return fm.M

    up = {}

    def differentiable(ev):
        d = d1.clone().requires_grad_(True)
        c = rgb1.clone().requires_grad_(True)
        prev = tuple(t.clone().requires_grad_(True) for t in (base[0], base[2], base[3]))
        ev[0].record()
        P, _, C, cc = fm.step_differentiable(c, d, K, p1, prev=prev)
        ev[1].record()
        if not up:
            up.update(P=torch.randn_like(P), C=torch.randn_like(C), cc=torch.randn_like(cc))
        torch.autograd.backward([P, C, cc], [up["P"], up["C"], up["cc"]])
        ev[2].record()
        assert d.grad is not None and c.grad is not None and all(t.grad is not None for t in prev)
        return fm.M

    def differentiable_normals(ev):
        d = d1.clone().requires_grad_(True)
        c = rgb1.clone().requires_grad_(True)
        prev = tuple(t.clone().requires_grad_(True) for t in (base[0], base[2], base[3], base[1]))
        ev[0].record()
        P, N, C, cc = fm.step_differentiable(c, d, K, p1, prev=prev, normal_gradient=True)
        ev[1].record()
        if "N" not in up:
            up.update(N=torch.randn_like(N))
        torch.autograd.backward([P, C, cc, N], [up["P"], up["C"], up["cc"], up["N"]])
        ev[2].record()
        assert d.grad is not None and c.grad is not None and all(t.grad is not None for t in prev)
        return fm.M

    def normal_maps_bwd_alone(ev):
        from e2ehip import _lib as L
        if "gd" not in up:
            up.update(gd=torch.empty(H, W, device=dev), gn=torch.randn(H, W, 3, device=dev), gg=torch.randn(H, W, 3, device=dev),
                      K1=K.contiguous(), P1=p1.contiguous())
        ev[0].record()
        L.call("e2e_normal_maps_bwd", depth=L.ptr(d1), K=L.ptr(up["K1"]), pose=L.ptr(up["P1"]), g_Nm=L.ptr(up["gn"]), g_Ng=L.ptr(up["gg"]),
               g_depth=L.ptr(up["gd"]), accumulate=0, B=1, H=H, W=W, stream=L.stream())
        ev[1].record()
        ev[2].record()

    res = {"plain": [], "diff_fwd": [], "diff_bwd": []}
    if a.normals:
        res.update(normals_fwd=[], normals_bwd=[], normal_maps_bwd=[])
    for i in range(a.warmup + a.reps):
        restore()
        t_plain, _, m_plain = timed(plain)
        matched = int(fm.table("unique").shape[0])
        restore()
        t_fwd, t_bwd, m_diff = timed(differentiable)
        assert m_plain == m_diff
        if a.normals:
            restore()
            t_nf, t_nb, m_n = timed(differentiable_normals)
            assert m_n == m_plain
            t_k, _, _ = timed(normal_maps_bwd_alone)
            if i >= a.warmup:
                res["normals_fwd"].append(t_nf)
                res["normals_bwd"].append(t_nb)
                res["normal_maps_bwd"].append(t_k)
        if i >= a.warmup:
            res["plain"].append(t_plain)
            res["diff_fwd"].append(t_fwd)
            res["diff_bwd"].append(t_bwd)
    print(json.dumps({"H": H, "W": W, "map_rows_before": M0, "map_rows_after": m_plain, "matched_pixels": matched, "reps": a.reps,
                      **{f"{k}_ms_median": round(statistics.median(v), 4) for k, v in res.items()},
                      **{f"{k}_ms_min": round(min(v), 4) for k, v in res.items()}}))


if __name__ == "__main__":
    main()
