#!/usr/bin/env python3
"""Time of the forward and the backward of the four disparity heads (csrc/disp_heads.hip) at the 480 x 640 pyramid, B = 2:
480x640x16, 240x320x32, 120x160x64, 60x80x128 -- next to the bytes each call has to move at the least.

    python tools/disp_head_bench.py [--batch 2 --height 480 --width 640 --reps 200 --warmup 20 --act sigmoid]

A call is a few microseconds to a few tens: `reps` calls are enqueued back to back between two device events and the window is divided
by `reps` (the time of a call in a stream of calls; the first launch and its code-object load are in the warm-up).  Five such windows per
entry, the median and the fastest are printed.  Bytes: forward reads x and writes y; backward (dx + dw + dbias) reads x, dy, y and writes
dx -- the weights and the partial sums are noise next to them.  One JSON line per head.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--act", default="sigmoid", choices=["none", "disp", "sigmoid"])
    a = ap.parse_args()
    from e2ehip import _lib as L
    from e2ehip.conv import ACT
    L.load()
    if not torch.cuda.is_available():
        raise SystemExit("disp_head_bench: no GPU (the heads have no CPU path)")
    dev, act, B = "cuda:0", ACT[None if a.act == "none" else a.act], a.batch
    g = torch.Generator().manual_seed(0)
    for s, C in enumerate((16, 32, 64, 128)):
        H, W = a.height >> s, a.width >> s
        x = torch.randn(B, H, W, C, generator=g).to(dev)
        w = (torch.randn(1, C, 3, 3, generator=g) / (9 * C) ** 0.5).to(dev)
        bias, dy = torch.randn(1, generator=g).to(dev), torch.randn(B, H, W, generator=g).to(dev)
        y, dx, dw, db = torch.empty(B, H, W, device=dev), torch.empty_like(x), torch.empty_like(w), torch.empty(1, device=dev)
        ws = torch.empty(L.query("e2e_disp_head_workspace_floats", B=B, H=H, W=W, Cin=C), device=dev)
        st = L.stream()

        def fwd():
            L.call("e2e_disp_head_fwd", L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), B, H, W, C, act, st)

        def bwd():
            L.call("e2e_disp_head_bwd", L.ptr(dy), L.ptr(y), L.ptr(x), L.ptr(w), L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, C, act, st)
        fwd()
        rec = {"B": B, "H": H, "W": W, "Cin": C, "act": a.act, "reps": a.reps}
        for name, fn, nbytes in (("fwd", fwd, 4 * (x.numel() + y.numel())), ("bwd", bwd, 4 * (2 * x.numel() + 2 * y.numel()))):
            window(fn, a.warmup)
            t = [window(fn, a.reps) for _ in range(5)]
            med = statistics.median(t)
            rec.update({f"{name}_us_median": round(med, 2), f"{name}_us_min": round(min(t), 2), f"{name}_MB": round(nbytes / 1e6, 3),
                        f"{name}_GBps_at_median": round(nbytes / med / 1e3, 1)})
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
