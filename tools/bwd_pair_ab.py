#!/usr/bin/env python3
"""Per-layer A/B of the paired backward (e2e_conv2d_bwd_pair_deferred: a layer's backward-data and backward-weight GEMMs as ONE launch)
against the two separate calls it replaces, on every convolution of the depth network at the benchmark size (batch 2, 480x640), both
orders of the two tile sets, in ONE process: HIP events, the variants interleaved round by round, medians of the rounds.  The backward-weight
slab reduction is deferred in both forms (as in the plan) and is not timed.

    python tools/bwd_pair_ab.py [rounds] > bwd_pair_ab.txt        (on an MI355X)"""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "end-to-end-self-supervised-slam_amd")]
from e2ehip import _lib as L  # noqa: E402

DEV = "cuda:0"
B = 2
# name, Cx, Cskip, up, H, W (full-res input of the conv), Cout, k, stride, pad, reflect, bias
LAYERS = [
    ("layer1", 64, 0, 1, 120, 160, 64, 3, 1, 1, 0), ("l2.0.c1/2", 64, 0, 1, 120, 160, 128, 3, 2, 1, 0), ("l2.0.ds", 64, 0, 1, 120, 160, 128, 1, 2, 0, 0),
    ("layer2", 128, 0, 1, 60, 80, 128, 3, 1, 1, 0), ("l3.0.c1/2", 128, 0, 1, 60, 80, 256, 3, 2, 1, 0), ("l3.0.ds", 128, 0, 1, 60, 80, 256, 1, 2, 0, 0),
    ("layer3", 256, 0, 1, 30, 40, 256, 3, 1, 1, 0), ("l4.0.c1/2", 256, 0, 1, 30, 40, 512, 3, 2, 1, 0), ("l4.0.ds", 256, 0, 1, 30, 40, 512, 1, 2, 0, 0),
    ("layer4", 512, 0, 1, 15, 20, 512, 3, 1, 1, 0), ("up(4,0)", 512, 0, 1, 15, 20, 256, 3, 1, 1, 1), ("up(4,1)", 256, 256, 2, 30, 40, 256, 3, 1, 1, 1),
    ("up(3,0)", 256, 0, 1, 30, 40, 128, 3, 1, 1, 1), ("up(3,1)", 128, 128, 2, 60, 80, 128, 3, 1, 1, 1), ("up(2,0)", 128, 0, 1, 60, 80, 64, 3, 1, 1, 1),
    ("up(2,1)", 64, 64, 2, 120, 160, 64, 3, 1, 1, 1), ("up(1,0)", 64, 0, 1, 120, 160, 32, 3, 1, 1, 1), ("up(1,1)", 32, 64, 2, 240, 320, 32, 3, 1, 1, 1),
    ("up(0,0)", 32, 0, 1, 240, 320, 16, 3, 1, 1, 1),
]
# how often each shape occurs in one backward pass of the network (BasicBlock convolutions: 2 blocks x 2 convs, the stage entry's conv1 and
# downsample once, its conv2 and the second block's two convs at the stage shape -- layer1 has no stage entry)
COUNT = {"layer1": 4, "layer2": 3, "layer3": 3, "layer4": 3}


def timeit(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    lib = L.load()
    st = L.stream()
    print(f"{'layer':10s} {'n':>2s} {'separate':>9s} {'pair w1st':>9s} {'pair d1st':>9s}   gain (best order)   us per call, median of {rounds} rounds")
    tot = {"sep": 0.0, 1: 0.0, 0: 0.0}
    for (name, Cx, Cs, up, H, W, Cout, k, s, p, pm) in LAYERS:
        Cin = Cx + Cs
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        pp = p if pm else 0
        g = torch.Generator().manual_seed(0)
        da = torch.randn(B, Ho, Wo, Cout, generator=g).to(DEV)
        wb = torch.randn(k * k * Cout, (Cin + 3) // 4 * 4, generator=g).to(DEV)
        src0 = torch.randn(B, H // up, W // up, Cx, generator=g).to(DEV)
        src1 = torch.randn(B, H, W, Cs, generator=g).to(DEV) if Cs else None
        dx = torch.empty(B, H + 2 * pp, W + 2 * pp, Cin, device=DEV)
        n_wsb = lib.e2e_conv2d_bwd_data_workspace_floats(B, H + 2 * pp, W + 2 * pp, Cin, k * k * Cout, s)
        wsb = torch.zeros(n_wsb, device=DEV) if n_wsb else None
        wsw = torch.empty(lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, pm), device=DEV)
        dw = torch.empty(Cout, Cin, k, k, device=DEV)
        db = torch.empty(Cout, device=DEV) if pm else None
        d = L.WgradReduceDesc()
        data = [L.ptr(da), L.ptr(wb), wb.shape[1], L.ptr(dx), B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm]
        wtail = [L.ptr(src0), L.ptr(src1), Cx, up, L.ptr(dw), L.ptr(db), L.ptr(wsw)]

        def separate():
            L.call("e2e_conv2d_bwd_data", *data, L.ptr(wsb), st)
            L.call("e2e_conv2d_bwd_weight_scaled_deferred", L.ptr(da), None, *wtail, B, H, W, Cin, Cout, Ho, Wo, k, k, s, p, pm, 0, 0.0, 1.0,
                   ctypes.byref(d), st)

        def pair(order):
            return lambda: L.call("e2e_conv2d_bwd_pair_deferred", *data, 0, None, 0, None, L.ptr(wsb), None, *wtail, 0, 0.0, 1.0, ctypes.byref(d), order, st)

        variants = {"sep": separate, 1: pair(1), 0: pair(0)}
        for f in variants.values():
            f(); f()
        torch.cuda.synchronize()
        res = {key: [] for key in variants}
        for _ in range(rounds):
            for key, f in variants.items():
                res[key].append(timeit(f))
        med = {key: statistics.median(v) for key, v in res.items()}
        n = COUNT.get(name, 1)
        for key in tot:
            tot[key] += n * med[key]
        best = min(med[1], med[0])
        print(f"{name:10s} {n:2d} {med['sep']:9.1f} {med[1]:9.1f} {med[0]:9.1f}   {100 * (med['sep'] - best) / med['sep']:+6.1f} %"
              f"   spread sep {min(res['sep']):.1f}-{max(res['sep']):.1f}")
        sys.stdout.flush()
    print(f"{'pass':10s} {'':2s} {tot['sep']:9.1f} {tot[1]:9.1f} {tot[0]:9.1f}   {100 * (tot['sep'] - tot[1]) / tot['sep']:+6.1f} % (wgrad first)"
          f"  {100 * (tot['sep'] - tot[0]) / tot['sep']:+6.1f} % (data first)   us per backward pass, weighted by COUNT")


if __name__ == "__main__":
    main()
