#!/usr/bin/env python3
"""Train-mode conv + BatchNorm [+ residual] [+ ReLU] of the ResNet-18 body (depth_estimation.networks._ConvBN.run with bn.training),
forward and forward + backward, on the native kernels (csrc/bn_train.hip) against the nn.BatchNorm2d module path (E2E_BN_NATIVE=0, read
at every call) of the same build -- the distinct layer shapes of a 2 x 480 x 640 input, C = 64 / 128 / 256 / 512 at 240 x 320 down to
15 x 20 -- and one whole-network train-mode forward + backward of DispResNet_Indoor(18).

    python tools/bn_train_bench.py [--batch 2 --height 480 --width 640 --reps 50 --warmup 10 --windows 5]

A call is the module-level call a training step makes (autograd and the host's launches included): `reps` calls are enqueued back to back
between two device events and the window is divided by `reps`.  The two arms ALTERNATE window by window; the median and the fastest of
`windows` windows per arm are printed, in microseconds.  Bytes are what the BatchNorm side of the native path has to move (the convolution
is the same launch in both arms): forward reads z twice (statistics, normalisation) and the residual once and writes y; backward reads
dy, y (with a ReLU) and z twice and writes dz (and the masked residual gradient with a ReLU + residual).  One JSON line per layer and
one for the network.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))

# name, Cin, Cout, kernel, stride, input height and width as a divisor of the frame's, relu, residual
LAYERS = (
    ("stem 7x7/2", 3, 64, 7, 2, 1, True, False),
    ("layer1 conv1", 64, 64, 3, 1, 4, True, False),
    ("layer1 conv2", 64, 64, 3, 1, 4, True, True),
    ("layer2 conv1/2", 64, 128, 3, 2, 4, True, False),
    ("layer2 conv2", 128, 128, 3, 1, 8, True, True),
    ("layer2 down", 64, 128, 1, 2, 4, False, False),
    ("layer3 conv1/2", 128, 256, 3, 2, 8, True, False),
    ("layer3 conv2", 256, 256, 3, 1, 16, True, True),
    ("layer3 down", 128, 256, 1, 2, 8, False, False),
    ("layer4 conv1/2", 256, 512, 3, 2, 16, True, False),
    ("layer4 conv2", 512, 512, 3, 1, 32, True, True),
    ("layer4 down", 256, 512, 1, 2, 16, False, False),
)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps            # microseconds per call


def alternate(fn, reps, warmup, windows):
    """{arm: [window times]} with the arms alternating window by window, each warmed up first."""
    t = {"native": [], "module": []}
    for arm in t:
        os.environ["E2E_BN_NATIVE"] = "1" if arm == "native" else "0"
        window(fn, warmup)
    for _ in range(windows):
        for arm in t:
            os.environ["E2E_BN_NATIVE"] = "1" if arm == "native" else "0"
            t[arm].append(window(fn, reps))
    os.environ.pop("E2E_BN_NATIVE", None)
    return t


def stats(rec, key, t):
    for arm, v in t.items():
        rec[f"{key}_{arm}_us_median"], rec[f"{key}_{arm}_us_min"] = round(statistics.median(v), 1), round(min(v), 1)
    rec[f"{key}_native_over_module"] = round(statistics.median(t["native"]) / statistics.median(t["module"]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_train_bench: no GPU (the kernels have no CPU path)")
    from depth_estimation.networks import DispResNet_Indoor, _ConvBN
    dev, B, CL = "cuda:0", a.batch, torch.channels_last
    g = torch.Generator().manual_seed(0)
    for name, Cin, Cout, k, stride, div, relu, has_res in LAYERS:
        Hin, Win = a.height // div, a.width // div
        conv = torch.nn.Conv2d(Cin, Cout, k, stride, k // 2, bias=False).to(dev)
        bn = torch.nn.BatchNorm2d(Cout).to(dev).train()
        x = torch.randn(B, Cin, Hin, Win, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_(Cin != 3)
        with torch.no_grad():
            y0 = _ConvBN.run(conv, bn, x, relu)
        res = torch.randn(y0.shape, generator=g).to(dev).contiguous(memory_format=CL).requires_grad_(True) if has_res else None
        dy = torch.randn(y0.shape, generator=g).to(dev).contiguous(memory_format=CL)

        def fwd():
            return _ConvBN.run(conv, bn, x, relu, residual=res)

        def both():
            fwd().backward(dy)
            conv.weight.grad = bn.weight.grad = bn.bias.grad = x.grad = None
            if res is not None:
                res.grad = None
        n = y0.numel()
        rec = {"layer": name, "B": B, "H": y0.shape[2], "W": y0.shape[3], "C": Cout, "relu": relu, "residual": has_res, "reps": a.reps,
               "bn_fwd_MB": round(4 * n * (3 + has_res) / 1e6, 3), "bn_bwd_MB": round(4 * n * (2 * (2 + relu) + 1 + (relu and has_res)) / 1e6, 3)}
        stats(rec, "fwd", alternate(fwd, a.reps, a.warmup, a.windows))
        stats(rec, "fwd_bwd", alternate(both, a.reps, a.warmup, a.windows))
        print(json.dumps(rec), flush=True)
    net = DispResNet_Indoor(18, False).to(dev).train()
    frame = torch.rand(B, a.height, a.width, 3, generator=g).to(dev)

    def step():
        net(frame, 0)[("disp", 0, 0)].mean().backward()
        net.zero_grad(set_to_none=True)
    rec = {"network": "DispResNet_Indoor(18) train mode, forward + backward", "B": B, "H": a.height, "W": a.width, "reps": max(a.reps // 5, 5)}
    stats(rec, "fwd_bwd", alternate(step, rec["reps"], 3, a.windows))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
