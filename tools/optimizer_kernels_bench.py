#!/usr/bin/env python3
"""Time the four fused optimiser launches (e2e_adam / sgd / rmsprop / adagrad _step_resident) at the depth network's bucket size, in one
process, alternating them: microseconds per launch and achieved bytes/s, counted from the arrays each update has to move
(Adam: reads p, g, m, v, writes p, m, v = 28 B per element; the others: reads p, g, state, writes p, state = 20 B).

    python tools/optimizer_kernels_bench.py [--n ELEMENTS] [--launches 200] [--rounds 5]

Device events around `launches` back-to-back launches (each a streaming kernel + the one-thread counter kernel), `rounds` rounds per
optimiser taken in turn; the median round is reported, the fastest and slowest next to it.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd"))


def bucket_elements():
    """Elements of the flat bucket the online driver builds: the depth network's used parameters without the frozen BatchNorm ones,
    every slice padded to 16 bytes."""
    from depth_estimation.networks import DispResNet_Indoor
    m = DispResNet_Indoor(num_layers=18, pretrained=False)
    frozen = {id(p) for name, p in m.named_parameters() if name.find("bn") != -1}
    return sum((p.numel() + 3) // 4 * 4 for p in m.used_parameters() if id(p) not in frozen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=0)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    n = a.n or bucket_elements()
    assert torch.cuda.is_available(), "needs the MI355X: a timing from anywhere else says nothing"
    from e2ehip import _lib as L
    dev = "cuda"
    gen = torch.Generator().manual_seed(0)
    g = (torch.randn(n, generator=gen) * 1e-2).to(dev)
    lr = torch.full((1,), 1e-5, device=dev)
    part = torch.ones(1, device=dev)
    sched = torch.tensor([[1e-5, 1.0]], device=dev).repeat(4, 1).contiguous()          # constant rows: the timed launches read row 1..4 and stay there
    common = dict(grad_sums=L.ptr(g), participants=L.ptr(part), n=n)
    runs = {}
    for name, nstate, kw in (("adam", 2, dict(beta1=0.9, beta2=0.999, eps=1e-8, schedule=L.ptr(sched), schedule_len=4)),
                             ("sgd", 1, dict(lr=L.ptr(lr), momentum=0.9, weight_decay=1e-3)),
                             ("rmsprop", 1, dict(lr=L.ptr(lr), alpha=0.99, eps=1e-8)),
                             ("adagrad", 1, dict(lr=L.ptr(lr), eps=1e-10))):
        p = torch.randn(n, generator=gen).to(dev)
        state = [torch.zeros(n, device=dev) for _ in range(nstate)]
        counter = torch.ones(1, device=dev, dtype=torch.int32)
        keys = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",), "rmsprop": ("square_avg",), "adagrad": ("sum",)}[name]
        args = L.bind(f"e2e_{name}_step_resident", params=L.ptr(p), step_counter=L.ptr(counter), stream=L.stream(),
                      **dict(zip(keys, map(L.ptr, state))), **common, **kw)
        runs[name] = dict(args=args, keep=(p, state, counter), bytes=4 * n * (3 + 2 * nstate), ms=[])
    for name, r in runs.items():                                                        # warm-up: code objects, clocks, every buffer touched
        for _ in range(20):
            L.call(f"e2e_{name}_step_resident", *r["args"])
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, r in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                L.call(f"e2e_{name}_step_resident", *r["args"])
            e1.record()
            e1.synchronize()
            r["ms"].append(e0.elapsed_time(e1) / a.launches)
    out = {"metric": "fused optimiser launch", "elements": n, "launches_per_round": a.launches, "rounds": a.rounds, "kernels": {}}
    for name, r in runs.items():
        ms = sorted(r["ms"])
        med = ms[len(ms) // 2]
        out["kernels"][name] = {"us": round(med * 1e3, 2), "us_min": round(ms[0] * 1e3, 2), "us_max": round(ms[-1] * 1e3, 2),
                                "bytes": r["bytes"], "TB_per_s": round(r["bytes"] / (med * 1e-3) / 1e12, 3)}
        assert all(bool(torch.isfinite(t).all()) for t in [r["keep"][0]] + r["keep"][1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
