#!/usr/bin/env python3
"""Steps/s of the online driver with MODEL.slam: PointFusion and with MODEL.slam: ICPSLAM (aggregation: every valid pixel of a fused
frame is appended, FusionMap.append_resident) on bench.py's synthetic 640x480 sequence: the same loop (3 steps per keyframe, map
update and index rebuild included), timed as bench.py times it (host clock around a synchronised region; the device-event time of the
same region is reported next to it).  bench.py measures the default (PointFusion) only.  The aggregated map
grows by H*W rows per keyframe (~18 M rows at the end of a 60-frame pass), so the 3-D loss's query cost grows through a pass: the
20-step figure and the whole-pass figure are different measurements.

    python tools/icpslam_steps_bench.py --steps 20 --warmup 5          # one JSON line per MODEL.slam value
    python tools/icpslam_steps_bench.py --steps 177 --warmup 5         # one whole pass
    python tools/icpslam_steps_bench.py --slam ICPSLAM --steps 20
"""
import argparse
import contextlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "end-to-end-self-supervised-slam_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def run(slam_name, a):
    import torch
    from e2ehip.synthetic import make_sequence
    from online_adaption import SLAM, default_config
    H, W, L, spk = a.height, a.width, a.seq_len, 3
    cfg = default_config(H, W, L)
    cfg.DEBUG.print_metrics = False
    cfg.DEMO.frame_threshold = 0.05
    cfg.MODEL.slam = slam_name
    seq = make_sequence(L, H, W, seed=1234, step=0.06, scene="plane")
    torch.manual_seed(20241004)          # bench.py NET_SEED: the network initialisation is part of the workload
    with contextlib.redirect_stdout(sys.stderr):
        slam = SLAM(cfg, sequence=seq)
    slam.set_refinement_mode()
    slam.first_iter = True
    sched = slam.keyframe_schedule()
    state = {"i": 0, "rows": 0}

    def run_steps(n):
        while n > 0:
            if state["i"] >= len(sched):
                state["rows"] = max(state["rows"], slam.map.check_capacity())     # end of a pass: one host read per 177 steps
                slam.reset_map()
                state["i"] = 0
            k = min(spk, n)
            nxt = sched[state["i"] + 1] if state["i"] + 1 < len(sched) else None
            slam.refinement(*sched[state["i"]], max_steps=k, next_pair=nxt)
            slam.first_iter = False
            state["i"] += 1
            n -= k

    run_steps(a.warmup)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()             # the value is timed as bench.py times its own: host clock around a synchronised region
    e0.record()
    run_steps(a.steps)
    e1.record()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    ms_events = e0.elapsed_time(e1)
    rows = max(state["rows"], slam.map.check_capacity())
    print(json.dumps({"metric": "online refinement steps/sec", "slam": slam_name, "value": a.steps / (ms * 1e-3), "unit": "steps/s",
                      "ms_per_step": ms / a.steps, "ms_per_step_device_events": ms_events / a.steps, "steps": a.steps, "warmup": a.warmup, "height": H, "width": W, "keyframes": len(sched),
                      "largest_map_rows": rows}), flush=True)
    slam.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slam", default="PointFusion,ICPSLAM")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--seq-len", type=int, default=60)
    a = ap.parse_args()
    for name in filter(None, a.slam.split(",")):
        run(name, a)


if __name__ == "__main__":
    main()
