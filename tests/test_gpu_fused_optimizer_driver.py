"""OPTIMIZATION.optimizer = SGD / RMSprop / Adagrad through the online driver (SLAM.main(): step plan, captured graphs, flat bucket):
the run completes, replaying the captured step equals launching it bit for bit -- under a learning rate that changes between two
keyframes, which the replays must see -- and one optimiser step inside the driver is the float64 update of its own inputs."""
import functools

import pytest
import torch

import fused_optim_cases as C
from oracle import depthnet

pytestmark = pytest.mark.gpu
H, W, FRAMES = 64, 96, 3
CHECKED_STEP = 3                 # the first step of the second keyframe: non-zero state, and the first one under the halved rate


@functools.lru_cache(maxsize=None)
def _sequence():
    from e2ehip.synthetic import make_sequence
    return make_sequence(FRAMES, H, W, seed=11), depthnet.random_state_dict(0)


def _run(kind, graphs, halve, record=None):
    """SLAM.main() over two keyframes; halve: param_groups[0]["lr"] *= 0.5 after the first keyframe, as a scheduler stepped between
    two keyframes would.  record: a list that receives (data, grad, state) before and (data, state) after optimiser step CHECKED_STEP."""
    from online_adaption import SLAM, default_config

    class Run(SLAM):
        def refinement(self, prev, cur, **kw):
            out = super().refinement(prev, cur, **kw)
            if halve and self.first_iter:                   # main() clears first_iter after the first keyframe's refinement returns
                self.optimizer.param_groups[0]["lr"] *= 0.5
            return out

    cfg = default_config(H, W, FRAMES)
    cfg.DEMO.frame_threshold = 0.0
    cfg.OPTIMIZATION.optimizer = kind
    seq, sd = _sequence()
    slam = Run(cfg, sequence=seq, state_dict=sd)
    slam.use_graphs = graphs
    opt = slam.optimizer
    assert type(opt) is C.fused_class(kind)
    lr0 = opt.param_groups[0]["lr"]
    if record is not None:
        inner, calls = opt.step, []

        def step(*a, **k):
            calls.append(1)
            watch = len(calls) - 1 == CHECKED_STEP
            arr = getattr(opt, opt.STATE[0][1])
            if watch:
                record.append((opt.flat.data.clone(), opt.flat.grad.clone(), arr.clone(), opt.param_groups[0]["lr"]))
            out = inner(*a, **k)
            if watch:
                record.append((opt.flat.data.clone(), arr.clone()))
            return out
        opt.step = step
    slam.main()
    torch.cuda.synchronize()
    assert len(slam.log) == 6 and opt.steps_done() == 6 and slam.map.M >= H * W
    assert opt.param_groups[0]["lr"] == (0.5 * lr0 if halve else lr0)
    assert opt._lr.item() == torch.tensor(opt.param_groups[0]["lr"], dtype=torch.float32).item()      # what the last launch read
    out = (torch.stack(slam.log), slam.map.live()[0].clone(), {k: v.detach().clone() for k, v in slam.models["depth"].state_dict().items()})
    slam.close()
    return out


@pytest.mark.parametrize("kind", C.KINDS)
def test_driver_runs_and_graph_replay_is_exact_under_a_changing_rate(kind):
    record = []
    log_g, map_g, sd_g = _run(kind, graphs=True, halve=True)
    log_e, map_e, sd_e = _run(kind, graphs=False, halve=True, record=record)
    assert torch.isfinite(log_g).all()
    assert torch.equal(log_g, log_e) and torch.equal(map_g, map_e)                 # replaying == launching, bit for bit
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), k
    # the same run without the halving differs: the changed rate reached the replayed launches (captured under the old one)
    log_c, map_c, sd_c = _run(kind, graphs=True, halve=False)
    assert torch.equal(log_c[:3], log_g[:3])                                       # identical until the rate changes ...
    assert any(not torch.equal(sd_c[k], sd_g[k]) for k in sd_g)                    # ... and not after
    # one update inside the eager run against the float64 formulas on its own inputs, bounds of the class-level comparison
    (p0, g, s0, lr), (p1, s1) = record
    assert lr == 0.5 * 1e-5 and bool(s0.any()) and bool(g.any())
    pr, sr = C.update64(kind, p0.cpu().double(), g.cpu().double(), s0.cpu().double(), float(torch.tensor(lr, dtype=torch.float32)), **C.HYPER[kind])
    pe, se = C.param_excess(p1, pr), C.state_excess(s1, sr)
    print(f"{kind} driver step {CHECKED_STEP}: parameters at {pe:.3f} of their bound, state at {se:.3f} of its bound")
    assert pe <= 1.0 and se <= 1.0
    assert not torch.equal(p1, p0)
