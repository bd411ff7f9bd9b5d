"""train_depth.Depth_Estimation with MODEL.refinement_mode = False: the network stays in train mode (train_depth.py:246-247) and every
BatchNorm of the ResNet body normalises with batch statistics.  The same run -- indoor network, 64 x 96, two keyframes, Adam -- once on
the native kernels (csrc/bn_train.hip; torch.nn.functional.batch_norm replaced by a function that raises) and once with
E2E_BN_NATIVE=0, the nn.BatchNorm2d module path that was the only one before the kernels existed: losses, counters and the parameters
after the steps agree."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import depthnet

pytestmark = pytest.mark.gpu
H, W = 64, 96
STEPS = 3


def _run():
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation, default_config
    cfg = default_config(H, W, (0, -1), STEPS)
    cfg.DEBUG.print_metrics = False
    cfg.MODEL.refinement_mode = False
    assert cfg.MODEL.depth_network == "indoor" and cfg.OPTIMIZATION.optimizer == "Adam"
    with contextlib.redirect_stdout(io.StringIO()):
        de = Depth_Estimation(cfg, sequence=make_sequence(2, H, W, seed=5), state_dict=depthnet.random_state_dict(0))
        log = de.train()
    m = de.models["depth"]
    assert m.training and m.encoder.encoder.bn1.training
    torch.cuda.synchronize()
    return np.array(log), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


def test_train_mode_run_native_against_the_module_path(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("torch.nn.functional.batch_norm was called on the native train-mode path")
    monkeypatch.delenv("E2E_BN_NATIVE", raising=False)
    with monkeypatch.context() as mp:
        mp.setattr(F, "batch_norm", refuse)
        log_n, sd_n = _run()                                           # must complete
    monkeypatch.setenv("E2E_BN_NATIVE", "0")
    log_m, sd_m = _run()
    assert len(log_n) == len(log_m) and len(log_n) >= STEPS and np.all(np.isfinite(log_n))
    np.testing.assert_allclose(log_n, log_m, rtol=1e-4)
    counters = [k for k in sd_n if k.endswith("num_batches_tracked")]
    assert len(counters) == 20
    start = depthnet.random_state_dict(0)
    for k in counters:
        assert int(sd_n[k]) == int(sd_m[k]) and int(sd_n[k]) > int(start[k]), k
    for k in sd_n:
        if sd_n[k].dtype.is_floating_point:
            assert float((sd_n[k] - sd_m[k]).abs().max()) <= 1e-4 * float(sd_m[k].abs().max()), k
