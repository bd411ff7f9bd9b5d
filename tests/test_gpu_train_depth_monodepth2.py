"""train_depth.Depth_Estimation with MODEL.depth_network: monodepth2 (ResnetEncoder + DepthDecoder, sigmoid disparity, depth through
convert_disp_to_depth times the fixed scale) on the GPU against the oracle's restatement of the harness (oracle/train_depth.py through
disp_head_ref.Monodepth2Trainer), under the tolerance tests/test_gpu_train_depth.py uses for the same harness; load_model(); the
reference's ValueError for an unknown network.  Smoothness stays off: the oracle harness feeds its losses the scaled disparity."""
import contextlib
import io

import numpy as np
import pytest
import torch

import disp_head_ref as R
from oracle import depthnet
from oracle import train_depth as otd

pytestmark = pytest.mark.gpu
H, W = 64, 96


def _config(frames, steps, cfg_mod=lambda c: None):
    from train_depth import default_config
    cfg = default_config(H, W, frames, steps)
    cfg.DEBUG.print_metrics = False
    cfg.MODEL.depth_network = "monodepth2"
    cfg_mod(cfg)
    return cfg


def _run(cfg, seq, state_dict):
    from train_depth import Depth_Estimation
    de = Depth_Estimation(cfg, sequence=seq, state_dict=state_dict)
    with contextlib.redirect_stdout(io.StringIO()):
        log = de.train()
    return np.array(log), de


def _oracle(frames, steps, seq, sd, regulariser):
    c = otd.Config()
    c.frames, c.refinement_steps, c.dual_disparity, c.depth_regularizer = tuple(frames), steps, False, regulariser
    colors, gt, K, poses = seq
    return np.array([r["loss"] for r in R.Monodepth2Trainer(sd, c).train_batch(colors, gt, poses, K)])


@pytest.mark.parametrize("regulariser,scales", [(False, [0]), (True, [0, 1, 2, 3])])
@pytest.mark.parametrize("frames", [(0, -1), (0, 1)])
def test_loss_trajectory_vs_oracle(frames, regulariser, scales):
    """three refinement steps; with the depth regulariser the decoder also carries (and evaluates) the three heads nothing reads"""
    from e2ehip.synthetic import make_sequence

    def mod(c):
        c.LOSS.depth_regularizer, c.DATA.scales = regulariser, scales
    seq = make_sequence(2, H, W, seed=5)
    sd = depthnet.random_state_dict(0)
    log, de = _run(_config(frames, 3, mod), seq, R.split_state_dict(sd, scales))
    assert sorted(de.models) == ["GT_SLAM", "SLAM", "depth_decoder", "depth_encoder"]
    assert len(de.train_params) == len(list(de.models["depth_encoder"].parameters())) + len(list(de.models["depth_decoder"].parameters()))
    want = _oracle(frames, 3, seq, sd, regulariser)
    print("monodepth2 driver", frames, "regulariser" if regulariser else "", log, want, np.abs(log / want - 1).max())
    np.testing.assert_allclose(log, want, rtol=1e-4)


def test_load_model_reads_the_two_files_and_skips_foreign_keys(tmp_path):
    from e2ehip.synthetic import make_sequence
    seq = make_sequence(2, H, W, seed=5)
    parts = R.split_state_dict(depthnet.random_state_dict(0), [0])
    torch.save({**parts["depth_encoder"], "height": torch.tensor(192), "width": torch.tensor(640)}, tmp_path / "depth_encoder.pth")
    torch.save({**parts["depth_decoder"], "use_stereo": torch.tensor(0), "decoder.99.conv.weight": torch.zeros(1)}, tmp_path / "depth_decoder.pth")

    def mod(c):
        c.MODEL.use_pretrained_models, c.MODEL.load_depth_path = True, str(tmp_path)
    cfg = _config((0, -1), 1, mod)
    assert cfg.MODEL.pretrained_models_list == ["depth_encoder", "depth_decoder"]
    loaded, _ = _run(cfg, seq, None)
    direct, _ = _run(_config((0, -1), 1), seq, parts)
    np.testing.assert_allclose(loaded[0], direct[0], rtol=1e-6)


def test_unknown_depth_network_is_the_references_value_error():
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation

    def mod(c):
        c.MODEL.depth_network = "outdoor"
    with pytest.raises(ValueError, match="not a valid depth network option"), contextlib.redirect_stdout(io.StringIO()):
        Depth_Estimation(_config((0, -1), 1, mod), sequence=make_sequence(2, H, W, seed=5))
