"""Host only: the cases of tests/multiscale_loss_ref.py, which tests/test_gpu_multiscale_loss.py holds ops.warp_photometric_multiscale against.

  - every case is admitted: on none of its scales does the rule of tests/warp_pose_ref.py / tests/warp_window_ref.py exclude a pixel;
  - the window form's selection is not trivial on any scale: an identity candidate wins somewhere, and each source's reprojection map;
  - the loss is the mean of the per-scale losses, every scale's disparity and every pose gets a gradient, and the coarse scales' gradients are
    not a rounding of the finest one's (each scale has its own disparity draw)."""
import pytest
import torch

import disp_pyramid_ref as DP
import multiscale_loss_ref as M
import warp_window_ref as WW


@pytest.mark.parametrize("B,mode", M.CASES)
def test_case_is_admitted(B, mode):
    c = M.case(B, mode)
    assert c["excluded"] == 0, f"{c['excluded']} pixels would have to be excluded"
    assert torch.isclose(c["loss"], c["per_scale"].mean(), rtol=1e-15, atol=0) and c["per_scale"].shape == (len(M.SHAPES),)
    assert sorted(c["g_disp"]) == list(range(len(M.SHAPES)))
    for k, g in c["g_disp"].items():
        assert g.shape == (B, 1, *M.SHAPES[k]) and float(g.abs().max()) > 0
    assert len(c["g_T"]) == mode[0] and all(float(g.abs().max()) > 0 for g in c["g_T"])


@pytest.mark.parametrize("B", (1, 2))
def test_window_selection_is_not_trivial(B):
    s = M.scene(B)
    depth = DP.pyramid_depth(s["disps"], M.SIZE, *M.LIMITS, M.SCALE)
    for k in range(len(M.SHAPES)):
        ev, _ = M.scale_eval(s, depth[k], M.WINDOW)
        assert WW.both_winners({"mode": M.WINDOW, WW.F64: ev}), k


def test_disparities_stay_inside_the_range_the_bounds_assume():
    for B in (1, 2):
        for d in M.scene(B)["disps"].values():
            assert float(d.min()) >= DP.D_LO and float(d.max()) <= DP.D_HI


def test_ops_refuse_bad_arguments_before_any_launch():
    from e2ehip import ops
    d = [torch.rand(2, 1, 8, 16), torch.rand(2, 1, 4, 8)]
    for bad, match in (([], "1 to 4 scales"), (d * 3, "1 to 4 scales"), ([d[0][:, 0]], r"expected \(B,1,h,w\)"), ([torch.rand(2, 2, 8, 16)], r"expected \(B,1,h,w\)"),
                       ([d[0], d[1][:1]], r"expected \(2,1,h,w\)"), ([torch.rand(2, 1, 9, 16)], "does not fit the full size")):
        with pytest.raises(ValueError, match=match):
            ops.disp_pyramid_depth(bad, (8, 16), 0.1, 80.0)
    for limits in ((0.0, 80.0), (80.0, 0.1), (1.0, 1.0)):
        with pytest.raises(ValueError, match="0 < min_depth < max_depth"):
            ops.disp_pyramid_depth(d, (8, 16), *limits)
    frames, mats = torch.rand(2, 3, 8, 16), torch.eye(4).expand(2, 4, 4)
    with pytest.raises(ValueError, match="1 or 2 source frames and as many poses"):
        ops.warp_photometric_multiscale(d, [frames], frames, mats, mats, [mats, mats], 0.1, 80.0)
    with pytest.raises(ValueError, match="target_frame"):
        ops.warp_photometric_multiscale(d, [frames], frames[:, :1], mats, mats, [mats], 0.1, 80.0)
    with pytest.raises(TypeError):                                             # geometric=True is not offered
        ops.warp_photometric_multiscale(d, [frames], frames, mats, mats, [mats], 0.1, 80.0, geometric=True)
