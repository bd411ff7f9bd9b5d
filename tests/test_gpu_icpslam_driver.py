"""The online driver with MODEL.slam: ICPSLAM (the reference's other map step, online_adaption.py:110-124: every valid pixel of a fused
frame is appended, no association, no fusion) against an aggregating oracle, its autograd form, the oracle's odometry and the
PointFusion driver with matching switched off."""
import numpy as np
import pytest
import torch

from median_pin import PinnedSLAM, pin
from oracle import depthnet, refine, warp_loss
from oracle import icp as oicp
from test_gpu_frame_append import aggregate_rows

pytestmark = pytest.mark.gpu


class AggregatingRefiner(refine.Refiner):
    """oracle.refine.Refiner whose map step is ICPSLAM's: the rows of vertex_normal_maps under the `valid` mask, row-major."""

    @torch.no_grad()
    def update_map(self, colors, gt_depths, poses, Kc):
        depths = self.predict_depths(colors)
        depths, _ = warp_loss.median_scale(depths, gt_depths)
        f = lambda t: t.float()
        for i in ((0, 1) if self.first_iter else (1,)):
            self.map = aggregate_rows(self.map, f(colors[0, i]), f(depths[i][0, 0]), f(Kc[0]), f(poses[0, i]), self.cfg.sigma)


def _cfg(H, W, L, slam="ICPSLAM"):
    from online_adaption import default_config
    cfg = default_config(H, W, L)
    cfg.DEMO.frame_threshold = 0.0
    cfg.MODEL.slam = slam
    return cfg


def _head40():
    sd = depthnet.random_state_dict(0)
    sd["decoder.decoder.10.conv.weight"] = sd["decoder.decoder.10.conv.weight"] * 40.0      # unique median element (tests/test_gpu_driver.py)
    return sd


def test_model_slam_values():
    from e2ehip.synthetic import make_sequence
    from online_adaption import SLAM
    seq = make_sequence(2, 64, 96, seed=7)
    for name, want in (("ICPSLAM", True), ("PointFusion", False)):
        with SLAM(_cfg(64, 96, 2, name), sequence=seq, state_dict=_head40()) as slam:
            assert slam.aggregate is want
    with pytest.raises(ValueError):
        SLAM(_cfg(64, 96, 2, "KinectFusion"), sequence=seq, state_dict=_head40())


def test_icpslam_two_keyframes_free_running_vs_aggregating_oracle():
    """test_gpu_driver.py::test_two_keyframes_free_running_vs_oracle with MODEL.slam: ICPSLAM on both sides (head x 40, the oracle names
    the median elements): every loss term incl. the 3-D term against the AGGREGATED map, ratio and metrics of all six steps at 1e-4
    relative -- the project's bound for these quantities (metrics: rtol 1e-4 with the atol 1e-6 of the teacher-forced test) -- and the
    map size exactly: predicted depths are never zero, so every fused frame adds H * W rows."""
    from e2ehip.synthetic import make_sequence
    H, W, L = 64, 96, 3
    seq = make_sequence(L, H, W, seed=7)
    colors, gt, K, poses = seq
    sd = _head40()
    ora = AggregatingRefiner(sd, refine.Config())
    recs = []
    for a, b in ((0, 1), (1, 2)):
        recs += ora.refine_pair(colors[:, [a, b]], gt[:, [a, b]], poses[:, [a, b]], K)
    assert ora.map["points"].shape[0] == 3 * H * W and "knn" in recs[3]
    slam = PinnedSLAM(_cfg(H, W, L), sequence=seq, state_dict=sd)
    slam.median_elements = [pin(r["median_indices"], "cuda") for r in recs]
    slam.main()
    log = torch.stack(slam.log).double().numpy()
    assert log.shape[0] == 6
    for key, got in (("photometric", log[:, 1]), ("reg", log[:, 2]), ("ratio", log[:, 3]), ("loss", log[:, 0])):
        ref = np.array([r[key] for r in recs])
        print(f"[icpslam free run] {key}: worst relative difference {np.abs(got - ref).max() / np.abs(ref).max():.3e}")
    ref3 = np.array([r["knn"] for r in recs[3:]])
    print(f"[icpslam free run] knn: relative differences {(np.abs(log[3:, 11] - ref3) / ref3).tolist()}")
    refm = np.array([r["metrics"] for r in recs])
    print(f"[icpslam free run] metrics: worst relative difference {(np.abs(log[:, 4:11] - refm) / np.maximum(np.abs(refm), 1e-30)).max():.3e}")
    np.testing.assert_allclose(log[:, 1], [r["photometric"] for r in recs], rtol=1e-4)
    np.testing.assert_allclose(log[:, 2], [r["reg"] for r in recs], rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(log[:, 3], [r["ratio"] for r in recs], rtol=1e-4)
    np.testing.assert_allclose(log[3:, 11], ref3, rtol=1e-4)
    np.testing.assert_allclose(log[:, 0], [r["loss"] for r in recs], rtol=1e-4)
    np.testing.assert_allclose(log[:, 4:11], refm, rtol=1e-4, atol=1e-6)
    assert slam.map.M == (len(slam.keyframe_schedule()) + 1) * H * W == 3 * H * W
    assert any(isinstance(k, tuple) and k[0] == "map" and k[3] is True for k in slam.step_plan._graphs)      # the aggregating map graph
    slam.close()


def _run_two_keyframes(mode, median_elements=None):
    from e2ehip.synthetic import make_sequence
    H, W, L = 64, 96, 3
    slam = PinnedSLAM(_cfg(H, W, L), sequence=make_sequence(L, H, W, seed=11), state_dict=_head40())
    slam.use_graphs = mode == "graphs"
    slam.median_elements = median_elements
    slam.median_elements_log = [] if median_elements is None else None
    slam.set_refinement_mode()
    slam.first_iter = True
    for prev, cur in slam.keyframe_schedule():
        (slam.refinement_autograd if mode == "autograd" else slam.refinement)(prev, cur)
        slam.first_iter = False
    torch.cuda.synchronize()
    out = (torch.stack(slam.log), [t.clone() for t in slam.map.live()], {k: v.detach().clone() for k, v in slam.models["depth"].state_dict().items()},
           slam.median_elements_log)
    slam.close()
    return out


def test_icpslam_launch_plan_equals_autograd_path_and_graph_replay_is_exact():
    """test_gpu_driver.py::test_launch_plan_equals_autograd_path_and_graph_replay_is_exact under MODEL.slam: ICPSLAM, same bounds: the
    captured form (map step incl. e2e_frame_append_dev replayed) equals the eager form bit for bit, and the autograd form
    (SLAM._update_map -> append_resident) to a few fp32 ulps."""
    log_g, map_g, sd_g, elems = _run_two_keyframes("graphs")
    assert len(elems) == 6 and all(e.numel() >= 1 for e in elems)
    log_e, map_e, sd_e, _ = _run_two_keyframes("eager", elems)
    log_a, map_a, sd_a, _ = _run_two_keyframes("autograd", elems)
    assert torch.equal(log_g, log_e)
    for x, y in zip(map_g, map_e):
        assert torch.equal(x, y)                                 # replaying == launching, bit for bit
    for k in sd_g:
        assert torch.equal(sd_g[k], sd_e[k]), k
    cont = [c for c in range(log_g.shape[1]) if c not in (8, 9, 10)]
    np.testing.assert_allclose(log_g[:, cont].numpy(), log_a[:, cont].numpy(), rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(log_g[:, 8:11].numpy(), log_a[:, 8:11].numpy(), rtol=0, atol=2.5 / (64 * 96))
    assert map_g[0].shape == map_a[0].shape == (3 * 64 * 96, 3)
    torch.testing.assert_close(map_g[0], map_a[0], rtol=5e-5, atol=5e-6)
    assert torch.equal(map_g[2], map_a[2])                       # colours: the same pixels in the same order
    for k in sd_g:
        if sd_g[k].dtype.is_floating_point:
            torch.testing.assert_close(sd_g[k], sd_a[k], rtol=0, atol=2.5e-5, msg=k)


def test_icpslam_gradicp_poses_vs_oracle_on_the_aggregated_map():
    """odom: gradicp + ICPSLAM on the launch plan: each keyframe's pose estimate (ResidentOdometry inside the captured map step) against
    oracle.icp.frame_to_model run on the SAME inputs -- the aggregated map as it stood before the frame, the driver's own predicted
    depth, the previous keyframe's dataset pose -- at the 2e-5 of test_gpu_icp.py::test_resident_odometry_equals_host_loop_and_oracle;
    and the frame is appended with the ESTIMATED pose (rows bit-exact against the oracle's rows for that pose)."""
    from e2ehip.synthetic import make_sequence
    from online_adaption import SLAM
    H, W, L = 64, 96, 3
    seq = make_sequence(L, H, W, seed=3, step=0.03, noise=0.0, scene="corner")
    cfg = _cfg(H, W, L)
    cfg.MODEL.odom = "gradicp"
    cfg.DEBUG.print_metrics = False
    slam = SLAM(cfg, sequence=seq, state_dict=_head40())
    slam.set_refinement_mode()
    slam.first_iter = True
    K = seq[2][0, 0]
    sched = slam.keyframe_schedule()
    assert sched == [(0, 1), (1, 2)]
    rows_before = 0
    for i, (prev, cur) in enumerate(sched):
        slam.refinement(prev, cur, next_pair=sched[i + 1] if i + 1 < len(sched) else None)
        slam.first_iter = False
        first = i == 0
        P_gpu = slam.estimated_poses[-1][0].cpu()
        depth = slam.step_plan.depth[1, 0].cpu()                 # the map step's own depth of the new keyframe (predict_depths)
        pts, nrm, col, _ = (t.cpu() for t in slam.map.live())
        known = rows_before + (H * W if first else 0)             # map the odometry saw: everything but this keyframe's frame
        assert pts.shape[0] == known + H * W
        P_ref, tr_ref = oicp.frame_to_model(pts[:known], nrm[:known], depth, K, seq[3][0, prev], mode="gradicp", numiters=cfg.MODEL.numiters)
        its, tr, ntgt, nact = slam._odo.check()
        print(f"[icpslam gradicp] keyframe {i}: |P - P_ref| max {np.abs(P_gpu.numpy() - P_ref).max():.3e}, iterations {its} / {len(tr_ref)}, targets {ntgt}")
        np.testing.assert_allclose(P_gpu.numpy(), P_ref, atol=2e-5, rtol=0)
        want = aggregate_rows({"points": pts[:0], "normals": nrm[:0], "colors": col[:0], "ccounts": torch.zeros(0)}, seq[0][0, cur], depth, K, P_gpu,
                              cfg.MODEL.sigma)
        assert torch.equal(pts[known:], want["points"]) and torch.equal(nrm[known:], want["normals"]) and torch.equal(col[known:], want["colors"])
        rows_before = pts.shape[0]
    assert any(isinstance(k, tuple) and k[0] == "map_odom" and k[4] is True for k in slam.step_plan._graphs)
    slam.close()


def test_icpslam_gradicp_autograd_form_poses_vs_oracle():
    """The same through SLAM.refinement_autograd (SLAM._update_map: host-driven icp.frame_to_model against the aggregated map, then
    append_resident with the estimated pose): poses against oracle.icp.frame_to_model on the same inputs at the 2e-5 of
    test_gpu_icp.py::test_frame_to_model_matches_oracle_and_ground_truth, appended rows bit-exact for that pose."""
    from e2ehip.synthetic import make_sequence
    from online_adaption import SLAM
    H, W, L = 64, 96, 3
    seq = make_sequence(L, H, W, seed=3, step=0.03, noise=0.0, scene="corner")
    cfg = _cfg(H, W, L)
    cfg.MODEL.odom = "gradicp"
    cfg.DEBUG.print_metrics = False
    slam = SLAM(cfg, sequence=seq, state_dict=_head40())
    slam.set_refinement_mode()
    slam.first_iter = True
    K = seq[2][0, 0]
    seen, inner = [], slam._update_map

    def recording_update_map(rgb_prev, rgb_cur, depth, pose_prev, pose_cur):
        seen.append(depth[1, 0].cpu().clone())                   # the depth the map step is given
        return inner(rgb_prev, rgb_cur, depth, pose_prev, pose_cur)
    slam._update_map = recording_update_map
    rows_before = 0
    for i, (prev, cur) in enumerate(slam.keyframe_schedule()):
        slam.refinement_autograd(prev, cur)
        slam.first_iter = False
        P_gpu, depth = slam.estimated_poses[-1][0].cpu(), seen[-1]
        pts, nrm, col, _ = (t.cpu() for t in slam.map.live())
        known = rows_before + (H * W if i == 0 else 0)
        assert pts.shape[0] == known + H * W
        P_ref, _ = oicp.frame_to_model(pts[:known], nrm[:known], depth, K, seq[3][0, prev], mode="gradicp", numiters=cfg.MODEL.numiters)
        print(f"[icpslam gradicp, autograd form] keyframe {i}: |P - P_ref| max {np.abs(P_gpu.numpy() - P_ref).max():.3e}")
        np.testing.assert_allclose(P_gpu.numpy(), P_ref, atol=2e-5, rtol=0)
        want = aggregate_rows({"points": pts[:0], "normals": nrm[:0], "colors": col[:0], "ccounts": torch.zeros(0)}, seq[0][0, cur], depth, K, P_gpu,
                              cfg.MODEL.sigma)
        assert torch.equal(pts[known:], want["points"]) and torch.equal(nrm[known:], want["normals"]) and torch.equal(col[known:], want["colors"])
        rows_before = pts.shape[0]
    assert len(seen) == 2 and slam.step_plan is None             # the launch plan was never built: this was the autograd form
    slam.close()


def test_icpslam_map_equals_pointfusion_driver_that_never_matches_480x640():
    """One 480x640 keyframe pair through the launch plan: the ICPSLAM driver's map rows equal, bit for bit, those of the PointFusion
    driver with dist_th = 0 (nothing ever matches: its map step degenerates to aggregation through the unfused launches).  The first
    keyframe has no 3-D term, so both runs see the same network in every step."""
    from e2ehip.synthetic import make_sequence
    from online_adaption import SLAM
    H, W, L = 480, 640, 2
    seq = make_sequence(L, H, W, seed=7)
    maps = {}
    for name in ("ICPSLAM", "PointFusion"):
        cfg = _cfg(H, W, L, name)
        cfg.MODEL.dist_th = 0.0
        cfg.DEBUG.print_metrics = False
        slam = SLAM(cfg, sequence=seq, state_dict=_head40())
        slam.main()
        maps[name] = ([t.clone() for t in slam.map.live()], slam.map.count.cpu())
        slam.close()
    assert torch.equal(maps["ICPSLAM"][1], maps["PointFusion"][1]) and int(maps["ICPSLAM"][1][0]) == 2 * H * W
    for n, x, y in zip(("points", "normals", "colors", "ccounts"), maps["ICPSLAM"][0], maps["PointFusion"][0]):
        assert torch.equal(x, y), n
