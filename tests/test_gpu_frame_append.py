"""The aggregation map step (gradslam update_map_aggregate = ICPSLAM._map; FusionMap.append_resident / e2e_frame_append_dev: one fused
kernel from depth / K / pose to map rows) against the existing PointFusion path with matching switched off, the CPU oracle, its own
capacity bound, and its captured form."""
import pytest
import torch

from oracle import pointfusion as opf
from test_gpu_pointfusion_knn import _K, _pose, _scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIGMA = 0.6


def _frames(H, W, seed):
    """Three consecutive frames of a moving camera: ~10 % zero-depth holes in the first and the last, none in the middle one."""
    frames = []
    for f, holes in enumerate((0.1, 0.0, 0.1)):
        d, c = _scene(H, W, seed + f, holes=holes)
        frames.append((c, d, _pose(0.4 * f, 0.7 * f, 0.1 * f, (0.02 * f, 0.01, -0.01 * f))))
    # conditions on the INPUT (not tolerances): an all-valid frame and frames with holes are both covered
    assert int((frames[1][1] == 0).sum()) == 0
    for k in (0, 2):
        frac = float((frames[k][1] == 0).float().mean())
        assert 0.05 < frac < 0.15, frac
    return frames


def aggregate_rows(state, colors, depth, K, pose, sigma=SIGMA):
    """CPU oracle of the aggregation step: the rows of oracle.pointfusion.vertex_normal_maps under the `valid` mask, row-major, appended."""
    maps = opf.vertex_normal_maps(depth, K, pose)
    v = maps["valid"]
    alpha = opf.fusion_alpha(maps["V"], sigma)
    return {"points": torch.cat([state["points"], maps["Vg"][v]], 0), "normals": torch.cat([state["normals"], maps["ng"][v]], 0),
            "colors": torch.cat([state["colors"], colors[v]], 0), "ccounts": torch.cat([state["ccounts"], alpha[v]], 0)}


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


@pytest.mark.parametrize("H,W", [(24, 32), (64, 96), (480, 640)])
def test_append_equals_pointfusion_step_that_never_matches(H, W):
    """dist_th = 0: `|.| < 0` is false for every map point, so step_resident (vertex / normal maps to memory, association, fusion of
    nothing, append) degenerates to plain aggregation -- the fused kernel must give the same map bit for bit."""
    from e2ehip.fusionmap import FusionMap
    K = _K(H, W).to(DEV)
    a, b = FusionMap(3 * H * W, H, W, DEV, dist_th=0.0, sigma=SIGMA), FusionMap(3 * H * W, H, W, DEV, sigma=SIGMA)
    for c, d, pose in _frames(H, W, 40):
        c, d, pose = _dev(c, d, pose)
        a.step_resident(c, d, K, pose)
        b.append_resident(c, d, K, pose)
        assert b._M is None                                  # nothing was read back
    assert torch.equal(a.count.cpu(), b.count.cpu())
    assert 2 * H * W < b.M < 3 * H * W
    for name, x, y in zip(("points", "normals", "colors", "ccounts"), a.live(), b.live()):
        assert torch.equal(x, y), name


def test_append_vs_cpu_oracle():
    from e2ehip.fusionmap import FusionMap
    H, W = 60, 80
    K = _K(H, W)
    m = FusionMap(3 * H * W, H, W, DEV, sigma=SIGMA)
    st = opf.empty_state()
    for c, d, pose in _frames(H, W, 50):
        st = aggregate_rows(st, c, d, K, pose)
        m.append_resident(*_dev(c, d, K, pose))
    P, Nn, C, cc = (t.cpu() for t in m.live())
    assert P.shape[0] == st["points"].shape[0]                # row count exact
    assert torch.equal(C, st["colors"])                       # row order exact: colours are copied, every pixel's is different
    # the bound of test_gpu_pointfusion_knn.py::test_pointfusion_step_tables_bitexact for APPENDED rows (its first frame is a pure append:
    # _assert_state(exact_geometry=True)): positions and normals bit-exact (IEEE +,-,*,/,sqrt), confidences 1e-6 relative (exp)
    assert torch.equal(P, st["points"]) and torch.equal(Nn, st["normals"])
    torch.testing.assert_close(cc, st["ccounts"], rtol=1e-6, atol=0)


def test_append_overflow_is_clamped_flagged_and_writes_nothing_beyond_capacity():
    """Capacity a few rows short of what three frames need: the live size stops at the capacity, the sticky word holds the size that
    was needed, check_capacity() raises, and sentinel rows directly behind the capacity stay untouched (the map arrays are views of
    larger buffers here, so an out-of-range row would land in memory this test owns)."""
    from e2ehip.fusionmap import FusionMap
    H, W = 64, 96
    K = _K(H, W)
    frames = _frames(H, W, 60)
    needed = sum(int((d != 0).sum()) for _, d, _ in frames)
    cap, guard, sentinel = needed - 7, 2 * H * W, -12345.0
    m = FusionMap(cap, H, W, DEV, sigma=SIGMA)
    big = {n: torch.full((cap + guard,) + s, sentinel, device=DEV) for n, s in (("points", (3,)), ("normals", (3,)), ("colors", (3,)), ("ccounts", ()))}
    for n, t in big.items():
        setattr(m, n, t[:cap])
    for c, d, pose in frames:
        m.append_resident(*_dev(c, d, K, pose))
    count = m.count.cpu()
    assert int(count[0]) == cap and int(count[2]) == needed
    for n, t in big.items():
        assert bool((t[cap:] == sentinel).all()), n
        assert not bool((t[:cap] == sentinel).any()), n        # every row below the capacity was written
    with pytest.raises(RuntimeError):
        m.check_capacity()
    # the rows that fit are the first `cap` rows of the unclamped result
    full = FusionMap(3 * H * W, H, W, DEV, sigma=SIGMA)
    for c, d, pose in frames:
        full.append_resident(*_dev(c, d, K, pose))
    for n in big:
        assert torch.equal(big[n][:cap], getattr(full, n)[:cap]), n


def test_append_replays_inside_a_captured_graph():
    """Every launch argument is constant (live size on the device): the call recorded once and replayed twice over the same frame
    buffers gives the rows of two eager calls."""
    from e2ehip.fusionmap import FusionMap
    H, W = 64, 96
    K = _K(H, W).to(DEV)
    frames = _frames(H, W, 70)[:2]
    eager, graphed = FusionMap(3 * H * W, H, W, DEV, sigma=SIGMA), FusionMap(3 * H * W, H, W, DEV, sigma=SIGMA)
    for c, d, pose in frames:
        eager.append_resident(*_dev(c, d), K, *_dev(pose))
    c_buf, d_buf, p_buf = torch.empty(H, W, 3, device=DEV), torch.empty(H, W, device=DEV), torch.empty(4, 4, device=DEV)
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            graphed.append_resident(c_buf, d_buf, K, p_buf)      # recorded, not executed
    cur.wait_stream(side)
    assert int(graphed.count.cpu()[0]) == 0
    for c, d, pose in frames:
        c_buf.copy_(c)
        d_buf.copy_(d)
        p_buf.copy_(pose)
        g.replay()
    torch.cuda.synchronize()
    graphed.mark_updated_on_device(index_current=False)
    assert torch.equal(eager.count.cpu(), graphed.count.cpu()) and graphed.M == eager.M > H * W
    for name, x, y in zip(("points", "normals", "colors", "ccounts"), eager.live(), graphed.live()):
        assert torch.equal(x, y), name
    del g
