"""The nearest-neighbour index at the size MODEL.slam: ICPSLAM takes it to: the aggregated map of one whole pass of the benchmark's
480x640 sequence is 60 x 307 200 = 18 432 000 rows (a PointFusion pass ends at 11.8 M; test_knn_grid_equals_brute checks 5.2 M)."""
import contextlib
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_grid_index_equals_brute_force_on_the_map_of_a_whole_icpslam_pass():
    """LOSS.three3d_loss queries this index in every step: the grid search over the map the driver itself built in a whole pass must
    return what the brute force returns, distances and indices bit for bit.  5 700 queries x 18.4 M rows = the pair count of
    test_knn_grid_equals_brute[dense_5m_map] (20 001 x 5.2 M): 60 % a few millimetres off map points, the rest anywhere in (and half a
    metre around) the map's bounding box, one exactly on a map point; cold, image-ordered and warm-started queries."""
    from e2ehip import _lib as L
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    from online_adaption import SLAM, default_config
    H, W, frames = 480, 640, 60
    cfg = default_config(H, W, frames)
    cfg.DEBUG.print_metrics = False
    cfg.MODEL.slam = "ICPSLAM"
    torch.manual_seed(20241004)                                  # the benchmark's network initialisation
    with contextlib.redirect_stdout(sys.stderr):
        slam = SLAM(cfg, sequence=make_sequence(frames, H, W, seed=1234, step=0.06, scene="plane"))
    slam.main()
    M = slam.map.M
    assert M == frames * H * W == 18_432_000
    pts = slam.map.points[:M]
    g = torch.Generator().manual_seed(5)
    n_near, n_far = 3420, 2279
    near = pts[torch.randint(0, M, (n_near,), generator=g).cuda()] + 0.004 * torch.randn(n_near, 3, generator=g).cuda()
    lo, hi = pts.min(0)[0], pts.max(0)[0]
    far = lo - 0.5 + torch.rand(n_far, 3, generator=g).cuda() * (hi - lo + 1.0)
    q = torch.cat([near, far, pts[5:6]], 0).contiguous()
    n1 = q.shape[0]
    index = slam.map.knn_index(H * W)                            # the driver's own index, rebuilt by the last keyframe's map graph
    db, ib = ops.knn1(q, pts.contiguous(), "brute")
    di, ii = ops.knn1(q, index)
    assert torch.equal(di, db) and torch.equal(ii, ib)
    d1, i1 = torch.empty(n1, device="cuda"), torch.empty(n1, dtype=torch.int64, device="cuda")
    index.query(q[:5696].contiguous(), 5696, d1, i1, L.stream(), row_len=64)             # as an 89 x 64 image: 8 x 8 tiles per wave
    assert torch.equal(d1[:5696], db.reshape(-1)[:5696]) and torch.equal(i1[:5696], ib.reshape(-1)[:5696])
    moved = (q[:5696] + 0.003 * torch.randn(5696, 3, generator=g).cuda()).contiguous()   # warm start from the neighbours of nearby points
    dm, im = ops.knn1(moved, pts.contiguous(), "brute")
    index.query(moved, 5696, d1, i1, L.stream(), row_len=64, warm=i1)
    assert torch.equal(d1[:5696], dm.reshape(-1)) and torch.equal(i1[:5696], im.reshape(-1))
    slam.close()
