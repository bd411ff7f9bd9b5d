"""Host-side reference of the K = 1 nearest-neighbour contract (tests/test_gpu_map_contracts.py): a chunked numpy brute force that evaluates
((dx*dx + dy*dy) + dz*dz) in np.float32 -- separate IEEE operations, no fused multiply-add -- and lets the first minimum win (np.argmin),
which is what include/e2eslam.h promises bit for bit.  It needs no compiled oracle and shares nothing with the code under test.
float64_check then states the result without reference to any fp32 order: the reported neighbour's float64 distance is within fp32
rounding of the true float64 minimum.  knn1_bwd / knn1_bwd_ref are the float64 gradients."""
import numpy as np

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24


def brute(p1, p2, chunk=2048):
    """p1 (n1,3), p2 (n2,3) float32 -> (dists float32 (n1,), idx int64 (n1,))"""
    p1, p2 = np.ascontiguousarray(p1, F32).reshape(-1, 3), np.ascontiguousarray(p2, F32).reshape(-1, 3)
    n1 = p1.shape[0]
    dists, idx = np.empty(n1, F32), np.empty(n1, np.int64)
    qx, qy, qz = (np.ascontiguousarray(p2[:, c])[None, :] for c in range(3))
    step = max(1, min(chunk, (1 << 24) // max(1, p2.shape[0])))
    for s in range(0, n1, step):
        a = p1[s:s + step]
        dx, dy, dz = a[:, 0:1] - qx, a[:, 1:2] - qy, a[:, 2:3] - qz
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == F32
        j = np.argmin(d, axis=1)                              # the first minimum
        idx[s:s + step] = j
        dists[s:s + step] = d[np.arange(a.shape[0]), j]
    return dists, idx


def float64_check(p1, p2, idx, sel=None, chunk=512):
    """-> the largest (d64(reported neighbour) - min64) / bound over the queries `sel` (default all), where the bound is fp32 rounding of
    the distance: each difference of two fp32 numbers is exact or rounded once (u32 relative), each square once, each sum once -- an
    fp32 distance is within 6 u32 of its float64 value, so the neighbour that wins in fp32 is within 12 u32 (relative) of the true
    minimum; 16 u32 d + the smallest fp32 number is the bound.  <= 1 passes."""
    p1, p2 = np.asarray(p1, F64).reshape(-1, 3), np.asarray(p2, F64).reshape(-1, 3)
    sel = np.arange(p1.shape[0]) if sel is None else np.asarray(sel)
    worst = 0.0
    for s in range(0, sel.size, chunk):
        q = sel[s:s + chunk]
        d = sum((p1[q][:, c:c + 1] - p2[None, :, c]) ** 2 for c in range(3))
        best = d.min(1)
        got = ((p1[q] - p2[idx[q]]) ** 2).sum(-1)
        worst = max(worst, float(((got - best) / (16 * U32 * got + 1e-45)).max()))
    return worst


def knn1_bwd(g, p1, p2, idx):
    g, p1, p2 = np.asarray(g, F64), np.asarray(p1, F64), np.asarray(p2, F64)
    return 2.0 * g[:, None] * (p1 - p2[idx])


def knn1_bwd_ref(g, p1, p2, idx):
    """-> (float64 scatter sum (n2,3), the same formula in fp32 with an fp32 running sum in query order, collisions per reference point)"""
    n2 = np.asarray(p2).shape[0]
    out = np.zeros((n2, 3))
    np.add.at(out, idx, -knn1_bwd(g, p1, p2, idx))
    g32, a, b = np.asarray(g, F32), np.asarray(p1, F32), np.asarray(p2, F32)
    v32 = (F32(-2.0) * g32)[:, None] * (a - b[idx])
    o32 = np.zeros((n2, 3), F32)
    np.add.at(o32, idx, v32)
    return out, o32, np.bincount(idx, minlength=n2)
