"""Case generators and float64 / extended-precision references for the contract modules of the SLAM adjoint side:
tests/test_gpu_pose_grad_contracts.py (csrc/pose_grad.hip) and tests/test_gpu_map_grad_contracts.py (csrc/pointfusion_grad.hip,
csrc/normal_maps_grad.hip).  TEST INFRASTRUCTURE ONLY: nothing here imports the GPU library; tests/test_slam_grad_contract_inputs.py
proves on the CPU that every case is what it claims to be.

The sizes of the cases are chosen against the kernels' staging constants (NT_TILE, NT_LONG, PG_MAX_PARTS, CP_BLOCK, the grid caps),
which hip_constants() reads out of the sources: a retune fails the host test, not silently the coverage."""
import functools
import os
import re

import numpy as np
import torch

import icp_grad_ref as I
import slam_chain_grad_ref as C
from oracle import warp_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "end-to-end-self-supervised-slam_amd", "csrc")
F64 = torch.float64


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def hip_constants():
    """The staging constants of the three sources, as the sources define them."""
    def num(text, pattern):
        m = re.search(pattern, text, re.M)
        assert m, f"the sources no longer match {pattern!r}"
        return int(m.group(1))

    pose, pf, pfg, nmg = _read("pose_grad.hip"), _read("pf_workspace.h"), _read("pointfusion_grad.hip"), _read("normal_maps_grad.hip")
    assert re.search(r"^#define\s+NT_TILE\s+\(PG_T\s*\*\s*NT_ITEMS\)", pose, re.M) and re.search(r"^#define\s+CP_BLOCK\s+\(PF_T\s*\*\s*CP_ITEMS\)", pf, re.M)
    c = dict(PG_T=num(pose, r"^#define\s+PG_T\s+(\d+)\b"), PG_MAX_PARTS=num(pose, r"^#define\s+PG_MAX_PARTS\s+(\d+)\b"),
             PG_NSUM=num(pose, r"^#define\s+PG_NSUM\s+(\d+)\b"), NT_ITEMS=num(pose, r"^#define\s+NT_ITEMS\s+(\d+)\b"),
             NT_LONG=num(pose, r"^#define\s+NT_LONG\s+(\d+)\b"), NT_LONG_GRID=num(pose, r"longs\s*>\s*(\d+)\s*\?\s*\1\s*:\s*longs"),
             NT_SHORT_GRID=num(pose, r"tblocks\s*>\s*(\d+)\s*\?\s*\1\s*:\s*tblocks"),
             PF_T=num(pf, r"^#define\s+PF_T\s+(\d+)\b"), CP_ITEMS=num(pf, r"^#define\s+CP_ITEMS\s+(\d+)\b"),
             PFG_GRID=num(pfg, r"pfg_grid\(int64_t n, int cap = (\d+)\)"), NM_GRID=num(nmg, r"blocks\s*>\s*(\d+)\s*\?\s*\1\s*:\s*blocks"))
    c["NT_TILE"] = c["PG_T"] * c["NT_ITEMS"]
    c["CP_BLOCK"] = c["PF_T"] * c["CP_ITEMS"]
    return c


# the distance threshold's edge, as tests/test_gpu_icp_contracts.py states it for the forward (the host test asserts they are the same)
EDGE = np.float32(0.0625)      # dist_thresh 0.25 squared, exact in float32
SPECIAL = (EDGE, np.nextafter(EDGE, np.float32(0)), np.nextafter(EDGE, np.float32(1)), np.float32("nan"), np.float32("inf"))
SPECIAL_KEPT = (False, True, False, False, False)
NE_BOUND = 1e-13               # x sum |terms|, as the ICP module's: float64 chains of a few dozen additions, margin for the order of the products
OUT_OF_RANGE = (-1, 0, 2 ** 32, -(2 ** 32))          # (0: + n_tgt); the last two are in range for whoever keeps only the low 32 bits


def groups(n, block=256, trip=65536):
    """The row ranges whose loss a summed output must show: the last row, every workgroup's rows, every whole grid-stride trip."""
    out = [(n - 1, n)] + [(a, min(a + block, n)) for a in range(0, n, block)]
    if n > trip:
        out += [(a, min(a + trip, n)) for a in range(0, n, trip)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1a. e2e_transform_points_bwd_t
# ---------------------------------------------------------------------------------------------------------------------------------------
TP_SIZES = {1: "smallest", 63: "partial wave", 256: "one partial", 257: "two partials", 16384: "64 partials: one trip of the second stage",
            16385: "65 partials: second trip, lane 0 only", 65536: "256 partials: the clamp, not yet a stride", 65537: "grid-stride, one row",
            70001: "grid-stride, ragged"}


@functools.lru_cache(maxsize=None)
def transform_case(n):
    """g, points (n,3) float32, offset from zero so that a lost row cannot cancel; terms (n,12) float64 (exact products of float32);
    want (12,) extended precision, scale (12,) = sum |terms|."""
    gen = torch.Generator().manual_seed(100 + n)
    g, p = torch.randn(n, 3, generator=gen) + 0.5, torch.randn(n, 3, generator=gen) + 0.5
    g64, p64 = g.double().numpy(), p.double().numpy()
    terms = np.concatenate([g64[:, :, None] * p64[:, None, :], g64[:, :, None]], 2).reshape(n, 12)        # row-major 3x4: [g p^T | g]
    ext = terms.astype(np.longdouble)
    return dict(n=n, g=g, points=p, terms=terms, want=ext.sum(0), scale=np.abs(ext).sum(0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1b. e2e_icp_normal_equations_bwd
# ---------------------------------------------------------------------------------------------------------------------------------------
NEB_SIZES = (1, 63, 256, 257, 65536, 70001)
NEB_TARGETS = (1, 7, 3000)
NEB_BOUND = 4.5e-7             # of the largest entry: the bound tests/test_gpu_pose_grad.py carries for this quantity


@functools.lru_cache(maxsize=None)
def ne_bwd_case(n, nt):
    """The forward contract's case (sources, targets, repeated indices, SPECIAL distances at the head and in the last workgroup) plus
    rows whose index is outside [0, nt).  keep_thresh / keep_all: the rows a threshold of 0.25 / a negative threshold keeps."""
    rng = np.random.default_rng(7000 * nt + n)
    src, tgt = rng.uniform(-2, 2, (n, 3)).astype(np.float32), rng.uniform(-2, 2, (nt, 3)).astype(np.float32)
    nrm = rng.standard_normal((nt, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    idx = rng.integers(0, nt, n).astype(np.int64)
    idx[-1] = nt - 1
    if n > 1:
        idx[0] = 0
    if n > 3:
        idx[2] = idx[1]
    dists = rng.uniform(0, 0.125, n).astype(np.float32)       # about half below 0.0625
    special, outside = {}, {}
    for k, v in enumerate(SPECIAL):
        for pos in ((k,) if n < 10 else (k, n - 1 - k)):
            if pos < n:
                dists[pos] = v
                special[pos] = SPECIAL_KEPT[k]
    if n >= 63:
        for k, v in enumerate(OUT_OF_RANGE):                  # next to the head and in the last workgroup; their distances pass the threshold
            for pos in (10 + k, n - 10 - k):
                idx[pos] = v + nt if v == 0 else v
                dists[pos] = np.float32(0.01)
                outside[pos] = int(idx[pos])
    inside = (idx >= 0) & (idx < nt)
    with np.errstate(invalid="ignore"):
        below = dists < EDGE
    adj = torch.from_numpy(rng.standard_normal(28))
    prior = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32))
    return dict(n=n, nt=nt, src=torch.from_numpy(src), tgt=torch.from_numpy(tgt), nrm=torch.from_numpy(nrm), idx=torch.from_numpy(idx),
                dists=torch.from_numpy(dists), adj=adj, prior=prior, special=special, outside=outside,
                keep_thresh=torch.from_numpy(below & inside), keep_all=torch.from_numpy(inside))


def ne_bwd_reference(case, keep):
    """float64 autograd of icp_grad_ref.sums over the kept rows -> (n,3)."""
    s64 = case["src"].double().requires_grad_(True)
    if not bool(keep.any()):
        return torch.zeros_like(s64).detach()
    AtA, Atb, err = I.sums(s64, case["tgt"].double(), case["nrm"].double(), case["idx"].clamp(0, case["nt"] - 1), keep)
    packed = torch.stack([AtA[r, c] for r in range(6) for c in range(r, 6)])
    adj = case["adj"]
    (want,) = torch.autograd.grad((adj[:21] * packed).sum() + (adj[21:27] * Atb).sum() + adj[27] * err, s64)
    return want


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1c. e2e_icp_normal_equations_bwd_tgt
# ---------------------------------------------------------------------------------------------------------------------------------------
NAMED_LENGTHS = (0, 1, 2, 63, 64, 65, 66, 128, 129, 700)      # NT_LONG = 64: a thread's longest segment, a wave's shortest, wave trips of 2 and 2 + 1
HUGE = 257 * 4096 + 5            # 258 tiles: k_nt_scan_tiles carries into its second chunk of 256
T4 = 4096                      # NT_TILE
TGT_CASES = {                  # named: {target: the number of kept rows that name it}, the ten NAMED_LENGTHS each once
    "lengths": dict(nt=300, named={0: 0, 1: 1, 2: 2, 50: 63, 51: 64, 52: 65, 53: 66, 100: 128, 101: 129, 299: 700}, random_rows=2000),
    "many_long": dict(nt=300, every=70),
    "nt4095": dict(nt=4095, named={4094: 65, 4093: 64, 0: 700, 10: 0, 2000: 1, 1: 2, 4000: 63, 3000: 66, 77: 128, 2048: 129}, random_rows=3000),
    "nt4096": dict(nt=4096, named={4095: 65, 4094: 64, 0: 700, 10: 0, 2000: 1, 1: 2, 4000: 63, 3000: 66, 77: 128, 2048: 129}, random_rows=3000),
    "nt4097": dict(nt=4097, named={4095: 64, 4096: 65, 4094: 129, 0: 700, 10: 0, 2000: 1, 1: 2, 4000: 63, 3000: 66, 77: 128}, random_rows=3000),
    "nt8193": dict(nt=8193, named={4095: 64, 4096: 65, 4097: 129, 8192: 700, 4094: 66, 10: 0, 6000: 1, 1: 2, 2048: 63, 0: 128}, random_rows=3000),
    "stride": dict(nt=9000, named={4095: 64, 4096: 65, 4097: 129, 8999: 700, 4094: 66, 10: 0, 6000: 1, 1: 2, 2048: 63, 0: 128}, n=70001),
    "huge": dict(nt=HUGE, named={0: 0, T4 - 1: 64, T4: 65, 255 * T4 - 1: 63, 255 * T4: 66, 256 * T4 - 1: 129, 256 * T4: 700, 256 * T4 + 1: 2,
                                 257 * T4: 128, HUGE - 1: 1}, random_rows=3000),
}
TGT_THRESH = 0.25


@functools.lru_cache(maxsize=None)
def tgt_case(name):
    """named[j] kept rows name target j; `every`: each target is named by exactly that many; the other
    kept rows name random other targets.  On top (but for `every`) come rows that must contribute nothing: distances at and beyond the
    threshold's edge, NaN, inf -- some of them naming the targets of length 0, 64 and 65 -- and indices outside [0, nt).  The source rows
    are then permuted, so the fill order is arbitrary, and the last row is a kept one."""
    spec = TGT_CASES[name]
    nt = spec["nt"]
    rng = np.random.default_rng(sorted(TGT_CASES).index(name) + 31)
    lengths = {}
    if "every" in spec:
        kept_idx = np.repeat(np.arange(nt, dtype=np.int64), spec["every"])
        drop_idx, drop_d = np.zeros(0, np.int64), np.zeros(0, np.float32)
    else:
        lengths = dict(spec["named"])
        assert sorted(lengths.values()) == list(NAMED_LENGTHS) and all(0 <= j < nt for j in lengths)
        named_rows = np.concatenate([np.full(l, j, np.int64) for j, l in lengths.items()])
        by_len = {l: j for j, l in lengths.items()}
        bad = [v for v, kept in zip(SPECIAL, SPECIAL_KEPT) if not kept]
        drop_idx = np.array([by_len[0], by_len[64], by_len[65], by_len[63]] * len(bad) + [v + nt if v == 0 else v for v in OUT_OF_RANGE] * 2, np.int64)
        drop_d = np.array([v for v in bad for _ in range(4)] + [0.01] * (2 * len(OUT_OF_RANGE)), np.float32)
        n_random = spec["random_rows"] if "random_rows" in spec else spec["n"] - named_rows.size - drop_idx.size
        others = np.setdiff1d(np.arange(nt, dtype=np.int64), np.fromiter(lengths, np.int64))
        kept_idx = np.concatenate([named_rows, rng.choice(others, n_random)])
    kept_d = rng.uniform(0, 0.06, kept_idx.size).astype(np.float32)
    kept_d[::17] = SPECIAL[1]                                  # the largest distance that is kept
    idx, dists = np.concatenate([kept_idx, drop_idx]), np.concatenate([kept_d, drop_d])
    n = idx.size
    perm = rng.permutation(n)
    last = int(np.nonzero(perm == 0)[0][0])                    # row 0 is a kept one (for `lengths`: the single row of its target)
    perm[[last, n - 1]] = perm[[n - 1, last]]
    idx, dists = idx[perm], dists[perm]
    with np.errstate(invalid="ignore"):
        keep = (dists < EDGE) & (idx >= 0) & (idx < nt)
    src, tgt = rng.uniform(-2, 2, (n, 3)).astype(np.float32), rng.uniform(-2, 2, (nt, 3)).astype(np.float32)
    nrm = rng.standard_normal((nt, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    prior = [torch.from_numpy(rng.standard_normal((nt, 3)).astype(np.float32)) for _ in range(2)]
    case = dict(name=name, n=n, nt=nt, lengths=lengths, src=torch.from_numpy(src), tgt=torch.from_numpy(tgt), nrm=torch.from_numpy(nrm),
                idx=torch.from_numpy(idx), dists=torch.from_numpy(dists), keep=torch.from_numpy(keep), adj=torch.from_numpy(rng.standard_normal(28)),
                prior=prior)
    g_t, g_n, S_t, S_n = C.ne_bwd_tgt_closed_form(case["src"], case["tgt"], case["nrm"], case["idx"], case["keep"], case["adj"], with_scale=True)
    case.update(want=(g_t, g_n), scale=(S_t, S_n), counts=torch.bincount(case["idx"][case["keep"]], minlength=nt))
    return case


def tgt_want(case, accumulate):
    """-> [(want, bound)] for g_tgt and g_tgt_normals: 2^-24 |want| + 1e-12 S, one float32 rounding of a float64 sum; under `accumulate`
    the prior is one more term."""
    out = []
    for w, S, p in zip(case["want"], case["scale"], case["prior"]):
        if accumulate:
            w, S = w + p.double(), S + p.double().abs()
        out.append((w, 2.0 ** -24 * w.abs() + 1e-12 * S))
    return out


def tgt_rows(case):
    """The kept rows' terms (float64): their row numbers, targets, and the (k,6) addends to [g_tgt | g_tgt_normals] of those targets."""
    keep, adj = case["keep"], case["adj"]
    U = torch.zeros(6, 6, dtype=F64)
    U[np.triu_indices(6)] = adj[:21]
    M, gbar, ebar = U + U.T, adj[21:27], adj[27]
    s, j = case["src"].double()[keep], case["idx"][keep]
    t, n = case["tgt"].double()[j], case["nrm"].double()[j]
    A = torch.cat([n, torch.cross(s, n, dim=-1)], -1)
    b = (n * (t - s)).sum(-1)
    Abar, bbar = A @ M.T + b[:, None] * gbar, A @ gbar + 2.0 * ebar * b
    rows = torch.cat([bbar[:, None] * n, bbar[:, None] * (t - s) + Abar[:, :3] + torch.cross(Abar[:, 3:], s, dim=-1)], 1)
    return torch.nonzero(keep)[:, 0].numpy(), j.numpy(), rows.numpy()


def tgt_workspace_bytes(n, nt):
    """The layout comment of csrc/pose_grad.hip: cnt[nt] long_count[1] | loc[nt] | tile_sum[tiles] | list[n] | sorted[n] | long_list[n / NT_LONG + 1]."""
    c = hip_constants()
    return 4 * (2 * nt + 1 + -(-nt // c["NT_TILE"]) + 2 * n + n // c["NT_LONG"] + 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1d. e2e_project3d_bwd_t
# ---------------------------------------------------------------------------------------------------------------------------------------
P3D_SHAPES = {(1, 2, 2): "smallest", (1, 128, 128): "64 partials", (2, 113, 145): "65 partials: second trip, lane 0 only; batched",
              (1, 256, 256): "256 partials", (2, 257, 257): "grid-stride, ragged; batched"}
CLAMP_SHAPE = (1, 37, 41)
CLAMP_ROWS = (5, 6, 7, 8)      # the band: rows 5-6 just above zero, rows 7-8 behind the camera
# The kernel forms its per-pixel terms in float32: no bound is derivable.  Measured on the MI355X, the largest difference to the float64
# reference relative to the largest entry of an item's g_T (g_z NULL / given): 1x2x2 7.1e-8 / 7.1e-8; 1x128x128 4.2e-8 / 7.9e-8; 2x113x145
# 2.0e-7 / 2.2e-7; 1x256x256 1.1e-7 / 2.3e-7; 2x257x257 1.4e-7 / 1.2e-7; the clamp case 1.9e-8 / 2.4e-8 (profiles/slam_grad_contracts.txt).
# The bound is ten times the largest, and never above 1e-4, the project's figure for tensors compared with float64.
P3D_MEASURED = 2.3e-7
P3D_BOUND = 10 * P3D_MEASURED


def _project_inputs(B, H, W, seed=0):
    """as _project_inputs of tests/test_gpu_pose_grad.py, the weights rounded to float32 on both sides"""
    from e2ehip.synthetic import icl_intrinsics
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H, dtype=F64), torch.linspace(0, 1, W, dtype=F64), indexing="ij")
    depth = torch.stack([2.0 + 0.6 * torch.sin(3.0 * xs + b) * torch.cos(2.0 * ys) + 0.3 * ys for b in range(B)])[:, None].float()   # in [1, 3]
    K = icl_intrinsics(H, W)[None].repeat(B, 1, 1)
    pts = warp_loss.backproject(depth.double(), torch.linalg.inv(K.double())).float()
    T = torch.stack([I.se3_exp(torch.tensor([0.03, -0.02, 0.015, 0.01, -0.012, 0.008], dtype=F64) * (1 + 0.5 * b)) for b in range(B)]).float()
    Wg = torch.randn(B, H, W, 2, generator=g, dtype=F64)
    Wz = torch.randn(B, 1, H, W, generator=g, dtype=F64)
    Wg[:, -1, -1] = torch.tensor([1.5, -1.5], dtype=F64)      # the last pixel's weights are not small by chance: its loss must show
    Wz[:, 0, -1, -1] = 1.5
    return pts, K, T, Wg.float(), Wz.float()


def project_terms(case, with_gz, gz_everywhere=False):
    """The closed form of include/e2eslam.h in float64: per pixel cbar, -> terms (B,N,16), pixel i's addend to g_T (row-major 4x4).
    gz_everywhere: as if the clamp passed its gradient below the bound too (what the clamp case must tell apart)."""
    pts, K, T = case["pts"].double(), case["K"].double(), case["T"].double()
    B, H, W = case["shape"]
    P = (K @ T)[:, :3]
    c = P @ pts                                                # (B,3,N)
    z = c[:, 2] + 1e-7
    u, v = c[:, 0] / z, c[:, 1] / z
    gg = case["Wg"].double().reshape(B, H * W, 2)
    gu, gv = gg[..., 0] * 2.0 / (W - 1), gg[..., 1] * 2.0 / (H - 1)
    cb = torch.stack([gu / z, gv / z, -(gu * u + gv * v) / z], 1)            # (B,3,N)
    if with_gz:
        gz = case["Wz"].double().reshape(B, H * W)
        cb[:, 2] += gz if gz_everywhere else gz * (c[:, 2] > 1e-3)
    Pbar = cb[:, :, None, :] * pts[:, None, :, :]              # (B,3,4,N)
    return torch.einsum("bik,bijn->bnkj", K[:, :3], Pbar).reshape(B, H * W, 16)


def project_reference(case, with_gz):
    """float64 autograd of oracle.warp_loss.project -> g_T (B,4,4)."""
    B, H, W = case["shape"]
    T64 = case["T"].double().requires_grad_(True)
    out = warp_loss.project(case["pts"].double(), case["K"].double(), T64, H, W, geometric=with_gz)
    s = (out[0] * case["Wg"].double()).sum()
    if with_gz:
        s = s + (out[1] * case["Wz"].double()).sum()
    (g,) = torch.autograd.grad(s, T64)
    return g


@functools.lru_cache(maxsize=None)
def project_case(shape):
    B, H, W = shape
    pts, K, T, Wg, Wz = _project_inputs(B, H, W)
    case = dict(shape=shape, pts=pts, K=K, T=T, Wg=Wg, Wz=Wz)
    case["want"] = {gz: project_reference(case, gz) for gz in (False, True)}
    return case


@functools.lru_cache(maxsize=None)
def clamp_case():
    """One frame seen through a pose that turns about the optical axis and shifts sideways only, so that camera-space z IS the point's z,
    bit for bit, in float32 as in float64.  The band's points are the band's pixels backprojected to z in [1e-4, 5e-4] (rows 5-6) and
    in [-0.5, -0.1] (rows 7-8): all below the clamp at 1e-3, none within 1e-4 of it or of 0.  Their grid weights are scaled by |z| / 2
    (1 / z would otherwise make the band the whole of g_T); their g_z weights are 1.5 + noise, a sum that cannot be missed."""
    B, H, W = CLAMP_SHAPE
    pts, K, _, Wg, Wz = _project_inputs(B, H, W, seed=3)
    T = I.se3_exp(torch.tensor([0.03, -0.02, 0.0, 0.0, 0.0, 0.05], dtype=F64)).float()[None]
    gen = torch.Generator().manual_seed(17)
    zb = torch.empty(len(CLAMP_ROWS), W, dtype=F64)
    zb[:2] = 1e-4 + 4e-4 * torch.rand(2, W, generator=gen, dtype=F64)
    zb[2:] = -0.1 - 0.4 * torch.rand(2, W, generator=gen, dtype=F64)
    depth = pts[:, 2].reshape(B, 1, H, W).double().clone()
    band = torch.zeros(H, W, dtype=torch.bool)
    band[list(CLAMP_ROWS)] = True
    depth[0, 0, list(CLAMP_ROWS)] = zb.float().double()
    pts = warp_loss.backproject(depth, torch.linalg.inv(K.double())).float()
    Wg, Wz = Wg.clone(), Wz.clone()
    Wg[0, list(CLAMP_ROWS)] *= (zb.abs() / 2.0).float()[..., None]
    Wz[0, 0, list(CLAMP_ROWS)] = 1.5 + 0.25 * Wz[0, 0, list(CLAMP_ROWS)]
    case = dict(shape=CLAMP_SHAPE, pts=pts, K=K, T=T, Wg=Wg, Wz=Wz, band=band)
    case["want"] = {gz: project_reference(case, gz) for gz in (False, True)}
    return case


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the map step (csrc/pointfusion_grad.hip) and the normal / alpha maps (csrc/normal_maps_grad.hip)
# ---------------------------------------------------------------------------------------------------------------------------------------
MAP_SHAPES = {(31, 33): "1023: one short block", (32, 32): "1024: one full block", (25, 41): "1025: the first pixel of the next block",
              (33, 125): "4125: five blocks", (263, 1000): "263000: 257 blocks, block 256 takes the second trip of the `before` loop",
              (725, 725): "525625: 1337 pixels behind the grid cap of the pixel passes"}
CAPACITY_CASES = {(32, 32): 300, (33, 125): 1500}             # rows left above the previous map: fewer than the fresh pixels
VALUE_SHAPES = ((32, 32), (25, 41))
MAP_POSE = (0.3, -0.2, 0.1, 0.2, -0.1, 0.3)


def _depth(H, W, phase=0.0):
    ys, xs = torch.meshgrid(torch.linspace(0, 1, H, dtype=F64), torch.linspace(0, 1, W, dtype=F64), indexing="ij")
    return (2.0 + 0.6 * torch.sin(3.0 * xs + phase) * torch.cos(2.0 * ys) + 0.3 * ys).float()                # in [1, 3]


def block_edge_holes(N, block=1024):
    """Flat pixel indices that get zero depth: the last pixel of block 0, the first of block 1 where the frame has a second pixel in it,
    and the same pair at the last block boundary, at the boundary into block 256 and the frame's last pixel.  The first pixel of the
    frame and of every other block stay valid."""
    holes = {min(block, N) - 1}
    nb = -(-N // block)
    if (N - 1) % block:                                       # (at 1025 the last pixel is the next block's first: it stays)
        holes.add(N - 1)
    for b in {1, nb - 1, 256}:
        if 0 < b < nb and b * block + 1 < N:
            holes |= {b * block - 1, b * block}
    return sorted(holes)


@functools.lru_cache(maxsize=None)
def map_case(H, W):
    """One live frame (smooth depth, a rectangular hole, 3 % scattered holes, holes at the block edges) and a previous map of a few
    hundred points in view: the frame's own surface at a lattice of pixels, moved by a millimetre or two, with the frame's normals there
    -- so that a few hundred pixels fuse and most are fresh.  float32 CPU tensors."""
    import normal_grad_ref as NG
    from e2ehip.synthetic import icl_intrinsics
    gen = torch.Generator().manual_seed(H * 1000 + W)
    depth = _depth(H, W)
    depth[torch.rand(H, W, generator=gen) < 0.03] = 0
    depth[2:5, 3:9] = 0
    flat = depth.reshape(-1)
    edge = block_edge_holes(H * W)
    first = [b for b in range(0, H * W, 1024) if b not in edge]
    flat[first] = _depth(H, W).reshape(-1)[first]             # (a scattered hole may have landed there)
    flat[edge] = 0
    K, pose = icl_intrinsics(H, W), I.se3_exp(torch.tensor(MAP_POSE, dtype=F64)).float()
    rgb = torch.rand(H, W, 3, generator=gen)
    fr = NG.frame(rgb.double(), depth.double(), K, pose)
    step = max(2, int(round((H * W / 300.0) ** 0.5)))
    lattice = torch.zeros(H, W, dtype=torch.bool)
    lattice[1:-1:step, 1:-1:step] = True
    pick = lattice & fr["valid"] & ((fr["ng"] ** 2).sum(-1) > 0.5)
    M = int(pick.sum())
    prev = {"points": (fr["Vg"][pick] + 0.002 * (torch.rand(M, 3, generator=gen, dtype=F64) - 0.5)).float(), "normals": fr["ng"][pick].float(),
            "colors": torch.rand(M, 3, generator=gen), "ccounts": 0.5 + 1.5 * torch.rand(M, generator=gen)}
    return dict(H=H, W=W, depth=depth, rgb=rgb, K=K, pose=pose, prev=prev, M=M, valid=depth != 0, edge_holes=edge)


def append_rows(case, unique, M, cap=None):
    """The numbering of the appended rows, on the CPU: pixel q is fresh when its depth is non-zero and the unique table does not hold it;
    its row is M + the fresh pixels before it in row-major order; -1 for every other pixel and for a row at or beyond the capacity.
    -> rows (H*W,) int64, the fresh count."""
    H, W = case["H"], case["W"]
    fresh = case["valid"].clone().reshape(-1)
    if unique.shape[0]:
        fresh[unique[:, 1] * W + unique[:, 2]] = False
    rows = torch.where(fresh, M + torch.cumsum(fresh.long(), 0) - 1, torch.full((H * W,), -1, dtype=torch.int64))
    if cap is not None:
        rows[rows >= cap] = -1
    return rows, int(fresh.sum())


NORMAL_SHAPES = {(1, 725, 725): "525625 pixels, 1337 behind the grid cap of 2048 workgroups", (2, 5, 7): "batched; every nrm == 0 case"}


@functools.lru_cache(maxsize=None)
def normal_case(shape):
    """depth (B,H,W) with holes in the last row, in the last column and (at 725 x 725) inside the region behind the grid cap; K (4,4),
    poses (B,4,4); upstream gradients and priors of order 1 (float32 values)."""
    import normal_grad_ref as NG
    import pointfusion_grad_ref as PG
    from e2ehip.synthetic import icl_intrinsics
    B, H, W = shape
    if (H, W) == (5, 7):
        d0 = NG.degenerate_frame()[0]
        d1 = d0.flip(1).clone()
        d1[4, 2] = d1[1, 6] = 0
        d0 = d0.clone()
        d0[4, 3] = d0[2, 6] = 0
        depth = torch.stack([d0, d1])
    else:
        depth = torch.stack([_depth(H, W, float(b)) for b in range(B)])
        depth[:, H - 1, 5::97] = 0                            # the last row
        depth[:, 7::89, W - 1] = 0                            # the last column
        depth[:, H - 2, W // 2:W // 2 + 3] = 0                # the row above: behind the cap as well
        depth[:, 100:103, 200:260] = 0
    poses = torch.stack([I.se3_exp(torch.tensor(MAP_POSE, dtype=F64) * (1 + b)) for b in range(B)]).float()
    w = {k: PG.weights((B, H, W, 3) if k in ("g_Nm", "g_Ng") else (B, H, W), 70 + i) for i, k in enumerate(("g_Nm", "g_Ng", "prior", "g_alpha"))}
    return dict(shape=shape, depth=depth, K=icl_intrinsics(H, W), poses=poses, **w)


def normal_maps_reference(case, mode):
    import normal_grad_ref as NG
    B = case["shape"][0]
    gn, gg = (case["g_Nm"] if mode != "g_Ng" else None), (case["g_Ng"] if mode != "g_Nm" else None)
    return torch.stack([NG.normal_maps_bwd_closed_form(case["depth"][b].double(), case["K"], case["poses"][b], None if gn is None else gn[b],
                                                       None if gg is None else gg[b]) for b in range(B)])


def alpha_bwd_reference(case, alpha, alpha_den):
    """d alpha / d depth = -2 (rx^2 + ry^2 + 1) d alpha / den in float64, with the forward's alpha (B,H,W) read back; 0 at a hole."""
    import normal_grad_ref as NG
    B, H, W = case["shape"]
    r = NG._rays(case["K"], H, W)
    d = case["depth"].double()
    g = case["g_alpha"] * (-2.0 * (r[..., 0] ** 2 + r[..., 1] ** 2 + 1.0) * d * alpha.double() / float(alpha_den))
    return g * (d != 0)
