"""Host-only: the cases of tests/slam_grad_contract_ref.py are what tests/test_gpu_pose_grad_contracts.py and
tests/test_gpu_map_grad_contracts.py claim -- each staging regime of csrc/pose_grad.hip, csrc/pointfusion_grad.hip and
csrc/normal_maps_grad.hip is reached by the case listed for it (asserted from the case's sizes and the constants read out of the
sources, so a retune of NT_TILE, NT_LONG, PG_MAX_PARTS or CP_BLOCK fails here), the kept sets and clamp margins are as stated, and every
summed output would show the loss of its last row, of any workgroup's rows or of a whole grid-stride trip at 100 times its bound.  No GPU."""
import numpy as np
import pytest
import torch

import slam_grad_contract_ref as R

F64 = torch.float64
FACTOR = 100.0


def _shows_every_group(terms, bound, what):
    """terms (n,K): row i's addend to each of K sums; bound (K,) absolute.  Deleting any group of rows moves some sum by >= FACTOR x bound."""
    n = terms.shape[0]
    worst = np.inf
    for a, b in R.groups(n):
        ratio = float((np.abs(terms[a:b].sum(0)) / bound).max())
        worst = min(worst, ratio)
        assert ratio >= FACTOR, f"{what}: losing rows [{a}, {b}) moves no output by {FACTOR:g} x its bound (the most: {ratio:.3g} x)"
    return worst


def test_the_constants_the_cases_are_sized_against():
    c = R.hip_constants()
    assert (c["PG_T"], c["PG_MAX_PARTS"], c["PG_NSUM"], c["NT_TILE"], c["NT_LONG"], c["NT_LONG_GRID"], c["NT_SHORT_GRID"]) == (256, 256, 12, 4096, 64, 256, 4096)
    assert (c["PF_T"], c["CP_BLOCK"], c["PFG_GRID"], c["NM_GRID"]) == (256, 1024, 2048, 2048)
    assert R.T4 == c["NT_TILE"]
    import test_gpu_icp_contracts as ICP                      # the forward's edge values: the same bits
    assert np.array_equal(np.array(R.SPECIAL).view(np.int32), np.array(ICP.SPECIAL).view(np.int32)) and R.SPECIAL_KEPT == ICP.SPECIAL_KEPT
    assert R.EDGE == ICP.EDGE and R.NE_BOUND == ICP.NE_BOUND


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1a / 1d: the partials and the second stage
# ---------------------------------------------------------------------------------------------------------------------------------------
def _parts(n, c):
    return min(-(-n // c["PG_T"]), c["PG_MAX_PARTS"])


def test_sizes_reach_every_path_of_the_two_stage_sums():
    c = R.hip_constants()
    stride = c["PG_T"] * c["PG_MAX_PARTS"]
    for sizes in (list(R.TP_SIZES), [h * w for _, h, w in R.P3D_SHAPES], list(R.NEB_SIZES)):
        parts = [_parts(n, c) for n in sizes]
        assert 1 in parts and c["PG_MAX_PARTS"] in parts
        assert any(n > stride for n in sizes) and any(n > stride and n % c["PG_T"] for n in sizes)          # the grid-stride trip, ragged
    for sizes in (list(R.TP_SIZES), [h * w for _, h, w in R.P3D_SHAPES]):
        parts = [_parts(n, c) for n in sizes]
        assert 64 in parts and 65 in parts                    # the second stage's lanes: exactly one trip, and lane 0's second
        assert any(p > 64 for p in parts) and stride in sizes
    assert stride + 1 in R.TP_SIZES
    assert any(B > 1 for B, _, _ in R.P3D_SHAPES)


@pytest.mark.parametrize("n", list(R.TP_SIZES), ids=lambda n: f"n{n}")
def test_transform_case_shows_every_lost_group(n):
    case = R.transform_case(n)
    assert case["terms"].shape == (n, 12) and (case["scale"] > 0).all()
    assert abs(float(case["g"].mean())) > 0.3 or n < 64       # offset from zero: a lost row cannot cancel
    worst = _shows_every_group(case["terms"], R.NE_BOUND * case["scale"].astype(np.float64), f"transform n={n}")
    print(f"1a n={n}: the least a lost group moves an output: {worst:.3g} x the bound")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1b: the kept sets
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.NEB_SIZES, ids=lambda n: f"n{n}")
def test_ne_bwd_case_keeps_what_the_forward_keeps(n):
    for nt in R.NEB_TARGETS:
        case = R.ne_bwd_case(n, nt)
        keep, every = case["keep_thresh"], case["keep_all"]
        for pos, kept in case["special"].items():
            assert bool(keep[pos]) == kept and bool(every[pos]), (n, nt, pos)
        assert (n < 63) == (not case["outside"])
        for pos, j in case["outside"].items():
            assert not (0 <= j < nt) and not bool(every[pos]) and not bool(keep[pos]) and float(case["dists"][pos]) < R.EDGE
        assert {j & 0xFFFFFFFF for j in case["outside"].values()} >= {0} or n < 63            # in range for whoever keeps 32 bits
        if n >= 63:
            assert 0 < int(keep.sum()) < int(every.sum()) < n
        assert int(case["idx"].max()) >= nt - 1 and (nt == 1 or n < 4 or int(case["idx"][2]) == int(case["idx"][1]))
        for k in (keep, every):                               # every kept row's gradient is non-zero: the kept set can be read off the output
            ref = R.ne_bwd_reference(case, k)
            assert torch.equal((ref != 0).any(1), k), (n, nt)
            if bool(k.any()):
                assert float(ref[k].abs().max(1)[0].min()) > 1e-6 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1c: segment lengths, tiles, the dropped rows
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.TGT_CASES))
def test_tgt_case_is_what_it_claims(name):
    c = R.hip_constants()
    case = R.tgt_case(name)
    n, nt, counts, idx, keep = case["n"], case["nt"], case["counts"], case["idx"], case["keep"]
    assert counts.shape == (nt,) and int(counts.sum()) == int(keep.sum()) and bool(keep[-1])
    assert R.tgt_workspace_bytes(n, nt) == 4 * (2 * nt + 1 + -(-nt // 4096) + 2 * n + n // 64 + 1)
    inside = (idx >= 0) & (idx < nt)
    if name == "many_long":
        assert n == 21000 and bool((counts == 70).all()) and 70 > c["NT_LONG"] and nt > c["NT_LONG_GRID"]      # more queued targets than waves
        assert bool(keep.all())
    else:
        for j, l in case["lengths"].items():
            assert int(counts[j]) == l, (name, j)
        assert {c["NT_LONG"] - 1, c["NT_LONG"], c["NT_LONG"] + 1, c["NT_LONG"] + 2, 2 * c["NT_LONG"], 2 * c["NT_LONG"] + 1} <= set(case["lengths"].values())
        assert 0 in case["lengths"].values() and max(case["lengths"].values()) > 10 * c["NT_LONG"]
        by_len = {l: j for j, l in case["lengths"].items()}
        with np.errstate(invalid="ignore"):
            dropped_d = ~(case["dists"].numpy() < R.EDGE)
        for l in (0, 63, 64, 65):                             # rows beyond the edge name them: counted, they would move the length across 64 / 65
            assert int((torch.from_numpy(dropped_d) & (idx == by_len[l])).sum()) == 4
        assert int((~inside).sum()) == 2 * len(R.OUT_OF_RANGE) and not bool(keep[~inside].any())
        assert bool((case["dists"][keep] == float(R.SPECIAL[1])).any())
        assert int((counts == 0).sum()) > 0                   # targets that no kept row names
    # the source rows are permuted: a segment's rows do not arrive in ascending order
    assert not bool((idx[keep][1:] >= idx[keep][:-1]).all())
    tile = torch.arange(nt) // c["NT_TILE"]
    loc = torch.cumsum(counts, 0) - counts                    # rows before j, all tiles
    if name in ("nt4097", "nt8193", "stride", "huge"):        # a target in a tile > 0 whose tile_sum is non-zero (4097: the tile's only target)
        tile_base = loc[tile * c["NT_TILE"]]
        assert bool(((counts > 0) & (tile > 0) & (tile_base > 0)).any())
        assert all(int(counts[j]) > 0 for j in (c["NT_TILE"] - 1, c["NT_TILE"]))
        if name != "nt4097":                                  # ... and with loc and tile_sum both non-zero
            assert bool(((counts > 0) & (tile > 0) & (tile_base > 0) & (loc - tile_base > 0)).any())
    if name == "nt8193":
        assert int(tile.max()) == 2 and int(counts[2 * c["NT_TILE"]:].sum()) > 0
    if name in ("nt4095", "nt4096"):
        assert int(tile.max()) == 0 and int(counts[nt - 1]) > 0
    if name == "stride":
        assert n == 70001 and n > c["PG_T"] * c["PG_MAX_PARTS"] and n % c["PG_T"]
    if name == "huge":
        tiles = -(-nt // c["NT_TILE"])
        assert tiles > c["PG_T"] and -(-nt // c["PG_T"]) > c["NT_SHORT_GRID"]                       # the scan's second chunk; sum_short's stride
        assert int(counts[c["PG_T"] * c["NT_TILE"]:].sum()) > 0 and int(counts[(c["PG_T"] + 1) * c["NT_TILE"]:].sum()) > 0
        assert all(int(counts[j]) > 0 for j in (255 * 4096 - 1, 255 * 4096, 256 * 4096 - 1, 256 * 4096, 256 * 4096 + 1, 257 * 4096, nt - 1))
    # the reference: the closed form is the autograd of the sums
    if nt <= 9000:
        t64, n64 = case["tgt"].double().requires_grad_(True), case["nrm"].double().requires_grad_(True)
        import icp_grad_ref as I
        AtA, Atb, err = I.sums(case["src"].double(), t64, n64, idx.clamp(0, nt - 1), keep)
        packed = torch.stack([AtA[r, k] for r in range(6) for k in range(r, 6)])
        adj = case["adj"]
        auto = torch.autograd.grad((adj[:21] * packed).sum() + (adj[21:27] * Atb).sum() + adj[27] * err, [t64, n64])
        for a, w in zip(auto, case["want"]):                 # (autograd goes through the 6x6 products: compared against the largest entry)
            assert float((a - w).abs().max()) <= 1e-12 * float(w.abs().max())
    # the rows' terms add up to the reference, and every lost group shows
    rows_i, rows_j, rows = R.tgt_rows(case)
    total = np.zeros((nt, 6))
    np.add.at(total, rows_j, rows)
    want = torch.cat(case["want"], 1).numpy()
    scale = torch.cat(case["scale"], 1).numpy()
    assert (np.abs(total - want) <= 1e-13 * scale).all()
    bound = torch.cat([b for _, b in R.tgt_want(case, 0)], 1).numpy()
    worst = np.inf
    for a, b in R.groups(n):
        sel = (rows_i >= a) & (rows_i < b)
        assert sel.any(), f"{name}: rows [{a}, {b}) hold no kept row"
        js, inv = np.unique(rows_j[sel], return_inverse=True)
        delta = np.zeros((js.size, 6))
        np.add.at(delta, inv, rows[sel])
        ratio = float((np.abs(delta) / np.maximum(bound[js], 1e-300)).max())
        worst = min(worst, ratio)
        assert ratio >= FACTOR, f"{name}: losing rows [{a}, {b}) moves no output by {FACTOR:g} x its bound"
    print(f"1c {name}: the least a lost group moves an output: {worst:.3g} x the bound")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1d: Project3D
# ---------------------------------------------------------------------------------------------------------------------------------------
def _project_groups(case, tag):
    B, H, W = case["shape"]
    for with_gz in (False, True):
        terms = R.project_terms(case, with_gz)
        want = case["want"][with_gz]
        assert float((terms.sum(1).reshape(B, 4, 4) - want).abs().max()) <= 1e-12 * float(want.abs().max())      # the closed form is the autograd
        for b in range(B):
            assert not bool(want[b, 3].any()) and float(want[b, :3].abs().min()) > 0
            bound = np.full(16, R.P3D_BOUND * float(want[b].abs().max()))
            worst = _shows_every_group(terms[b].numpy(), bound, f"project3d {tag} item {b} g_z {with_gz}")
    return worst


@pytest.mark.parametrize("shape", list(R.P3D_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_project_case_shows_every_lost_group(shape):
    case = R.project_case(shape)
    B = shape[0]
    if B > 1:                                                 # the items differ: a partial taken from the other batch row shows
        w = case["want"][True]
        assert float((w[0] - w[1]).abs().max()) > 1e-2 * float(w.abs().max())
    assert float(case["pts"][:, 2].min()) > 0.5               # nothing at the clamp
    _project_groups(case, "x".join(map(str, shape)))


def test_clamp_case_margins_and_what_the_reference_tells_apart():
    case = R.clamp_case()
    B, H, W = case["shape"]
    K, T, band = case["K"], case["T"], case["band"].reshape(-1)
    P32 = (K @ T)[0, 2]
    assert torch.equal(P32, torch.tensor([0.0, 0.0, 1.0, 0.0])) and torch.equal((K.double() @ T.double())[0, 2], P32.double())
    z = (K.double() @ T.double())[0, :3] @ case["pts"][0].double()
    assert torch.equal(z[2], case["pts"][0, 2].double())      # camera-space z is the point's z, bit for bit
    zb = z[2][band]
    assert int(band.sum()) == len(R.CLAMP_ROWS) * W
    assert bool((zb < 1e-3 - 1e-4).all()) and bool(((zb - 0.0).abs() >= 1e-4).all())          # none within 1e-4 of the clamp or of 0
    assert int(((zb > 0) & (zb <= 5e-4)).sum()) == 2 * W and int((zb <= -0.1).sum()) == 2 * W
    assert bool((z[2][~band] > 0.5).all())
    # the band's g_z term is absent, its grid term is present: both at FACTOR x the bound
    want, want_no_gz = case["want"][True], case["want"][False]
    top = float(want.abs().max())
    leak = R.project_terms(case, True, gz_everywhere=True).sum(1).reshape(B, 4, 4)
    assert float((leak - want).abs().max()) >= FACTOR * R.P3D_BOUND * top
    terms = R.project_terms(case, True)
    assert float(terms[0][band].sum(0).abs().max()) >= FACTOR * R.P3D_BOUND * top
    gz_only = (want - want_no_gz)                             # what g_z adds: the pixels above the clamp only
    above = R.project_terms(case, True)[0][~band].sum(0) - R.project_terms(case, False)[0][~band].sum(0)
    assert float((gz_only[0].reshape(-1) - above).abs().max()) <= 1e-12 * top
    _project_groups(case, "clamp")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2: the map step's cases, the normal maps' cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_map_shapes_reach_every_path_of_the_ordered_scan():
    c = R.hip_constants()
    sizes = [h * w for h, w in R.MAP_SHAPES]
    blocks = [-(-n // c["CP_BLOCK"]) for n in sizes]
    assert c["CP_BLOCK"] - 1 in sizes and c["CP_BLOCK"] in sizes and c["CP_BLOCK"] + 1 in sizes
    assert any(1 < b <= c["PF_T"] for b in blocks) and max(blocks) > c["PF_T"]                 # the `before` loop's second trip: block index >= PF_T
    assert 263 * 1000 in sizes and -(-263000 // c["CP_BLOCK"]) == c["PF_T"] + 1
    assert max(sizes) - c["PFG_GRID"] * c["PF_T"] == 1337                                     # the pixel passes' trip behind the grid cap
    for shape in R.CAPACITY_CASES:
        case = R.map_case(*shape)
        assert shape in R.MAP_SHAPES and int(case["valid"].sum()) - case["M"] > R.CAPACITY_CASES[shape] > 0      # at most M pixels fuse
    assert all(s in R.MAP_SHAPES for s in R.VALUE_SHAPES)


@pytest.mark.parametrize("shape", list(R.MAP_SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_case_has_the_holes_and_the_small_map_it_claims(shape):
    c = R.hip_constants()
    H, W = shape
    case = R.map_case(H, W)
    n, valid = H * W, case["valid"].reshape(-1)
    assert 100 <= case["M"] <= 400 and int(valid.sum()) - case["M"] > n // 2                   # a few hundred points; most pixels are fresh
    holes = torch.nonzero(~valid)[:, 0]
    assert 0.02 * n < holes.numel() < 0.1 * n
    assert not bool(valid[min(n, c["CP_BLOCK"]) - 1])                                         # the last pixel of block 0
    assert bool((holes % c["CP_BLOCK"] == 0).any()) == (n > c["CP_BLOCK"] + 1)                # a block's first pixel
    firsts = torch.arange(0, n, c["CP_BLOCK"])
    assert bool(valid[0]) and int(valid[firsts].sum()) >= firsts.numel() - 3                  # ... and valid ones there too
    assert not bool(valid[case["edge_holes"]].any())
    if n == c["CP_BLOCK"] + 1:
        assert bool(valid[n - 1])                             # the first pixel of the next block is a fresh one
    if n > c["PF_T"] * c["CP_BLOCK"]:
        b = c["PF_T"] * c["CP_BLOCK"]
        assert not bool(valid[b - 1]) and not bool(valid[b]) and int(valid[b:].sum()) > 500
    prev = case["prev"]
    assert all(prev[k].shape[0] == case["M"] for k in prev) and float(prev["ccounts"].min()) >= 0.5
    assert bool(((prev["normals"] ** 2).sum(1) > 0.9).all())
    # the numbering helper: rows are M .. M + fresh - 1 in row-major order, -1 elsewhere, and the capacity cuts the tail
    rows, fresh = R.append_rows(case, torch.zeros(0, 3, dtype=torch.int64), case["M"])
    assert fresh == int(valid.sum()) and torch.equal(rows[valid], case["M"] + torch.arange(fresh)) and bool((rows[~valid] == -1).all())
    cut, _ = R.append_rows(case, torch.tensor([[0, 0, 0]]), case["M"], cap=case["M"] + 10)
    assert int(cut[0]) == -1 and int((cut >= 0).sum()) == 10 and int(cut.max()) == case["M"] + 9


@pytest.mark.parametrize("shape", list(R.NORMAL_SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_normal_case_has_holes_where_it_claims(shape):
    c = R.hip_constants()
    B, H, W = shape
    case = R.normal_case(shape)
    hole = case["depth"] == 0
    assert bool(hole[:, H - 1].any(1).all()) and bool(hole[:, :, W - 1].any(1).all()) and bool(hole[:, :H - 1, :W - 1].any())
    assert 0 < int(hole.sum()) < 0.2 * hole.numel()
    if B == 1:
        behind = H * W - c["NM_GRID"] * c["PF_T"]
        assert behind == 1337 == H * W - c["PFG_GRID"] * c["PF_T"]
        tail = hole.reshape(-1)[-behind:]
        assert bool(tail.any()) and not bool(tail.all()) and bool(hole[0, H - 2].any())       # holes inside the second trip, in two rows
        first_row_behind = (H * W - behind) // W
        assert first_row_behind == H - 2
    else:
        assert not torch.equal(case["depth"][0], case["depth"][1])
    for mode in ("g_Nm", "g_Ng", "both"):
        ref = R.normal_maps_reference(case, mode)
        assert torch.isfinite(ref).all() and not bool(ref[hole].any()) and float(ref.abs().max()) > 0
