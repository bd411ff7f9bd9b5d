"""Host-only: the inputs of tests/test_gpu_map_contracts.py and their float64 reference (tests/pointfusion_contract_ref.py).  Every random
case leaves at most 1 % of its map points and of its pixels undecidable (the only ones a GPU comparison may skip), every constructed case
none; each constructed case really contains what it is there for (exact ties resolved by index, half-pixel projections, zero confidences
that pass through a fuse, points in each frame-edge window, behind the camera, at z' = 0; more than 1024 count blocks in the large map);
and on the decidable set the float64 reference and the fp32 oracle (oracle/pointfusion.py) agree: tables exactly, payloads within fp32
rounding -- two independent statements of the semantics checked against each other without a GPU."""
import numpy as np
import pytest
import torch

import pointfusion_contract_ref as R
from oracle import pointfusion as opf

ALL_RANDOM = list(R.RANDOM_CASES) + ["large"]
CAP = 0.01


@pytest.mark.parametrize("name", ALL_RANDOM)
def test_random_cases_skip_at_most_one_per_cent(name):
    ref = R.reference(name)
    pt, px = R.skipped(ref)
    a = ref["assoc"]
    print(f"{name}: M {a['M']}, active {a['active'].shape[0]}, similar {a['similar'].shape[0]}, unique {a['unique'].shape[0]}, "
          f"undecidable points {pt:.4%}, pixels {px:.4%}")
    assert pt <= CAP and px <= CAP
    H, W, M = R.RANDOM_CASES.get(name, (16, 24, None))            # ("large" is a 16 x 24 frame)
    if min(H, W) > 1 and (M is None or M > 1):
        assert a["unique"].shape[0] > 0.3 * min(a["M"], H * W, 2000), "the case is trivial"      # (a map of one point may match or not)
        assert M is not None or a["similar"].shape[0] > 1.3 * a["unique"].shape[0], "too few pixels with two contenders"
    if min(H, W) == 1:                                          # one row or one column: no cross product, every normal is exactly 0
        assert not ref["maps"]["n"].any() and a["active"].shape[0] > 0 and a["similar"].shape[0] == 0


@pytest.mark.parametrize("name", R.CONSTRUCTED_CASES)
def test_constructed_cases_are_fully_decidable(name):
    ref = R.reference(name)
    a = ref["assoc"]
    assert not a["und_pt"].any() and not a["und_px"].any(), (np.nonzero(a["und_pt"])[0][:10], np.nonzero(a["und_px"])[0][:10])
    K = R.get_case(name)["K"]
    assert K[0, 0] == K[1, 1] == 64 and K[0, 2] == int(K[0, 2]) and K[1, 2] == int(K[1, 2])


def test_large_map_needs_the_scan_carry():
    c, ref = R.large_case(), R.reference("large")
    M = c["state"]["ccounts"].shape[0]
    assert -(-M // 1024) > 1024
    a = ref["assoc"]
    n = a["similar"][:, 0]
    assert a["unique"].shape[0] > 300 and 2000 < a["active"].shape[0] < 0.1 * M
    assert n.min() < 1024 and n.max() >= M - 1024                         # matches in the first and the last count block
    assert len(np.unique(n // (1024 * 1024))) == 2                        # ... and on both sides of the carry


def test_ties_case_holds_its_three_kinds():
    ref = R.reference("ties")
    a, c = ref["assoc"], R.get_case("ties")
    H, W = c["H"], c["W"]
    half = (c["state"]["ccounts"].shape[0] - 4) // 2
    assert half == H * W
    cnt = a["counts"]
    assert cnt["ties"] == (H - 1) * (W - 1) - 2                           # every pixel with a normal, but the two planted ones
    assert cnt["by_conf"] == 1 and cnt["by_dist"] == 1
    win = a["winner_of_pix"]
    assert win[5 * W + 7] == 2 * half and win[9 * W + 12] == 2 * half + 3  # A (confidence) ; D (distance, the higher index)
    rest = a["unique"][a["unique"][:, 0] < 2 * half]
    assert rest.shape[0] == cnt["ties"] and (rest[:, 0] < half).all()     # every tie from the lower copy
    assert a["unique"].shape[0] == cnt["ties"] + 2


def test_rounding_case_holds_half_pixels():
    a = R.reference("rounding")["assoc"]
    assert a["counts"]["half"] == 6
    assert a["active"][:, 1:].tolist() == [[3, 4], [3, 6], [6, 10], [8, 12], [2, 6], [10, 16]]     # round-half-even, (h, w)
    m = a["margins"]
    assert ((m["half_u"] == 0) | (m["half_v"] == 0)).all() and ((m["half_u"] == 0) & (m["half_v"] == 0)).sum() == 2
    assert a["unique"].shape[0] == 6


def test_edges_case_holds_every_window():
    a = R.reference("edges")["assoc"]
    cnt = a["counts"]
    assert (cnt["win_u_lo"], cnt["win_u_hi"], cnt["win_v_lo"], cnt["win_v_hi"]) == (2, 2, 2, 2)
    assert cnt["behind_in_range"] == 3 and cnt["z_zero"] == 2
    assert a["active"][:, 0].tolist() == [0, 1, 2, 3, 4, 5, 10, 11]         # the four just outside, the three behind and the two at z' = 0 are not
    assert a["active"][:6, 1:].tolist() == [[4, 0], [5, 23], [0, 6], [15, 7], [0, 0], [15, 23]]


def test_far_band_case_holds_zero_confidences():
    c = R.get_case("far_band_second")
    H, W = c["H"], c["W"]
    first, second = R.reference("far_band_first"), R.reference("far_band_second")
    assert first["assoc"]["M"] == 0 and (first["after"]["ccounts"] == 0).sum() == H // 2 * W
    assert (c["state"]["ccounts"] == 0).sum() == H // 2 * W and c["state"]["ccounts"].shape[0] == H * W
    assert second["after"]["c0_fused"] == H // 2 * W
    zero = c["state"]["ccounts"] == 0
    matched = np.zeros(H * W, bool)
    matched[second["assoc"]["unique"][:, 0]] = True
    assert (zero & matched).sum() > 100 and (zero & ~matched).sum() > 0   # zero confidences that match and that pass
    for k in ("points", "normals", "colors"):
        assert not second["after"][k][:H * W][zero].any()                 # where(c + a == 0, 1, c + a): written as zeros
        assert np.isfinite(second["after"][k]).all()


def test_no_correspondence_case():
    c, ref = R.get_case("no_correspondence"), R.reference("no_correspondence")
    a, M = ref["assoc"], c["state"]["ccounts"].shape[0]
    assert a["active"].shape[0] == 0 and a["counts"]["behind_in_range"] == M - c["W"]      # (v -> 2 cy - v: row 0 leaves the frame)
    for k in ("points", "normals", "colors", "ccounts"):
        assert np.array_equal(ref["after"][k][:M], c["state"][k].astype(np.float64))
    assert ref["after"]["ccounts"].shape[0] == M + c["H"] * c["W"]


@pytest.mark.parametrize("name", ALL_RANDOM + list(R.CONSTRUCTED_CASES))
def test_reference_and_oracle_agree_on_the_decidable_set(name):
    ref, c = R.reference(name), R.get_case(name)
    after, tables, maps = R.oracle(name)
    R.compare_tables(ref, tables)
    for k in ("V", "Vg"):
        err, top = np.abs(maps[k] - ref["maps"][k]).max(), np.abs(ref["maps"][k]).max()
        assert err <= 8 * R.FEW * top, (k, err)
    for k in ("n", "ng"):
        assert (np.abs(maps[k] - ref["maps"][k]).max(-1) <= ref["maps"]["dn"] + R.FEW).all(), k
    assert np.abs(maps["alpha"] - ref["maps"]["alpha32"]).max() <= 200 * R.U32          # exp of an argument of up to ~-125 carrying the fp32 roundings of |V|^2 and 2 sigma^2
    errs = R.state_errors(ref, after, tables["unique"], c["depth"] != 0)
    print(name, {k: f"{e:.2e} of {t:.3g}" for k, (e, t) in errs.items()})
    dn = float(ref["maps"]["dn"].max())
    for k, (e, top) in errs.items():
        assert e <= (4 * dn if k == "normals" else 8 * R.FEW * max(top, 1e-30)), (k, e, top)


def test_vertex_maps_gradient_and_transform_against_the_oracle():
    """the remaining float64 restatements, against autograd through the fp32 oracle and against its transform_pointcloud"""
    c = R.get_case("33x37")
    rng = np.random.default_rng(5)
    gV, gVg = rng.standard_normal((1, 33, 37, 3)), rng.standard_normal((1, 33, 37, 3))
    d = torch.from_numpy(c["depth"]).clone().requires_grad_(True)
    m = opf.vertex_normal_maps(d, torch.from_numpy(c["K"]), torch.from_numpy(c["pose"]))
    ((m["V"] * torch.from_numpy(gV[0]).float()).sum() + (m["Vg"] * torch.from_numpy(gVg[0]).float()).sum()).backward()
    ref = R.vertex_maps_bwd(c["depth"][None], c["K"][None], c["pose"][None], gV.astype(np.float32), gVg.astype(np.float32))
    assert np.abs(d.grad.numpy() - ref[0]).max() <= 16 * R.FEW * np.abs(ref).max()
    assert not ref[0][c["depth"] == 0].any() and (c["depth"] == 0).any()
    p = rng.uniform(-2, 2, (100, 3)).astype(np.float32)
    T = R.pose_of(10, 20, -30, (0.5, 1.0, -2.0))
    assert np.abs(opf.transform_pointcloud(torch.from_numpy(p), torch.from_numpy(T)).numpy() - R.transform_points(p, T)).max() <= R.FEW * 4
    back = R.transform_points(R.transform_points(p, T) - T[:3, 3].astype(np.float64), T, True)      # R^T (R p) = p
    assert np.abs(back - p).max() <= 1e-6
