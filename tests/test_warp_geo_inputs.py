"""Host-only: what tests/warp_geo_ref.py claims about its cases, proved without a GPU -- the caps, the decided validity of every case,
n_s and the open gates, the admitted cases the pose comparison rests on, the gate scene and the two crafted scenes."""
import torch

import warp_contract_ref as R
import warp_geo_ref as G
from warp_contract_ref import F32, F64


def test_every_case_stays_under_the_cap_and_its_validity_is_decided():
    for c in G.CASES:
        case = G.geo_case(*c)
        assert G.excluded_fraction(case) <= G.CAP_EXCLUDED, (c, G.excluded_fraction(case))
        assert not case["valid_band"].any(), f"{c}: a pixel lies in the validity band, n_s is not decided"
        S = c[3][0]
        assert tuple(case["n"]) == G.N_VALID[c[0]][:S] == tuple(case["base"][F32]["n"][:S]), (c, case["n"])
        assert all(n > 0 for n in case["n"]), f"{c}: a gate is closed at geo_min_valid = 0"
        for k in range(S):
            assert float(case[F64]["G"][k]) > 0 and float(case[F64]["g_ds"][k].abs().max()) > 0, f"{c}: source {k} has no geometric term"
            assert not case["src_excluded"][k].all() and (~case["grad_excluded"]).any()
        assert int(((case[F64]["select"] != case[F32]["select"]) & ~case["near"]).sum()) == 0, f"{c}: the selection flips outside the near-ties"


def test_the_admitted_cases():
    """admission is decided by the references on the machine that runs them (the float32 error, hence every band, moves a little with the CPU's
    math library).  Whatever the machine: every case of (1,3,5) is admitted; most of (2,9,33) -- B = 2, one row and one column past a tile --
    with both paddings and an S = 2 mode under the mask; (2,17,33) adds cases two tile rows high; (1,37,53) serves the depth gradients only"""
    adm = {c for c in G.CASES if G.admitted(G.geo_case(*c))}
    assert {c for c in G.CASES if c[0] == (1, 3, 5)} <= adm
    assert sum(1 for c in adm if c[0] == (2, 9, 33)) >= 16
    for pad in (0, 1):
        assert any(c[0] == (2, 9, 33) and c[1] == pad and c[2] == 1 and c[3][0] == 2 for c in adm), pad
    assert sum(1 for c in adm if c[0] == (2, 17, 33)) >= 4
    for pad in (0, 1):
        for mask in (0, 1):
            for mode in G.MODES:
                assert G.pooled("g_T", pad, mask, mode) > 0 and G.pooled("g_depth", pad, mask, mode) > 0 and G.pooled("g_ds", pad, mask, mode) > 0


def test_the_gate_scene():
    n0, n1 = G.N_VALID[G.GATE_SHAPE]
    assert 0 < n0 < n1 < 10000
    for pad in (0, 1):
        c = G.geo_case(G.GATE_SHAPE, pad, 1, (2, 1, 1), None, False, n0)
        assert float(c[F64]["G"][0]) == 0 and float(c[F32]["G"][0]) == 0 and float(c[F64]["G"][1]) > 0          # n_0 > n_0 is false: strict
        assert float(c[F64]["g_ds"][0].abs().max()) == 0 and float(c[F64]["g_ds"][1].abs().max()) > 0
        shut = G.geo_case(G.GATE_SHAPE, pad, 1, (2, 1, 1), None, False, 10000)
        assert all(float(g) == 0 for g in shut[F64]["G"]) and all(float(g.abs().max()) == 0 for g in shut[F64]["g_ds"])


def _cells(grid64, H, W, pad):
    ix, iy = R.source_index(grid64[..., 0], W, False, F64), R.source_index(grid64[..., 1], H, False, F64)
    if pad == 1:
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    return [len({(int(y), int(x)) for y, x in zip(iy[b].floor().flatten(), ix[b].floor().flatten())}) for b in range(grid64.shape[0])]


def test_the_crafted_scenes():
    for shape in G.CRAFTED_SHAPES:
        B, H, W = shape
        for pad in (0, 1):
            c = G.crafted("behind", shape, pad)
            assert G.excluded_fraction(c) <= G.CAP_EXCLUDED
            for k in range(2):
                b = c["base"][F64]
                valid, c2 = b["valid"][k] > 0, b["c2"][k]
                below = valid & (c2 < G.ZCLAMP)
                assert int(below.sum()) >= 120 and int((valid & (c2 >= G.ZCLAMP)).sum()) >= 18, (shape, pad, k)
                assert float(c2.abs().min()) > 0.5                        # nothing near the clamp or the projection's singularity
                assert not c["geo"][k]["zclamp"].any() and not c["geo"][k]["vband"].any()
                assert c["base"][F32]["n"][k] == b["n"][k]
            # no gradient through wd under the clamp, yet the one through the sampling position is there
            below0 = (c["base"][F64]["valid"][0] > 0) & (c["base"][F64]["c2"][0] < G.ZCLAMP)
            assert int((c[F64]["g_depth"][below0] != 0).sum()) >= 100
            c = G.crafted("pileup", shape, pad)
            assert G.excluded_fraction(c) <= G.CAP_EXCLUDED
            for k in range(2):
                b = c["base"][F64]
                assert int(b["valid"][k].sum()) == B * H * W == c["base"][F32]["n"][k]
                assert max(_cells(b["grid"][k], H, W, pad)) <= 16, _cells(b["grid"][k], H, W, pad)
                assert float(c[F64]["g_ds"][k].abs().max()) > 0 and int((c[F64]["g_ds"][k] != 0).sum()) <= 64


def test_the_source_gradient_stays_inside_its_batch_element_and_source():
    """B = 2 with distinct K and T: the float64 g_depth_src of a source is nonzero only on the taps of its own valid pixels"""
    c = G.geo_case((2, 9, 33), 1, 1, (2, 1, 1))
    b = c["base"][F64]
    for k in range(2):
        taps = G.footprint(b["grid"][k], 9, 33, 1, b["valid"][k] > 0)
        assert not (c[F64]["g_ds"][k][~taps] != 0).any() and (c[F64]["g_ds"][k][taps] != 0).any()
    assert not torch.equal(b["valid"][0], b["valid"][1])
