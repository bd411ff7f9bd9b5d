"""Host-only qualification of tests/pyramid_smoothness_ref.py, the reference the GPU tests of csrc/disp_pyramid_smooth.hip rely on:

  1. the reference (F.avg_pool2d + oracle.warp_loss.normalised_smoothness + autograd, float64) equals the second, independent float64
     formulation (raw sums scaled by |inv|; gradient sign(inv) gn inv - raw |inv| inv / N) within 1e-12 relative;
  2. every case but `flat` keeps neighbouring normalised disparities 2^-16 apart, so no sign can differ between a reference and a
     correct kernel, and no element has to be excluded;
  3. the derived bounds discriminate: the formulation run in float32 (an emulation of the term) passes them, and each seeded fault fails
     them in every case where it applies."""
import pytest
import torch

import pyramid_smoothness_ref as R

REGULAR = [n for n in sorted(R.CASES) if not R.CASES[n].get("flat")]
MULTI_TILE = [n for n in REGULAR if any(w > R.TILE[1] for _, w in R.CASES[n]["scales"].values())]
FAULTS = [("halo", n) for n in MULTI_TILE] + [("square_box", n) for n in ("two_by_two", "anisotropic")] + \
         [("no_mean", n) for n in REGULAR] + [("swap", "zero_two")]


def _rel(a, b):
    return float((a - b).abs().max()) / float(b.abs().max())


@pytest.mark.parametrize("name", REGULAR)
def test_reference_equals_the_second_formulation(name):
    c = R.case(name)
    other = R.formulation(c["disps"], c["img"], c["weights"])
    assert _rel(other["total"], c["ref"]["total"]) <= 1e-12
    for k in c["disps"]:
        assert _rel(other["loss"][k], c["ref"]["loss"][k]) <= 1e-12, (name, k)
        assert _rel(other["grad"][k], c["ref"]["grad"][k]) <= 1e-12, (name, k)


@pytest.mark.parametrize("name", REGULAR)
def test_cases_keep_the_signs_apart(name):
    gap = R.min_gap(R.case(name)["disps"])
    print(f"{name}: smallest |n_p - n_q| = {gap:.3g} (needs {R.GAP:.3g})")
    assert gap >= R.GAP


def test_multi_tile_cases_exist():
    assert {"four", "zero_two", "ragged", "strided"} <= set(MULTI_TILE)
    h, w = R.CASES["ragged"]["scales"][0]
    assert h % R.TILE[0] and w % R.TILE[1] and h > R.TILE[0] and w > R.TILE[1]


def test_flat_case_is_exactly_zero():
    c = R.case("flat")
    assert float(c["ref"]["total"]) == 0 and all(float(v) == 0 for v in c["ref"]["loss"].values())
    assert all(float(g.abs().max()) == 0 for g in c["ref"]["grad"].values())


@pytest.mark.parametrize("name", REGULAR)
def test_float32_emulation_passes_the_bounds(name):
    c = R.case(name)
    worst = R.worst(R.formulation(c["disps"], c["img"], c["weights"], dtype=torch.float32), c)
    print(f"{name}: float32 emulation, of the bounds: {worst}")
    assert max(worst.values()) <= 1, worst


@pytest.mark.parametrize("fault,name", FAULTS)
def test_seeded_faults_fail_the_bounds(fault, name):
    c = R.case(name)
    worst = R.worst(R.formulation(c["disps"], c["img"], c["weights"], dtype=torch.float32, fault=fault), c)
    print(f"{name}: fault {fault}, of the bounds: {max(worst.values()):.3g}")
    assert max(worst.values()) > 1, worst
