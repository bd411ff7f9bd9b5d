"""Host-only: what tests/warp_window_ref.py claims about its cases, proved for the generator and the salts as they are -- the 2 % cap on every
case, no pixel in the band of the validity mask, an empty exclusion set on every pose case, both winners in every non-trivial mode, exact
ties present (and compared), the float32 and float64 selections equal outside the near-ties, and the reference's own selection logic
(torch.cat + torch.min over dim 1, as oracle.train_depth forms it) equal to the module's first minimum, value, index and gradient.  And, over
the sources: the device code the window shares with the pair is defined once."""
import glob
import os
import re

import pytest
import torch

import warp_window_ref as Wr
from warp_contract_ref import F32, F64


def test_shapes_modes_and_salts_are_the_declared_ones():
    assert Wr.SHAPES == [(1, 3, 5), (2, 9, 33), (2, 17, 33), (1, 37, 53)] and set(Wr.SALT) == set(Wr.SHAPES)
    assert Wr.MODES == [(2, 0, 0), (2, 1, 0), (2, 0, 1), (2, 1, 1), (1, 0, 1), (1, 1, 1)]
    assert len(Wr.CASES) == 4 * 2 * 2 * 6 and Wr.CAP_EXCLUDED == 0.02
    assert [Wr.terms_of(m) for m in Wr.MODES] == [0, 4, 2, 6, 2, 6]
    assert [Wr.n_identity(m) for m in Wr.MODES] == [0, 0, 1, 2, 1, 1]
    s = Wr.scene(2, 9, 33)
    assert not torch.equal(s["K"][0], s["K"][1]) and not torch.equal(s["T"][0][0], s["T"][0][1]) and not torch.equal(s["T"][0], s["T"][1])
    assert s["noise"].shape == (2, 2, 9, 33) and 0 < float(s["noise"].abs().max()) < 1e-4


@pytest.mark.parametrize("shape", Wr.SHAPES, ids=str)
def test_cap_valid_band_and_selection_agreement(shape):
    worst = 0.0
    for case in (Wr.window_case(*c) for c in Wr.CASES if c[0] == shape):
        tag = (case["shape"], case["pad"], case["use_mask"], case["mode"])
        frac = Wr.excluded_fraction(case)
        worst = max(worst, frac)
        assert frac <= Wr.CAP_EXCLUDED, f"{tag}: {100 * frac:.2f} % of the pixels excluded"
        assert not case["valid_band"].any(), f"{tag}: a pixel in the band of the validity mask"
        for k in range(case["mode"][0]):
            assert torch.equal(case["base"][F64]["valid"][k], case["base"][F32]["valid"][k]), f"{tag}: the two references' masks differ"
        flips = (case[F64]["select"] != case[F32]["select"]) & ~case["near"]
        assert not flips.any(), f"{tag}: {int(flips.sum())} selection flips between float32 and float64 outside the near-ties"
        assert case[F64]["cands"].shape[1] == Wr.n_identity(case["mode"]) + (case["mode"][0] if case["mode"][1] else 1)
        if case["mode"] == Wr.TRIVIAL:
            assert not case[F64]["select"].any() and not case["near"].any()
    print(f"\n{shape}: largest excluded fraction {100 * worst:.2f} %")


def test_pose_cases_have_empty_exclusion_sets_and_cover_the_modes():
    for c in Wr.POSE_CASES:
        case = Wr.window_case(*c)
        assert not case["grad_excluded"].any(), f"{c}: {int(case['grad_excluded'].sum())} excluded pixels in a pose case"
        for k, g in enumerate(case[F64]["g_T"]):
            assert float(g.abs().max()) > 0, f"{c}: g_T of source {k} is identically zero"
    for mode in Wr.MODES:
        assert all(any(c[2] == mask and c[3] == mode and c[0][0] == 2 for c in Wr.POSE_CASES) for mask in (0, 1)), mode      # B = 2, several tiles
        for pad in (0, 1):
            assert any(c[1] == pad and c[0][0] == 2 and c[3][0] == mode[0] for c in Wr.POSE_CASES), (pad, mode)
            for mask in (0, 1):
                assert any(c[1:] == (pad, mask, mode) for c in Wr.POSE_CASES), (pad, mask, mode)
    assert len(set(Wr.POSE_CASES)) == len(Wr.POSE_CASES) and set(Wr.POSE_CASES) <= set(Wr.CASES)
    case = Wr.window_case(*Wr.EXPANDED_CASE, None, True)              # one (4,4) pose per source behind both batch elements
    assert not case["grad_excluded"].any() and not case["valid_band"].any() and Wr.both_winners(case)
    assert all(g.shape == (4, 4) and float(g.abs().max()) > 0 for g in case[F64]["g_T"])


def test_both_winners_in_every_non_trivial_mode():
    for c in Wr.CASES:
        if c[3] != Wr.TRIVIAL:
            assert Wr.both_winners(Wr.window_case(*c)), f"{c}: a winner is missing"


def test_exact_ties_are_present_and_go_to_the_first_candidate():
    seen = 0
    for case in Wr.all_cases():
        tie = case["exact"] & ~case["grad_excluded"]
        if not tie.any():
            continue
        seen += int(tie.sum())
        c = case[F64]["cands"]
        first = (c == c.amin(1, keepdim=True)).float().argmax(1)
        assert torch.equal(case[F64]["select"][tie], first[tie]) and torch.equal(case[F32]["select"][tie], first[tie])
        assert ((c == c.amin(1, keepdim=True)).sum(1)[tie] >= 2).all()
    assert seen > 0, "no exact tie in any case"
    # both reprojection maps identical where both samples fall outside under zero padding: the case the header names
    case = Wr.window_case((2, 17, 33), 0, 0, (2, 1, 0))
    assert (case["exact"] & (case[F64]["cands"][:, 0] == case[F64]["cands"][:, 1])).any()


@pytest.mark.parametrize("mode", Wr.MODES, ids=str)
def test_first_minimum_is_the_reference_selection(mode):
    """the harness's own expression (oracle.train_depth: cat((auto, photo), 1), torch.min(dim=1)[0].mean()) gives the module's loss, select and
    gradients"""
    shape, pad, mask = (2, 9, 33), 0, 1
    case = Wr.window_case(shape, pad, mask, mode)
    s = case["scene"]
    for dt in (F64, F32):
        b = Wr.maps(s, pad, mask, dt)
        S = mode[0]
        photo, auto = b["rep"][:, :S], b["idn"][:, :S]
        if not mode[1]:
            photo = photo.mean(1, keepdim=True)
        if mode[2]:
            auto = auto + s["noise"][:, :S].to(dt) if mode[1] else auto.mean(1, keepdim=True)
            photo = torch.cat((auto, photo), 1)
        value, index = torch.min(photo, dim=1)
        loss = value.mean()
        g = torch.autograd.grad(loss, [b["d"]] + b["T"][:S])
        assert torch.equal(index, case[dt]["select"]) and torch.equal(value.detach(), case[dt]["pmap"]) and torch.equal(loss.detach(), case[dt]["loss"])
        assert torch.equal(g[0], case[dt]["g_depth"]) and all(torch.equal(a, c) for a, c in zip(g[1:], case[dt]["g_T"]))


def test_first_minimum_lets_a_nan_win():
    c = torch.tensor([[3.0, float("nan"), 1.0, float("nan")], [2.0, 1.0, 1.0, 5.0]]).t().reshape(1, 4, 2)[:, :, :, None]
    value, sel = Wr.first_min(c)
    want_v, want_i = torch.min(c, dim=1)
    assert torch.equal(sel, want_i) and torch.equal(torch.isnan(value), torch.isnan(want_v))
    assert sel.flatten().tolist() == [1, 1]


def test_crafted_case_has_one_winner_everywhere():
    for winner in (0, 1):
        case = Wr.crafted(winner)
        for dt in (F64, F32):
            assert (case[dt]["select"] == winner).all()
            assert float(case[dt]["g_T"][1 - winner].abs().max()) == 0.0 and float(case[dt]["g_T"][winner].abs().max()) > 0
        c = case[F64]["cands"]
        assert float((c[:, 1 - winner] - c[:, winner]).min()) > 0.3                # far from a tie
        # the loser's map is not flat: given weight, it would have a gradient
        b = Wr.maps(case["scene"], case["pad"], case["use_mask"], F64, srcs=case["srcs"])
        g, = torch.autograd.grad(b["rep"][:, 1 - winner].mean(), b["T"][1 - winner])
        assert float(g.abs().max()) > 0


def test_shared_device_code_of_the_pair_family_is_defined_once():
    """across csrc/*.hip and csrc/*.h: one struct Stats, one definition each of window_stats, ssim_value, ssim_partials and sample3, one
    __global__ whose name ends in reduce_partials and one whose name ends in bwd_pose_final (the window uses the pair's); one struct FirstMin,
    one definition each of photo_value and source_weight, and one tile kernel per direction for the window and its geometric form together:
    one __global__ named k_warp_photo_window_fwd or k_warp_photo_geo*_fwd and one named ..._bwd (templates <PAD, GEO> and <PAD, POSE, GEO>
    of warp_photo_window.hip), and no file warp_photo_geo.hip"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "end-to-end-self-supervised-slam_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert len(files) >= 20                                                            # 22 at the time of writing: the glob still finds them
    text = {os.path.basename(f): open(f).read() for f in files}
    kernel = r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s+)?void\s+\w*%s\s*\("
    patterns = {"struct Stats": r"\bstruct\s+Stats\b\s*\{", "reduce_partials": kernel % "reduce_partials", "bwd_pose_final": kernel % "bwd_pose_final"}
    patterns["struct FirstMin"] = r"\bstruct\s+FirstMin\b\s*\{"
    for d in ("fwd", "bwd"):                                                           # the window's and the geometric form's tile kernel are ONE template
        what = f"k_warp_photo_window_{d} (the one tile kernel of e2e_warp_photo_window_{d} and e2e_warp_photo_geo_{d})"
        patterns[what] = kernel % (r"k_warp_photo_(?:window|geo)\w*_" + d)
    for fn in ("window_stats", "ssim_value", "ssim_partials", "sample3", "photo_value", "source_weight"):
        patterns[fn + "("] = r"^__device__[^;{(\n]*\b" + fn + r"\s*\([^;{]*\{"          # a definition: a body follows the parameter list
    for what, pat in patterns.items():
        found = [name for name, src in text.items() for _ in re.finditer(pat, src, re.M)]
        assert len(found) == 1, f"{what}: defined {len(found)} times, in {found}"
    assert "k_warp_photo_bwd_pose_final" in text["warp_photo_pose.hip"] and "k_reduce_partials" in text["warp_photo.hip"]
    assert "warp_photo_geo.hip" not in text, "warp_photo_geo.hip is back: the geometric form is the GEO = true instantiation of warp_photo_window.hip"
    assert "k_warp_photo_window_fwd" in text["warp_photo_window.hip"] and "k_warp_photo_window_bwd" in text["warp_photo_window.hip"]
