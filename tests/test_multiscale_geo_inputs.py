"""Host-only: what tests/multiscale_geo_ref.py claims about its cases, proved on the CPU by the references alone -- every group scene stays
within warp_geo_ref's rules (its exclusion cap, no pixel in a validity band), the counts n_{s,g} of a gated case are pairwise distinct and its
geo_min_valid is one group's count, so that a group is closed and one is open; one case has a group without any valid projection; the scenes
of the operator test exclude nothing on any scale and open every gate."""
import pytest
import torch

import multiscale_geo_ref as M
import warp_geo_ref as G
from warp_contract_ref import F64


def test_the_case_list_is_the_fixed_one():
    assert M.GROUP_SHAPES == [(1, 13, 37), (2, 9, 33)] and M.GROUPS == (1, 2, 3, 4) and M.SOURCES == (1, 2)
    assert len(M.CASES) == 16 and len(M.GATED) == 12 and M.ZERO in M.CASES
    assert all(len(set(M.SALTS[shape])) == 4 for shape in M.GROUP_SHAPES)
    assert len(set(M.G_LOSS)) == len(M.G_LOSS) == 1 + 2 * 4 and all(x != 0 for x in M.G_LOSS)


@pytest.mark.parametrize("shape", M.GROUP_SHAPES, ids=str)
def test_group_scenes_stay_within_the_rules(shape):
    Ks, Ts, ds = [], [], []
    for salt in M.SALTS[shape]:
        for S in M.SOURCES:
            c = M.group_case(shape, salt, S)
            assert G.excluded_fraction(c) <= M.CAP_EXCLUDED, (shape, salt, S, G.excluded_fraction(c))
            assert not c["valid_band"].any(), f"{shape} salt {salt}: a pixel lies in a validity band, n is not decided"
            for k in range(S):                                   # the count is the float64 decision, and float32 agrees
                assert c["n"][k] == int(c["base"][F64]["valid"][k].sum()) > 0
        s = M.group_scene(shape, salt)
        Ks.append(s["K"]), Ts.append(s["T"][0]), ds.append(s["dsrc"][0])
    for i in range(4):                                           # distinct K, T and source depths per group
        for j in range(i):
            assert not torch.equal(Ks[i], Ks[j]) and not torch.equal(Ts[i], Ts[j]) and not torch.equal(ds[i], ds[j])


@pytest.mark.parametrize("case", M.GATED, ids=str)
def test_gated_cases_close_one_group_and_open_another(case):
    shape, groups, S = case
    n = M.counts(shape, groups, S)
    gmin = M.gate_of(case)
    for s in range(S):
        assert len(set(n[s])) == groups, f"{case}: the counts of source {s} are not pairwise distinct: {n[s]}"
    assert gmin in n[0]                                          # exactly one group's count, the way warp_geo_ref.GATE_SHAPE does it
    assert sum(x > gmin for x in n[0]) == groups - 1 and sum(x <= gmin for x in n[0]) == 1


def test_stacking_is_scale_major():
    shape, groups = (2, 9, 33), 3
    st = M.stacked(shape, groups)
    assert st["B"] == 6 and st["depth"].shape == (6, 9, 33) and st["T"][1].shape == (6, 4, 4) and st["noise"].shape == (6, 2, 9, 33)
    for g, s in enumerate(M.scenes(shape, groups)):
        assert torch.equal(st["depth"][2 * g:2 * g + 2], s["depth"]) and torch.equal(st["K"][2 * g:2 * g + 2], s["K"])
        assert torch.equal(st["dsrc"][1][2 * g:2 * g + 2], s["dsrc"][1]) and torch.equal(st["src"][0][2 * g:2 * g + 2], s["src"][0])
    assert M.group_g_loss(3, 2, 1) == (M.G_LOSS[0] / 3, M.G_LOSS[2], M.G_LOSS[5])


def test_the_zero_case_has_a_group_without_any_valid_projection():
    shape, groups, S = M.ZERO
    n = M.counts(shape, groups, S, zero_group=M.ZERO_GROUP)
    assert all(n[s][M.ZERO_GROUP] == 0 for s in range(S)) and all(n[s][g] > 0 for s in range(S) for g in range(groups) if g != M.ZERO_GROUP)
    c = M.group_case(shape, M.SALTS[shape][M.ZERO_GROUP], S, away=True)
    assert G.excluded_fraction(c) <= M.CAP_EXCLUDED and not c["valid_band"].any()
    assert float(c["base"][F64]["m"][0].min()) > 2 and float(c["base"][F64]["m"][1].min()) > 2      # far outside, not on the edge
    assert all(float(x) == 0 for x in c[F64]["G"]) and bool(torch.isfinite(c[F64]["g_depth"]).all())


@pytest.mark.parametrize("B,S", M.OP_CASES)
def test_operator_cases_exclude_nothing_and_open_every_gate(B, S):
    c = M.op_case(B, S)
    assert c["excluded"] == 0
    assert c["count"].shape == (4, S) and int(c["count"].min()) > M.OP_MIN_VALID
    assert c["per_scale"].shape == (4, S) and float(c["per_scale"].min()) > 0
    assert [tuple(c["g_disp"][k].shape) for k in range(4)] == [(B, 1, *hw) for hw in M.SCALE_SHAPES]
    for k in range(4):
        assert float(c["g_disp"][k].abs().max()) > 0 and all(float(c["g_dsrc"][s][k].abs().max()) > 0 for s in range(S))
    assert all(float(t.abs().max()) > 0 for t in c["g_T"])
    assert M.FACTOR == 10 and M.EXISTING_WORST > 0
