"""Host only: the float64 references and the cases of tests/disp_pyramid_ref.py, which tests/test_gpu_disp_pyramid_contracts.py and
tests/test_gpu_multiscale_loss.py hold csrc/disp_pyramid.hip against.

  - the reference's forward is float64 F.interpolate(bilinear, align_corners=False) + the conversion formula, its adjoint is autograd;
  - the footprint a coarse index is said to own is exactly the set of fine indices whose stencil touches it (a brute-force table);
  - every case reaches the regimes its entry claims;
  - a fine pixel missing from a footprint moves g_disp by at least 100 times the bound, so the bound can tell;
  - the built library exports the entry points, the header parses, and the GPU contract module calls every entry point of the file."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import disp_pyramid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(R.CASES)
ENTRY_POINTS = ("e2e_disp_pyramid_depth_fwd", "e2e_disp_pyramid_depth_bwd")


def _case(name):
    c = R.CASES[name]
    disps, g = R.inputs(name)
    return c, disps, g, (c["size"], *c["limits"], c["scale"])


@pytest.mark.parametrize("name", CASES)
def test_reference_forward_is_interpolate_and_the_conversion(name):
    c, disps, _, args = _case(name)
    lo, hi = 1 / c["limits"][1], 1 / c["limits"][0]
    want = torch.stack([c["scale"] / (lo + (hi - lo) * F.interpolate(disps[k].double(), size=c["size"], mode="bilinear", align_corners=False))
                        for k in sorted(disps)])
    got = R.pyramid_depth(disps, *args)
    assert got.shape == (len(disps), c["B"], 1, *c["size"]) and got.dtype == torch.float64
    assert ((got - want).abs() <= 1e-13 * want.abs()).all()


@pytest.mark.parametrize("name", CASES)
def test_reference_adjoint_is_autograd(name):
    c, disps, g, args = _case(name)
    leaves = {k: v.double().requires_grad_(True) for k, v in disps.items()}
    want = torch.autograd.grad((R.pyramid_depth(leaves, *args) * g.double()).sum(), [leaves[k] for k in sorted(leaves)])
    got = R.pyramid_depth_bwd(g, disps, *args)
    for k, w in zip(sorted(disps), want):
        assert got[k].shape == disps[k].shape
        assert (got[k] - w).abs().max() <= 1e-12 * w.abs().max()


@pytest.mark.parametrize("name", CASES)
def test_footprint_is_the_set_of_fine_indices_whose_stencil_touches(name):
    c = R.CASES[name]
    for shape in c["scales"].values():
        for n, N in zip(shape, c["size"]):
            y0, y1, wy = R.stencil(n, N)
            assert ((0 <= y0) & (y0 <= y1) & (y1 < n) & (0 <= wy) & (wy < 1)).all()
            owners = [set() for _ in range(n)]
            for y in range(N):                                                  # the brute-force table
                owners[int(y0[y])].add(y)
                owners[int(y1[y])].add(y)
            for j in range(n):
                first, last = R.footprint(j, n, N)
                assert owners[j] == set(range(first, last + 1)), (name, n, N, j)
            assert torch.allclose(R.axis_matrix(n, N).sum(0), torch.ones(N, dtype=torch.float64), rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", CASES)
def test_case_reaches_its_regimes(name):
    c = R.CASES[name]
    H, W = c["size"]
    seen = set()
    if len(c["scales"]) < 4 and sorted(c["scales"]) != list(range(len(c["scales"]))):
        seen.add("absent")                                                      # a NULL slot before a present one
    for shape in c["scales"].values():
        clamped = [[bool(((2 * torch.arange(N) + 1) * n - N < 0).any()), bool((R.stencil(n, N)[0] + 1 > n - 1).any())]
                   for n, N in zip(shape, c["size"])]
        if clamped[0][0] and clamped[1][0]:
            seen.add("clamped_sy")
        if clamped[0][1] and clamped[1][1]:
            seen.add("clamped_y1")
        if shape == (1, 1):
            seen.add("all_clamped")
        if tuple(shape) == tuple(c["size"]):
            seen.add("identity")
        if not R.exact_ratio(shape, c["size"]):
            seen.add("inexact")
        lanes = R.lanes_per_pixel(shape, c["size"])
        if lanes == 64:
            seen.add("wave_per_pixel")
        per_group = R.BWD_THREADS // lanes
        if -(-H // R.FWD_TILE[0]) * -(-W // R.FWD_TILE[1]) > 1 and shape[0] * shape[1] > per_group:
            seen.add("multi_tile")                                              # several workgroups a plane, forward and backward
        # the forward tile's edge inside a footprint (a coarse column owns fine columns on both sides of column 64), ragged last tiles
        # both ways, and a backward workgroup that ends inside a coarse row
        if (W % R.FWD_TILE[1] and H % R.FWD_TILE[0] and per_group % shape[1]
                and any(a < R.FWD_TILE[1] <= b for a, b in (R.footprint(i, shape[1], W) for i in range(shape[1])))):
            seen.add("tile_edge")
    assert c["reaches"] <= seen, (name, sorted(c["reaches"] - seen))


@pytest.mark.parametrize("name", CASES)
def test_a_dropped_fine_pixel_moves_the_gradient_by_100_bounds(name):
    """What a footprint walk that misses one fine pixel would give, against the bound the GPU module applies: for the coarse pixels at
    two corners and in the middle, the fine pixel with the largest term of the footprint's sum.  (A pixel in the corner of a 16 x 16
    footprint has weight 1/256 and moves the sum by a few bounds only: the bound grows with the footprint.)"""
    c, disps, g, args = _case(name)
    gu = R.g_u(g, disps, *args)
    for s, k in enumerate(sorted(disps)):
        shape = disps[k].shape[2:]
        full, tol = R.gather(gu[s], shape, c["size"]), R.bwd_tolerance(gu[s], shape, c["size"])
        My, Mx = R.axis_matrix(shape[0], c["size"][0]), R.axis_matrix(shape[1], c["size"][1])
        for j, i in {(0, 0), (shape[0] - 1, shape[1] - 1), (shape[0] // 2, shape[1] // 2)}:
            for b in range(c["B"]):
                term = My[j][:, None] * Mx[i][None, :] * gu[s][b, 0].abs()
                y, x = divmod(int(term.argmax()), c["size"][1])
                moved = (R.gather(gu[s], shape, c["size"], drop=(y, x)) - full)[b, 0, j, i].abs()
                assert moved >= 100 * tol[b, 0, j, i], (name, k, (j, i), (y, x), float(moved / tol[b, 0, j, i]))


def test_library_exports_the_entry_points_and_the_header_parses():
    import e2ehip
    from e2ehip import _lib
    lib = e2ehip.load()
    with open(os.path.join(ROOT, "include", "e2eslam.h")) as f:
        protos, _ = _lib.parse_header(f.read())
    for name in ENTRY_POINTS:
        assert name in protos and hasattr(lib, name), name
    assert [p for p, _ in protos["e2e_disp_pyramid_depth_fwd"][1]] == \
        ["disp0", "disp1", "disp2", "disp3", "h0", "w0", "h1", "w1", "h2", "w2", "h3", "w3", "B", "H", "W", "min_depth", "max_depth", "scale",
         "depth", "stream"]
    assert [p for p, _ in protos["e2e_disp_pyramid_depth_bwd"][1]] == \
        ["g_depth", "disp0", "disp1", "disp2", "disp3", "h0", "w0", "h1", "w1", "h2", "w2", "h3", "w3", "B", "H", "W", "min_depth", "max_depth",
         "scale", "g_disp0", "g_disp1", "g_disp2", "g_disp3", "stream"]


def test_every_entry_point_of_the_file_has_a_contract_case():
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    proto = r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\("
    declared = set(re.findall(proto, read("include", "e2eslam.h"), re.M))
    implemented = set(re.findall(proto, read("end-to-end-self-supervised-slam_amd", "csrc", "disp_pyramid.hip"), re.M))
    assert implemented == set(ENTRY_POINTS) and implemented <= declared
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", read("tests", "test_gpu_disp_pyramid_contracts.py")))
    assert not implemented - called, f"no contract case calls {sorted(implemented - called)}"
