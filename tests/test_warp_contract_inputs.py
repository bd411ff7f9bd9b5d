"""Host-only: the inputs of tests/test_gpu_warp_photo_contracts.py, built through the same helpers (tests/warp_contract_ref.py).  Every case
excludes at most 1 % of its elements by the kink rules, keeps its planted on-kink samples under 5 %, and really holds the edges it is there
for: depths that are zero and negative, points behind the camera and on both sides of z_out's clamp outside the gate's band, samples on pixel
centres and on +-1, the four memory layouts, all-zero windows, y == x, pixels that leave the image."""
import pytest
import torch

import warp_contract_ref as R
from oracle import warp_loss as wl

F64, F32 = R.F64, R.F32


def _share(mask):
    return float(mask.float().mean()) if mask.numel() else 0.0


@pytest.mark.parametrize("shape", R.BHW_SHAPES, ids=str)
def test_backproject_inputs(shape):
    c = R.backproject_case(*shape)
    B, H, W = shape
    assert (c["depth"] == 0).any() and (c["depth"] < 0).any() and (c["depth"] > 0).any()
    assert (c["invK"][:, 0, 1] != 0).all()                             # skew
    assert B == 1 or not torch.equal(c["invK"][0], c["invK"][1])
    assert torch.equal(c[F64]["cam"][:, 3], torch.ones(B, H * W, dtype=F64))
    assert c["g_cam"][:, 3].abs().min() > 0 or H * W > 100             # row 3 of the upstream gradient is live
    assert (shape == R.BHW_SHAPES[-1]) == (H * W > 2048 * 256) and (H * W <= 2049 * 256)


@pytest.mark.parametrize("shape", R.BHW_SHAPES, ids=str)
def test_project_inputs(shape):
    c = R.project_case(*shape)
    B, H, W = shape
    r64, kind = c[F64], c["kind"]
    assert set(c["points"][:, 3].unique().tolist()) == {0.5, 1.0, 2.0}
    assert (c["T"][:, :3, :3] - torch.eye(3)).abs().amax((1, 2)).min() > 0.05 and c["T"][:, :3, 3].abs().min() > 0
    assert _share(c["valid_band"]) <= 0.01 and _share(c["gate_band"]) <= 0.01
    assert 0.2 < _share(r64["valid"] > 0) < 0.9                        # both sides of max|grid| = 1
    if H * W < 10000:
        for b in range(B):
            assert all((kind[b] == k).sum() >= (1 if H * W < 10 else 2) for k in (R.BEHIND, R.NEAR_BELOW, R.NEAR_ABOVE))
        c2 = r64["c2"]
        assert (c2[kind == R.BEHIND] < -0.4).all()
        assert ((c2[kind == R.NEAR_BELOW] > 0) & (c2[kind == R.NEAR_BELOW] < R.ZCLAMP)).all()
        assert ((c2[kind == R.NEAR_ABOVE] > R.ZCLAMP) & (c2[kind == R.NEAR_ABOVE] < 1.25e-3)).all()
        assert not c["gate_band"][kind != R.ORDINARY].any()            # the planted points are off the gate's band: all of them are compared
        assert (c2[kind == R.ORDINARY] > 0.4).all()
        # the gradient through z_out differs from the one without exactly where c2 is above the clamp
        dz = (r64["g_points_z"] - r64["g_points"]).abs().amax(1)
        assert (dz[c2 > R.ZCLAMP] > 0).all() and (dz[c2 < R.ZCLAMP] == 0).all()
        assert r64["g_points"][:, 3].abs().min() > 0                   # the w row is live
    else:
        assert not c["near"].any()


GS_ALL = R.GS_CASES + [(R.GS_LOOP, "nchw"), (R.GS_CONVERT, "nchw")]


@pytest.mark.parametrize("shape,layout", GS_ALL, ids=str)
def test_grid_sample_inputs(shape, layout):
    B, C, Hi, Wi, Ho, Wo = shape
    view = R.layout_view(layout, R.grid_sample_case(shape, layout, 1, 0)["base"], B)
    assert view.shape == (B, C, Hi, Wi)
    if layout == "nhwc":
        assert view.stride(1) == 1 and (C == 1 or not view.is_contiguous())
    if layout == "cols":
        assert view.stride(3) == 2 and view.stride(2) == 2 * Wi
    if layout == "expand":
        assert view.stride(0) == 0 and B == 2
    for pad, align in ((1, 0),) if shape == R.GS_CONVERT else ((0, 0), (0, 1), (1, 0), (1, 1)):
        c = R.grid_sample_case(shape, layout, pad, align)
        n_pl = int(c["planted"].sum())
        assert _share(c["kink"]) <= 0.01, (pad, align, _share(c["kink"]))
        assert n_pl < 0.05 * B * Ho * Wo and (n_pl >= 2 or Ho * Wo < 40)
        assert float(c["grid"].min()) < -1.2 and float(c["grid"].max()) > 1.2 or Ho * Wo < 40
        if n_pl >= 2:
            gp = c["grid"][c["planted"]]
            ix = R.source_index(gp[:, 0], Wi, align, F64)
            assert ((ix - ix.round()).abs() < 1e-4).any(), "no sample on a pixel centre"
            assert (gp.abs() == 1).any(), "no sample on +-1"
    assert (shape == R.GS_CONVERT) == (B * C * Hi * Wi > 4096 * 256)
    assert (shape == R.GS_LOOP) == (Ho * Wo > 2048 * 256)


@pytest.mark.parametrize("kind", R.PH_KINDS)
@pytest.mark.parametrize("shape", R.PH_SHAPES, ids=str)
def test_photometric_inputs(shape, kind):
    c = R.photometric_case(shape, kind)
    B, C, H, W = shape
    x, y = c["x"], c["y"]
    for dt in (F64, F32):                                              # the unclamped value is the oracle's, bit for bit
        assert torch.equal(R.ssim_unclamped(x.to(dt), y.to(dt)).clamp(0, 1), wl.ssim(x.to(dt), y.to(dt)))
    for up in R.PH_UPSTREAM:
        assert _share(c["excluded"][up]) <= 0.01, (up, _share(c["excluded"][up]))
    assert all(b >= 0 for b in c["bound"].values()) and c["bound"]["ssim"] > 0 and c["bound"]["gx_ps"] > 0
    if kind == "same":
        assert torch.equal(x, y) and not c[F64]["ssim"].any() and not c[F64]["pmap"].any()
        assert torch.equal(x, R.photometric_case(shape, "uniform")["x"]) and not c[F32]["ssim"].any()
        assert all(c["bound"][k] == R.CAP * float(v.abs().max()) for k, v in R.photometric_case(shape, "uniform")[F64].items())
    if kind == "masked":
        zero = R.zero_region(H, W)
        assert not x[:, :, zero].any() and not y[:, :, zero].any() and x[:, :, ~zero].all()
        windows = ~R.dilate(~zero[None], 1)[0]                         # windows that read zeros only (reflection stays inside the region's rows)
        if W >= 3:
            assert windows.any() and not c[F64]["ssim"][:, :, windows].any()
        if H >= 7 and W >= 7:
            assert zero[1:6, 1:6].all() and zero[:, W - 1].all() and windows[3, 3]
    if kind == "randn":
        assert (x < 0).any() and (y < 0).any()
    if kind == "uniform":
        assert 0 < float(c[F64]["ssim"].min()) and float(c[F64]["ssim"].max()) < 1


@pytest.mark.parametrize("shape", R.FUSED_SHAPES, ids=str)
def test_fused_inputs(shape):
    B, H, W = shape
    for pad in (0, 1):
        for use_mask in (0, 1):
            for reg_kind in (0, 1, 2):
                c = R.fused_case(shape, pad, use_mask, reg_kind)
                assert not c["valid_band"].any()                       # so the two losses compare as they are
                assert _share(c["grad_excluded"]) <= 0.01, (pad, use_mask, reg_kind, _share(c["grad_excluded"]))
                assert not c["pmap_excluded"].any() and not c["reg_excluded_t"].any() and not c["reg_excluded_s"].any()
                out = _share(c[F64]["valid"] == 0)
                assert H * W < 15 or 0.05 < out < 0.7, out             # some pixels leave the image, most stay
                if use_mask and H * W >= 15:
                    assert (R.ssim_unclamped(c[F64]["synth"] * c[F64]["valid"][:, None], c["scene"]["tgt"].double() * c[F64]["valid"][:, None]) == 0).any() \
                        or H * W < 100                                 # all-zero windows, as in every real step
