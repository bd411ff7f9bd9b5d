"""LOSS.geometric / smoothness / auto_masking / min_reprojection on the captured launch plan (e2e_warp_photo_terms_lossgrad,
e2e_smoothness_norm_lossgrad, e2ehip.fused.TermsLossGradPlan, RefineStepPlan(geometric=..., ...), SLAM.plan_loss_terms) against the
oracle's Refiner.flagged_image_losses in float64 and against the operator-by-operator form (SLAM.refinement_autograd)."""
import types

import numpy as np
import pytest
import torch

from median_pin import PinnedSLAM, pin
from oracle import depthnet, refine, warp_loss

pytestmark = pytest.mark.gpu
GRAD_TOL = 1e-4          # per tensor, relative to its largest element (tests/test_gpu_driver.py)
VALUE_RTOL = 1e-4        # the bound csrc/warp_photo_fused.hip states for this path
FLAG_SETS = [("geometric",), ("smoothness",), ("auto_masking",), ("min_reprojection",), ("geometric", "smoothness"),
             ("min_reprojection", "auto_masking"), ("geometric", "smoothness", "min_reprojection", "auto_masking")]
SHAPES = [(120, 160), (118, 150), (480, 640)]
# the terms kernel below one 32x16 tile and with a one-column last tile (the shapes tests/test_gpu_warp_photo.py gives the default kernel),
# for the two configurations that need no 10000 valid projections
SMALL_SHAPES = [(8, 33), (20, 70)]
SMALL_FLAG_SETS = [("auto_masking",), ("min_reprojection", "auto_masking")]
SHAPE_FLAGS = [(h, w, f) for h, w in SHAPES for f in FLAG_SETS] + [(h, w, f) for h, w in SMALL_SHAPES for f in SMALL_FLAG_SETS]
# inputs per shape: seeds for which the fp32 oracle stays inside the kink allowance against the fp64 oracle for every configuration below
# (evaluated on the CPU alone; _inputs' docstring) -- the allowance is then not spent on the comparand's own rounding
SEEDS = {(120, 160): 5, (118, 150): 5, (480, 640): 5, (64, 96): 5, (8, 33): 5, (20, 70): 5}
W_GEO, W_SMOOTH, W_REG = 0.5, 1e-3, 1e-2
NEAR_RY = 30.0           # degrees about y: 120x160 then keeps just under 10000 of its 19200 projections inside (asserted where used)


def kink_cap(n):
    """Pixels that may sit on a kink of the loss (the minimum's selection, clamp, |.|, the valid border, a bilinear tap boundary):
    the allowance tests/test_gpu_driver.py gives d loss / d depth."""
    return max(4, 1e-3 * n)


def _inputs(H, W, seed, rz=1.0, ry=0.5, t=(0.05, 0.01, 0.02)):
    """One keyframe pair as independent leaves: target / source depth, their regulariser references, the source frame's disparity.
    tests/synth.py's generators; a seed is used only if fp32-oracle vs fp64-oracle gradients stay inside kink_cap for every
    configuration (compare() asserts it again for the configuration at hand)."""
    from synth import make_pair, smooth_depth
    s = make_pair(H, W, seed=seed, rz=rz, ry=ry, t=t)
    g = torch.Generator().manual_seed(seed + 1000)
    s["depth_src"] = smooth_depth(H, W, g)
    s["init_tgt"] = s["depth"] + 0.02 * torch.randn(1, 1, H, W, generator=g)
    s["init_src"] = s["depth_src"] + 0.02 * torch.randn(1, 1, H, W, generator=g)
    s["disp_src"] = 1.0 / smooth_depth(H, W, g)
    s["noise"] = 0.02 * torch.randn(1, 1, H, W, generator=g)
    return s


def oracle_eval(s, flags, padding, mask, reg, dtype, noise=None, w_geo=W_GEO):
    """Refiner.flagged_image_losses (+ the regulariser of refine_pair) on the leaves of `s` in `dtype`.
    -> dict(photo, reg, geo, smooth, total, g_tgt, g_src, g_disp, count)"""
    c = lambda x: x.to(dtype)
    d_tgt, d_src, disp = (c(s[k]).clone().requires_grad_(True) for k in ("depth", "depth_src", "disp_src"))
    src, tgt = c(s["src"]).permute(0, 3, 1, 2), c(s["tgt"]).permute(0, 3, 1, 2)
    K, invK, T = c(s["K"]), c(s["invK"]), c(s["T"])

    def run(wg, ws):
        cfg = refine.Config()
        cfg.padding_mode, cfg.photometric_mask = padding, mask
        for f in flags:
            setattr(cfg, f, True)
        cfg.geometric_weight, cfg.smoothness_weight = wg, ws
        cfg.tie_break_noise = None if noise is None else c(noise)
        me = types.SimpleNamespace(cfg=cfg, disps=[disp, None])
        return refine.Refiner.flagged_image_losses(me, [d_src, d_tgt], src, tgt, K, invK, T)
    total, photo = run(w_geo, W_SMOOTH)
    out = {"photo": float(photo.detach()), "reg": 0.0}
    with torch.no_grad():
        out["geo"] = float(run(1.0, 0.0)[0] - photo) if "geometric" in flags else 0.0
        out["smooth"] = float(run(0.0, 1.0)[0] - photo) if "smoothness" in flags else 0.0
        _, valid = warp_loss.project(warp_loss.backproject(d_tgt, invK), K, T, *tgt.shape[2:])
        out["count"] = int(valid.sum())
    if reg:
        r = warp_loss.depth_regularizer(c(s["init_src"]), d_src, reg) + warp_loss.depth_regularizer(c(s["init_tgt"]), d_tgt, reg)
        total = total + W_REG * r
        out["reg"] = float(r.detach())
    total.backward()
    z = lambda t, like: torch.zeros_like(like) if t.grad is None else t.grad
    out.update(total=float(total.detach()), g_tgt=z(d_tgt, d_tgt).detach(), g_src=z(d_src, d_src).detach(), g_disp=z(disp, disp).detach())
    return out


def gpu_eval(s, flags, padding, mask, reg, noise=None, w_geo=W_GEO):
    from e2ehip.fused import TermsLossGradPlan
    dev = torch.device("cuda")
    H, W = s["depth"].shape[2:]
    plan = TermsLossGradPlan(1, H, W, dev, padding, mask, reg, 1.0, W_REG if reg else 0.0, w_geometric=w_geo, w_smoothness=W_SMOOTH,
                             **{f: True for f in flags})
    t = {k: v.to(dev).contiguous() for k, v in s.items()}
    plan.g_depth_src.zero_()
    plan.bind(t["depth"], t["depth_src"], t["init_tgt"] if reg else None, t["init_src"] if reg else None,
              t["src"].permute(0, 3, 1, 2), t["tgt"].permute(0, 3, 1, 2), t["K"], t["invK"], t["T"])
    if noise is not None:
        assert plan.noise is not None
        plan.noise.copy_(noise.to(dev))
    _, g_tgt, g_src = plan.step()
    g_disp = torch.zeros(1, 1, H, W, device=dev)
    plan.smoothness_step(t["disp_src"], g_disp)
    torch.cuda.synchronize()
    l5 = plan.loss5.cpu().double()
    total = float(l5[0] + (W_REG * l5[1] if reg else 0.0) + plan.weighted_extra().cpu().double())
    return dict(photo=float(l5[0]), reg=float(l5[1]), geo=float(l5[2]), smooth=float(l5[3]), count=int(l5[4]), total=total,
                g_tgt=g_tgt.cpu().double(), g_src=g_src.cpu().double() if plan.writes_g_depth_src else torch.zeros(1, 1, H, W).double(),
                g_disp=g_disp.cpu().double())


def grad_outliers(a, ref):
    """(pixels beyond GRAD_TOL of the reference's max, that max)"""
    m = float(ref.abs().max())
    return int(((a.double() - ref.double()).abs() > GRAD_TOL * m).sum()), m


def compare(gpu, ora, ora32, n, what):
    print(f"[{what}] " + " ".join(f"{k}: {gpu[k]:.9g} / {ora[k]:.9g}" for k in ("photo", "reg", "geo", "smooth", "total")) + f" count {gpu['count']} / {ora['count']}")
    stats = {}
    for k in ("g_tgt", "g_src", "g_disp"):
        stats[k] = (grad_outliers(gpu[k], ora[k]), grad_outliers(ora32[k], ora[k])[0])
    print(f"[{what}] gradient pixels beyond {GRAD_TOL} of max (GPU vs fp64 (n, max), fp32 oracle vs fp64): {stats}")
    for k in ("photo", "reg", "geo", "smooth", "total"):
        np.testing.assert_allclose(gpu[k], ora[k], rtol=VALUE_RTOL, atol=1e-12, err_msg=f"{what}: {k}")
    for k, ((n_out, gmax), n32) in stats.items():
        assert n32 <= kink_cap(n), f"{what}: the input does not qualify -- fp32 oracle vs fp64 oracle: {n32} pixels of {k} beyond the bound"
        if gmax == 0.0:
            assert float(gpu[k].abs().max()) == 0.0, f"{what}: {k} must be exactly zero"
        else:
            assert n_out <= kink_cap(n), f"{what}: {k}: {n_out} pixels beyond {GRAD_TOL} of max {gmax:.3e} (allowed {kink_cap(n)})"


@pytest.mark.parametrize("reg", [None, "l1", "l2"], ids=["noreg", "l1", "l2"])
@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("padding", ["border", "zeros"])
@pytest.mark.parametrize("H,W,flags", SHAPE_FLAGS, ids=[f"{h}x{w}-" + "+".join(f) for h, w, f in SHAPE_FLAGS])
def test_terms_lossgrad_vs_fp64_oracle(H, W, flags, padding, mask, reg):
    """Loss components and d/d depth_tgt, d/d depth_src, d/d disp[0] of the new entry points against the float64 oracle: values to
    1e-4 relative; gradients to 1e-4 of the tensor's maximum with at most max(4, 1e-3 N) pixels exempt (kinks), after checking that
    the fp32 oracle itself stays inside that allowance on this input.  118x150 is no multiple of the 32x16 tile; 8x33 is lower than a
    tile with one column in its last tile, 20x70 has a 4-row and a 6-column remainder.  The allowance max(4, 1e-3 N) is 4 pixels at both
    small shapes, against the 8 pixels of 8x33's one-column tile: a fault in half of that column would pass, one in all of it would not."""
    s = _inputs(H, W, SEEDS[(H, W)])
    ora = oracle_eval(s, flags, padding, mask, reg, torch.float64)
    ora32 = oracle_eval(s, flags, padding, mask, reg, torch.float32)
    gpu = gpu_eval(s, flags, padding, mask, reg)
    if "geometric" in flags:
        assert ora["count"] > 10000 and abs(gpu["count"] - ora["count"]) <= 4 and ora["geo"] > 0.0
    compare(gpu, ora, ora32, H * W, f"{H}x{W} {'+'.join(flags)} {padding} mask={mask} reg={reg}")


def test_geometric_term_needs_more_than_10000_valid_pixels():
    """losses.py:84-95: `if mask.sum() > 10000` else a constant 0.  64x96 has 6144 pixels: term and gradients exactly 0 (so the 64x96
    driver comparisons never see a non-zero geometric term); 120x160 with the usual pair: non-zero (covered above, re-asserted);
    120x160 with a pair rotated so far that just under 10000 projections stay inside: exactly 0 again."""
    for (H, W), kw, live in (((64, 96), {}, False), ((120, 160), {}, True), ((120, 160), dict(ry=NEAR_RY), False)):
        s = _inputs(H, W, SEEDS[(H, W)], **kw)
        ora = oracle_eval(s, ("geometric",), "border", True, None, torch.float64)
        ora32 = oracle_eval(s, ("geometric",), "border", True, None, torch.float32)
        gpu = gpu_eval(s, ("geometric",), "border", True, None)
        print(f"[10000 rule {H}x{W} {kw}] valid: gpu {gpu['count']} oracle {ora['count']}; geometric term gpu {gpu['geo']} oracle {ora['geo']}")
        assert abs(gpu["count"] - ora["count"]) <= 4
        if live:
            assert ora["count"] > 10000 and gpu["geo"] > 0.0 and float(gpu["g_src"].abs().max()) > 0.0
        else:
            assert ora["count"] <= 10000 and ora["geo"] == 0.0
            if kw:
                assert 9000 <= ora["count"] < 10000, ora["count"]           # "just below"
            assert gpu["geo"] == 0.0 and float(gpu["g_src"].abs().max()) == 0.0
            # ... and nothing of it in d/d depth_tgt: bit-identical with any weight on the term
            heavy = gpu_eval(s, ("geometric",), "border", True, None, w_geo=1000.0)
            assert torch.equal(heavy["g_tgt"], gpu["g_tgt"])
        compare(gpu, ora, ora32, H * W, f"10000 rule {H}x{W} {kw}")


def test_tie_break_noise_changes_the_selection_and_matches_the_oracle():
    """min_reprojection + auto_masking: a fixed noise plane on the identity map (online_adaption.py:498).  Crafted so that the plane
    matters: its amplitude (0.02) is of the size of the difference of the two maps, so the per-pixel minimum picks differently."""
    import torch.nn.functional as F
    H, W = 120, 160
    flags = ("min_reprojection", "auto_masking")
    s = _inputs(H, W, SEEDS[(H, W)])
    noise = s["noise"]
    # the oracle's selection with and without the plane
    d = s["depth"].double()
    src, tgt = s["src"].double().permute(0, 3, 1, 2), s["tgt"].double().permute(0, 3, 1, 2)
    synth, valid, _ = warp_loss.inverse_warp(d, src, s["K"].double(), s["invK"].double(), s["T"].double(), "border")
    rep, ident = warp_loss.photometric(synth * valid, tgt * valid), warp_loss.photometric(src * valid, tgt * valid)
    changed = int(((ident <= rep) != (ident + noise.double() <= rep)).sum())
    assert changed >= 1
    res = {}
    for name, nz in (("plain", None), ("noise", noise)):
        ora = oracle_eval(s, flags, "border", True, "l2", torch.float64, noise=nz)
        ora32 = oracle_eval(s, flags, "border", True, "l2", torch.float32, noise=nz)
        gpu = gpu_eval(s, flags, "border", True, "l2", noise=nz)
        compare(gpu, ora, ora32, H * W, f"tie-break {name} ({changed} selections differ)")
        res[name] = gpu
    assert res["plain"]["photo"] != res["noise"]["photo"] and not torch.equal(res["plain"]["g_tgt"], res["noise"]["g_tgt"])


# ---- driver level -------------------------------------------------------------------------------------------------------------------
def _cfg(H, W, L, flags):
    from online_adaption import default_config
    cfg = default_config(H, W, L)
    cfg.DEMO.frame_threshold = 0.0
    for f in flags:
        setattr(cfg.LOSS, f, True)
    return cfg


def _sd():
    sd = depthnet.random_state_dict(0)
    sd["decoder.decoder.10.conv.weight"] = sd["decoder.decoder.10.conv.weight"] * 40.0       # unique median (tests/test_gpu_driver.py)
    return sd


class _zero_randn:
    """The reference's random tie-break noise switched off (as test_off_by_default_loss_flags_vs_oracle does)."""

    def __enter__(self):
        self.real = torch.randn
        torch.randn = lambda *a, **k: torch.zeros(*a, **{kk: v for kk, v in k.items() if kk == "device"})

    def __exit__(self, *exc):
        torch.randn = self.real


def test_flagged_run_rides_on_the_captured_plan():
    """geometric + smoothness with plan_loss_terms: main() builds the step plan and its backward graph is captured.  (Without the
    feature the run falls back to refinement_autograd: step_plan stays None.)"""
    import online_adaption as oa
    from e2ehip.synthetic import make_sequence
    H, W, L = 64, 96, 2
    cfg = _cfg(H, W, L, ("geometric", "smoothness"))
    slam = oa.SLAM(cfg, sequence=make_sequence(L, H, W, seed=21), state_dict=_sd())
    assert slam.plan_loss_terms is False, "default off"
    slam.plan_loss_terms = True
    slam.main()
    assert slam.step_plan is not None
    assert any(isinstance(k, tuple) and k[0] == "bwd" for k in slam.step_plan._graphs), list(slam.step_plan._graphs)
    assert len(slam.log) == 3 and slam.map.M >= H * W
    cfg.LOSS.supervise_depth = True
    assert not slam._plan_eligible()                   # the one flag that stays on the autograd form
    slam.close()


DRIVER_FLAGS = [("geometric", "smoothness"), ("min_reprojection", "auto_masking"), ("auto_masking",),
                ("geometric", "smoothness", "min_reprojection", "auto_masking")]


@pytest.mark.parametrize("flags", DRIVER_FLAGS, ids=["+".join(f) for f in DRIVER_FLAGS])
@pytest.mark.parametrize("H,W", [(64, 96), (128, 160)], ids=["64x96", "128x160"])
def test_plan_loss_flags_vs_oracle_two_keyframes(H, W, flags):
    """test_off_by_default_loss_flags_vs_oracle's comparison through the launch plan: 3 refinement steps over the first keyframe and 3
    over a second one (3-D loss active), loss / photometric / regulariser at 2e-4, ratio at 1e-4 (that test's bounds), tie-break noise
    zero on both sides.  The one discrete choice of a step -- which near-tied prediction is the median element -- is the oracle's
    (PinnedSLAM.median_elements, as in test_tum_shaped_sequence_vs_oracle_first_keyframe).  128x160 rather than 120x160: the launch plan
    needs height and width to be multiples of 32 (e2ehip.netplan); 20480 pixels keep the geometric term live (> 10000 valid)."""
    from e2ehip.synthetic import make_sequence
    L = 3
    seq = make_sequence(L, H, W, seed=21)
    sd = _sd()
    cfg = _cfg(H, W, L, flags)
    ocfg = refine.Config()
    for f in flags:
        setattr(ocfg, f, True)
    cfg.LOSS.geometric_weight, cfg.LOSS.smoothness_weight = ocfg.geometric_weight, ocfg.smoothness_weight
    colors, gt, K, poses = seq
    ora = refine.Refiner(sd, ocfg)
    recs = []
    for a, b in ((0, 1), (1, 2)):
        recs += ora.refine_pair(colors[:, [a, b]], gt[:, [a, b]], poses[:, [a, b]], K)
    assert len(recs) == 6 and "knn" in recs[3]
    with _zero_randn():
        slam = PinnedSLAM(cfg, sequence=seq, state_dict=sd)
        slam.plan_loss_terms = True
        slam.median_elements = [pin(r["median_indices"], "cuda") for r in recs]
        slam.main()
    assert slam.step_plan is not None and any(isinstance(k, tuple) and k[0] == "bwd" for k in slam.step_plan._graphs)
    log = torch.stack(slam.log)
    print(f"[plan flags {H}x{W} {flags}] loss {log[:, 0].tolist()} vs {[r['loss'] for r in recs]}; photometric {log[:, 1].tolist()} vs "
          f"{[r['photometric'] for r in recs]}; 3-D {log[:, -1].tolist()} vs {[r.get('knn', 0.0) for r in recs]}")
    np.testing.assert_allclose(log[:, 0].numpy(), [r["loss"] for r in recs], rtol=2e-4)
    np.testing.assert_allclose(log[:, 1].numpy(), [r["photometric"] for r in recs], rtol=2e-4)
    np.testing.assert_allclose(log[:, 2].numpy(), [r["reg"] for r in recs], rtol=2e-4, atol=1e-9)
    np.testing.assert_allclose(log[:, 3].numpy(), [r["ratio"] for r in recs], rtol=1e-4)
    assert slam.map.M >= H * W
    slam.close()


def test_plan_form_equals_autograd_form_and_replay_equals_eager():
    """All four flags at 128x160 (a multiple of 32, as the launch plan needs; the geometric term is live there): the 48 parameter gradients of the first step through the plan
    against SLAM.refinement_autograd + compute_flagged_losses (operator-by-operator kernels) within GRAD_TOL of each tensor's maximum;
    then the SAME step again from the same state as a replay of the captured graph -- every captured argument is constant, so it
    reproduces the eager execution.  d/d depth_src is a float-atomic scatter (include/e2eslam.h): a different arrival order moves a
    pixel's gradient by about one fp32 ulp (2^-24 relative), and a parameter gradient is a sum over the H*W pixels, so two executions
    may differ by sqrt(H*W) * 2^-24 of a tensor's maximum (8.5e-6 here) -- that is the bound, instead of bit equality."""
    import online_adaption as oa
    from e2ehip.synthetic import make_sequence
    H, W, L = 128, 160, 2
    flags = ("geometric", "smoothness", "min_reprojection", "auto_masking")
    seq, sd = make_sequence(L, H, W, seed=21), _sd()

    def first_moments(slam):
        opt = slam.optimizer
        offs = {id(p): o for p, o in zip(opt.flat.params, opt.flat.offsets)}
        return {k: (opt.m[offs[id(p)]:offs[id(p)] + p.numel()].clone() / 0.1) for k, p in slam.models["depth"].named_parameters() if id(p) in offs and p.requires_grad}

    with _zero_randn():
        plan = oa.SLAM(_cfg(H, W, L, flags), sequence=seq, state_dict=sd)
        plan.plan_loss_terms = True
        plan.set_refinement_mode()
        plan.first_iter = True
        sp = plan._step_plan()
        opt = plan.optimizer
        opt._resident_state()
        w0 = [p.detach().clone() for p in opt.flat.params]
        counter0 = opt._counter.clone()
        plan._load_pair(sp, 0, 1)
        sp.step(True, None)                                     # eager (and captured right after)
        elems = [(sp.delta.reshape(-1) == sp.md).nonzero().reshape(-1).to(torch.int32)]
        g_eager = first_moments(plan)
        assert float(sp.loss.loss5[4]) > 10000 and float(sp.loss.loss5[2]) > 0.0 and float(sp.loss.loss5[3]) > 0.0
        with torch.no_grad():                                   # back to the initial state, then the captured graph
            for p, w in zip(opt.flat.params, w0):
                p.data.copy_(w)
            opt.m.zero_()
            opt.v.zero_()
            opt._counter.copy_(counter0)
        sp.net.refresh_layouts()
        assert any(isinstance(k, tuple) and k[0] == "bwd" for k in sp._graphs)
        sp.step(True, None)
        g_replay = first_moments(plan)
        auto = PinnedSLAM(_cfg(H, W, L, flags), sequence=seq, state_dict=sd)
        assert not auto.plan_loss_terms and not auto._plan_eligible()
        auto.median_elements = elems
        auto.set_refinement_mode()
        auto.first_iter = True
        auto.refinement_autograd(0, 1, max_steps=1)
        g_auto = first_moments(auto)
    assert len(g_eager) == 48 and sorted(g_auto) == sorted(g_eager)
    worst_a, worst_r = (0.0, ""), (0.0, "")
    for k in g_eager:
        m = float(g_auto[k].abs().max()) + 1e-30
        worst_a = max(worst_a, (float((g_eager[k] - g_auto[k]).abs().max()) / m, k))
        worst_r = max(worst_r, (float((g_replay[k] - g_eager[k]).abs().max()) / (float(g_eager[k].abs().max()) + 1e-30), k))
    print(f"[plan vs autograd] worst parameter-gradient difference / tensor max: {worst_a}; replay vs eager: {worst_r}")
    assert worst_a[0] <= GRAD_TOL, worst_a
    assert worst_r[0] <= (H * W) ** 0.5 * 2.0 ** -24, worst_r
    plan.close()
    auto.close()
