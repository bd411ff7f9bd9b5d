"""monodepth2's multi-scale photometric loss on the GPU: ops.disp_pyramid_depth, ops.warp_photometric_multiscale and LOSS.multiscale of
train_depth.Depth_Estimation.

Ops.  The pyramid op against the float64 reference of tests/disp_pyramid_ref.py under its derived bounds.  The multi-scale loss against the
float64 composition of tests/multiscale_loss_ref.py (the reference pyramid feeding the oracle's warp and photometric loss per scale, then the
mean) on its four admitted cases: the loss, photometric_per_scale, the gradient of every disparity and of every pose.  That bound is a
measured one (profiles/disp_pyramid.txt): on the same inputs the EXISTING route -- F.interpolate in fp32, ops.depth_from_disp_range and one
ops.warp_photometric / warp_photometric_window per scale, torch's autograd between them -- was held against float64; the new route is allowed
ten times the largest max|x - r64| / max|r64| any quantity of any case showed there (multiscale_loss_ref.EXISTING_WORST), the margin
profiles/slam_grad_contracts.txt took for its measured bound: two fp32 routes that sum in different orders.  Each case prints both routes'
figures before it asserts.

Driver.  One step of Depth_Estimation with the monodepth2 network, DATA.scales [0,1,2,3], 64 x 96, two frames: with LOSS.multiscale the heads
of scales 1-3 get a gradient, the two pyramid entry points are launched and the loss is the operator composition's; without it (False or
absent) nothing of that happens and the launch list is the same as ever; the three refusals."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import disp_head_ref as DH
import disp_pyramid_ref as DP
import multiscale_loss_ref as M
from oracle import depthnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = M.FACTOR * M.EXISTING_WORST
DP_PAD = "border"                    # multiscale_loss_ref.PAD = 1


def _rel(x, r64):
    return float((x.detach().cpu().double() - r64).abs().max()) / float(r64.abs().max())


# ---- ops ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["four", "zero_two", "ragged", "one_pixel"])
def test_disp_pyramid_depth_op(name):
    from e2ehip import ops
    c = DP.CASES[name]
    cpu_disps, cpu_g = DP.inputs(name)
    leaves = [cpu_disps[k].to(DEV).requires_grad_(True) for k in sorted(cpu_disps)]
    depth = ops.disp_pyramid_depth(leaves, c["size"], *c["limits"], c["scale"])
    assert depth.shape == (len(leaves), c["B"], 1, *c["size"])
    grads = torch.autograd.grad(depth, leaves, cpu_g.to(DEV))
    args = (c["size"], *c["limits"], c["scale"])
    ref, ref_g, gu = DP.pyramid_depth(cpu_disps, *args), DP.pyramid_depth_bwd(cpu_g, cpu_disps, *args), DP.g_u(cpu_g, cpu_disps, *args)
    for s, k in enumerate(sorted(cpu_disps)):
        shape = tuple(cpu_disps[k].shape[2:])
        ef = ((depth[s].detach().cpu().double() - ref[s]).abs() / (DP.fwd_ops(shape, c["size"]) * DP.EPS * ref[s].abs())).max()
        eb = ((grads[s].cpu().double() - ref_g[k]).abs() / DP.bwd_tolerance(gu[s], shape, c["size"])).max()
        print(f"ops.disp_pyramid_depth {name} scale {k}: fwd {float(ef):.3g} bwd {float(eb):.3g} of their bounds")
        assert ef <= 1 and eb <= 1
    if tuple(cpu_disps[min(cpu_disps)].shape[2:]) == tuple(c["size"]):           # the full-size scale is depth_from_disp_range, bit for bit
        assert torch.equal(depth[0], ops.depth_from_disp_range(leaves[0].detach(), *c["limits"], c["scale"]))


def _inputs(B, mode):
    """the case's operands on the GPU: disparities and poses as leaves; with B = 1 the frames are NCHW views of NHWC memory"""
    s = M.case(B, mode)["scene"]
    S = mode[0]
    frame = (lambda t: t.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)) if B == 1 else (lambda t: t.to(DEV))
    return dict(disps=[s["disps"][k].to(DEV).requires_grad_(True) for k in range(len(M.SHAPES))], srcs=[frame(t) for t in s["src"][:S]],
                tgt=frame(s["tgt"]), K=s["K"].to(DEV), invK=s["invK"].to(DEV), Ts=[t.to(DEV).requires_grad_(True) for t in s["T"][:S]],
                noise=s["noise"].to(DEV) if mode == M.WINDOW else None, flags=dict(min_reprojection=bool(mode[1]), auto_masking=bool(mode[2])))


def _existing_route(t):
    """F.interpolate in fp32 + ops.depth_from_disp_range + one fused pair per scale, torch's autograd between them -> (loss, per_scale)"""
    from e2ehip import ops
    per_scale = []
    for d in t["disps"]:
        depth = ops.depth_from_disp_range(F.interpolate(d, size=M.SIZE, mode="bilinear", align_corners=False), *M.LIMITS, M.SCALE)
        if len(t["srcs"]) == 1 and not any(t["flags"].values()):
            out = ops.warp_photometric(depth, t["srcs"][0], t["tgt"], t["K"], t["invK"], t["Ts"][0], padding_mode=DP_PAD, use_mask=True)
        else:
            out = ops.warp_photometric_window(depth, t["srcs"], t["tgt"], t["K"], t["invK"], t["Ts"], padding_mode=DP_PAD, use_mask=True,
                                              tie_noise=t["noise"], **t["flags"])
        per_scale.append(out["photometric"])
    per_scale = torch.stack(per_scale)
    return per_scale.mean(), per_scale.detach()


def _new_route(t):
    from e2ehip import ops
    out = ops.warp_photometric_multiscale(t["disps"], t["srcs"], t["tgt"], t["K"], t["invK"], t["Ts"], *M.LIMITS, M.SCALE, padding_mode=DP_PAD,
                                          use_mask=True, tie_noise=t["noise"], **t["flags"])
    assert not out["photometric_per_scale"].requires_grad and out["depth"].shape == (len(M.SHAPES), t["tgt"].shape[0], 1, *M.SIZE)
    return out["photometric"], out["photometric_per_scale"]


def figures(B, mode, route):
    """{quantity: max|x - r64| / max|r64|} of one route on one case"""
    c = M.case(B, mode)
    t = _inputs(B, mode)
    loss, per_scale = route(t)
    loss.backward()
    out = {"loss": _rel(loss, c["loss"]), "per_scale": _rel(per_scale, c["per_scale"])}
    for k, d in enumerate(t["disps"]):
        out[f"g_disp{k}"] = _rel(d.grad, c["g_disp"][k])
    for j, T in enumerate(t["Ts"]):
        out[f"g_T{j}"] = _rel(T.grad, c["g_T"][j])
    return out


@pytest.mark.parametrize("B,mode", M.CASES)
def test_multiscale_loss_against_float64(B, mode):
    assert M.case(B, mode)["excluded"] == 0
    old, new = figures(B, mode, _existing_route), figures(B, mode, _new_route)
    for q in new:
        print(f"multiscale B={B} mode={mode} {q}: existing route {old[q]:.3g}, new route {new[q]:.3g}, bound {BOUND:.3g}")
    worst = max(new, key=new.get)
    assert new[worst] <= BOUND, (worst, new[worst], BOUND)


def test_multiscale_loss_is_deterministic_and_expands_one_pose():
    """two calls give the same bits; a (4,4) pose expanded over a batch of two gets the sum over the batch and the scales"""
    from e2ehip import ops
    t = _inputs(2, M.PAIR)
    T = t["Ts"][0][0].detach().clone().requires_grad_(True)
    runs = []
    for _ in range(2):
        out = ops.warp_photometric_multiscale(t["disps"], t["srcs"], t["tgt"], t["K"], t["invK"], [T.expand(2, 4, 4)], *M.LIMITS, M.SCALE)
        runs.append((out["photometric"].detach(),) + torch.autograd.grad(out["photometric"], t["disps"] + [T]))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert runs[0][-1].shape == (4, 4) and float(runs[0][-1].abs().max()) > 0


# ---- driver ---------------------------------------------------------------------------------------------------------------------------
H, W = 64, 96
SCALES = [0, 1, 2, 3]


def _config(multiscale="absent", network="monodepth2", **loss):
    from train_depth import default_config
    cfg = default_config(H, W, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.MODEL.depth_network = network
    cfg.DATA.scales = SCALES if network == "monodepth2" else [0]
    if multiscale != "absent":
        cfg.LOSS.multiscale = multiscale
    for k, v in loss.items():
        setattr(cfg.LOSS, k, v)
    return cfg


@pytest.fixture(scope="module")
def steps():
    """one step with the key True, False and absent on the same sequence and weights -> {key: (loss, driver, launched entry points, the
    composition's loss)}"""
    from e2ehip import ops, profile
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation
    seq = make_sequence(2, H, W, seed=5)
    parts = DH.split_state_dict(depthnet.random_state_dict(0), SCALES)
    out = {}
    for key in (True, False, "absent"):
        cfg = _config(key)
        de = Depth_Estimation(cfg, sequence=seq, state_dict=parts)
        composed = []
        fused = de.compute_losses_fused

        def spy(inputs, de=de, cfg=cfg, fused=fused, composed=composed):
            with torch.no_grad():                                            # the operator route on what the step is about to see
                per_scale = []
                for s in SCALES:
                    up = F.interpolate(inputs["disp", de._tgt_index, s], size=(H, W), mode="bilinear", align_corners=False)
                    depth = ops.depth_from_disp_range(up, cfg.DATA.min_depth, cfg.DATA.max_depth, de._depth_scale)
                    per_scale.append(ops.warp_photometric(depth, inputs["source_frame", -1], inputs["target_frame"], inputs["K"], inputs["Inverse_K"],
                                                          inputs["T", -1], padding_mode=cfg.MODEL.padding_mode, use_mask=True)["photometric"])
                composed.append(float(torch.stack(per_scale).mean()))
            return fused(inputs)
        if key is True:
            de.compute_losses_fused = spy
        with profile.KernelTimer() as timer, contextlib.redirect_stdout(io.StringIO()):
            log = de.train()
        out[key] = (log[0], de, [r[0] for r in timer.rows], composed[0] if composed else None)
    return out


def _head_grads(de):
    named = dict(de.models["depth_decoder"].named_parameters())
    return {s: [p.grad for n, p in named.items() if n.startswith(f"decoder.{10 + s}.")] for s in SCALES}


def test_driver_multiscale_trains_the_coarse_heads(steps):
    loss, de, launched, composed = steps[True]
    heads = _head_grads(de)
    for s in SCALES:
        assert heads[s] and all(g is not None and float(g.abs().max()) > 0 for g in heads[s]), f"the head of scale {s} got no gradient"
    spied = launched.count("e2e_warp_photo_fwd") - 1                          # the composition's own launches, one pair forward per scale
    assert spied == len(SCALES)
    assert launched.count("e2e_disp_pyramid_depth_fwd") == 1 and launched.count("e2e_disp_pyramid_depth_bwd") == 1
    print(f"driver LOSS.multiscale: loss {loss:.8g}, operator composition {composed:.8g}, relative {abs(loss / composed - 1):.3g}, bound {BOUND:.3g}")
    assert abs(loss - composed) <= BOUND * abs(composed)


@pytest.mark.parametrize("key", [False, "absent"])
def test_driver_without_the_key_is_todays_step(steps, key):
    loss, de, launched, _ = steps[key]
    heads = _head_grads(de)
    assert heads[0] and all(g is not None and float(g.abs().max()) > 0 for g in heads[0])
    for s in SCALES[1:]:
        assert all(g is None or float(g.abs().max()) == 0 for g in heads[s]), f"the head of scale {s} got a gradient"
    assert not [n for n in launched if n.startswith("e2e_disp_pyramid_")]
    assert launched == steps["absent"][2] and loss == steps["absent"][0]


def test_driver_refusals():
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation
    seq = make_sequence(2, H, W, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="LOSS.multiscale"):
            Depth_Estimation(_config(True, network="indoor"), sequence=seq)
        with pytest.raises(NotImplementedError, match="LOSS.multiscale.*LOSS.geometric"):
            Depth_Estimation(_config(True, geometric=True), sequence=seq)
        with pytest.raises(NotImplementedError, match="LOSS.multiscale.*fused_losses"):
            Depth_Estimation(_config(True), sequence=seq, fused_losses=False)
