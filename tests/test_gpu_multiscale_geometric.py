"""The geometric-consistency term on every scale of monodepth2's disparity pyramid: ops.warp_photometric_multiscale(geometric=True) and
LOSS.multiscale_geometric of train_depth.Depth_Estimation.

Op.  A 16x32 frame with disparities 16x32, 8x16, 4x8, 2x4, B in {1, 2}, S in {1, 2}, geo_min_valid low enough that every gate opens, against the
float64 composition of tests/multiscale_geo_ref.py (disp_pyramid_ref feeding warp_geo_ref's maps per scale, then the means): the loss,
geometric, geometric_per_scale, geo_count (exact) and the gradient of every target disparity, every source disparity and every pose.  The
bound is a measured one (profiles/multiscale_geo.txt), taken the way tests/test_gpu_multiscale_loss.py takes its own: on the same inputs the
EXISTING per-scale route -- F.interpolate in fp32, ops.depth_from_disp_range for the target and each source, one
ops.warp_photometric_window(geometric=True) per scale, torch's autograd between them -- was held against float64, and the new route is allowed
ten times the largest max|x - r64| / max|r64| any quantity of any case showed there (multiscale_geo_ref.EXISTING_WORST).  Each case prints
both routes' figures before it asserts.

Driver.  One step of Depth_Estimation with the monodepth2 network, DATA.scales [0,1,2,3], 96x128 (where the reference's gate of 10000 is open),
frames (0, -1).  With LOSS.multiscale, LOSS.geometric and LOSS.multiscale_geometric the heads of scales 1-3 get a gradient, geo_count exceeds
10000 on every scale, the grouped pair is launched once each way and e2e_warp_photo_geo_fwd not at all, and the loss is the per-scale
operator composition's within the bound above; without the new key the launch list and the loss are those of a config that never had it; the
two ValueErrors and the unchanged NotImplementedError."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import disp_head_ref as DH
import multiscale_geo_ref as M
from oracle import depthnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = M.FACTOR * M.EXISTING_WORST
PAD = "border"                       # multiscale_geo_ref.PAD = 1


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


class _Recorder:
    """the names of the entry points that go through L.call while it is active"""

    def __init__(self, L):
        self.L, self.names = L, []

    def __enter__(self):
        self.real = self.L.call
        self.L.call = lambda name, *a, **k: (self.names.append(name), self.real(name, *a, **k))[1]
        return self

    def __exit__(self, *exc):
        self.L.call = self.real


def _rel(x, r64):
    return float((x.detach().cpu().double().reshape(r64.shape) - r64).abs().max()) / float(r64.abs().max())


# ---- op -------------------------------------------------------------------------------------------------------------------------------
def _inputs(B, S):
    """the case's operands on the GPU: every disparity and pose a leaf; with B = 1 the frames are NCHW views of NHWC memory"""
    s = M.op_scene(B)
    frame = (lambda t: t.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)) if B == 1 else (lambda t: t.to(DEV))
    leaf = lambda t: t.to(DEV).requires_grad_(True)
    n = len(M.SCALE_SHAPES)
    mode = M.MODE[S]
    return dict(disps=[leaf(s["disps"][k]) for k in range(n)], dsrcs=[[leaf(s["dsrc_disps"][j][k]) for k in range(n)] for j in range(S)],
                srcs=[frame(t) for t in s["src"][:S]], tgt=frame(s["tgt"]), K=s["K"].to(DEV), invK=s["invK"].to(DEV),
                Ts=[leaf(t) for t in s["T"][:S]], noise=s["noise"][:, :S].contiguous().to(DEV),
                flags=dict(min_reprojection=bool(mode[1]), auto_masking=bool(mode[2])))


def _existing_route(t):
    """what a user can assemble without the feature -> (loss, geometric (S,), per scale (G,S) detached, geo_count (G,S))"""
    from e2ehip import ops
    up = lambda d: ops.depth_from_disp_range(F.interpolate(d, size=M.SIZE, mode="bilinear", align_corners=False), *M.LIMITS, M.SCALE)
    photo, geo, count = [], [], []
    for k, d in enumerate(t["disps"]):
        out = ops.warp_photometric_window(up(d), t["srcs"], t["tgt"], t["K"], t["invK"], t["Ts"], padding_mode=PAD, use_mask=True,
                                          tie_noise=t["noise"], geometric=True, depth_srcs=[up(p[k]) for p in t["dsrcs"]],
                                          geo_min_valid=M.OP_MIN_VALID, **t["flags"])
        photo.append(out["photometric"])
        geo.append(out["geometric"])
        count.append(out["geo_count"])
    geo = torch.stack(geo)
    return torch.stack(photo).mean(), geo.mean(0), geo.detach(), torch.stack(count)


def _new_route(t):
    from e2ehip import ops
    L = _L()
    with _Recorder(L) as rec:
        out = ops.warp_photometric_multiscale(t["disps"], t["srcs"], t["tgt"], t["K"], t["invK"], t["Ts"], *M.LIMITS, M.SCALE, padding_mode=PAD,
                                              use_mask=True, tie_noise=t["noise"], geometric=True, disp_srcs=t["dsrcs"],
                                              geo_min_valid=M.OP_MIN_VALID, **t["flags"])
    S = len(t["srcs"])
    assert rec.names == ["e2e_disp_pyramid_depth_fwd"] * (1 + S) + ["e2e_warp_photo_geo_groups_fwd"], rec.names
    assert not out["geometric_per_scale"].requires_grad and not out["photometric_per_scale"].requires_grad and out["geometric"].requires_grad
    assert out["geo_count"].dtype == torch.int32 and out["geometric"].shape == (S,)
    return out["photometric"], out["geometric"], out["geometric_per_scale"], out["geo_count"]


def figures(B, S, route):
    """{quantity: max|x - r64| / max|r64|} of one route on one case; geo_count is held exactly"""
    L = _L()
    c = M.op_case(B, S)
    t = _inputs(B, S)
    loss, geometric, per_scale, count = route(t)
    assert count.shape == (len(M.SCALE_SHAPES), S) and torch.equal(count.cpu().long(), c["count"]), (count.tolist(), c["count"].tolist())
    with _Recorder(L) as rec:
        (loss + sum(M.OP_WEIGHTS[j] * geometric[j] for j in range(S))).backward()
    if route is _new_route:                                                   # one autograd node covers the pair
        assert sorted(rec.names) == ["e2e_disp_pyramid_depth_bwd"] * (1 + S) + ["e2e_warp_photo_geo_groups_bwd"], rec.names
    out = {"loss": _rel(loss, c["loss"]), "geometric": _rel(geometric, c["geometric"]), "per_scale": _rel(per_scale, c["per_scale"])}
    for k, d in enumerate(t["disps"]):
        out[f"g_disp{k}"] = _rel(d.grad, c["g_disp"][k])
        for j in range(S):
            out[f"g_dsrc{j}_{k}"] = _rel(t["dsrcs"][j][k].grad, c["g_dsrc"][j][k])
    for j, T in enumerate(t["Ts"]):
        out[f"g_T{j}"] = _rel(T.grad, c["g_T"][j])
    return out


@pytest.mark.parametrize("B,S", M.OP_CASES)
def test_multiscale_geometric_against_float64(B, S):
    assert M.op_case(B, S)["excluded"] == 0
    old, new = figures(B, S, _existing_route), figures(B, S, _new_route)
    for q in new:
        print(f"multiscale geometric B={B} S={S} {q}: existing route {old[q]:.3g}, new route {new[q]:.3g}, bound {BOUND:.3g}")
    worst = max(new, key=new.get)
    assert new[worst] <= BOUND, (worst, new[worst], BOUND)


def test_multiscale_geometric_refusals_and_defaults():
    from e2ehip import ops
    L = _L()
    t = _inputs(1, 2)
    args = (t["disps"], t["srcs"], t["tgt"], t["K"], t["invK"], t["Ts"], *M.LIMITS, M.SCALE)
    with pytest.raises(ValueError, match="disp_srcs"):
        ops.warp_photometric_multiscale(*args, geometric=True)
    with pytest.raises(ValueError, match="disp_srcs"):
        ops.warp_photometric_multiscale(*args, geometric=True, disp_srcs=t["dsrcs"][:1])
    with pytest.raises(ValueError, match="disp_srcs"):
        ops.warp_photometric_multiscale(*args, geometric=True, disp_srcs=[t["dsrcs"][0], t["dsrcs"][1][:3]])
    with pytest.raises(ValueError, match="disp_srcs"):
        ops.warp_photometric_multiscale(*args, geometric=True, disp_srcs=[t["dsrcs"][0], t["dsrcs"][1][::-1]])
    with pytest.raises(ValueError, match="geo_min_valid"):
        ops.warp_photometric_multiscale(*args, geometric=True, disp_srcs=t["dsrcs"], geo_min_valid=-1)
    for name in ("K", "invK"):
        bad = list(args)
        bad[3 if name == "K" else 4] = t[name].clone().requires_grad_()
        with pytest.raises(NotImplementedError, match="inv_K" if name == "invK" else "K"):
            ops.warp_photometric_multiscale(*bad, geometric=True, disp_srcs=t["dsrcs"])
    with _Recorder(L) as rec:                                                 # the defaults leave today's call as it is
        out = ops.warp_photometric_multiscale(*args)
    assert sorted(out) == ["depth", "photometric", "photometric_per_scale"]
    assert rec.names == ["e2e_disp_pyramid_depth_fwd", "e2e_warp_photo_window_fwd"], rec.names


# ---- driver ---------------------------------------------------------------------------------------------------------------------------
H, W = 96, 128
SCALES = [0, 1, 2, 3]
GROUPED = ["e2e_warp_photo_geo_groups_fwd", "e2e_warp_photo_geo_groups_bwd"]


def _config(key="absent", multiscale=True, geometric=True):
    from train_depth import default_config
    cfg = default_config(H, W, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.MODEL.depth_network = "monodepth2"
    cfg.DATA.scales = SCALES
    cfg.LOSS.multiscale, cfg.LOSS.geometric = multiscale, geometric
    if key != "absent":
        cfg.LOSS.multiscale_geometric = key
    return cfg


def _step(cfg, spy_composition=False):
    """one step -> (loss, driver, launched entry points of the step itself, the composition's loss, geo_count (G,S) the op returned)"""
    from e2ehip import ops
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation
    L = _L()
    seq = make_sequence(2, H, W, seed=5)
    de = Depth_Estimation(cfg, sequence=seq, state_dict=DH.split_state_dict(depthnet.random_state_dict(0), SCALES))
    seen = dict(composed=None, count=None)
    fused, real_op = de.compute_losses_fused, ops.warp_photometric_multiscale

    def op(*a, **k):
        out = real_op(*a, **k)
        if "geo_count" in out:
            seen["count"] = out["geo_count"].cpu()
        return out

    with _Recorder(L) as rec, contextlib.redirect_stdout(io.StringIO()):
        def spy(inputs):
            first = len(rec.names)
            with torch.no_grad():                                             # the operator route on what the step is about to see
                up = lambda d: ops.depth_from_disp_range(F.interpolate(d, size=(H, W), mode="bilinear", align_corners=False), cfg.DATA.min_depth,
                                                         cfg.DATA.max_depth, de._depth_scale)
                photo, geo = [], []
                for s in SCALES:
                    out = ops.warp_photometric_window(up(inputs["disp", de._tgt_index, s]), [inputs["source_frame", -1]], inputs["target_frame"],
                                                      inputs["K"], inputs["Inverse_K"], [inputs["T", -1]], padding_mode=cfg.MODEL.padding_mode,
                                                      use_mask=True, geometric=True, depth_srcs=[up(inputs["disp", de._src_index[-1], s])])
                    photo.append(out["photometric"])
                    geo.append(out["geometric"])
                seen["composed"] = float(torch.stack(photo).mean() + torch.stack(geo).mean(0).mean() * cfg.LOSS.geometric_weight)
            del rec.names[first:]                                             # the composition's own launches are not the step's
            return fused(inputs)
        if spy_composition:
            de.compute_losses_fused = spy
        ops.warp_photometric_multiscale = op
        try:
            log = de.train()
        finally:
            ops.warp_photometric_multiscale = real_op
    return log[0], de, rec.names, seen["composed"], seen["count"]


def _head_grads(de):
    named = dict(de.models["depth_decoder"].named_parameters())
    return {s: [p.grad for n, p in named.items() if n.startswith(f"decoder.{10 + s}.")] for s in SCALES}


def test_driver_multiscale_geometric_trains_the_coarse_heads_on_one_grouped_pair():
    loss, de, launched, composed, count = _step(_config(True), spy_composition=True)
    heads = _head_grads(de)
    for s in SCALES:
        assert heads[s] and all(g is not None and float(g.abs().max()) > 0 for g in heads[s]), f"the head of scale {s} got no gradient"
    assert count.shape == (len(SCALES), 1) and int(count.min()) > 10000, count.tolist()                  # the reference's gate is open on every scale
    assert [launched.count(n) for n in GROUPED] == [1, 1], launched
    assert not [n for n in launched if n.startswith("e2e_warp_photo_") and n not in GROUPED], launched     # no e2e_warp_photo_geo_fwd, no window, no pair
    assert launched.count("e2e_disp_pyramid_depth_fwd") == 2 and launched.count("e2e_disp_pyramid_depth_bwd") == 2
    print(f"driver LOSS.multiscale_geometric: loss {loss:.8g}, operator composition {composed:.8g}, relative {abs(loss / composed - 1):.3g}, "
          f"bound {BOUND:.3g}, geo_count {count.tolist()}")
    assert abs(loss - composed) <= BOUND * abs(composed)


def test_driver_without_the_key_is_todays_step():
    absent = _step(_config("absent", geometric=False))
    false = _step(_config(False, geometric=False))
    assert false[2] == absent[2] and false[0] == absent[0]
    assert not [n for n in absent[2] if "geo" in n] and absent[2].count("e2e_warp_photo_fwd") == 1


def test_driver_refusals():
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation
    seq = make_sequence(2, H, W, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="LOSS.multiscale_geometric"):
            Depth_Estimation(_config(True, multiscale=False), sequence=seq)
        with pytest.raises(ValueError, match="LOSS.multiscale_geometric"):
            Depth_Estimation(_config(True, geometric=False), sequence=seq)
        for key in (False, "absent"):
            with pytest.raises(NotImplementedError, match="LOSS.multiscale.*LOSS.geometric"):
                Depth_Estimation(_config(key), sequence=seq)
