"""monodepth2's multi-scale smoothness on the GPU: ops.disp_pyramid_smoothness and LOSS.multiscale_smoothness of
train_depth.Depth_Estimation.

Op.  ops.disp_pyramid_smoothness on the `four`, `ragged` and `anisotropic` cases of tests/pyramid_smoothness_ref.py against its float64
reference under its derived bounds: the weighted value, the per-scale values, and the gradients through torch.autograd.grad with an upstream
gradient that is not 1 (a power of two, so that the bound scales with it exactly); the loss-only call under torch.no_grad(); the ValueErrors.

Driver.  One step of Depth_Estimation as tests/test_gpu_multiscale_loss.py sets it up (monodepth2 network, DATA.scales [0,1,2,3], 64 x 96,
two frames) with LOSS.multiscale and LOSS.smoothness on and the new key True, False and absent.  With True the new entry point is launched
exactly once and e2e_smoothness_lossgrad / e2e_mean_normalize not at all, and the step's loss is the loss of the absent run minus its
scale-0 smoothness term plus the operator composition of the multi-scale term (F.avg_pool2d, ops.mean_normalize, ops.smoothness per scale,
taken by a spy under no_grad on the same inputs) -- within the measured relative bound times the margin of tests/multiscale_loss_ref.py
(FACTOR * EXISTING_WORST), of the loss.  With False or absent the launch list and the loss are the same and the new entry point is absent."""
import contextlib
import io

import pytest
import torch
import torch.nn.functional as F

import disp_head_ref as DH
import multiscale_loss_ref as M
import pyramid_smoothness_ref as R
from oracle import depthnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = M.FACTOR * M.EXISTING_WORST
UPSTREAM = -4.0


# ---- op -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["four", "ragged", "anisotropic"])
def test_disp_pyramid_smoothness_op(name):
    from e2ehip import ops
    c = R.case(name)
    keys = sorted(c["disps"])
    leaves = [c["disps"][k].to(DEV).requires_grad_(True) for k in keys]
    img = c["img"].to(DEV)
    out = ops.disp_pyramid_smoothness(leaves, img, weights=[c["weights"][k] for k in keys])
    assert out["smoothness"].dim() == 0 and out["smoothness"].requires_grad
    assert out["smoothness_per_scale"].shape == (len(keys),) and not out["smoothness_per_scale"].requires_grad
    grads = torch.autograd.grad(out["smoothness"], leaves, torch.tensor(UPSTREAM, device=DEV))
    got = dict(loss={k: out["smoothness_per_scale"][i].cpu() for i, k in enumerate(keys)}, total=out["smoothness"].detach().cpu(),
               grad={k: grads[i].cpu() / UPSTREAM for i, k in enumerate(keys)})
    worst = R.worst(got, c)
    print(f"ops.disp_pyramid_smoothness {name}: of the bounds: " + ", ".join(f"{q} {v:.3g}" for q, v in worst.items()))
    assert max(worst.values()) <= 1, worst
    with torch.no_grad():                                                     # the loss-only call: the same bits, no graph
        alone = ops.disp_pyramid_smoothness(leaves, img, weights=[c["weights"][k] for k in keys])
    assert not alone["smoothness"].requires_grad and torch.equal(alone["smoothness"], out["smoothness"].detach())
    assert torch.equal(alone["smoothness_per_scale"], out["smoothness_per_scale"])


def test_disp_pyramid_smoothness_default_weights_and_partial_grad():
    """weights default to 1 a scale; a disparity that needs no gradient gets none, the others theirs"""
    from e2ehip import ops
    c = R.case("four")
    keys = sorted(c["disps"])
    leaves = [c["disps"][k].to(DEV).requires_grad_(k != 1) for k in keys]
    out = ops.disp_pyramid_smoothness(leaves, c["img"].to(DEV))
    ref_total = sum(c["ref"]["loss"][k] for k in keys)
    tol = sum(c["bounds"]["loss"][k] for k in keys) + R.EPS * abs(ref_total)
    assert abs(out["smoothness"].item() - float(ref_total)) <= float(tol)
    out["smoothness"].backward()
    assert leaves[1].grad is None
    for i, k in enumerate(keys):
        if k != 1:
            err = ((leaves[i].grad.cpu().double() - c["ref"]["grad"][k] / c["weights"][k]).abs() / (c["bounds"]["grad"][k] / abs(c["weights"][k]))).max()
            assert float(err) <= 1, (k, float(err))


def test_disp_pyramid_smoothness_refuses():
    from e2ehip import ops
    img = torch.rand(2, 3, 32, 64, device=DEV)
    d = lambda h, w, B=2, C=1: torch.rand(B, C, h, w, device=DEV)
    for disps, kw in (([], {}), ([d(32, 64)] * 5, {}), ([d(32, 64, C=2)], {}), ([d(32, 64)[0]], {}), ([d(32, 64, B=1)], {}),
                      ([d(64, 64)], {}), ([d(32, 128)], {}),                  # larger than the image
                      ([d(1, 64)], {}), ([d(32, 1)], {}),                     # an axis of one pixel
                      ([d(24, 64)], {}), ([d(32, 48)], {}),                   # no integer ratio
                      ([d(32, 64), d(16, 32)], dict(weights=[1.0]))):
        with pytest.raises(ValueError):
            ops.disp_pyramid_smoothness(disps, img, **kw)
    with pytest.raises(ValueError):
        ops.disp_pyramid_smoothness([d(32, 64)], img[:, :2])


# ---- driver ---------------------------------------------------------------------------------------------------------------------------
H, W = 64, 96
SCALES = [0, 1, 2, 3]


def _config(key="absent", multiscale=True, smoothness=True):
    from train_depth import default_config
    cfg = default_config(H, W, (0, -1), 1)
    cfg.DEBUG.print_metrics = False
    cfg.MODEL.depth_network = "monodepth2"
    cfg.DATA.scales = SCALES
    cfg.LOSS.multiscale = multiscale
    cfg.LOSS.smoothness = smoothness
    cfg.LOSS.smoothness_weight = 1.0                                          # (default 1e-3: the term would vanish below the loss's bound)
    if key != "absent":
        cfg.LOSS.multiscale_smoothness = key
    return cfg


@pytest.fixture(scope="module")
def steps():
    """one step with the key True, False and absent on the same sequence and weights -> {key: (loss, launched entry points, and for True
    the spy's (scale-0 term of today, operator composition of the multi-scale term), both times LOSS.smoothness_weight)}"""
    from e2ehip import ops, profile
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation
    seq = make_sequence(2, H, W, seed=5)
    parts = DH.split_state_dict(depthnet.random_state_dict(0), SCALES)
    out = {}
    for key in (True, False, "absent"):
        cfg = _config(key)
        de = Depth_Estimation(cfg, sequence=seq, state_dict=parts)
        spied = []
        term = de.compute_smoothness_loss

        def spy(inputs, cfg=cfg, term=term, spied=spied):
            with torch.no_grad():
                img = inputs["target_frame"]
                today = ops.smoothness(ops.mean_normalize(inputs["disp", 0, 0]), img)
                composed = 0
                for s in SCALES:
                    d = inputs["disp", 0, s]
                    img_s = F.avg_pool2d(img, (img.shape[2] // d.shape[2], img.shape[3] // d.shape[3]))
                    composed = composed + ops.smoothness(ops.mean_normalize(d), img_s) / (2 ** s * len(SCALES))
                spied.append((float(today) * cfg.LOSS.smoothness_weight, float(composed) * cfg.LOSS.smoothness_weight))
            return term(inputs)
        if key is True:                                                        # False and absent run unobserved: today's launch list
            de.compute_smoothness_loss = spy
        with profile.KernelTimer() as timer, contextlib.redirect_stdout(io.StringIO()):
            log = de.train()
        out[key] = (log[0], [r[0] for r in timer.rows], spied[0] if spied else None)
    return out


def test_driver_multiscale_smoothness(steps):
    loss, launched, (today, composed) = steps[True]
    absent_loss, absent_launched, _ = steps["absent"]
    assert launched.count("e2e_disp_pyramid_smoothness_lossgrad") == 1
    # the spy's own compositions launch e2e_smoothness_lossgrad and e2e_mean_normalize 1 + len(SCALES) times each; the step adds none
    assert launched.count("e2e_smoothness_lossgrad") == 1 + len(SCALES) and launched.count("e2e_mean_normalize") == 1 + len(SCALES)
    assert absent_launched.count("e2e_smoothness_lossgrad") == 1 and absent_launched.count("e2e_mean_normalize") == 2
    # the runs share the sequence and the weights, so the scale-0 term the spy took is the term the absent run added
    expected = absent_loss - today + composed
    print(f"driver LOSS.multiscale_smoothness: loss {loss:.9g}, expected {expected:.9g} (scale-0 term {today:.6g}, multi-scale term "
          f"{composed:.6g}), relative {abs(loss / expected - 1):.3g}, bound {BOUND:.3g}")
    assert abs(loss - expected) <= BOUND * abs(expected)
    assert composed != today


@pytest.mark.parametrize("key", [False, "absent"])
def test_driver_without_the_key_is_todays_step(steps, key):
    loss, launched, _ = steps[key]
    assert "e2e_disp_pyramid_smoothness_lossgrad" not in launched
    assert launched == steps["absent"][1] and loss == steps["absent"][0]


def test_driver_refusals():
    from e2ehip.synthetic import make_sequence
    from train_depth import Depth_Estimation
    seq = make_sequence(2, H, W, seed=5)
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError, match="LOSS.multiscale_smoothness.*LOSS.multiscale.*LOSS.smoothness"):
            Depth_Estimation(_config(True, multiscale=False), sequence=seq)
        with pytest.raises(ValueError, match="LOSS.multiscale_smoothness.*LOSS.multiscale.*LOSS.smoothness"):
            Depth_Estimation(_config(True, smoothness=False), sequence=seq)
