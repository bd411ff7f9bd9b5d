"""float64 numpy statement of the two entry points of csrc/bn_train.hip, written from the contracts in include/e2eslam.h, and the
seeded inputs of the cases that tests/test_bn_train_ref.py qualifies against torch.nn.BatchNorm2d (float64) and
tests/test_gpu_bn_train_contracts.py runs on the device.

    fwd(...)  -> y, the pre-activation, save_mean, save_rstd, the updated running_mean / running_var / num_batches_tracked, and the
                 UNDECIDABLE set of the ReLU: |pre-activation| < UNDECIDABLE * max |pre-activation| (an fp32 evaluation may land on
                 either side of zero there; empty without a ReLU);
    bwd(...)  -> dz, dresidual, dgamma, dbeta, and per channel what the undecidable elements could move in dbeta / dgamma:
                 sum |dy| and sum |dy * xhat| over them.

Everything is (P, C): P = B*H*W pixels, NHWC memory."""
import functools

import numpy as np

EPS = 1e-5
UNDECIDABLE = 1e-5
BOUND = 2e-5                # forward outputs, statistics, running buffers: of that output's maximum (conv_fwd_ref.BOUND)
GRAD_BOUND = 5e-5           # gradients (test_gpu_conv_bwd_contracts.GRAD_BOUND)

# name: ((B, H, W, C), relu, residual, channel means in standard deviations)
CASES = {
    "a": ((2, 1, 1, 4), True, True, 0.0),           # P = 2, the smallest legal; dz cancels almost completely
    "b": ((1, 3, 5, 8), True, False, 0.0),          # odd P, one partial quad row
    "c": ((2, 3, 2, 512), True, True, 0.0),         # layer4 of a 64x96 frame: many channels, 12 pixels
    "d": ((2, 16, 24, 64), True, False, 0.0),       # a stage at 64x96
    "e": ((1, 7, 9, 2048), False, False, 0.0),      # Bottleneck width, several channel blocks
    "f": ((2, 32, 48, 64), True, True, 50.0),       # the cancellation case
    "g": ((1, 37, 53, 100), True, True, 0.0),       # C no multiple of 64, odd sizes
    "h": ((2, 60, 80, 64), True, True, 3.0),        # several slices per channel
    "i": ((2, 120, 160, 64), True, False, 0.0),     # the most slices the suite sees
}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Seeded fp32 inputs of a case (read-only arrays, computed once): z, residual, dy (P, C); gamma (positive), gamma_mixed (both
    signs), beta, running_mean, running_var (C)."""
    (B, H, W, C), relu, has_res, off = CASES[name]
    P = B * H * W
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + P)
    sigma = rng.uniform(0.5, 2.0, C)
    mu = rng.normal(0.0, 0.3, C) * sigma + off * sigma * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    t = {
        "z": rng.normal(0.0, 1.0, (P, C)) * sigma + mu,
        "residual": rng.normal(0.0, 1.0, (P, C)),
        "dy": rng.normal(0.0, 1.0, (P, C)),
        "gamma": rng.uniform(0.5, 1.5, C),
        "gamma_mixed": rng.uniform(0.5, 1.5, C) * np.where(rng.random(C) < 0.5, -1.0, 1.0),
        "beta": rng.normal(0.0, 0.5, C),
        "running_mean": rng.normal(0.0, 1.0, C),
        "running_var": rng.uniform(0.5, 1.5, C),
    }
    t = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in t.items()}
    for v in t.values():
        v.setflags(write=False)
    return t


def fwd(z, gamma, beta, residual, relu, eps, momentum, running_mean, running_var, num_batches_tracked):
    """e2e_bn_train_fwd.  gamma / beta / residual / the three running arguments may be None."""
    z = np.asarray(z, np.float64)
    P, C = z.shape
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)                                  # biased
    rstd = 1.0 / np.sqrt(var + eps)
    xhat = (z - mean) * rstd
    pre = xhat * (1.0 if gamma is None else np.asarray(gamma, np.float64)) + (0.0 if beta is None else np.asarray(beta, np.float64))
    if residual is not None:
        pre = pre + np.asarray(residual, np.float64)
    out = {"pre": pre, "y": np.maximum(pre, 0.0) if relu else pre, "save_mean": mean, "save_rstd": rstd, "var": var,
           "undecidable": (np.abs(pre) < UNDECIDABLE * np.abs(pre).max()) if relu else np.zeros(pre.shape, bool)}
    if running_mean is not None:
        out.update(running(mean, var, P, momentum, running_mean, running_var, num_batches_tracked))
    return out


def running(mean, var, P, momentum, running_mean, running_var, num_batches_tracked):
    """The update of the three buffers from a batch's mean and BIASED variance (momentum < 0: nn.BatchNorm2d(momentum=None))."""
    n = int(num_batches_tracked) + 1
    f = momentum if momentum >= 0 else 1.0 / n
    return {"running_mean": (1.0 - f) * np.asarray(running_mean, np.float64) + f * mean,
            "running_var": (1.0 - f) * np.asarray(running_var, np.float64) + f * var * (P / (P - 1.0)),      # unbiased
            "num_batches_tracked": n}


def bwd(dy, mask, z, gamma, save_mean, save_rstd, undecidable=None):
    """e2e_bn_train_bwd.  mask: [y > 0] (None: no ReLU); gamma None: 1."""
    dy, z = np.asarray(dy, np.float64), np.asarray(z, np.float64)
    P, C = z.shape
    g = dy if mask is None else dy * mask
    xhat = (z - np.asarray(save_mean, np.float64)) * np.asarray(save_rstd, np.float64)
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    a = (1.0 if gamma is None else np.asarray(gamma, np.float64)) * np.asarray(save_rstd, np.float64)
    out = {"dz": a * (g - dbeta / P - xhat * dgamma / P), "dresidual": g, "dgamma": dgamma, "dbeta": dbeta, "g": g, "xhat": xhat,
           "dz_scale": np.abs(a) * np.abs(g).max()}
    und = np.zeros(z.shape, bool) if undecidable is None else undecidable
    out["und_dbeta"] = (np.abs(dy) * und).sum(0)
    out["und_dgamma"] = (np.abs(dy * xhat) * und).sum(0)
    return out


def rel(got, ref):
    """max |got - ref| / max |ref|"""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))
