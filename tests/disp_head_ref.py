"""Float64 references of the contracts include/e2eslam.h states for csrc/disp_heads.hip (host only; no tests in this file), written from
the header's comments:

    e2e_disp_head_fwd          y  = act(bias + conv3x3(reflection_pad_1(x), w)),  x (B,H,W,Cin) NHWC, w (1,Cin,3,3), y (B,H,W)
    e2e_disp_head_bwd          dz = dy * act'(y) from the activation's OUTPUT; dx, dw, dbias = the convolution's adjoints of dz
    e2e_disp_range_depth_fwd   depth  = scale / (lo + (hi - lo) disp),  lo = 1 / max_depth, hi = 1 / min_depth
    e2e_disp_range_depth_bwd   g_disp = -g_depth scale (hi - lo) / (lo + (hi - lo) disp)^2

torch.nn.functional and autograd in float64 on the CPU (float32 when asked: the input qualification of tests/test_disp_head_ref.py, after
tests/conv_fwd_ref.py -- a case is used only if the float32 evaluation stays within a quarter of the bound of the float64 one).  Also a
plain-torch restatement of the monodepth2 network (ResnetEncoder + DepthDecoder with a sigmoid head at every scale) on oracle.depthnet's
encoder and decoder layout, and the oracle trainer of the driver's monodepth2 branch.  The GPU modules and the host check share the
deterministic inputs below."""
import zlib

import torch
import torch.nn.functional as F

from conv_fwd_ref import BOUND, QUALIFY, rel  # noqa: F401  (the project's forward bound and error measure)
from oracle import depthnet
from oracle import train_depth as otd

ACT_NONE, ACT_DISP, ACT_SIGMOID = 0, 3, 4
ACTS = (ACT_NONE, ACT_DISP, ACT_SIGMOID)
GRAD_BOUND = 5e-5                   # tests/test_gpu_conv_bwd_contracts.GRAD_BOUND: max |gpu - r64| / max |r64| of a gradient
GRAD_QUALIFY = GRAD_BOUND / 4
CINS = (16, 32, 64, 128)
# (B,H,W): both reflections on every pixel; the middle pixel next to both borders; small odd sizes; a row longer than a workgroup pass;
# a pixel count that is no multiple of 64 with ragged partial ranges; several workgroups
SHAPES = ((1, 2, 2), (1, 3, 3), (2, 5, 7), (1, 3, 130), (2, 33, 17), (2, 24, 40))
# dbias (and a column of dw) is a sum of signed terms that can nearly cancel, and the error measure divides by its size: a draw qualifies
# only if the float32 CPU evaluation stays within GRAD_QUALIFY of the float64 one.  Of the salts 0 .. 7 tried on the CPU, 2, 3, 5 and 7
# qualify every case; 5 does with the widest margin (worst forward 1.1e-6 of 5e-6, worst gradient 2.2e-6 of 1.25e-5).
SEED_SALT = 5
RANGE_CASES = tuple((n, lim, scale) for n in (1, 63, 4099) for lim in ((0.1, 80.0), (0.5, 10.0)) for scale in (1.0, 6.9))


def activation(z, act):
    if act == ACT_SIGMOID:
        return torch.sigmoid(z)
    if act == ACT_DISP:
        return 10 * torch.sigmoid(z) + 0.01
    return z


def act_deriv_from_output(y, act):
    """act'(u) from y = act(u), as the header states it"""
    if act == ACT_SIGMOID:
        return y * (1 - y)
    if act == ACT_DISP:
        s = (y - 0.01) / 10
        return 10 * s * (1 - s)
    return torch.ones_like(y)


def head_inputs(Cin, B, H, W):
    """the float32 operands of one case on the CPU, from a seed that depends on the case alone: x, w ~ randn / sqrt(9 Cin), bias and
    the gradient dy of the activated output"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(("disp_head", Cin, B, H, W, SEED_SALT)).encode()))
    return {"x": torch.randn(B, H, W, Cin, generator=g), "w": torch.randn(1, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5,
            "bias": torch.randn(1, generator=g), "dy": torch.randn(B, H, W, generator=g)}


def head_pre(x, w, bias, dtype=torch.float64):
    xp = F.pad(x.to(dtype).permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
    return F.conv2d(xp, w.to(dtype), None if bias is None else bias.to(dtype))[:, 0]


def head_fwd(x, w, bias, act, dtype=torch.float64):
    """x (B,H,W,Cin) NHWC, w (1,Cin,3,3), bias (1,) or None -> (B,H,W)"""
    return activation(head_pre(x, w, bias, dtype), act)


def head_bwd(dy, y, x, w, act, dtype=torch.float64):
    """the backward contract: (dx (B,H,W,Cin), dw (1,Cin,3,3), dbias (1,)) from the gradient dy of the activated output and the saved
    output y; dz by the header's formula, the convolution's adjoints by autograd"""
    dz = dy.detach().to(dtype) * act_deriv_from_output(y.detach().to(dtype), act)
    xv, wv = (v.detach().to(dtype).clone().requires_grad_(True) for v in (x, w))
    bv = torch.zeros(1, dtype=dtype, requires_grad=True)
    dx, dw, db = torch.autograd.grad((head_pre(xv, wv, bv, dtype) * dz).sum(), (xv, wv, bv))
    return dx, dw, db


def head_grads_autograd(x, w, bias, dy, act, dtype=torch.float64):
    """the same gradients by autograd through the activation itself (what test_disp_head_ref.py holds head_bwd against)"""
    xv, wv, bv = (v.detach().to(dtype).clone().requires_grad_(True) for v in (x, w, bias))
    y = head_fwd(xv, wv, bv, act, dtype)
    return (y.detach(),) + torch.autograd.grad((y * dy.to(dtype)).sum(), (xv, wv, bv))


def range_inputs(n, limits, scale):
    g = torch.Generator().manual_seed(zlib.crc32(repr(("range", n, limits, scale)).encode()))
    return {"disp": torch.rand(n, generator=g) * 0.998 + 0.001, "g": torch.randn(n, generator=g)}       # disp in (0, 1)


def range_depth(disp, min_depth, max_depth, scale, dtype=torch.float64):
    lo, hi = 1 / torch.tensor(max_depth, dtype=dtype), 1 / torch.tensor(min_depth, dtype=dtype)
    return scale / (lo + (hi - lo) * disp.to(dtype))


def range_depth_bwd(g, disp, min_depth, max_depth, scale, dtype=torch.float64):
    lo, hi = 1 / torch.tensor(max_depth, dtype=dtype), 1 / torch.tensor(min_depth, dtype=dtype)
    return -g.to(dtype) * scale * (hi - lo) / (lo + (hi - lo) * disp.to(dtype)) ** 2


def range_depth_grad_autograd(g, disp, min_depth, max_depth, scale):
    d = disp.double().requires_grad_(True)
    return torch.autograd.grad((range_depth(d, min_depth, max_depth, scale) * g.double()).sum(), d)[0]


# ---- the monodepth2 network: ResnetEncoder + DepthDecoder (networks.py:107-154) on oracle.depthnet's parts ---------------------------
def decoder_multiscale(sd, feats, scales=range(4), head=torch.sigmoid):
    """{scale: head(dispconv_scale(x_scale))} in the order the decoder evaluates them (3, 2, 1, 0); sd holds oracle.depthnet's keys"""
    lay = depthnet.decoder_layout()
    conv = lambda i, x: depthnet._conv3x3_reflect(x, sd[lay[i][0] + ".weight"], sd[lay[i][0] + ".bias"])
    x, idx, out = feats[-1], 0, {}
    for i in range(4, -1, -1):
        x = F.elu(conv(idx, x))
        x = F.interpolate(x, scale_factor=2, mode="nearest")
        if i > 0:
            x = torch.cat([x, feats[i - 1]], 1)
        x = F.elu(conv(idx + 1, x))
        idx += 2
        if i in scales:
            out[i] = head(conv(10 + i, x))
    return out


def monodepth2_forward(sd, image_nhwc, scales=range(4)):
    return decoder_multiscale(sd, depthnet.encoder_forward(sd, image_nhwc), scales)


def split_state_dict(sd, scales=range(4)):
    """{"depth_encoder": ..., "depth_decoder": ...}: oracle.depthnet's flat state dict by the prefixes `encoder.` / `decoder.`, the
    decoder's heads restricted to `scales` (DepthDecoder(scales=[0]) has the 16 -> 1 head only)."""
    drop = tuple("decoder.decoder.%d." % (10 + s) for s in range(4) if s not in scales)
    return {"depth_encoder": {k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")},
            "depth_decoder": {k[len("decoder."):]: v for k, v in sd.items() if k.startswith("decoder.") and not k.startswith(drop)}}


class Monodepth2Trainer(otd.Trainer):
    """oracle.train_depth.Trainer for MODEL.depth_network: monodepth2.  The trainer computes depth = (1 / predict()) * scale; with
    predict() = lo + (hi - lo) * sigmoid(.) that is convert_disp_to_depth * scale (train_depth.py:297-312), so everything else is
    reused as it is.  (Its smoothness term would read this scaled disparity, not the sigmoid: keep it off.)"""
    min_depth, max_depth = 0.1, 80.0

    def predict(self, frame):
        lo, hi = 1 / self.max_depth, 1 / self.min_depth
        return lo + (hi - lo) * monodepth2_forward(self.sd, frame, scales=(0,))[0]
