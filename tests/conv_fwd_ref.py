"""Float64 reference of the forward convolution contract of include/e2eslam.h (host only; no tests in this file):

    out (B,Ho,Wo,Cout) = act( scale[c] * conv(x) + shift[c] (+ residual) ),
    x = cat( nearest_upsample(src0 (B,Hs/up,Ws/up,C1), up), src1 (B,Hs,Ws,Cin-C1) ), padded by `pad` with zeros (pad_mode 0) or by reflection (1);

the scalar path (Cin % 16 != 0) reads (v - in_sub) * in_mul, and its zero padding is the zero of the NORMALISED image.  Everything is NHWC
in and out, torch.nn.functional in float64 on the CPU (float32 when asked: the input-qualification check of tests/test_conv_fwd_ref.py).
Also the two GEMM weight layouts as plain permutes, the 1-channel disparity head, and the deterministic inputs of a layer, which the GPU
module (tests/test_gpu_conv_fwd_contracts.py) and the host check share.  tests/test_conv_fwd_ref.py holds every function here against
explicit loops."""
import collections
import zlib

import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_ELU, ACT_DISP = 0, 1, 2, 3
BOUND = 2e-5                      # max |gpu - r64| / max |r64| (tests/test_gpu_conv.py holds the same kernels to it)
QUALIFY = BOUND / 4               # an input qualifies if the float32 reference stays within this of the float64 one
STEM_NORM = (0.45, 1 / 0.225)     # depth_estimation/networks.py:50

# One layer: batch, input channels, full-resolution source grid, output channels, kernel, stride, padding (pad_mode 1: reflection), the
# channels of src0 (C1 == Cin: one source), its upsample factor, and whether the call passes the input normalisation (scalar path only).
Layer = collections.namedtuple("Layer", "B Cin Hs Ws Cout KH KW stride pad pad_mode C1 up norm")


def layer(B, Cin, Hs, Ws, Cout, k=3, stride=1, pad=1, pad_mode=0, C1=None, up=1, norm=False, kw=None):
    return Layer(B, Cin, Hs, Ws, Cout, k, k if kw is None else kw, stride, pad, pad_mode, Cin if C1 is None else C1, up, norm)


def ceil4(n):
    return (n + 3) // 4 * 4


def out_size(s):
    return (s.Hs + 2 * s.pad - s.KH) // s.stride + 1, (s.Ws + 2 * s.pad - s.KW) // s.stride + 1


def activation(y, act):
    if act == ACT_RELU:
        return F.relu(y)
    if act == ACT_ELU:
        return F.elu(y)
    if act == ACT_DISP:
        return 10 * torch.sigmoid(y) + 0.01
    return y


def conv_raw(src0, src1, up, w, stride, pad, pad_mode, in_sub=0.0, in_mul=1.0, dtype=torch.float64):
    """conv(x) of the contract, NHWC: src0 (B,Hs/up,Ws/up,C1), src1 (B,Hs,Ws,Cin-C1) or None, w (Cout,Cin,KH,KW) as torch lays it out"""
    x = src0.to(dtype).permute(0, 3, 1, 2)
    if in_sub != 0.0 or in_mul != 1.0:
        x = (x - torch.tensor(in_sub, dtype=dtype)) * torch.tensor(in_mul, dtype=dtype)
    if up != 1:
        x = F.interpolate(x, scale_factor=up, mode="nearest")
    if src1 is not None:
        x = torch.cat([x, src1.to(dtype).permute(0, 3, 1, 2)], 1)
    if pad_mode == 1 and pad:
        x = F.pad(x, (pad,) * 4, mode="reflect")
        pad = 0
    return F.conv2d(x, w.to(dtype), None, stride, pad).permute(0, 2, 3, 1).contiguous()


def epilogue(z, scale, shift, residual, act):
    """act(scale[c] * z + shift[c] (+ residual)) in z's precision; z and residual (B,Ho,Wo,Cout)"""
    y = z
    if scale is not None:
        y = y * scale.to(z.dtype)
    if shift is not None:
        y = y + shift.to(z.dtype)
    if residual is not None:
        y = y + residual.to(z.dtype)
    return activation(y, act)


def conv_fwd(src0, src1, up, w, scale, shift, residual, stride, pad, pad_mode, act, in_sub=0.0, in_mul=1.0, dtype=torch.float64):
    return epilogue(conv_raw(src0, src1, up, w, stride, pad, pad_mode, in_sub, in_mul, dtype), scale, shift, residual, act)


def w_fwd(w, ld, fill=0.0):
    """[(kh,kw,ci)][ld] from (Cout,Cin,KH,KW); the ld - Cout padding columns hold `fill`"""
    Cout, Cin, KH, KW = w.shape
    m = torch.full((KH * KW * Cin, ld), fill, dtype=w.dtype)
    m[:, :Cout] = w.permute(2, 3, 1, 0).reshape(KH * KW * Cin, Cout)
    return m


def w_bwd(w, ld, factor=None, fill=0.0):
    """[(kh,kw,co)][ld] from (Cout,Cin,KH,KW), every output channel's rows times factor[co] where given (in w's precision)"""
    Cout, Cin, KH, KW = w.shape
    if factor is not None:
        w = w * factor.to(w.dtype).view(-1, 1, 1, 1)
    m = torch.full((KH * KW * Cout, ld), fill, dtype=w.dtype)
    m[:, :Cin] = w.permute(2, 3, 0, 1).reshape(KH * KW * Cout, Cin)
    return m


def head_fwd(x, w, bias, act, dtype=torch.float64):
    """the disparity head: x (B,H,W,16) NHWC, w (1,16,3,3), bias (1,) or None -> (B,H,W); 3x3 under reflection padding"""
    xp = F.pad(x.to(dtype).permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
    y = F.conv2d(xp, w.to(dtype), None if bias is None else bias.to(dtype))
    return activation(y[:, 0], act)


def make_inputs(s):
    """the float32 operands of layer `s` on the CPU, from a seed that depends on the layer alone: sources, weight, a scale of both signs
    (0.5 .. 1.5 in magnitude), shift and residual"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(s)).encode()))
    Ho, Wo = out_size(s)
    shape0 = (s.B, s.Hs // s.up, s.Ws // s.up, s.C1)
    t = {"src0": torch.rand(*shape0, generator=g) if s.norm else torch.randn(*shape0, generator=g)}
    t["src1"] = torch.randn(s.B, s.Hs, s.Ws, s.Cin - s.C1, generator=g) if s.C1 < s.Cin else None
    t["w"] = torch.randn(s.Cout, s.Cin, s.KH, s.KW, generator=g) / (s.Cin * s.KH * s.KW) ** 0.5
    sign = torch.where(torch.rand(s.Cout, generator=g) < 0.5, -1.0, 1.0)
    if s.Cout > 1:
        sign[0], sign[-1] = 1.0, -1.0                       # both signs whatever the draw
    t["scale"] = sign * (torch.rand(s.Cout, generator=g) + 0.5)
    t["shift"] = torch.randn(s.Cout, generator=g)
    t["res"] = torch.randn(s.B, Ho, Wo, s.Cout, generator=g)
    return t


def norm_of(s):
    return STEM_NORM if s.norm else (0.0, 1.0)


def layer_raw(s, t, dtype=torch.float64):
    return conv_raw(t["src0"], t["src1"], s.up, t["w"], s.stride, s.pad, s.pad_mode, *norm_of(s), dtype=dtype)


def layer_out(t, z, epi):
    """the contract's output from conv(x) = z under the operand choice epi = (scale given, shift given, residual given, act)"""
    sc, sh, rs, act = epi
    return epilogue(z, t["scale"] if sc else None, t["shift"] if sh else None, t["res"] if rs else None, act)


def rel(a, ref):
    """the project's error measure: max |a - ref| / max |ref| over the whole output"""
    return ((a.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


def head_inputs(B, H, W):
    g = torch.Generator().manual_seed(1000 * B + 37 * H + W)
    return {"x": torch.randn(B, H, W, 16, generator=g), "w": torch.randn(1, 16, 3, 3, generator=g) / 12.0, "bias": torch.randn(1, generator=g)}
