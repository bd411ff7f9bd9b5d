"""Per-entry-point launch timing with HIP events on the stream each call is launched on (bench.py's in-run roofline
figures; `torch.cuda.Event` alone only sees torch's current stream, the backward-weight chains may run on a side stream).

    with KernelTimer() as kt:
        ...                       # any code that goes through e2ehip._lib.call
    kt.summary()  ->  {entry point: {"calls", "ms", "flops", "bytes"}}

Every C-ABI call is bracketed by one event pair, so an entry point that launches several kernels (a split-K GEMM and its
epilogue, a backward-weight GEMM and its slab reduction) is timed as a whole; one pair costs about 2 us of stream time,
which the figures include (they read slightly LOW as rates, never high)."""
import ctypes

import torch

from . import _lib as L


_CONV = ("e2e_conv2d_fwd", "e2e_conv2d_bwd_data", "e2e_conv2d_bwd_data_acc", "e2e_conv2d_bwd_data_fused", "e2e_conv2d_bwd_weight",
         "e2e_conv2d_bwd_weight_scaled", "e2e_conv2d_bwd_weight_scaled_deferred")
_WARP = ("e2e_warp_photo_lossgrad_hostgeo", "e2e_warp_photo_lossgrad", "e2e_warp_photo_lossgrad_chain")


def _named(name, a):
    """The argument vector of one call as {parameter name of include/e2eslam.h: value}."""
    return dict(zip(L.PARAMS[name], a))


def _conv_geometry(name, a):
    """(B, Hs, Ws, Cin, Cout, Ho, Wo, KH, KW) of one convolution GEMM call, or None for any other entry point."""
    if name not in _CONV:
        return None
    p = _named(name, a)
    if "Ho" not in p:                                   # the forward takes no output size
        p["Ho"], p["Wo"] = (p["Hs"] + 2 * p["pad"] - p["KH"]) // p["stride"] + 1, (p["Ws"] + 2 * p["pad"] - p["KW"]) // p["stride"] + 1
    return tuple(p[k] for k in ("B", "Hs", "Ws", "Cin", "Cout", "Ho", "Wo", "KH", "KW"))


def _conv_flops(name, a):
    """Algorithmic FLOPs of one convolution GEMM call from its argument list (2 x pixels x Cout x Cin x KH x KW)."""
    g = _conv_geometry(name, a)
    if g is None:
        return 0.0
    B, Hs, Ws, Cin, Cout, Ho, Wo, KH, KW = g
    return 2.0 * B * Ho * Wo * Cout * Cin * KH * KW


def _conv_bytes(name, a):
    """Algorithmic (compulsory) HBM bytes of one convolution call: every operand once -- the gathered input domain, the weights, the
    result -- in fp32.  (An upsampled / concatenated input counts with its gather domain B x Hs x Ws x Cin: an upper bound of what has to
    be read; the backward-weight form reads dZ and the input and writes dW.)"""
    g = _conv_geometry(name, a)
    if g is None:
        return 0
    B, Hs, Ws, Cin, Cout, Ho, Wo, KH, KW = g
    return 4 * (B * Hs * Ws * Cin + Cout * Cin * KH * KW + B * Ho * Wo * Cout)


def _warp_bytes(name, a):
    """Algorithmic HBM bytes of one fused warp + photometric (+ regulariser) loss-and-gradient launch:
    reads depth 4N + src 12N + tgt 12N (+ init_t, init_s, depth_s 12N), writes g_tgt 4N (+ g_src 4N)."""
    if name not in _WARP:
        return 0
    p = _named(name, a)
    return (32 + (16 if p["reg_kind"] else 0)) * p.get("B", 1) * p["H"] * p["W"]


class KernelTimer:
    def __init__(self):
        self.rows = []
        self._streams = {}

    def __enter__(self):
        self._prev = L.PROFILE_HOOK[0]
        L.PROFILE_HOOK[0] = self
        return self

    def __exit__(self, *exc):
        L.PROFILE_HOOK[0] = self._prev

    def _stream(self, ptr):
        s = self._streams.get(ptr)
        if s is None:
            s = self._streams[ptr] = torch.cuda.ExternalStream(ptr) if ptr else torch.cuda.default_stream()
        return s

    def around(self, name, args, fn):
        plain = [a.value if isinstance(a, ctypes.c_void_p) else a for a in args]
        s = self._stream(int(_named(name, plain).get("stream") or 0))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        rc = fn()
        e1.record(s)
        self.rows.append((name, e0, e1, _conv_flops(name, plain), _warp_bytes(name, plain) + _conv_bytes(name, plain)))
        return rc

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1, fl, by in self.rows:
            r = out.setdefault(name, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0})
            r["calls"] += 1
            r["ms"] += e0.elapsed_time(e1)
            r["flops"] += fl
            r["bytes"] += by
        return out
