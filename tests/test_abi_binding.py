"""The ctypes binding is derived from include/e2eslam.h: every prototype parses and is bound, the three ctypes structs match the header's
typedefs, keyword calls bind by the header's parameter names, and e2ehip.profile accounts by those names.  No GPU: the library loads
without one, and only host-only entry points are called."""
import ctypes
import os
import re

import pytest

from test_abi import ROOT, declared_symbols

C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double}
# the tiny convolution of tests/test_gpu_abi_binding.py: apart from KH = KW every value is distinct, so a transposed pair shows
GEOM = dict(B=2, Hs=12, Ws=20, Cin=8, Cout=16, Ho=6, Wo=10, KH=3, KW=3, stride=2, pad=1, pad_mode=0, C1=8, up=1, in_sub=0.0, in_mul=1.0)
FWD = dict(src0=101, src1=None, w_fwd=102, ld_fwd=16, scale=None, shift=103, residual=None, out=104, act=1, workspace=None, stream=None)


def _fwd_keywords():
    """Exactly the parameters of e2e_conv2d_fwd (which takes no Ho / Wo)."""
    return {**{k: v for k, v in GEOM.items() if k not in ("Ho", "Wo")}, **FWD}


@pytest.fixture(scope="module")
def L():
    from e2ehip import _lib
    _lib.load()
    return _lib


def _header():
    txt = open(os.path.join(ROOT, "include", "e2eslam.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_every_prototype_is_parsed_exported_and_bound(L):
    lib = L.load()
    syms = declared_symbols()
    assert sorted(L.SIGNATURES) == sorted(L.PARAMS) == sorted(L.RESTYPES) == syms and len(syms) >= 123
    for name in syms:
        fn = getattr(lib, name)
        assert list(fn.argtypes) == L.SIGNATURES[name] and fn.restype is L.RESTYPES[name], name
        assert len(fn.argtypes) == len(L.PARAMS[name]), name
        assert len(set(L.PARAMS[name])) == len(L.PARAMS[name]), f"{name}: parameter names repeat"
    # the parameter count of every prototype, counted independently of the loader: commas of the declaration
    for ret, name, params in re.findall(r"([\w \*]+?)\s*\b(e2e_\w+)\s*\(([^)]*)\)\s*;", _header()):
        want = 0 if params.strip() == "void" else params.count(",") + 1
        assert len(L.PARAMS[name]) == want, name
        # ... and its types, against the C vocabulary: a pointer is a void*, everything else its own ctype
        for decl, got in zip(params.split(",") if want else [], L.SIGNATURES[name]):
            base = re.sub(r"\bconst\b", "", decl).rsplit(None, 1)[0].strip() if "*" not in decl else "*"
            assert got is (ctypes.c_void_p if base == "*" else L.Strides if base == "e2e_strides" else C_TYPES[base]), (name, decl)
        ret = ret.strip()
        assert L.RESTYPES[name] is (ctypes.c_char_p if ret == "const char*" else C_TYPES[ret]), name


def test_loader_names_what_it_cannot_bind(L):
    with pytest.raises(L.E2EError, match="e2e_new"):
        L.parse_header("int e2e_new(const float* x, unsigned n);")
    with pytest.raises(L.E2EError, match="e2e_odd"):
        L.parse_header("int e2e_odd(int (*callback)(int), int n);")
    with pytest.raises(L.E2EError, match="e2e_twice"):
        L.parse_header("int e2e_twice(int n, float n);")
    with pytest.raises(L.E2EError, match="e2e_ret"):
        L.parse_header("unsigned e2e_ret(int n);")


@pytest.mark.parametrize("cname, cls", [("e2e_strides", "Strides"), ("e2e_wgrad_reduce_desc", "WgradReduceDesc"), ("e2e_copy_desc", "CopyDesc")])
def test_struct_layouts_match_the_header(L, cname, cls):
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (cname, cname), _header(), flags=re.S).group(1)
    want = []                                            # (field, width in bytes, is a pointer), in declaration order
    for decl in filter(str.strip, body.split(";")):
        m = re.fullmatch(r"\s*(?:const\s+)?([\w ]+?)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)\s*", decl)
        width = ctypes.sizeof(ctypes.c_void_p) if m.group(2) else ctypes.sizeof(C_TYPES[m.group(1)])
        want += [(f.strip(), width, bool(m.group(2))) for f in m.group(3).split(",")]
    fields = getattr(L, cls)._fields_
    assert [(n, ctypes.sizeof(t), t is ctypes.c_void_p) for n, t in fields] == want
    offsets = [getattr(getattr(L, cls), n).offset for n, _ in fields]
    assert offsets == sorted(offsets) and ctypes.sizeof(getattr(L, cls)) % 8 == 0


def test_bind_positional_keyword_and_mixed_agree(L):
    name = "e2e_conv2d_fwd"
    by_name = L.bind(name, **_fwd_keywords())
    assert len(by_name) == 25 and dict(zip(L.PARAMS[name], by_name)) == _fwd_keywords()
    assert L.bind(name, *by_name) == by_name                                     # a positional vector comes back unchanged
    assert L.bind(name, *by_name[:10], **{k: v for k, v in _fwd_keywords().items() if k in L.PARAMS[name][10:]}) == by_name
    assert L.bind(name, geom=GEOM, **FWD) == by_name                             # the mapping holds Ho / Wo, which the forward does not take
    assert L.bind(name, geom=GEOM, **{**FWD, "B": 1})[10] == 1                   # an explicit keyword wins over the mapping
    assert L.bind(name, by_name[0], geom={**GEOM, "src0": "ignored"}, **{k: v for k, v in FWD.items() if k != "src0"}) == by_name
    assert L.bind("e2e_version") == ()


def test_bind_refuses_missing_unknown_and_duplicated_names(L):
    name, kw = "e2e_conv2d_fwd", _fwd_keywords()
    with pytest.raises(TypeError, match="e2e_conv2d_fwd.*'stride'"):
        L.bind(name, **{k: v for k, v in kw.items() if k != "stride"})
    with pytest.raises(TypeError, match="e2e_conv2d_fwd.*'Ho'"):
        L.bind(name, Ho=6, **kw)                                                 # only the mapping may carry names the prototype lacks
    with pytest.raises(TypeError, match="e2e_conv2d_fwd.*'strid'"):
        L.bind(name, geom=GEOM, strid=2, **FWD)
    with pytest.raises(TypeError, match="e2e_conv2d_fwd.*'src0'"):
        L.bind(name, 101, **kw)
    with pytest.raises(TypeError, match="e2e_conv2d_fwd"):
        L.bind(name, *range(26))
    with pytest.raises(TypeError, match="e2e_conv2d_fwd.*'stream'"):
        L.bind(name, *range(24))
    with pytest.raises(TypeError):
        L.call(name, 101, **kw)                                                  # refused before anything is launched


def test_host_only_entry_points_called_both_ways(L):
    def wgrad():
        return (L.WgradReduceDesc * 3)(*[L.WgradReduceDesc(slabs=64, dw=128, S=2, Mpad=64, Npad=64, Cout=co, Cin=ci, KH=k, KW=k, has_bias=hb, zl=zl)
                                         for co, ci, k, hb, zl in ((64, 64, 3, 0, 8), (128, 64, 1, 1, 2), (16, 32, 3, 1, 8))])

    def copies():
        return (L.CopyDesc * 3)(*[L.CopyDesc(src=4096, dst=8192, bytes=b) for b in (16, 4096, 1 << 20)])
    for fn, make in (("e2e_wgrad_reduce_batch_prepare", wgrad), ("e2e_copy_batch_prepare", copies)):
        a, b = make(), make()
        ta, tb = L.query(fn, a, 3), L.query(fn, descs_host=b, n=3)
        assert ta == tb > 0 and [d.first_item for d in a] == [d.first_item for d in b] and a[2].first_item > a[1].first_item > 0
    # a few layer shapes of the network (tests/test_gpu_bwd_pair.py NETWORK): B, Cin, H, W, Cout, k, stride, pad
    for B, Cin, H, W, Cout, k, s, p in ((2, 64, 120, 160, 64, 3, 1, 1), (2, 64, 120, 160, 128, 3, 2, 1), (2, 256, 30, 40, 512, 1, 2, 0),
                                        (2, 512, 15, 20, 512, 3, 1, 1), (2, 32, 240, 320, 16, 3, 1, 1)):
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        g = dict(B=B, Hs=H, Ws=W, Cin=Cin, Cout=Cout, Ho=Ho, Wo=Wo, KH=k, KW=k, stride=s, pad=p, pad_mode=0, C1=Cin, up=1, in_sub=0.0, in_mul=1.0)
        n = L.query("e2e_conv2d_wgrad_workspace_floats", B, Ho, Wo, Cin, Cout, k, k, 1)
        assert n == L.query("e2e_conv2d_wgrad_workspace_floats", geom=g, has_bias=1) and n > 0
        n = L.query("e2e_conv2d_bwd_data_workspace_floats", B, H, W, Cin, k * k * Cout, s)
        assert n == L.query("e2e_conv2d_bwd_data_workspace_floats", geom=g, Hd=H, Wd=W, cols=Cin, K=k * k * Cout) and n >= 0
        o1, o2 = (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
        L.call("e2e_conv_gemm_choice", B * Ho * Wo, Cout, k * k * Cin, 32, 1, o1)
        L.call("e2e_conv_gemm_choice", rows=B * Ho * Wo, cols=Cout, K=k * k * Cin, chunk_depth=32, allow_split=1, out3_host=o2)
        assert list(o1) == list(o2) and o1[0] > 0 and o1[1] > 0 and o1[2] >= 1


def test_profile_accounts_by_parameter_name(L):
    from e2ehip import profile
    data = dict(w_bwd=1, ld_bwd=8, dxp=2, workspace=None, stream=None)
    wgrad = dict(out_scale=None, src0=1, src1=None, dw=2, dbias=None, workspace=3, accumulate=0, stream=None)
    vectors = {
        "e2e_conv2d_fwd": L.bind("e2e_conv2d_fwd", geom=GEOM, **FWD),
        "e2e_conv2d_bwd_data": L.bind("e2e_conv2d_bwd_data", geom=GEOM, dz=1, **data),
        "e2e_conv2d_bwd_data_fused": L.bind("e2e_conv2d_bwd_data_fused", geom=GEOM, da=1, accumulate=0, x_in=None, in_act=0, pre_add=None, **data),
        "e2e_conv2d_bwd_weight_scaled": L.bind("e2e_conv2d_bwd_weight_scaled", geom=GEOM, da=1, **wgrad),
        "e2e_conv2d_bwd_weight_scaled_deferred": L.bind("e2e_conv2d_bwd_weight_scaled_deferred", geom=GEOM, da=1, desc_out_host=None, **wgrad),
    }
    for name, vec in vectors.items():
        assert profile._conv_flops(name, vec) == 276480 and profile._conv_bytes(name, vec) == 27648, name
        assert profile._warp_bytes(name, vec) == 0
    # the paired backward and everything that is no convolution GEMM stay unaccounted, as before
    assert profile._conv_flops("e2e_conv2d_act_bwd", (1, 2, None, 3, 10, 16, 1, None)) == 0.0
    assert profile._conv_bytes("e2e_conv2d_bwd_pair_deferred", ()) == 0
    lossgrad = dict(depth_tgt=1, src=2, src_strides=None, tgt=3, tgt_strides=None, use_mask=1, padding_mode=1, reg_init_tgt=None, reg_init_src=None,
                    depth_src=None, w_photo=1.0, w_reg=0.01, loss_out=None, g_depth_tgt=4, g_depth_src=None, workspace=5, H=48, W=64, stream=None)
    for reg, per_pixel in ((0, 32), (2, 48)):
        v = L.bind("e2e_warp_photo_lossgrad", K=1, inv_K=2, T=3, B=2, reg_kind=reg, **lossgrad)
        assert profile._warp_bytes("e2e_warp_photo_lossgrad", v) == per_pixel * 2 * 48 * 64
        v = L.bind("e2e_warp_photo_lossgrad_hostgeo", geometry12_host=1, reg_kind=reg, **lossgrad)
        assert profile._warp_bytes("e2e_warp_photo_lossgrad_hostgeo", v) == per_pixel * 48 * 64
