"""ctypes binding of libe2eslam_hip.so (the C ABI declared in include/e2eslam.h).

There is deliberately NO fallback: if the shared library is missing or a tensor is not on a HIP
device the call raises.  The CPU restatement lives in oracle/ and is test infrastructure only.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libe2eslam_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "e2eslam.h")

c_fp = ctypes.c_void_p
c_int = ctypes.c_int
c_i64 = ctypes.c_int64
c_f32 = ctypes.c_float


class Strides(ctypes.Structure):
    _fields_ = [("sb", c_i64), ("sc", c_i64), ("sh", c_i64), ("sw", c_i64)]


class WgradReduceDesc(ctypes.Structure):
    """e2e_wgrad_reduce_desc (include/e2eslam.h): the slab reduction a deferred backward-weight call leaves to do."""
    _fields_ = [("slabs", c_fp), ("dw", c_fp), ("dbias", c_fp), ("scale", c_fp)] + \
               [(n, c_int) for n in ("S", "Mpad", "Npad", "Cout", "Cin", "KH", "KW", "has_bias", "accumulate", "zl")] + [("first_item", ctypes.c_longlong)]


class CopyDesc(ctypes.Structure):
    """e2e_copy_desc (include/e2eslam.h)."""
    _fields_ = [("src", c_fp), ("dst", c_fp), ("bytes", ctypes.c_longlong), ("first_item", ctypes.c_longlong)]


class E2EError(RuntimeError):
    pass


# the C vocabulary of include/e2eslam.h; every pointer (device or host) is a void*
_CTYPES = {"int": c_int, "int64_t": c_i64, "long long": ctypes.c_longlong, "float": c_f32, "double": ctypes.c_double,
           "e2e_strides": Strides}
_STRUCTS = {"e2e_strides": Strides, "e2e_wgrad_reduce_desc": WgradReduceDesc, "e2e_copy_desc": CopyDesc}


def _ctype(decl, what):
    """'const float* x' -> ('x', c_void_p); raises E2EError naming `what` for a type outside the vocabulary."""
    m = re.fullmatch(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*(\*?)\s*(\w+)", decl.strip())
    if not m or (not m.group(2) and m.group(1) not in _CTYPES):
        raise E2EError(f"include/e2eslam.h: cannot bind `{decl.strip()}` in {what}")
    return m.group(3), c_fp if m.group(2) else _CTYPES[m.group(1)]


def parse_header(text):
    """-> ({entry point: (restype, ((parameter name, ctype), ...))}, {struct name: [(field name, ctype), ...]})."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*(#|extern\b|\}\s*$).*$", "", text, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", text, flags=re.S):
        fields = structs[name] = []
        for decl in filter(str.strip, body.split(";")):
            first, *more = decl.split(",")
            fields.append(_ctype(first, f"struct {name}"))
            fields += [(n.strip(), fields[-1][1]) for n in more]
    text = re.sub(r"typedef\s+struct.*?\}\s*\w+\s*;", "", text, flags=re.S)
    protos = {}
    for decl in filter(str.strip, text.split(";")):
        m = re.fullmatch(r"\s*(const char\*|\w+(?:\s+\w+)?)\s+(e2e_\w+)\s*\((.*)\)\s*", decl, flags=re.S)
        if not m or (m.group(1) != "const char*" and m.group(1) not in _CTYPES):
            raise E2EError(f"include/e2eslam.h: cannot bind the declaration `{' '.join(decl.split())}`")
        ret, name, params = m.groups()
        params = () if params.strip() == "void" else tuple(_ctype(p, name) for p in params.split(","))
        if len({n for n, _ in params}) != len(params) or name in protos:
            raise E2EError(f"include/e2eslam.h: duplicate name in the declaration of {name}")
        protos[name] = (ctypes.c_char_p if ret == "const char*" else _CTYPES[ret], params)
    return protos, structs


SIGNATURES, RESTYPES, PARAMS, _NAMESET = {}, {}, {}, {}     # filled by load(): name -> argtypes / restype / parameter names (in order, as a set)
_lib = None


def load():
    """Load the shared library (once) and give every prototype of the header its ctypes signature.  Raises E2EError if the
    library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise E2EError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                           "(there is no CPU / PyTorch fallback for the hot path)")
        with open(HEADER_PATH) as f:
            protos, structs = parse_header(f.read())
        for n, cls in _STRUCTS.items():
            if structs.get(n) != list(cls._fields_):
                raise E2EError(f"include/e2eslam.h: struct {n} and its ctypes class {cls.__name__} differ")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, params) in protos.items():
            fn = getattr(lib, name)
            fn.argtypes = SIGNATURES[name] = [t for _, t in params]
            fn.restype = RESTYPES[name] = restype
            PARAMS[name] = tuple(n for n, _ in params)
            _NAMESET[name] = frozenset(PARAMS[name])
        _lib = lib
    return _lib


PROFILE_HOOK = [None]           # e2ehip.profile.KernelTimer while a timing pass is active


def bind(name, *args, geom=None, **kw):
    """The argument vector of entry point `name`: a positional prefix, then the remaining parameters by the names the header gives
    them.  `geom` is a mapping that may hold more names than the prototype declares (a layer's geometry, shared by the forward, the
    backward forms and the workspace queries): it fills what neither `args` nor `kw` gives.  Every keyword must name a parameter that
    is not already given positionally, and every parameter must be given: TypeError otherwise, before anything is launched."""
    load()
    names = PARAMS[name]
    if len(args) > len(names):
        raise TypeError(f"{name}: takes {len(names)} arguments, {len(args)} given")
    if not kw.keys() <= _NAMESET[name]:
        raise TypeError(f"{name}: no parameter named {sorted(kw.keys() - _NAMESET[name])}")
    if args and not kw.keys().isdisjoint(names[:len(args)]):
        raise TypeError(f"{name}: {sorted(kw.keys() & set(names[:len(args)]))} given both positionally and by name")
    named = {**geom, **kw} if geom else kw
    try:
        return args + tuple(map(named.__getitem__, names[len(args):]))
    except KeyError as e:
        raise TypeError(f"{name}: missing parameter {e.args[0]!r}") from None


def call(name, *args, **kw):
    """Launch an entry point that returns a status; see bind() for the keyword form."""
    if kw:
        args = bind(name, *args, **kw)
    lib = load()
    hook = PROFILE_HOOK[0]
    rc = getattr(lib, name)(*args) if hook is None else hook.around(name, args, lambda: getattr(lib, name)(*args))
    if rc != 0:
        raise E2EError(f"{name} failed ({rc}): {lib.e2e_last_error().decode()}")


def query(name, *args, **kw):
    """An entry point that returns a value (workspace sizes, the *_batch_prepare totals): no status check, no timing."""
    return getattr(load(), name)(*(bind(name, *args, **kw) if kw else args))


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(t, name="tensor", dtype=torch.float32):
    """Validate a tensor for the HIP path and return it."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise E2EError(f"{name}: the e2eslam hot path runs on the HIP device only (got a {t.device} tensor); "
                       "there is no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def strides4(t):
    """Element strides of a (B,C,H,W)-indexed view."""
    s = t.stride()
    return Strides(s[0], s[1], s[2], s[3])
