"""The refused calls and the size queries of the fused warp-photometric family (ten entry points, nine queries), as a fixed list, and the
recorder of tests/warp_host_refusals.json.

A refused call returns before any HIP call, so the library answers without a GPU and every non-NULL pointer here is a dummy integer that
nothing dereferences.  The table holds (return code, e2e_last_error()) per case and the value per query AS THE PARENT COMMIT'S BUILD GAVE
THEM; it is never regenerated from the code under test:

    python tests/warp_host_refusals.py <checkout of the parent commit, built> <its commit hash>

loads the library that lies next to THAT checkout's package and fails if any case is not refused with E2E_ERR_ARG there, so no case can
drop out silently and no case can ever reach a launch."""
import ctypes
import itertools
import json
import os
import sys

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "warp_host_refusals.json")
E2E_ERR_ARG = -1
PADDING_ZEROS, PADDING_BORDER = 0, 1                     # E2E_PADDING_* of include/e2eslam.h

PAIR = ["e2e_warp_photo_fwd", "e2e_warp_photo_bwd", "e2e_warp_photo_bwd_pose", "e2e_warp_photo_bwd_intrinsics"]
WINDOW = ["e2e_warp_photo_window_fwd", "e2e_warp_photo_window_bwd", "e2e_warp_photo_window_bwd_intrinsics"]
GEO = ["e2e_warp_photo_geo_fwd", "e2e_warp_photo_geo_bwd", "e2e_warp_photo_geo_bwd_intrinsics"]
ENTRIES = PAIR + WINDOW + GEO
QUERY_NAMES = ["e2e_warp_photo_workspace_floats", "e2e_warp_photo_bwd_pose_workspace_bytes", "e2e_warp_photo_bwd_intrinsics_workspace_bytes",
               "e2e_warp_photo_window_workspace_floats", "e2e_warp_photo_window_bwd_workspace_bytes", "e2e_warp_photo_geo_workspace_floats",
               "e2e_warp_photo_geo_bwd_workspace_bytes", "e2e_warp_photo_window_bwd_intrinsics_workspace_bytes",
               "e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes"]

# the pointers an entry point does not insist on (with reg_kind = 0 and S = 2, the base of every case); every other pointer is mandatory
OPTIONAL = {"stream", "pmap", "tie_noise", "reg_init_tgt", "reg_init_src", "depth_src"}
OPTIONAL_IN = {"e2e_warp_photo_bwd": {"g_depth_src"}, "e2e_warp_photo_bwd_pose": {"g_depth_src"},
               "e2e_warp_photo_bwd_intrinsics": {"g_depth_src", "g_T"}, "e2e_warp_photo_window_bwd": {"g_T", "workspace"},
               "e2e_warp_photo_geo_bwd": {"g_T"}, "e2e_warp_photo_window_bwd_intrinsics": {"g_T"}, "e2e_warp_photo_geo_bwd_intrinsics": {"g_T"}}
REFUSES_WIDE_BATCH = [e for e in ENTRIES if e not in ("e2e_warp_photo_fwd", "e2e_warp_photo_bwd")]          # B > 65535
BASE = {"B": 2, "H": 9, "W": 33, "S": 2, "use_mask": 1, "padding_mode": PADDING_BORDER, "reg_kind": 0, "terms": 6, "geo_min_valid": 0}


def _lib():
    from e2ehip import _lib
    _lib.load()
    return _lib


def pointers(entry):
    L = _lib()
    return [n for n, t in zip(L.PARAMS[entry], L.SIGNATURES[entry]) if t is ctypes.c_void_p and n != "stream"]


def mandatory(entry):
    return [n for n in pointers(entry) if n not in OPTIONAL | OPTIONAL_IN.get(entry, set())]


def reg_buffers(entry):
    return ["reg_init_tgt", "reg_init_src", "depth_src"] + (["g_depth_src"] if entry != "e2e_warp_photo_fwd" else [])


def single_faults(entry):
    """[(tag, overrides)]: one fault each.  A pointer named in the overrides with None is NULL."""
    out = [(f"null:{p}", {p: None}) for p in mandatory(entry)]
    out += [("B=0", {"B": 0}), ("H=1", {"H": 1}), ("W=1", {"W": 1}), ("BHW>=2^31", {"B": 65535, "H": 256, "W": 256})]
    if entry in REFUSES_WIDE_BATCH:
        out.append(("B=65536", {"B": 65536, "H": 2, "W": 2}))
    out += [(f"padding_mode={v}", {"padding_mode": v}) for v in (-1, 2, 7) if v not in (PADDING_ZEROS, PADDING_BORDER)]
    if entry in PAIR:
        out += [(f"reg_kind={v}", {"reg_kind": v}) for v in (-1, 3)]
        out += [(f"reg_kind=1,null:{p}", {"reg_kind": 1, p: None}) for p in reg_buffers(entry)]
    else:
        out += [(f"S={v}", {"S": v}) for v in (0, 3)] + [(f"terms={v}", {"terms": v}) for v in (1, 8)]
        if entry in GEO:
            out.append(("geo_min_valid=-1", {"geo_min_valid": -1}))
        if entry == "e2e_warp_photo_window_bwd":
            out.append(("g_T without workspace", {"workspace": None}))
    return out


def check_groups(entry):
    """one representative fault per check the entry point makes, for the pairs that pin the order of the checks"""
    g = [("dims", {"H": 1}), ("pointer", {"depth_tgt": None}), ("padding", {"padding_mode": 7})]
    if entry in REFUSES_WIDE_BATCH:
        g.append(("grid", {"B": 65536, "W": 2}))
    if entry in PAIR:
        g += [("reg_kind", {"reg_kind": 3}), ("reg_buffers", {"reg_kind": 1, "reg_init_tgt": None})]
    else:
        g += [("S", {"S": 3}), ("terms", {"terms": 8})]
        if entry in GEO:
            g.append(("geo_min_valid", {"geo_min_valid": -1}))
        if entry == "e2e_warp_photo_window_bwd":
            g.append(("g_T without workspace", {"workspace": None}))
    return g


def build_cases():
    cases = []
    for e in ENTRIES:
        cases += [(f"{e}|{tag}", e, ov) for tag, ov in single_faults(e)]
        for (ta, a), (tb, b) in itertools.combinations(check_groups(e), 2):
            if all(a[k] == b[k] for k in a.keys() & b.keys()):                     # e.g. reg_kind = 3 and reg_kind = 1 cannot both hold
                cases.append((f"{e}|{ta}+{tb}", e, {**a, **b}))
    return cases


def build_queries():
    grid = [(S, B, H, W) for S in (0, 1, 2, 3) for B in (0, 1, 2) for H, W in ((0, 5), (3, 5), (8, 32), (9, 33), (17, 33), (37, 53), (480, 640))]
    out = []
    for q in QUERY_NAMES:
        if "window" in q or "geo" in q:
            out += [(q, a) for a in grid]
        else:
            out += [(q, a[1:]) for a in grid if a[0] == 0]
    return out


def arguments(entry, overrides):
    L = _lib()
    v = {**BASE, **overrides}
    args = []
    for i, (n, t) in enumerate(zip(L.PARAMS[entry], L.SIGNATURES[entry])):
        if t is L.Strides:
            args.append(L.Strides(3 * v["H"] * v["W"], v["H"] * v["W"], v["W"], 1))
        elif t is ctypes.c_void_p:
            args.append(None if n == "stream" or (n in overrides and overrides[n] is None) else ctypes.c_void_p(0x10000 + 0x1000 * i))
        else:
            args.append(v[n])
    return args


def run():
    """-> {"refusals": {case: [rc, message]}, "queries": {"name(args)": value}} from the library that e2ehip._lib loads"""
    L = _lib()
    lib = L.load()
    refusals = {}
    for cid, entry, ov in build_cases():
        rc = getattr(lib, entry)(*arguments(entry, ov))
        refusals[cid] = [rc, lib.e2e_last_error().decode() if rc else ""]
    queries = {f"{q}{tuple(a)}": getattr(lib, q)(*a) for q, a in build_queries()}
    return {"refusals": refusals, "queries": queries}


def write_table(table):
    """one entry per line, sorted"""
    rows = lambda d: ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(d.items()))
    with open(TABLE, "w") as f:
        f.write('{"parent": %s,\n"refusals": {\n%s\n},\n"queries": {\n%s\n}}\n' % (json.dumps(table["parent"]), rows(table["refusals"]), rows(table["queries"])))


if __name__ == "__main__":
    checkout, commit = sys.argv[1:3]
    sys.path.insert(0, os.path.join(checkout, "end-to-end-self-supervised-slam_amd"))
    table = run()
    assert os.path.dirname(_lib().LIB_PATH).startswith(os.path.abspath(checkout)), _lib().LIB_PATH
    bad = {c: r for c, r in table["refusals"].items() if r[0] != E2E_ERR_ARG}
    assert not bad, f"not refused with E2E_ERR_ARG on the parent: {bad}"
    write_table({"parent": commit, **table})
    print(f"{len(table['refusals'])} refusals, {len(table['queries'])} queries recorded from {commit}")
