"""The entry points of the map side -- csrc/pointfusion.hip (vertex / normal maps, association, tables, fusion, append, aggregation append)
and csrc/knn.hip (every e2e_knn1_* form) -- called by name through e2ehip._lib, against references that do not share their arithmetic:

  map step   tests/pointfusion_contract_ref.py, a float64 restatement in the natural operation order that also says which decisions an
             fp32 evaluation can be asked to reproduce (tests/test_pointfusion_contract_ref.py proves on the CPU that the random cases
             skip at most 1 % and the constructed cases nothing).  Tables and counts: exactly equal on the decidable set.  Payloads:
             within 4 x the fp32 CPU oracle's own error against the same float64 reference on the same inputs, never below 2 ulp of the
             quantity's largest magnitude.  Where the kernel's arithmetic is IEEE in the oracle's order (everything but exp) the file's
             own contract, bit-equality with oracle/pointfusion.py, is kept as well -- on every row, decidable or not.
  neighbours tests/knn_contract_ref.py: a numpy float32 brute force (exact IEEE, first minimum wins) compared bit for bit, and a float64
             statement of the same result.

Every output buffer is NaN- or poison-filled and followed by a guard band that must come back untouched; workspaces and indices are
allocated at exactly the size their queries return, guard band behind.  Refused calls (arguments the host code checks before any launch)
must raise and leave every output as it was."""
import functools

import numpy as np
import pytest
import torch

import knn_contract_ref as KR
import pointfusion_contract_ref as R
from oracle import pointfusion as opf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
POISON = -0x5A5A5A5A
RECORD = []                                                   # (case, quantity, gpu error, oracle error, bound): printed by the last test


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _nan(n):
    return torch.full((int(n) + GUARD,), float("nan"), device=DEV, dtype=torch.float32)


def _poison(n, dtype=torch.int64):
    return torch.full((int(n) + GUARD,), POISON, device=DEV, dtype=dtype)


def _bytes(n):
    return torch.full((int(n) + GUARD,), 0xA5, device=DEV, dtype=torch.uint8)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _filled(a, cap_elems):
    """a NaN buffer of cap_elems + GUARD floats whose head holds `a`"""
    buf = _nan(cap_elems)
    flat = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1))
    buf[:flat.numel()] = flat.to(DEV)
    return buf


def _guard_ok(buf, n, what):
    tail = buf[int(n):]
    if buf.dtype.is_floating_point:
        assert torch.isnan(tail).all(), f"{what}: written past the end"
    elif buf.dtype == torch.uint8:
        assert (tail == 0xA5).all(), f"{what}: written past the size its query returned"
    else:
        assert (tail == POISON).all(), f"{what}: written past the end"


def _written(buf, n, what):
    _guard_ok(buf, n, what)
    assert not torch.isnan(buf[:int(n)]).any(), f"{what}: {int(torch.isnan(buf[:int(n)]).sum())} of {n} elements not written"
    return buf[:int(n)].cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def _check(case, what, gpu, ref64, oracle32):
    """the payload rule: max|gpu - float64| <= max(4 x max|oracle - float64|, 2 ulp of max|float64|)"""
    ref64 = np.asarray(ref64, np.float64)
    e_gpu = float(np.abs(np.asarray(gpu, np.float64) - ref64).max()) if ref64.size else 0.0
    e_or = float(np.abs(np.asarray(oracle32, np.float64) - ref64).max()) if ref64.size else 0.0
    bnd = R.bound(e_or, float(np.abs(ref64).max()) if ref64.size else 0.0)
    RECORD.append((case, what, e_gpu, e_or, bnd))
    print(f"{case}: {what}: gpu {e_gpu:.3e}  oracle {e_or:.3e}  bound {bnd:.3e}")
    assert e_gpu <= bnd, f"{case}: {what}: |gpu - float64| = {e_gpu:.3e} > {bnd:.3e} (oracle {e_or:.3e})"


# ---------------------------------------------------------------------------------------------------------------------------------------
# vertex / normal maps, their depth gradient, transform_points
# ---------------------------------------------------------------------------------------------------------------------------------------
FRAMES = {"16x24": (16, 24), "33x37": (33, 37), "1x8": (1, 8), "8x1": (8, 1), "72x100": (72, 100), "far_band": (16, 24)}


@functools.lru_cache(maxsize=None)
def _batch(name):
    """B = 2: two depth images with DIFFERENT intrinsics and poses"""
    H, W = FRAMES[name]
    c = R.get_case("far_band_second" if name == "far_band" else name)
    d0, K0, p0 = c["depth"], c["K"], c["pose"]
    d1, _ = R.scene(H, W, 77 + H)
    K1 = K0.copy()
    K1[0, 0], K1[1, 1], K1[0, 2], K1[1, 2] = K0[0, 0] * 1.37, K0[1, 1] * 0.81, K0[0, 2] + 1.25, K0[1, 2] - 0.75
    p1 = R.pose_of(-7.0, 11.0, 23.0, (-0.4, 0.9, 0.3))
    depth, K, pose = np.stack([d0, d1]), np.stack([K0, K1]), np.stack([p0, p1])
    ref = R.frame_maps(depth, K, pose)
    ora = [opf.vertex_normal_maps(torch.from_numpy(depth[b]), torch.from_numpy(K[b]), torch.from_numpy(pose[b])) for b in range(2)]
    o = {k: np.stack([ora[b][k].numpy() for b in range(2)]) for k in ("V", "n", "Vg", "ng")}
    o["alpha"] = np.stack([opf.fusion_alpha(ora[b]["V"], R.SIGMA).numpy() for b in range(2)])
    return depth, K, pose, ref, o


def _maps(depth, K, pose, want=("V", "n", "Vg", "ng", "alpha")):
    L = _L()
    B, H, W = depth.shape
    d, Kd, pd = _dev(depth), _dev(K), _dev(pose)
    out = {k: _nan(B * H * W * (1 if k == "alpha" else 3)) for k in want}
    L.call("e2e_vertex_normal_maps", depth=L.ptr(d), K=L.ptr(Kd), pose=L.ptr(pd), alpha_den=float(R.ALPHA_DEN), V=L.ptr(out.get("V")), Nm=L.ptr(out.get("n")),
           Vg=L.ptr(out["Vg"]), Ng=L.ptr(out.get("ng")), alpha=L.ptr(out.get("alpha")), B=B, H=H, W=W, stream=L.stream())
    torch.cuda.synchronize()
    return {k: _written(v, B * H * W * (1 if k == "alpha" else 3), k).reshape((B, H, W) + (() if k == "alpha" else (3,))) for k, v in out.items()}


@pytest.mark.parametrize("name", list(FRAMES))
def test_vertex_normal_maps_batched_against_float64(name):
    depth, K, pose, ref, o = _batch(name)
    got = _maps(depth, K, pose)
    for b in range(2):                                        # per image: a kernel that read image 0's K or pose for image 1 fails here
        for k in ("V", "n", "Vg", "ng"):
            _check(f"maps {name}[{b}]", k, got[k][b], ref[k][b], o[k][b])
        ok = depth[b] != 0                                    # alpha over the valid pixels (a hole has |V| = 0: exp(-0) = 1 exactly, which would
        _check(f"maps {name}[{b}]", "alpha", got["alpha"][b][ok], ref["alpha32"][b][ok], o["alpha"][b][ok])      # set the floor of the bound at 2 ulp of 1)
        assert (got["alpha"][b][~ok] == 1).all()
        for k in ("V", "n", "Vg", "ng"):
            assert np.array_equal(got[k][b], o[k][b]), f"{name}[{b}]: {k} is not bit-identical to the fp32 oracle"
    if name == "far_band":
        far = depth[0] == 9.5
        assert far.sum() == 8 * 24 and not got["alpha"][0][far].any() and (got["alpha"][0][~far] > 0).all()      # exactly 0 beyond 8.6 m
    if min(FRAMES[name]) == 1:
        assert not got["n"].any() and not got["ng"].any()      # no cross product along a line: nrm == 0, the normal is exactly 0
    only = _maps(depth, K, pose, want=("Vg",))                # every optional output NULL
    assert _same_bits(only["Vg"], got["Vg"])


@pytest.mark.parametrize("name", ["33x37", "8x1", "72x100"])
def test_vertex_maps_bwd_batched_against_float64(name):
    L = _L()
    depth, K, pose, _, _ = _batch(name)
    B, H, W = depth.shape
    rng = np.random.default_rng(H * W)
    gV, gVg = rng.standard_normal((B, H, W, 3)).astype(np.float32), rng.standard_normal((B, H, W, 3)).astype(np.float32)
    d, Kd, pd, gVd, gVgd = _dev(depth), _dev(K), _dev(pose), _dev(gV), _dev(gVg)
    for what, a, b in (("gV and gVg", gV, gVg), ("gV only", gV, None), ("gVg only", None, gVg)):
        ref = R.vertex_maps_bwd(depth, K, pose, a, b)
        ora = []
        for i in range(B):
            dd = torch.from_numpy(depth[i]).clone().requires_grad_(True)
            m = opf.vertex_normal_maps(dd, torch.from_numpy(K[i]), torch.from_numpy(pose[i]))
            loss = 0.0
            if a is not None:
                loss = loss + (m["V"] * torch.from_numpy(a[i])).sum()
            if b is not None:
                loss = loss + (m["Vg"] * torch.from_numpy(b[i])).sum()
            loss.backward()
            ora.append(dd.grad.numpy())
        out = _nan(B * H * W)
        L.call("e2e_vertex_maps_bwd", depth=L.ptr(d), K=L.ptr(Kd), pose=L.ptr(pd), g_V=L.ptr(gVd) if a is not None else None,
               g_Vg=L.ptr(gVgd) if b is not None else None, g_depth=L.ptr(out), B=B, H=H, W=W, stream=L.stream())
        torch.cuda.synchronize()
        got = _written(out, B * H * W, "g_depth").reshape(B, H, W)
        for i in range(B):
            _check(f"maps_bwd {name}[{i}]", what, got[i], ref[i], ora[i])
        assert not got[depth == 0].any()


@pytest.mark.parametrize("n", [1, 255, 1000, 8192 * 256 + 999], ids=lambda n: f"n{n}")
def test_transform_points_against_float64(n):
    L = _L()
    rng = np.random.default_rng(n)
    p = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    T = R.pose_of(10, 20, -30, (0.5, 1.0, -2.0))
    Tt = np.eye(4, dtype=np.float32)
    Tt[:3, :3] = T[:3, :3].T
    pd, Td = _dev(p), _dev(T)
    for tr, To in ((0, T), (1, Tt)):
        out = _nan(n * 3)
        L.call("e2e_transform_points", L.ptr(pd), L.ptr(Td), L.ptr(out), n, tr, L.stream())
        torch.cuda.synchronize()
        got = _written(out, n * 3, "out").reshape(n, 3)
        ora = opf.transform_pointcloud(torch.from_numpy(p), torch.from_numpy(To)).numpy()
        _check(f"transform_points n={n}", "R^T p" if tr else "R p + t", got, R.transform_points(p, T, bool(tr)), ora)
        assert np.array_equal(got, ora), "not bit-identical to the fp32 oracle"
    out = _nan(3)
    L.call("e2e_transform_points", L.ptr(pd), L.ptr(Td), L.ptr(out), 0, 0, L.stream())       # n = 0: accepted, nothing written
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the map step: associate -> the three tables -> fuse + append, host-count forms and _dev forms
# ---------------------------------------------------------------------------------------------------------------------------------------
class Step:
    """one map step of a case on the GPU.  form "host": e2e_pf_associate / e2e_pf_fuse_append, capacity exactly what the step needs + 3,
    fused with the ORACLE's alpha (so that every row can be compared with the fp32 oracle bit for bit).  form "dev": the _dev entry
    points, capacity well above the live count, fused with the alpha the maps kernel computed."""

    def __init__(self, name, form, cap=None):
        L = self.L = _L()
        c = self.case = R.get_case(name)
        self.name, self.form = name, form
        H, W = self.H, self.W = c["H"], c["W"]
        M = self.M = c["state"]["ccounts"].shape[0]
        N = H * W
        self.cap = cap if cap is not None else (M + N + 3 if form == "host" else M + N + 5000)
        self.st = {k: _filled(c["state"][k], self.cap * (1 if k == "ccounts" else 3)) for k in ("points", "normals", "colors", "ccounts")}
        self.count = _poison(3)
        self.count[:3] = torch.tensor([M, 0, 0], device=DEV)
        nbytes = L.query("e2e_pf_workspace_bytes", self.cap, H, W)
        assert nbytes > 0 and nbytes % 256 == 0
        self.ws, self.nbytes = _bytes(nbytes), nbytes
        self.K, self.pose = _dev(c["K"]), _dev(c["pose"])
        self.depth, self.rgb = _dev(c["depth"]), _dev(c["rgb"])
        g = _maps(c["depth"][None], c["K"][None], c["pose"][None])
        self.maps = {k: v[0] for k, v in g.items()}
        self.Vg, self.Ng = _dev(self.maps["Vg"]), _dev(self.maps["ng"])
        self.alpha = _dev(R.oracle(name)[2]["alpha"] if form == "host" else self.maps["alpha"])

    def associate(self):
        L, s = self.L, self.st
        if self.form == "host":
            L.call("e2e_pf_associate", map_points=L.ptr(s["points"]), map_normals=L.ptr(s["normals"]), map_ccounts=L.ptr(s["ccounts"]), M=self.M,
                   K=L.ptr(self.K), pose=L.ptr(self.pose), Vg=L.ptr(self.Vg), Ng=L.ptr(self.Ng), dist_th=R.DIST_TH, dot_th=R.DOT_TH,
                   workspace=L.ptr(self.ws), map_capacity=self.cap, H=self.H, W=self.W, stream=L.stream())
        else:
            L.call("e2e_pf_associate_dev", map_points=L.ptr(s["points"]), map_normals=L.ptr(s["normals"]), map_ccounts=L.ptr(s["ccounts"]),
                   map_count_dev=L.ptr(self.count), K=L.ptr(self.K), pose=L.ptr(self.pose), Vg=L.ptr(self.Vg), Ng=L.ptr(self.Ng), dist_th=R.DIST_TH,
                   dot_th=R.DOT_TH, workspace=L.ptr(self.ws), map_capacity=self.cap, H=self.H, W=self.W, stream=L.stream())
        torch.cuda.synchronize()

    def tables(self):
        L = self.L
        out = {}
        for which, name in enumerate(("active", "similar", "unique")):
            most = self.M if which < 2 else min(self.M, self.H * self.W)
            rows, cnt = _poison(most * 3), _poison(1)
            L.call("e2e_pf_table", which, self.M, L.ptr(self.ws), self.cap, self.H, self.W, L.ptr(rows), L.ptr(cnt), L.stream())
            torch.cuda.synchronize()
            _guard_ok(cnt, 1, "count_out")
            k = int(cnt[0])
            assert 0 <= k <= most, f"{name}: count {k}"
            _guard_ok(rows, most * 3, f"{name} rows")
            assert (rows[k * 3:most * 3] == POISON).all(), f"{name}: rows written beyond the count"
            out[name] = rows[:k * 3].cpu().numpy().reshape(k, 3)
        return out

    def fuse_append(self, depth=None):
        """-> the live row count after the step (host form: *new_count_out, which is the count the step NEEDED)"""
        L, s = self.L, self.st
        depth = self.depth if depth is None else depth
        if self.form == "host":
            new = _poison(1)
            L.call("e2e_pf_fuse_append", map_points=L.ptr(s["points"]), map_normals=L.ptr(s["normals"]), map_colors=L.ptr(s["colors"]),
                   map_ccounts=L.ptr(s["ccounts"]), M=self.M, map_capacity=self.cap, depth=L.ptr(depth), Vg=L.ptr(self.Vg), Ng=L.ptr(self.Ng),
                   rgb=L.ptr(self.rgb), alpha=L.ptr(self.alpha), workspace=L.ptr(self.ws), H=self.H, W=self.W, new_count_out=L.ptr(new), stream=L.stream())
            torch.cuda.synchronize()
            _guard_ok(new, 1, "new_count_out")
            return int(new[0])
        L.call("e2e_pf_fuse_append_dev", map_points=L.ptr(s["points"]), map_normals=L.ptr(s["normals"]), map_colors=L.ptr(s["colors"]),
               map_ccounts=L.ptr(s["ccounts"]), map_count_dev=L.ptr(self.count), map_capacity=self.cap, depth=L.ptr(depth), Vg=L.ptr(self.Vg),
               Ng=L.ptr(self.Ng), rgb=L.ptr(self.rgb), alpha=L.ptr(self.alpha), workspace=L.ptr(self.ws), H=self.H, W=self.W, stream=L.stream())
        torch.cuda.synchronize()
        _guard_ok(self.count, 3, "map_count_dev")
        return int(self.count[0])

    def state(self, rows):
        """the first `rows` rows as numpy, after checking that nothing beyond them (up to the capacity and past it) was written"""
        _guard_ok(self.ws, self.nbytes, "workspace")
        out = {}
        for k, buf in self.st.items():
            w = 1 if k == "ccounts" else 3
            assert torch.isnan(buf[rows * w:]).all(), f"{k}: written beyond row {rows} (capacity {self.cap})"
            a = buf[:rows * w].cpu().numpy()
            out[k] = a.reshape(rows, 3) if w == 3 else a
        return out


STEP_CASES = list(R.RANDOM_CASES) + ["large"] + list(R.CONSTRUCTED_CASES)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_map_step_against_float64_and_the_oracle(name, form):
    ref, c = R.reference(name), R.get_case(name)
    after_o, tab_o, _ = R.oracle(name)
    s = Step(name, form)
    s.associate()
    tabs = s.tables()
    pt, px = R.compare_tables(ref, tabs)                      # exactly equal on the decidable set
    assert pt <= 0.01 and px <= 0.01 and (name not in R.CONSTRUCTED_CASES or pt == px == 0)
    RECORD.append((f"step {name} {form}", "skipped share", pt, px, 0.01))
    for k in ("active", "similar", "unique"):                # ... and the file's own contract: the fp32 oracle's tables, every row
        assert np.array_equal(tabs[k], tab_o[k]), f"{k} table differs from the fp32 oracle's"
    rows = s.fuse_append()
    assert rows == after_o["ccounts"].shape[0] and (pt + px > 0 or rows == ref["after"]["ccounts"].shape[0])
    got = s.state(rows)
    assert not any(np.isnan(v).any() for v in got.values())
    valid = c["depth"] != 0
    e_gpu, e_or = R.state_errors(ref, got, tabs["unique"], valid), R.state_errors(ref, after_o, tab_o["unique"], valid)
    for k in ("points", "normals", "colors", "ccounts"):
        bnd = R.bound(e_or[k][0], e_or[k][1])
        RECORD.append((f"step {name} {form}", k, e_gpu[k][0], e_or[k][0], bnd))
        print(f"step {name} {form}: {k}: gpu {e_gpu[k][0]:.3e}  oracle {e_or[k][0]:.3e}  bound {bnd:.3e}")
        assert e_gpu[k][0] <= bnd, f"{name} {form}: {k}: {e_gpu[k][0]:.3e} > {bnd:.3e}"
    if form == "host":                                        # IEEE arithmetic in the oracle's order on the oracle's alpha: the same bits
        for k in ("points", "normals", "colors", "ccounts"):
            assert np.array_equal(got[k], after_o[k]), f"{k}: not bit-identical to the fp32 oracle"
    else:
        assert s.count[:3].tolist() == [rows, rows, 0]
    if name == "no_correspondence":                           # the map stays bitwise untouched, the whole frame is appended
        assert tabs["active"].shape[0] == 0 and rows == s.M + s.H * s.W
        assert all(_same_bits(got[k][:s.M], c["state"][k]) for k in got)
    if name == "far_band_second":                             # c + a == 0: the rows are written as zeros, not as 0/0
        zero = c["state"]["ccounts"] == 0
        assert zero.sum() == 8 * 24 and all(not got[k][:s.M][zero].any() for k in got)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_map_step_overflow_clamps_and_flags(form):
    """capacity for only half of what the frame appends: rows beyond it are dropped, nothing is written behind it; the host form reports the
    needed count, the _dev form clamps the live count and raises the sticky flag, which a later step that fits does not lower"""
    name = "16x24"
    ref, after_o = R.reference(name), R.oracle(name)[0]
    M, need = ref["assoc"]["M"], after_o["ccounts"].shape[0]
    assert need - M > 20
    cap = M + (need - M) // 2
    s = Step(name, form, cap=cap)
    s.associate()
    rows = s.fuse_append()
    got = s.state(cap)                                        # (checks the guard band behind the capacity)
    for k in ("points", "normals", "colors", "ccounts"):     # the rows below the capacity are those of the step that had room
        if form == "host":
            assert np.array_equal(got[k], after_o[k][:cap]), f"{k}: not the first {cap} rows of the fp32 oracle's map"
        else:
            assert np.allclose(got[k], after_o[k][:cap], rtol=1e-5, atol=1e-7), k
    if form == "host":
        assert rows == need
    else:
        assert s.count[:3].tolist() == [cap, need, need]
        s.associate()
        assert s.fuse_append(depth=torch.zeros_like(s.depth)) == cap       # nothing to append: fits
        assert s.count[:3].tolist() == [cap, cap, need]                    # the flag stays


@pytest.mark.parametrize("name", ["16x24", "33x37", "1x8", "8x1", "72x100", "far_band_first"])
def test_frame_append_dev_against_float64(name):
    L = _L()
    c = R.get_case(name)
    H, W = c["H"], c["W"]
    maps = {k: v[0] for k, v in R.frame_maps(c["depth"][None], c["K"][None], c["pose"][None]).items()}
    ref = R.frame_append(maps, c["rgb"])
    om = opf.vertex_normal_maps(torch.from_numpy(c["depth"]), torch.from_numpy(c["K"]), torch.from_numpy(c["pose"]))
    ov = om["valid"]
    ora = dict(points=om["Vg"][ov].numpy(), normals=om["ng"][ov].numpy(), colors=c["rgb"][ov.numpy()], ccounts=opf.fusion_alpha(om["V"], R.SIGMA)[ov].numpy())
    k0, n = 7, ref["ccounts"].shape[0]                         # seven rows already live
    depth, rgb, Kd, pd = _dev(c["depth"]), _dev(c["rgb"]), _dev(c["K"]), _dev(c["pose"])
    assert n == int((c["depth"] != 0).sum())
    for cap, kept in ((k0 + n + 3, n), (k0 + n // 2, n // 2)):
        st = {k: _filled(np.full((k0, 1 if k == "ccounts" else 3), 0.25, np.float32), cap * (1 if k == "ccounts" else 3))
              for k in ("points", "normals", "colors", "ccounts")}
        count = _poison(3)
        count[:3] = torch.tensor([k0, 0, 0], device=DEV)
        nbytes = L.query("e2e_pf_workspace_bytes", cap, H, W)
        ws = _bytes(nbytes)
        L.call("e2e_frame_append_dev", map_points=L.ptr(st["points"]), map_normals=L.ptr(st["normals"]), map_colors=L.ptr(st["colors"]),
               map_ccounts=L.ptr(st["ccounts"]), map_count_dev=L.ptr(count), map_capacity=cap, depth=L.ptr(depth), rgb=L.ptr(rgb),
               K=L.ptr(Kd), pose=L.ptr(pd), alpha_den=float(R.ALPHA_DEN), workspace=L.ptr(ws), H=H, W=W, stream=L.stream())
        torch.cuda.synchronize()
        _guard_ok(ws, nbytes, "workspace")
        _guard_ok(count, 3, "map_count_dev")
        assert count[:3].tolist() == [k0 + kept, k0 + n, 0 if kept == n else k0 + n]
        for k, buf in st.items():
            w = 1 if k == "ccounts" else 3
            assert torch.isnan(buf[(k0 + kept) * w:]).all(), f"{k}: written beyond the live rows (capacity {cap})"
            a = buf[:(k0 + kept) * w].cpu().numpy().reshape(k0 + kept, w)
            assert (a[:k0] == 0.25).all(), f"{k}: the live rows were touched"
            _check(f"frame_append {name} cap {cap}", k, a[k0:], ref[k][:kept].reshape(kept, w), ora[k][:kept].reshape(kept, w))
            if k != "ccounts":
                assert np.array_equal(a[k0:], ora[k][:kept]), f"{k}: not bit-identical to the fp32 oracle"


def test_map_entry_points_refuse_bad_arguments():
    L = _L()
    E, st = L.E2EError, L.stream()
    f = _nan(64)
    out = [_nan(64) for _ in range(5)]
    rows, cnt = _poison(64), _poison(3)
    ws = _bytes(L.query("e2e_pf_workspace_bytes", 16, 2, 2))
    p, o = L.ptr(f), [L.ptr(t) for t in out]
    big = 32768                                               # 1 x 32768 x 32768 x 3 >= 2^31: refused from the dims alone, the buffers are tiny

    def refused(name, *args, **kw):
        with pytest.raises(E, match=name):
            L.call(name, *args, **kw)
        torch.cuda.synchronize()
        assert all(torch.isnan(t).all() for t in out) and (rows == POISON).all() and (cnt == POISON).all() and (ws == 0xA5).all(), \
            f"{name}: an output changed although the call was refused"

    for bad in (dict(depth=None), dict(K=None), dict(pose=None), dict(Vg=None), dict(B=0), dict(H=0), dict(H=big, W=big)):
        refused("e2e_vertex_normal_maps", **{**dict(depth=p, K=p, pose=p, alpha_den=0.72, V=o[0], Nm=o[1], Vg=o[2], Ng=o[3], alpha=o[4], B=1, H=2, W=2, stream=st), **bad})
    for bad in (dict(depth=None), dict(g_depth=None), dict(g_V=None, g_Vg=None), dict(W=-1), dict(H=big, W=big)):
        refused("e2e_vertex_maps_bwd", **{**dict(depth=p, K=p, pose=p, g_V=p, g_Vg=p, g_depth=o[0], B=1, H=2, W=2, stream=st), **bad})
    for args in ((None, p, o[0], 4, 0), (p, None, o[0], 4, 0), (p, p, None, 4, 0), (p, p, o[0], -1, 0)):
        refused("e2e_transform_points", *args, st)
    assoc = dict(map_points=p, map_normals=p, map_ccounts=p, M=4, K=p, pose=p, Vg=p, Ng=p, dist_th=0.05, dot_th=0.9, workspace=L.ptr(ws), map_capacity=16, H=2, W=2, stream=st)
    for bad in (dict(M=17), dict(M=-1), dict(K=None), dict(workspace=None), dict(map_points=None), dict(H=0)):
        refused("e2e_pf_associate", **{**assoc, **bad})
    adev = {k: v for k, v in assoc.items() if k != "M"}
    for bad in (dict(map_capacity=0), dict(map_count_dev=None), dict(map_points=None), dict(W=0)):
        refused("e2e_pf_associate_dev", **{**adev, "map_count_dev": L.ptr(cnt), **bad})
    for args in ((3, 4, L.ptr(ws), 16), (-1, 4, L.ptr(ws), 16), (0, 17, L.ptr(ws), 16), (0, 4, None, 16)):
        refused("e2e_pf_table", *args, 2, 2, L.ptr(rows), L.ptr(cnt), st)
    refused("e2e_pf_table", 0, 4, L.ptr(ws), 16, 2, 2, None, L.ptr(cnt), st)
    refused("e2e_pf_table", 0, 4, L.ptr(ws), 16, 2, 2, L.ptr(rows), None, st)
    fuse = dict(map_points=o[0], map_normals=o[1], map_colors=o[2], map_ccounts=o[3], M=4, map_capacity=16, depth=p, Vg=p, Ng=p, rgb=p, alpha=p,
                workspace=L.ptr(ws), H=2, W=2, new_count_out=L.ptr(cnt), stream=st)
    for bad in (dict(M=17), dict(alpha=None), dict(new_count_out=None), dict(map_colors=None), dict(H=0)):
        refused("e2e_pf_fuse_append", **{**fuse, **bad})
    fdev = {k: v for k, v in fuse.items() if k not in ("M", "new_count_out")}
    for bad in (dict(map_capacity=0), dict(map_count_dev=None), dict(rgb=None), dict(W=0)):
        refused("e2e_pf_fuse_append_dev", **{**fdev, "map_count_dev": L.ptr(cnt), **bad})
    fa = dict(map_points=o[0], map_normals=o[1], map_colors=o[2], map_ccounts=o[3], map_count_dev=L.ptr(cnt), map_capacity=16, depth=p, rgb=p, K=p, pose=p,
              alpha_den=0.72, workspace=L.ptr(ws), H=2, W=2, stream=st)
    for bad in (dict(map_capacity=0), dict(K=None), dict(map_count_dev=None), dict(H=big, W=big)):
        refused("e2e_frame_append_dev", **{**fa, **bad})
    assert L.query("e2e_pf_workspace_bytes", -1, 2, 2) == 0 and L.query("e2e_pf_workspace_bytes", 16, 0, 2) == 0 and L.query("e2e_pf_workspace_bytes", 16, 2, -3) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# nearest neighbour
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cloud(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "box":
        p = rng.uniform(-2, 2, (n, 3))
    elif kind == "small":                                     # 0.4 m across: below 127 x GRID_HMIN, the cell size is the floor
        p = rng.uniform(-0.2, 0.2, (n, 3)) + [1.0, -2.0, 3.0]
    elif kind == "planar":                                    # one axis with a single cell
        p = rng.uniform(-2, 2, (n, 3))
        p[:, 1] = 0.75
    elif kind == "single":
        p = np.tile([[0.5, -1.5, 2.5]], (n, 1))
    elif kind == "surface":
        uv = rng.uniform(-2, 2, (n, 2))
        p = np.stack([uv[:, 0], uv[:, 1], 2.0 + 0.3 * np.sin(uv[:, 0] * 2) * np.cos(uv[:, 1] * 3)], 1)
    p = p.astype(np.float32)
    if kind != "single" and n >= 8:
        p[n // 2] = p[1]                                      # duplicates: the smaller index must win
        p[n - 1] = p[1]
    return p


def _queries(p2, n1, seed):
    """near the references (a third exactly ON one: distance 0, and duplicates tie), a few far away"""
    rng = np.random.default_rng(seed)
    q = p2[rng.integers(0, p2.shape[0], n1)] + rng.normal(0, 0.05, (n1, 3)).astype(np.float32)
    on = rng.random(n1) < 0.3
    q[on] = p2[rng.integers(0, p2.shape[0], int(on.sum()))]
    far = rng.random(n1) < 0.05
    q[far] += rng.uniform(-3, 3, (int(far.sum()), 3)).astype(np.float32)
    if n1 > 1:
        q[1] = p2[min(1, p2.shape[0] - 1)]                    # on the duplicated point
    return q.astype(np.float32)


def _expect(what, d, i, ref):
    rd, ri = ref
    assert np.array_equal(i, ri), f"{what}: {int((i != ri).sum())} of {i.size} neighbours differ from the float32 brute force"
    assert _same_bits(d, rd), f"{what}: distances differ from the float32 brute force"


def _fwd(p1, p2, algorithm):
    L = _L()
    n1, n2 = p1.shape[0], p2.shape[0]
    nbytes = L.query("e2e_knn1_workspace_bytes", n1, n2)
    ws, d, i = _bytes(nbytes), _nan(n1), _poison(n1)
    p1d, p2d = _dev(p1), _dev(p2)
    L.call("e2e_knn1_fwd", L.ptr(p1d), n1, L.ptr(p2d), n2, L.ptr(d), L.ptr(i), L.ptr(ws), algorithm, L.stream())
    torch.cuda.synchronize()
    _guard_ok(ws, nbytes, "workspace")
    _guard_ok(i, n1, "idx")
    return _written(d, n1, "dists"), i[:n1].cpu().numpy()


@pytest.mark.parametrize("n2", [1, 3, 1023, 1024, 1025, 2049])
def test_knn_brute_force_tile_and_slice_edges(n2):
    p2 = _cloud("box", n2, n2)
    for n1 in (1, 255, 256, 257):
        p1 = _queries(p2, n1, n1)
        ref = KR.brute(p1, p2)
        for algo in (1, 0, 2):                                # brute, auto (n2 < 8192: brute) and the grid: identical
            d, i = _fwd(p1, p2, algo)
            _expect(f"n1={n1} n2={n2} algorithm {algo}", d, i, ref)
        assert KR.float64_check(p1, p2, ref[1]) <= 1.0
        if n2 >= 1023 and n1 >= 255:
            assert (ref[1] == 1).any() and not (ref[1] == n2 - 1).any() and not (ref[1] == n2 // 2).any()      # the duplicates resolve to the first


@pytest.mark.parametrize("n2", [8191, 8192])
def test_knn_auto_switch(n2):
    p2 = _cloud("surface", n2, 5)
    p1 = _queries(p2, 700, 6)
    ref = KR.brute(p1, p2)
    assert KR.float64_check(p1, p2, ref[1]) <= 1.0
    for algo in (0, 1, 2):
        d, i = _fwd(p1, p2, algo)
        _expect(f"n2={n2} algorithm {algo}", d, i, ref)


@pytest.mark.parametrize("n2", [3000, 3001, 3002, 3003])
def test_knn_index_build_from_a_misaligned_reference(n2):
    """the reference cloud starts 0, 4, 8 and 12 bytes past a 16-byte boundary (a slice of a larger flat buffer): the bounding-box pass
    reads float4s only when it may, and its scalar tail covers n2 % 4 points"""
    L = _L()
    p2 = _cloud("surface", n2, n2)
    p1 = _queries(p2, 500, 9)
    ref = KR.brute(p1, p2)
    flat = torch.zeros(n2 * 3 + 8, device=DEV)
    assert flat.data_ptr() % 16 == 0
    results, p1d = [], _dev(p1)
    for off in (0, 1, 2, 3):
        view = flat[off:off + n2 * 3]
        view.copy_(_dev(p2).reshape(-1))
        assert view.data_ptr() % 16 == 4 * off
        nbytes = L.query("e2e_knn1_workspace_bytes", 500, n2)
        idx_buf = _bytes(nbytes)
        d, i = _nan(500), _poison(500)
        L.call("e2e_knn1_index_build", L.ptr(view), n2, 500, L.ptr(idx_buf), L.stream())
        L.call("e2e_knn1_index_query", L.ptr(p1d), 500, n2, 500, L.ptr(idx_buf), L.ptr(d), L.ptr(i), L.stream())
        torch.cuda.synchronize()
        _guard_ok(idx_buf, nbytes, "index")
        _guard_ok(i, 500, "idx")
        results.append((_written(d, 500, "dists"), i[:500].cpu().numpy()))
        _expect(f"n2={n2} offset {4 * off} bytes", *results[-1], ref)
        assert _same_bits(results[-1][0], results[0][0]) and np.array_equal(results[-1][1], results[0][1])


class DevIndex:
    """a resident reference set: capacity well above the live count (the rows above it hold points that would win if read), the count on
    the device, the index at exactly the size its query returns"""

    def __init__(self, p2, max_queries, cells=0):
        L = self.L = _L()
        self.n2, self.cap, self.mq, self.cells = p2.shape[0], p2.shape[0] * 2 + 1000, max_queries, cells
        self.ref = torch.zeros(self.cap, 3, device=DEV)
        self.ref[:self.n2] = _dev(p2)
        self.count = _dev(np.array([self.n2], np.int64))
        q = ("e2e_knn1_index_capacity_bytes_res", max_queries, self.cap, cells) if cells else ("e2e_knn1_index_capacity_bytes", max_queries, self.cap)
        self.nbytes = L.query(*q)
        assert self.nbytes > 0
        self.index = _bytes(self.nbytes)
        if cells:
            L.call("e2e_knn1_index_build_dev_res", L.ptr(self.ref), L.ptr(self.count), self.cap, max_queries, L.ptr(self.index), cells, L.stream())
        else:
            L.call("e2e_knn1_index_build_dev", L.ptr(self.ref), L.ptr(self.count), self.cap, max_queries, L.ptr(self.index), L.stream())
        torch.cuda.synchronize()

    def trap(self, p1):
        """the dead rows above the live count become copies of the queries: distance 0 if anything reads them"""
        k = min(self.cap - self.n2, p1.shape[0])
        self.ref[self.n2:self.n2 + k] = _dev(p1[:k])

    def query(self, p1, how, row_len=0, warm=None, alias=False):
        L = self.L
        n1 = p1.shape[0]
        d, i = _nan(n1), _poison(n1)
        p1d = _dev(p1)
        w = None
        if warm is not None:
            if alias:
                i[:n1] = _dev(warm)
                w = i
            else:
                w = _dev(warm)
        if how == "dev":
            L.call("e2e_knn1_index_query_dev", L.ptr(p1d), n1, self.cap, self.mq, L.ptr(self.index), L.ptr(d), L.ptr(i), L.stream())
        elif how == "image":
            L.call("e2e_knn1_index_query_dev_image", L.ptr(p1d), n1, row_len, self.cap, self.mq, L.ptr(self.index), L.ptr(d), L.ptr(i), L.stream())
        elif how == "warm":
            L.call("e2e_knn1_index_query_dev_image_warm", p1=L.ptr(p1d), n1=n1, row_len=row_len, ref_points=L.ptr(self.ref), warm_idx=L.ptr(w),
                   n2_capacity=self.cap, max_queries=self.mq, index=L.ptr(self.index), dists=L.ptr(d), idx=L.ptr(i), stream=L.stream())
        else:
            L.call("e2e_knn1_index_query_dev_res", p1=L.ptr(p1d), n1=n1, ref_points=L.ptr(self.ref) if w is not None else None, warm_idx=L.ptr(w),
                   n2_capacity=self.cap, max_queries=self.mq, index=L.ptr(self.index), cells_per_axis=self.cells, dists=L.ptr(d), idx=L.ptr(i), stream=L.stream())
        torch.cuda.synchronize()
        _guard_ok(self.index, self.nbytes, "index")
        _guard_ok(i, n1, "idx")
        return _written(d, n1, "dists"), i[:n1].cpu().numpy()


def _warm_candidates(ref_idx, n2, seed):
    """right, random, negative, >= the live count (the first dead row, and far beyond), in turn"""
    rng = np.random.default_rng(seed)
    w = ref_idx.copy()
    k = np.arange(w.size) % 5
    w[k == 1] = rng.integers(0, n2, int((k == 1).sum()))
    w[k == 2] = -1 - rng.integers(0, 5, int((k == 2).sum()))
    w[k == 3] = n2
    w[k == 4] = n2 + 12345678
    return w


@pytest.mark.parametrize("kind,n2", [("surface", 9000), ("small", 5000), ("planar", 5000), ("single", 1), ("single", 300), ("box", 8191)])
def test_knn_resident_index_forms(kind, n2):
    p2 = _cloud(kind, n2, n2 + 1)
    rows, row_len = 24, 40                                    # 960 queries: whole 8 x 8 tiles
    p1 = _queries(p2, rows * row_len, 17)
    ref = KR.brute(p1, p2)
    assert KR.float64_check(p1, p2, ref[1]) <= 1.0
    ix = DevIndex(p2, rows * row_len + 7)
    ix.trap(p1)
    warm = _warm_candidates(ref[1], n2, 3)
    for what, kw in (("dev", dict(how="dev")), ("image tiles", dict(how="image", row_len=row_len)), ("image, row_len 0", dict(how="image", row_len=0)),
                     ("image, row_len not a multiple of 8", dict(how="image", row_len=30)), ("warm", dict(how="warm", row_len=row_len, warm=warm)),
                     ("warm, aliased with idx", dict(how="warm", row_len=row_len, warm=warm, alias=True)),
                     ("warm, plain order", dict(how="warm", row_len=30, warm=warm))):
        d, i = ix.query(p1, **kw)
        _expect(f"{kind} n2={n2} {what}", d, i, ref)
    d, i = _fwd(p1, p2, 2)                                    # the one-shot grid on the same cloud
    _expect(f"{kind} n2={n2} one-shot grid", d, i, ref)
    d, i = ix.query(p1[:333], "dev")                          # fewer queries than the index was built for
    _expect(f"{kind} n2={n2} 333 queries", d, i, (ref[0][:333], ref[1][:333]))


@functools.lru_cache(maxsize=None)
def _res_case():
    p2 = _cloud("surface", 9000, 31)
    p1 = _queries(p2, 40000, 32)
    return p2, p1, KR.brute(p1, p2)


def test_knn_reference_of_the_large_query_set_in_float64():
    p2, p1, ref = _res_case()
    assert KR.float64_check(p1, p2, ref[1], sel=np.arange(0, 40000, 10)) <= 1.0


@pytest.mark.parametrize("cells", [4, 32, 256])
def test_knn_resolution_forms(cells):
    """n1 = 40 000 > 32 768: the per-lane pass in plain order, cold and warm-started; n1 = 2000: a wave per query from the start"""
    p2, p1, ref = _res_case()
    ix = DevIndex(p2, 40000, cells=cells)
    ix.trap(p1)
    warm = _warm_candidates(ref[1], 9000, 4)
    for what, q, r, w in (("40000 cold", p1, ref, None), ("40000 warm", p1, ref, warm), ("2000 cold", p1[:2000], (ref[0][:2000], ref[1][:2000]), None), ("2000 warm", p1[:2000], (ref[0][:2000], ref[1][:2000]), warm[:2000])):
        d, i = ix.query(q, "res", warm=w)
        _expect(f"cells {cells} {what}", d, i, r)


def test_knn_backward_against_float64():
    L = _L()
    rng = np.random.default_rng(41)
    n1, n2 = 1000, 300
    p2 = _cloud("box", n2, 42)
    p1 = _queries(p2, n1, 43)
    g = rng.standard_normal(n1).astype(np.float32)
    _, idx = KR.brute(p1, p2)
    out = _nan(n1 * 3)
    gd, p1d, p2d, idxd = _dev(g), _dev(p1), _dev(p2), _dev(idx)
    L.call("e2e_knn1_bwd", L.ptr(gd), L.ptr(p1d), L.ptr(p2d), L.ptr(idxd), n1, L.ptr(out), L.stream())
    torch.cuda.synchronize()
    got = _written(out, n1 * 3, "g_p1").reshape(n1, 3)
    a, b = p1, p2[idx]
    ora = (np.float32(2.0) * g)[:, None] * (a - b)
    _check("knn1_bwd", "g_p1", got, KR.knn1_bwd(g, p1, p2, idx), ora)


def _bwd_ref(g, p1, p2, idx):
    L = _L()
    n1, n2 = p1.shape[0], p2.shape[0]
    scratch, out = _poison(3 * n2 + 1), _nan(n2 * 3)
    gd, p1d, p2d, idxd = _dev(g), _dev(p1), _dev(p2), _dev(idx)
    L.call("e2e_knn1_bwd_ref", L.ptr(gd), L.ptr(p1d), L.ptr(p2d), L.ptr(idxd), n1, n2, L.ptr(scratch), L.ptr(out), L.stream())
    torch.cuda.synchronize()
    _guard_ok(scratch, 3 * n2 + 1, "scratch_fixed")
    _guard_ok(out, n2 * 3, "g_p2")
    return out[:n2 * 3].cpu().numpy().reshape(n2, 3)


def test_knn_backward_wrt_the_reference_cloud():
    rng = np.random.default_rng(51)
    n1, n2 = 3000, 40
    p2 = rng.uniform(-2, 2, (n2, 3)).astype(np.float32)
    p2[27] = [0.5, -0.25, 1.0]                                # dyadic: p1 - p2 below is exactly (1, 0, 0)
    idx = rng.integers(0, 5, n1)                              # hundreds of queries share each of five neighbours
    idx[:20] = np.arange(20, 40)                              # ... twenty have one, fifteen none
    p1 = (p2[idx] + rng.normal(0, 0.3, (n1, 3))).astype(np.float32)
    g = rng.standard_normal(n1).astype(np.float32)
    ref, o32, count = KR.knn1_bwd_ref(g, p1, p2, idx)
    assert count[:5].min() > 500 and (count[20:] == 1).all() and not count[5:20].any()
    got = _bwd_ref(g, p1, p2, idx)
    e_gpu, e_or = float(np.abs(got - ref).max()), float(np.abs(o32 - ref).max())
    bnd = R.bound(e_or, np.abs(ref).max()) + float(count.max()) * 2.0 ** -48
    RECORD.append(("knn1_bwd_ref", "g_p2", e_gpu, e_or, bnd))
    print(f"knn1_bwd_ref: gpu {e_gpu:.3e}  oracle formula {e_or:.3e}  bound {bnd:.3e}")
    assert e_gpu <= bnd and not got[5:20].any()
    assert _same_bits(_bwd_ref(g, p1, p2, idx), got), "two runs differ"
    # a contribution of 4096 or more poisons everything; one just below does not
    p1b, gb = p1.copy(), g.copy()
    assert idx[7] == 27
    p1b[7] = p2[27] + np.float32([1.0, 0.0, 0.0])
    gb[7] = np.float32(-2048.0)                               # -2 g (p1 - p2) = 4096 exactly
    assert np.isnan(_bwd_ref(gb, p1b, p2, idx)).all()
    gb[7] = np.nextafter(np.float32(-2048.0), np.float32(0))
    got = _bwd_ref(gb, p1b, p2, idx)
    ref = KR.knn1_bwd_ref(gb, p1b, p2, idx)[0]
    assert np.isfinite(got).all() and np.abs(got - ref).max() <= 4 * R.ulp32(4096.0)


def test_knn_entry_points_refuse_bad_arguments():
    L = _L()
    E, st = L.E2EError, L.stream()
    f, d, i = _nan(64), _nan(64), _poison(64)
    ws = _bytes(L.query("e2e_knn1_index_capacity_bytes_res", 8, 8, 4))
    p, w = L.ptr(f), L.ptr(ws)

    def refused(name, *args):
        with pytest.raises(E, match=name):
            L.call(name, *args)
        torch.cuda.synchronize()
        assert torch.isnan(d).all() and (i == POISON).all() and (ws == 0xA5).all(), f"{name}: an output changed although the call was refused"

    for args in ((None, 4, p, 4, L.ptr(d), L.ptr(i), w, 1), (p, 4, None, 4, L.ptr(d), L.ptr(i), w, 1), (p, 4, p, 4, None, L.ptr(i), w, 1), (p, 4, p, 4, L.ptr(d), None, w, 1),
                 (p, 4, p, 4, L.ptr(d), L.ptr(i), None, 1), (p, 0, p, 4, L.ptr(d), L.ptr(i), w, 1), (p, 4, p, 0, L.ptr(d), L.ptr(i), w, 1),
                 (p, 4, p, 4, L.ptr(d), L.ptr(i), w, 3), (p, 4, p, 4, L.ptr(d), L.ptr(i), w, -1)):
        refused("e2e_knn1_fwd", *args, st)
    refused("e2e_knn1_index_build", None, 4, 8, w, st)
    refused("e2e_knn1_index_build", p, 0, 8, w, st)
    refused("e2e_knn1_index_build", p, 4, 0, w, st)
    refused("e2e_knn1_index_query", p, 9, 4, 8, w, L.ptr(d), L.ptr(i), st)                    # n1 > max_queries
    refused("e2e_knn1_index_query", p, 4, 4, 8, w, None, L.ptr(i), st)
    refused("e2e_knn1_index_build_dev", p, None, 8, 8, w, st)
    refused("e2e_knn1_index_build_dev", p, L.ptr(i), 0, 8, w, st)
    refused("e2e_knn1_index_query_dev", p, 9, 8, 8, w, L.ptr(d), L.ptr(i), st)
    refused("e2e_knn1_index_query_dev_image", p, 9, 0, 8, 8, w, L.ptr(d), L.ptr(i), st)
    refused("e2e_knn1_index_query_dev_image", p, 4, -8, 8, 8, w, L.ptr(d), L.ptr(i), st)
    refused("e2e_knn1_index_query_dev_image_warm", p, 9, 0, p, L.ptr(i), 8, 8, w, L.ptr(d), L.ptr(i), st)
    refused("e2e_knn1_index_query_dev_image_warm", p, 4, 0, None, L.ptr(i), 8, 8, w, L.ptr(d), L.ptr(i), st)
    for cells in (3, 257):
        refused("e2e_knn1_index_build_dev_res", p, L.ptr(i), 8, 8, w, cells, st)
        refused("e2e_knn1_index_query_dev_res", p, 4, None, None, 8, 8, w, cells, L.ptr(d), L.ptr(i), st)
        assert L.query("e2e_knn1_index_capacity_bytes_res", 8, 8, cells) == 0
    refused("e2e_knn1_index_query_dev_res", p, 9, None, None, 8, 8, w, 4, L.ptr(d), L.ptr(i), st)
    refused("e2e_knn1_index_query_dev_res", p, 4, p, None, 8, 8, w, 4, L.ptr(d), L.ptr(i), st)     # a reference without candidates
    refused("e2e_knn1_index_query_dev_res", p, 4, None, L.ptr(i), 8, 8, w, 4, L.ptr(d), L.ptr(i), st)
    refused("e2e_knn1_bwd", p, p, p, L.ptr(i), 0, L.ptr(d), st)
    refused("e2e_knn1_bwd", p, p, p, None, 4, L.ptr(d), st)
    refused("e2e_knn1_bwd_ref", p, p, p, L.ptr(i), 4, 0, L.ptr(i), L.ptr(d), st)
    refused("e2e_knn1_bwd_ref", p, p, p, L.ptr(i), 4, 4, None, L.ptr(d), st)
    assert L.query("e2e_knn1_workspace_bytes", 0, 4) == 0 and L.query("e2e_knn1_workspace_bytes", 4, 0) == 0
    assert L.query("e2e_knn1_index_capacity_bytes", 0, 4) == 0 and L.query("e2e_knn1_index_capacity_bytes", 4, -1) == 0
    assert L.query("e2e_knn1_index_capacity_bytes_res", 8, 8, 4) > 0 and L.query("e2e_knn1_index_capacity_bytes_res", 8, 8, 256) > L.query("e2e_knn1_index_capacity_bytes_res", 8, 8, 4)


def test_zz_record_of_the_payload_comparisons():
    """the figures of every payload comparison of this run (pytest -s; profiles/map_contracts.txt keeps a copy): measured error, the fp32
    oracle's error on the same inputs, the bound that results -- and, for every map step, the skipped shares of points and pixels"""
    for case, what, a, b, c in RECORD:
        print(f"RECORD | {case} | {what} | {a:.3e} | {b:.3e} | {c:.3e}")
        assert a <= c or what == "skipped share"
