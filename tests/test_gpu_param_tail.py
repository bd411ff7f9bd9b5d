"""The two kernels that end a step's parameter update: the batched slab reduction of the deferred backward-weight GEMMs
(e2e_wgrad_reduce_batch_prepare + e2e_wgrad_reduce_batched) and the batched weight-layout transform (e2e_conv_weight_layouts_batched).

The batched reduction in the tree is the one that was there before this file (a wave-owned form was measured and rejected,
profiles/param_tail_reduce_wave_items_rejected.txt): its tests here are regression cover for the next attempt, written against the
interface and not against the kernel's work-item layout.  The layout kernel is the one this file was written with.

Reduction: every layer runs e2e_conv2d_bwd_weight_scaled_deferred, the descriptors go through ONE batched launch, and the result must
equal e2e_conv2d_bwd_weight_scaled (the per-layer kernel, the reference of the association of the slab sum) bit for bit, and a float64
weight gradient within the tolerance tests/test_gpu_conv.py uses for backward-weight (5e-5 of max |dW|).

Layers (B, channels, pixels) and what each one provides -- the slab count S and the association rule zl are READ from the descriptors
the planner returns and asserted in test_the_planner_gave_the_slab_counts_the_loops_need:
  bn64     3x3 64 -> 64, folded-BatchNorm scale, B = 2 at 32 x 48: implicit GEMM, zl = 8 with an S that is no multiple of 8
  cat96    3x3 (32 up x2 + 64 skip) -> 32, bias, reflection padding, B = 1 at 32 x 48: Kconv + 1 = 865 is no multiple of 4 (bias column
           in a quad of its own); ragged last block of input channels (96 = 64 + 32)
  thin16   3x3 16 -> 16, bias, reflection padding, B = 2 at 72 x 48: the thin patch kernel writes one slab per 4 image rows and batch
           element, S = 36 > 4 * zl -- 72 rows, more than the other layers' 32, because no path of the planner reaches S > 32 below that
  down1x1  1x1 64 -> 128, stride 2, scale, B = 2 at 32 x 48: 1x1 (dW contiguous in the GEMM's column order), zl = 2 with an odd S
  stem     7x7 3 -> 64, stride 2, input normalisation, B = 2 at 32 x 48: Cin = 3, the scalar scatter
  wide     3x3 1088 -> 512, B = 1 at 8 x 8: 512 x 2448 quads (512 x 17 blocks of 64 input channels) -- far more work items (19 584 groups of 64 quads) than
           workgroups a launch can keep resident, so a grid-stride loop over the items has to run
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: B, Cin, C1, up, Hs, Ws, Cout, k, stride, pad, pad_mode (1 = reflect), bias, scale
LAYERS = {
    "bn64": (2, 64, 64, 1, 32, 48, 64, 3, 1, 1, 0, False, True),
    "cat96": (1, 96, 32, 2, 32, 48, 32, 3, 1, 1, 1, True, False),
    "thin16": (2, 16, 16, 1, 72, 48, 16, 3, 1, 1, 1, True, False),
    "down1x1": (2, 64, 64, 1, 32, 48, 128, 1, 2, 0, 0, False, True),
    "stem": (2, 3, 3, 1, 32, 48, 64, 7, 2, 3, 0, False, True),
    "wide": (1, 1088, 1088, 1, 8, 8, 512, 3, 1, 1, 0, False, True),
}
ORDER_A = ["bn64", "cat96", "thin16", "down1x1", "stem", "wide"]
ORDER_B = ["wide", "stem", "thin16", "bn64", "down1x1", "cat96"]          # the descriptor lookup depends on the order of the table


def _L():
    from e2ehip import _lib as L
    L.load()
    return L


def _fp64(spec, src0, src1, da, scale):
    B, Cin, C1, up, Hs, Ws, Cout, k, stride, pad, pm, has_bias, has_scale = spec
    x = src0.double().permute(0, 3, 1, 2)
    if Cin == 3:
        x = (x - 0.45) * (1 / 0.225)
    if up != 1:
        x = F.interpolate(x, scale_factor=up, mode="nearest")
    if src1 is not None:
        x = torch.cat([x, src1.double().permute(0, 3, 1, 2)], 1)
    if pm == 1:
        x, pad = F.pad(x, (pad,) * 4, mode="reflect"), 0
    cols = F.unfold(x, k, padding=pad, stride=stride)                  # (B, Cin k k, P), rows in (ci, kh, kw) order
    g = da.double().reshape(B, -1, Cout)                               # (B, P, Cout)
    dw = torch.einsum("bpo,bcp->oc", g, cols).reshape(Cout, Cin, k, k)
    if scale is not None:
        dw = dw * scale.double().view(-1, 1, 1, 1)
    return dw, g.sum((0, 1))


class _Layer:
    """inputs of one layer, its float64 gradient, and per accumulate flag: the per-layer result and a deferred descriptor with its slabs"""

    def __init__(self, name, seed):
        L = _L()
        lib = L.load()
        self.name, self.spec = name, LAYERS[name]
        B, Cin, C1, up, Hs, Ws, Cout, k, stride, pad, pm, has_bias, has_scale = self.spec
        g = torch.Generator().manual_seed(seed)
        Ho, Wo = (Hs + 2 * pad - k) // stride + 1, (Ws + 2 * pad - k) // stride + 1
        self.src0 = torch.randn(B, Hs // up, Ws // up, C1, generator=g).to(DEV)
        self.src1 = torch.randn(B, Hs, Ws, Cin - C1, generator=g).to(DEV) if C1 < Cin else None
        self.da = torch.randn(B, Ho, Wo, Cout, generator=g).to(DEV)
        self.scale = (torch.rand(Cout, generator=g) + 0.5).to(DEV) if has_scale else None
        self.fill_w = torch.randn(Cout, Cin, k, k, generator=g).to(DEV)
        self.fill_b = torch.randn(Cout, generator=g).to(DEV) if has_bias else None
        self.ref64 = _fp64(self.spec, self.src0, self.src1, self.da, self.scale)
        n_ws = lib.e2e_conv2d_wgrad_workspace_floats(B, Ho, Wo, Cin, Cout, k, k, 1 if has_bias else 0)
        self.per_layer, self.desc, self.keep = {}, {}, []
        for acc in (0, 1):
            for deferred in (False, True):
                dw, db = self.sinks(acc)
                ws = torch.empty(n_ws, device=DEV)
                args = [L.ptr(self.da), L.ptr(self.scale), L.ptr(self.src0), L.ptr(self.src1), C1, up, L.ptr(dw), L.ptr(db), L.ptr(ws), B, Hs, Ws, Cin, Cout,
                        Ho, Wo, k, k, stride, pad, pm, acc, 0.45 if Cin == 3 else 0.0, 1 / 0.225 if Cin == 3 else 1.0]
                if deferred:
                    d = L.WgradReduceDesc()
                    L.call("e2e_conv2d_bwd_weight_scaled_deferred", *args, ctypes.byref(d), L.stream())
                    self.desc[acc] = d
                    self.keep.append(ws)                                   # the slabs stay untouched until (and while) they are reduced
                else:
                    L.call("e2e_conv2d_bwd_weight_scaled", *args, L.stream())
                    self.per_layer[acc] = (dw, db)
        torch.cuda.synchronize()

    def sinks(self, acc):
        """fresh dW / dbias: pre-filled when the call accumulates, NaN when it overwrites"""
        if acc:
            return self.fill_w.clone(), (self.fill_b.clone() if self.fill_b is not None else None)
        return torch.full_like(self.fill_w, float("nan")), (torch.full_like(self.fill_b, float("nan")) if self.fill_b is not None else None)

    def desc_into(self, acc, dw, db):
        """the deferred descriptor (same slabs) pointed at other sinks"""
        L = _L()
        d = L.WgradReduceDesc.from_buffer_copy(bytes(self.desc[acc]))
        d.dw, d.dbias = dw.data_ptr(), (db.data_ptr() if db is not None else None)
        return d


@pytest.fixture(scope="module")
def layers():
    return {name: _Layer(name, 100 + i) for i, name in enumerate(ORDER_A)}


def _reduce(descs):
    L = _L()
    arr = (L.WgradReduceDesc * len(descs))(*descs)
    total = L.load().e2e_wgrad_reduce_batch_prepare(arr, len(descs))
    assert total > 0
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
    L.call("e2e_wgrad_reduce_batched", L.ptr(table), len(descs), total, L.stream())
    torch.cuda.synchronize()
    return total


def test_the_planner_gave_the_slab_counts_the_loops_need(layers):
    d = {n: layers[n].desc[0] for n in ORDER_A}
    print({n: (x.S, x.zl) for n, x in d.items()})
    assert {x.zl for x in d.values()} == {2, 8}
    assert d["bn64"].zl == 8 and d["bn64"].S % 8 != 0                 # a ragged last turn of the eight accumulators
    assert d["down1x1"].zl == 2 and d["down1x1"].S % 2 != 0
    assert d["thin16"].S > 4 * d["thin16"].zl                         # more than four whole turns: the unrolled round runs more than once
    assert d["cat96"].has_bias and (9 * 96 + 1) % 4 != 0
    assert d["wide"].Cout * ((d["wide"].Cin + 63) // 64) > 8192 and d["wide"].Cout * (9 * d["wide"].Cin // 4) // 64 > 8192


@pytest.mark.parametrize("acc", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("order", ["A", "B"])
def test_one_launch_over_all_layers_equals_the_per_layer_kernel(layers, order, acc):
    names = ORDER_A if order == "A" else ORDER_B
    sinks = {n: layers[n].sinks(acc) for n in names}
    _reduce([layers[n].desc_into(acc, *sinks[n]) for n in names])
    for n in names:
        dw_r, db_r = layers[n].per_layer[acc]
        assert torch.isfinite(dw_r).all()
        assert torch.equal(dw_r, sinks[n][0]), f"{n}: dW differs in {(dw_r != sinks[n][0]).sum().item()} of {dw_r.numel()} elements"
        if db_r is not None:
            assert torch.equal(db_r, sinks[n][1]), f"{n}: dbias"


@pytest.mark.parametrize("acc", [0, 1], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("name", ORDER_A)
def test_a_table_of_one_descriptor(layers, name, acc):
    lay = layers[name]
    dw, db = lay.sinks(acc)
    _reduce([lay.desc_into(acc, dw, db)])
    assert torch.equal(lay.per_layer[acc][0], dw), name
    if db is not None:
        assert torch.equal(lay.per_layer[acc][1], db), name


@pytest.mark.parametrize("name", ORDER_A)
def test_batched_reduction_against_float64(layers, name):
    lay = layers[name]
    dw, db = lay.sinks(0)
    _reduce([lay.desc_into(0, dw, db)])
    dw64, db64 = lay.ref64
    e = ((dw.double() - dw64).abs().max() / (dw64.abs().max() + 1e-30)).item()
    print(name, "dW error / max|dW|", e)
    assert e < 5e-5, f"{name}: {e:.2e}"
    if db is not None:
        eb = ((db.double() - db64).abs().max() / (db64.abs().max() + 1e-30)).item()
        assert eb < 5e-5, f"{name} dbias: {eb:.2e}"


# ---------------------------------------------------------------------------------------------------------------------
# weight layouts
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 3, 7), (64, 64, 3), (32, 96, 3), (16, 16, 3), (128, 64, 1), (256, 512, 3), (40, 20, 3)]     # the last: both tile edges ragged


def _layout_case(shapes, with_scale, with_wb, packed, seed):
    """rows of the descriptor table and the expected w_fwd / w_bwd by plain indexing; packed: the weights are views into one flat buffer
    that starts one float past an aligned address (parameters in a flat bucket are not 16-byte aligned)"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.empty(sum(co * ci * k * k for co, ci, k in shapes) + 1, device=DEV)
    off, rows, checks, keep = 1, [], [], [flat]
    for i, (Cout, Cin, k) in enumerate(shapes):
        T = k * k
        w = (torch.randn(Cout, Cin, k, k, generator=g)).to(DEV)
        if packed:
            view = flat[off:off + w.numel()].view(Cout, Cin, k, k)
            view.copy_(w)
            w, off = view, off + w.numel()
        stem = k == 7
        ldf, ldb = (Cout + 3) // 4 * 4 + (4 if i % 2 else 0), (Cin + 3) // 4 * 4 + (4 if i % 3 == 0 else 0)
        wf = torch.zeros(T * Cin, ldf, device=DEV)
        wb = torch.zeros(T * Cout, ldb, device=DEV) if (with_wb and not stem) else None          # the stem has no backward-data layout
        sc = (torch.rand(Cout, generator=g) + 0.5).to(DEV) if (with_scale and wb is not None) else None
        rows.append([w.data_ptr(), wf.data_ptr(), wb.data_ptr() if wb is not None else 0, Cout, Cin, k, k, ldf, ldb, sc.data_ptr() if sc is not None else 0])
        ef = torch.zeros_like(wf)
        ef[:, :Cout] = w.permute(2, 3, 1, 0).reshape(T * Cin, Cout)
        eb = None
        if wb is not None:
            eb = torch.zeros_like(wb)
            ws = w * sc.view(-1, 1, 1, 1) if sc is not None else w                              # one fp32 multiply
            eb[:, :Cin] = ws.permute(2, 3, 0, 1).reshape(T * Cout, Cin)
        checks.append(((Cout, Cin, k), wf, ef, wb, eb))
        keep += [w, sc]
    return rows, checks, keep


@pytest.mark.parametrize("packed", [False, True], ids=["aligned", "flat_bucket"])
@pytest.mark.parametrize("with_wb", [True, False], ids=["wb", "no_wb"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "bsc"])
@pytest.mark.parametrize("shapes", [SHAPES, SHAPES[5:6], SHAPES[6:7], SHAPES[0:1]], ids=["seven", "one_big", "one_ragged", "one_stem"])
def test_weight_layouts_batched(shapes, with_scale, with_wb, packed):
    L = _L()
    rows, checks, keep = _layout_case(shapes, with_scale, with_wb, packed, seed=7 + len(shapes))
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    L.call("e2e_conv_weight_layouts_batched", L.ptr(desc), len(rows), L.stream())
    torch.cuda.synchronize()
    for shape, wf, ef, wb, eb in checks:
        assert torch.equal(wf, ef), f"w_fwd of {shape}: {(wf != ef).sum().item()} elements differ (padded columns must stay zero)"
        if wb is not None:
            assert torch.equal(wb, eb), f"w_bwd of {shape}: {(wb != eb).sum().item()} elements differ"


def test_more_tiles_than_workgroups_and_a_table_longer_than_the_prefix():
    """The flat tile list against the launch: (a) two 1x1 1024 x 1024 layers (1024 tiles each) and a 3x3 512 x 512 layer (256 tiles) are 2304
    tiles, more than the 8 workgroups per compute unit the host launches on a 256-CU device (2048): the grid-stride loop takes a second turn, in
    which a workgroup that transposed a T = 1 tile of the first layer re-uses its LDS tile for a T = 9 tile of the last; (b) 260 small layers,
    more than the 256 the kernel's prefix holds, so the host splits the table over two launches."""
    L = _L()
    for shapes, seed in (([(1024, 1024, 1), (1024, 1024, 1), (512, 512, 3)], 31), ([(16, 16, 3), (24, 8, 1)] * 130, 32)):
        rows, checks, keep = _layout_case(shapes, True, True, False, seed=seed)
        desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
        L.call("e2e_conv_weight_layouts_batched", L.ptr(desc), len(rows), L.stream())
        torch.cuda.synchronize()
        for i, (shape, wf, ef, wb, eb) in enumerate(checks):
            assert torch.equal(wf, ef), f"layer {i} w_fwd of {shape}"
            assert torch.equal(wb, eb), f"layer {i} w_bwd of {shape}"
