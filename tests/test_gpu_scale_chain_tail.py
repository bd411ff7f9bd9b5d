"""k_scale_chain_bwd with the partial sums of S = sum(g * delta) fetched into LDS by the whole workgroup (the product's form) against
the form whose thread 0 reads them from global memory one after the other (E2E_SCALE_CHAIN_STAGED=0): thread 0 adds the same values
in the same order in double and rounds once, so g_disp is the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# 614 400: the benchmark's 480 x 640 x 2 (512 partials); 300: 2 partials, fewer than threads; 256 * 512 + 1: the first size past one
# element per thread of the 512 workgroups
@pytest.mark.parametrize("n", [614400, 300, 256 * 512 + 1])
def test_staged_partials_give_the_same_bits(n, monkeypatch):
    from e2ehip import _lib as L
    g = torch.Generator().manual_seed(n)
    disp = (torch.rand(n, generator=g) * 0.9 + 0.05).to(DEV)
    g_depth = torch.randn(n, generator=g).to(DEV)
    mgt = torch.tensor([2.5], device=DEV)
    ws = torch.empty(L.load().e2e_depth_scale_workspace_bytes(), device=DEV, dtype=torch.uint8)
    delta, depth, med, ratio = (torch.empty(k, device=DEV) for k in (n, n, 1, 1))
    L.call("e2e_depth_scale_fwd", L.ptr(disp), L.ptr(mgt), L.ptr(delta), L.ptr(depth), L.ptr(med), L.ptr(ratio), L.ptr(ws), n, L.stream())
    out = {}
    for staged in ("1", "0"):
        monkeypatch.setenv("E2E_SCALE_CHAIN_STAGED", staged)
        gd = torch.full((n,), float("nan"), device=DEV)
        L.call("e2e_depth_scale_bwd", L.ptr(g_depth), L.ptr(delta), L.ptr(mgt), L.ptr(med), L.ptr(gd), L.ptr(ws), n, L.stream())
        torch.cuda.synchronize()
        out[staged] = gd
    assert not torch.isnan(out["1"]).any()
    assert torch.equal(out["1"], out["0"])
    # the correction term is there at all: the median element's gradient differs from rho * g alone
    d = delta.double()
    plain = -(d * d) * (ratio.double() * g_depth.double())
    assert ((out["1"].double() - plain).abs() > 0).sum().item() >= 1
