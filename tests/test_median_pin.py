"""tests/median_pin.py::pin, the one place that turns an oracle record's median_indices into the named-element argument (CPU only)."""
import pytest
import torch


def test_pin_names_at_most_64_elements_as_int32():
    from e2ehip import ops
    from median_pin import pin
    t = pin(list(range(100, 164)), "cpu")
    assert t.dtype == torch.int32 and t.shape == (64,) and t.tolist() == list(range(100, 164))
    assert pin([7], "cpu").tolist() == [7]
    with pytest.raises(AssertionError, match="65 elements hold the median"):
        pin(list(range(65)), "cpu")
    assert pin(list(range(65)), "cpu", allow_truncate=True).tolist() == list(range(64))      # explicit, never silent
    # the operator's own argument check: int32 and on the device -- pin's dtype passes it, this host copy stops at the device half
    disp, mgt = torch.ones(2, 1, 4, 4), torch.ones(1)
    with pytest.raises(TypeError, match="device int32"):
        ops.depth_from_disp_median_scaled(disp, mgt, t)
    with pytest.raises(TypeError, match="device int32"):
        ops.depth_from_disp_median_scaled(disp, mgt, t.long())
