"""Test instrumentation: naming the median ELEMENTS of a refinement step (no fixtures; the driver tests import it).

The median element of the stacked predictions is where two correct fp32 evaluations of the refinement loop can part: among 614 400
depths the median's neighbours lie ~1e-6 away, and the ratio's backward puts a sum over all pixels on the element(s) that hold the
median.  The tests name one run's elements to the other (e2e_depth_scale_bwd_at puts the gradient on exactly those) and compare
everything else.  The product classes know nothing of this: they offer the seams overridden below."""
import torch

from e2ehip import _lib as L
from e2ehip.stepplan import RefineStepPlan
from online_adaption import SLAM

MAX_NAMED = 64          # e2e_depth_scale_bwd_at takes 1..64 named elements (include/e2eslam.h)


def pin(indices, device, allow_truncate=False):
    """An oracle record's `median_indices` (flat indices into the stacked (2,1,H,W) predictions of every element equal to the median)
    as the device int32 tensor the named-element entry points take.  More than 64 holders is an error, not a silent slice: dropping
    tied holders changes where the gradient lands.  allow_truncate: the caller has a stated reason to keep the first 64 only."""
    indices = list(indices)
    if not allow_truncate:
        assert len(indices) <= MAX_NAMED, f"{len(indices)} elements hold the median; at most {MAX_NAMED} can be named"
    return torch.tensor(indices[:MAX_NAMED], dtype=torch.int32, device=device)


class PinnedStepPlan(RefineStepPlan):
    """median_elements_override: None, or device int32 indices of the elements the ratio's gradient lands on in the next step(s)
    instead of on this evaluation's own median holders."""
    median_elements_override = None

    def _median_chain_backward(self, st):
        ov = self.median_elements_override
        L.call("e2e_depth_scale_bwd_at", L.ptr(self.g_depth), L.ptr(self.delta), L.ptr(self.median_gt), L.ptr(self.md), L.ptr(ov),
               0 if ov is None else int(ov.numel()), L.ptr(self.net.disp.g), L.ptr(self.ws_scale), self.g_depth.numel(), st)

    def _backward_key(self, use_3d, ikey):
        # the element list is a launch argument frozen into the captured graph: one graph per list
        ov = self.median_elements_override
        return super()._backward_key(use_3d, ikey) + (None if ov is None else (ov.data_ptr(), ov.numel()),)


class PinnedSLAM(SLAM):
    """median_elements[k]: device int32 indices for refinement step k of this object (both forms of the step), or None.
    median_elements_log: when a list, every launch-plan step appends the indices of its own median holders."""
    step_plan_class = PinnedStepPlan
    median_elements = None
    median_elements_log = None

    def _before_plan_step(self, sp):
        if self.median_elements is not None:
            sp.median_elements_override = self.median_elements[self.refinement_steps_done]

    def _after_plan_step(self, sp):
        if self.median_elements_log is not None:
            self.median_elements_log.append((sp.delta.reshape(-1) == sp.md).nonzero().reshape(-1).to(torch.int32))

    def _scale_gradient_elements(self):
        return None if self.median_elements is None else self.median_elements[self.refinement_steps_done]
