"""Host-only: every entry point that include/e2eslam.h declares and csrc/depth_ops.hip, aux_losses.hip or nn_misc.hip implements is
called by one of the two contract modules (tests/test_gpu_depth_aux_contracts.py, tests/test_gpu_nn_misc_contracts.py); the same for
csrc/icp.hip and tests/test_gpu_icp_contracts.py, for csrc/warp_photo.hip and tests/test_gpu_warp_photo_contracts.py, for
csrc/warp_photo_fused.hip and tests/test_gpu_lossgrad_contracts.py, for the forward
entry points of csrc/conv.hip and tests/test_gpu_conv_fwd_contracts.py, and for the map side -- csrc/pointfusion.hip (but
e2e_pf_active_subsample_dev, which the ICP gate owns) and csrc/knn.hip -- and tests/test_gpu_map_contracts.py.  The adjoint side of
the SLAM chain has the same gates: csrc/pose_grad.hip and tests/test_gpu_pose_grad_contracts.py, csrc/pointfusion_grad.hip with
csrc/normal_maps_grad.hip and tests/test_gpu_map_grad_contracts.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "end-to-end-self-supervised-slam_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_every_entry_point_of_the_three_files_has_a_contract_case():
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set()
    for name in ("depth_ops.hip", "aux_losses.hip", "nn_misc.hip"):
        implemented |= set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, name), re.M))
    names = declared & implemented
    assert len(names) >= 37, sorted(names)                                # 15 + 11 + 11 at the time of writing: the greps still find them
    assert implemented <= declared, sorted(implemented - declared)
    tests = _read(ROOT, "tests", "test_gpu_depth_aux_contracts.py") + _read(ROOT, "tests", "test_gpu_nn_misc_contracts.py")
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", tests))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


def test_every_entry_point_of_the_icp_file_has_a_contract_case():
    """csrc/icp.hip's entry points, and e2e_pf_active_subsample_dev of csrc/pointfusion.hip (the odometry's target selection), are all
    called by tests/test_gpu_icp_contracts.py."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "icp.hip"), re.M))
    names = (declared & implemented) | {"e2e_pf_active_subsample_dev"}
    assert len(names) >= 8, sorted(names)                                 # 7 + 1 at the time of writing: the greps still find them
    assert implemented <= declared, sorted(implemented - declared)
    assert "e2e_pf_active_subsample_dev" in declared
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_icp_contracts.py")))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


def test_every_entry_point_of_the_warp_photo_file_has_a_contract_case():
    """csrc/warp_photo.hip's entry points (view synthesis, photometric loss, the fused pair and its workspace query) are all called by
    tests/test_gpu_warp_photo_contracts.py."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "warp_photo.hip"), re.M))
    names = declared & implemented
    assert len(names) >= 12, sorted(names)                                # 12 at the time of writing: the greps still find them
    assert implemented <= declared, sorted(implemented - declared)
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_warp_photo_contracts.py")))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


def test_every_entry_point_of_the_fused_lossgrad_file_has_a_contract_case():
    """csrc/warp_photo_fused.hip's entry points (the one-launch loss and gradient, its host-geometry and chained forms, the flush and the
    workspace query) are all called by tests/test_gpu_lossgrad_contracts.py."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "warp_photo_fused.hip"), re.M))
    names = declared & implemented
    assert len(names) >= 5, sorted(names)                                 # 5 at the time of writing: the greps still find them
    assert implemented <= declared, sorted(implemented - declared)
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_lossgrad_contracts.py")))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


CONV_FWD_ENTRY_POINTS = {
    "e2e_conv2d_fwd", "e2e_conv2d_fwd_tuned", "e2e_head_fwd", "e2e_conv_weight_layouts", "e2e_conv_weight_layouts_batched",
    "e2e_conv2d_splitk_workspace_floats", "e2e_conv_tuned_workspace_floats", "e2e_conv_gemm_choice", "e2e_conv_workspace_flag_floats",
    "e2e_conv_streamk_error_index",
}


def test_every_forward_entry_point_of_the_conv_file_has_a_contract_case():
    """The forward side of csrc/conv.hip (the backward side has tests/test_gpu_conv_bwd_contracts.py, e2e_conv2d_fwd_entry_pair its own
    module): declared, implemented and called by tests/test_gpu_conv_fwd_contracts.py."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "conv.hip"), re.M))
    assert len(CONV_FWD_ENTRY_POINTS) == 10
    assert CONV_FWD_ENTRY_POINTS <= declared, sorted(CONV_FWD_ENTRY_POINTS - declared)
    assert CONV_FWD_ENTRY_POINTS <= implemented, sorted(CONV_FWD_ENTRY_POINTS - implemented)
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_conv_fwd_contracts.py")))
    assert not CONV_FWD_ENTRY_POINTS - called, f"no contract case calls {sorted(CONV_FWD_ENTRY_POINTS - called)}"


def test_every_entry_point_of_the_pointfusion_file_has_a_contract_case():
    """csrc/pointfusion.hip's entry points (vertex / normal maps and their depth gradient, transform_points, the workspace query, the
    association, the tables, the fusion and the append in their host-count and resident forms, the aggregation append) are all called
    by tests/test_gpu_map_contracts.py; e2e_pf_active_subsample_dev belongs to the ICP gate above."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "pointfusion.hip"), re.M))
    assert "e2e_pf_active_subsample_dev" in implemented
    names = (declared & implemented) - {"e2e_pf_active_subsample_dev"}
    assert len(names) >= 10, sorted(names)                                # 10 at the time of writing: the greps still find them
    assert implemented <= declared, sorted(implemented - declared)
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_map_contracts.py")))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


def test_every_entry_point_of_the_knn_file_has_a_contract_case():
    """csrc/knn.hip's entry points (the one-shot search and its workspace query, the index over a host-counted and over a resident
    reference set, its image, warm-started and resolution-parameterised queries with their size queries, the two backward halves) are
    all called by tests/test_gpu_map_contracts.py.  The file implements and the header declares FOURTEEN e2e_knn1_* entry points (the
    issue that asked for this gate counted sixteen); the gate asks for all that exist, at least those fourteen."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "knn.hip"), re.M))
    names = declared & implemented
    assert len(names) >= 14, sorted(names)                                # 14 at the time of writing: the greps still find them
    assert names == {n for n in declared if n.startswith("e2e_knn1_")}, "an e2e_knn1_* entry point that csrc/knn.hip does not implement"
    assert implemented <= declared, sorted(implemented - declared)
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_map_contracts.py")))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


def test_every_entry_point_of_the_pose_grad_file_has_a_contract_case():
    """csrc/pose_grad.hip's entry points (the adjoint of the ICP normal equations with respect to the sources and to the targets, the
    pose gradients of transform_points and Project3D, the three workspace queries) are all called by
    tests/test_gpu_pose_grad_contracts.py."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, "pose_grad.hip"), re.M))
    names = declared & implemented
    assert len(names) >= 7, sorted(names)                                 # 7 at the time of writing: the greps still find them
    assert implemented <= declared, sorted(implemented - declared)
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_pose_grad_contracts.py")))
    assert not names - called, f"no contract case calls {sorted(names - called)}"


def test_every_entry_point_of_the_map_grad_files_has_a_contract_case():
    """csrc/pointfusion_grad.hip's entry points (the step's tape and its size, the step's adjoint, the depth gradient of the fusion
    confidence, the normals' tape, its size and the normals' adjoint) and csrc/normal_maps_grad.hip's one (the adjoint of the normal
    map) are all called by tests/test_gpu_map_grad_contracts.py."""
    declared = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(ROOT, "include", "e2eslam.h"), re.M))
    called = set(re.findall(r"[\"'.](e2e_\w+)[\"'(]", _read(ROOT, "tests", "test_gpu_map_grad_contracts.py")))
    for name, least in (("pointfusion_grad.hip", 7), ("normal_maps_grad.hip", 1)):
        implemented = set(re.findall(r"^(?:int|int64_t|long long)\s+(e2e_\w+)\s*\(", _read(CSRC, name), re.M))
        names = declared & implemented
        assert len(names) >= least, (name, sorted(names))                 # 7 + 1 at the time of writing: the greps still find them
        assert implemented <= declared, (name, sorted(implemented - declared))
        assert not names - called, f"no contract case calls {sorted(names - called)} of {name}"
