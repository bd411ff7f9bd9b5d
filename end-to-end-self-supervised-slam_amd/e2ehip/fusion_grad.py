"""The differentiable form of the PointFusion map step (FusionMap.step_differentiable): the kernels of FusionMap.step plus one tape
launch in the forward, csrc/pointfusion_grad.hip in the backward.  The differentiation rule is stated in include/e2eslam.h: the
association, the validity mask, the append order, the pose (unless pose_gradient) and the intrinsics are constants, the normals carry no
gradient unless normal_gradient (then e2e_pf_fuse_normals_tape / e2e_pf_fuse_normals_bwd run as well).

Opt-in (gradslam.slam.PointFusion(map_gradient=True)); FusionMap.step, step_resident and the captured driver do not come here."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from .ops import vertex_normal_maps


class _FuseStep(torch.autograd.Function):
    """(Vg, rgb, alpha of the live frame; points, colors, ccounts of the map before the step) -> the same three of the map after it.
    The resident map `fm` holds the values of the previous map (the three tensors are its autograd handles) and is advanced in place;
    the outputs are copies of its live rows, so a later step cannot change what autograd or the caller holds.
    With the normals' gradient two more inputs follow (Ng of the live frame, the normals of the map before the step) and the normals
    after the step are a fourth output; without them this is the three-output function, launch for launch."""

    @staticmethod
    def forward(ctx, Vg, rgb, alpha, prev_points, prev_colors, prev_ccounts, fm, maps, depth, K, pose, Ng=None, prev_normals=None):
        M0, H, W = fm.M, fm.H, fm.W
        with_normals = Ng is not None
        shapes = [("prev_points", prev_points, (M0, 3)), ("prev_colors", prev_colors, (M0, 3)), ("prev_ccounts", prev_ccounts, (M0,))]
        if with_normals:
            shapes.append(("prev_normals", prev_normals, (M0, 3)))
        for n, t, shape in shapes:
            if tuple(t.shape) != shape:
                raise ValueError(f"{n}: expected {shape} (the resident map has {M0} rows), got {tuple(t.shape)}")
        rgb, depth = L.dev(rgb, "rgb").contiguous(), L.dev(depth, "depth").contiguous()
        tape = torch.empty(L.query("e2e_pf_fuse_tape_bytes", H, W), device=fm.device, dtype=torch.uint8)
        fm.associate(maps, K, pose)
        L.call("e2e_pf_fuse_tape", map_points=L.ptr(fm.points), map_colors=L.ptr(fm.colors), map_ccounts=L.ptr(fm.ccounts), M=M0,
               map_capacity=fm.cap, depth=L.ptr(depth), workspace=L.ptr(fm.ws), H=H, W=W, tape=L.ptr(tape), stream=L.stream())
        if with_normals:
            ntape = torch.empty(L.query("e2e_pf_fuse_normals_tape_bytes", H, W), device=fm.device, dtype=torch.uint8)
            L.call("e2e_pf_fuse_normals_tape", tape=L.ptr(tape), map_normals=L.ptr(fm.normals), M=M0, ntape=L.ptr(ntape), H=H, W=W,
                   stream=L.stream())
        fm.fuse_append(maps, rgb, depth)
        P, C, cc = fm.points[:fm.M].clone(), fm.colors[:fm.M].clone(), fm.ccounts[:fm.M].clone()
        ctx.with_normals = with_normals
        ctx.sizes = (M0, fm.M, H, W)
        ctx.set_materialize_grads(False)
        if not with_normals:
            ctx.save_for_backward(tape, maps["Vg"], rgb, maps["alpha"], cc)
            return P, C, cc
        ctx.save_for_backward(tape, maps["Vg"], rgb, maps["alpha"], cc, ntape, maps["ng"])
        return P, C, cc, fm.normals[:fm.M].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, gP, gC, gcc, gN=None):
        tape, Vg, rgb, alpha, cc = ctx.saved_tensors[:5]
        M0, M1, H, W = ctx.sizes
        n_in = 13 if ctx.with_normals else 11
        if gP is None and gC is None and gcc is None and gN is None:
            return (None,) * n_in
        f = dict(device=Vg.device, dtype=torch.float32)
        need = ctx.needs_input_grad
        shapes = ((H, W, 3), (H, W, 3), (H, W), (M0, 3), (M0, 3), (M0,))
        out = [None] * 6
        ran = False
        if (gP is not None or gC is not None or gcc is not None) and any(need[:6]):
            out = [torch.empty(shape, **f) if n else None for n, shape in zip(need[:6], shapes)]
            gP, gC, gcc = (g.contiguous() if g is not None else None for g in (gP, gC, gcc))
            L.call("e2e_pf_fuse_bwd", tape=L.ptr(tape), Vg=L.ptr(Vg), rgb=L.ptr(rgb), alpha=L.ptr(alpha), g_points=L.ptr(gP), g_colors=L.ptr(gC),
                   g_ccounts=L.ptr(gcc), ccounts_after=L.ptr(cc), M_before=M0, M_after=M1, g_Vg=L.ptr(out[0]), g_rgb=L.ptr(out[1]),
                   g_alpha=L.ptr(out[2]), g_prev_points=L.ptr(out[3]), g_prev_colors=L.ptr(out[4]), g_prev_ccounts=L.ptr(out[5]), H=H, W=W,
                   stream=L.stream())
            ran = True
        if not ctx.with_normals:
            return (*out, None, None, None, None, None)
        g_Ng = g_prevN = None
        if gN is not None and (need[2] or need[5] or need[11] or need[12]):
            ntape, Ng = ctx.saved_tensors[5:]
            if not ran:                                     # the normals' share is all there is of these two
                out[2] = torch.empty(shapes[2], **f) if need[2] else None
                out[5] = torch.empty(shapes[5], **f) if need[5] else None
            g_Ng = torch.empty(H, W, 3, **f) if need[11] else None
            g_prevN = torch.empty(M0, 3, **f) if need[12] else None
            L.call("e2e_pf_fuse_normals_bwd", tape=L.ptr(tape), ntape=L.ptr(ntape), Ng=L.ptr(Ng), alpha=L.ptr(alpha), g_normals=L.ptr(gN.contiguous()),
                   ccounts_after=L.ptr(cc), M_before=M0, M_after=M1, g_Ng=L.ptr(g_Ng), g_prev_normals=L.ptr(g_prevN), g_alpha=L.ptr(out[2]),
                   g_prev_ccounts=L.ptr(out[5]), accumulate=int(ran), H=H, W=W, stream=L.stream())
        return (*out, None, None, None, None, None, g_Ng, g_prevN)


def step_differentiable(self, rgb, depth, K, pose, prev=None, pose_gradient=False, normal_gradient=False):
    """FusionMap.step_differentiable (self: the FusionMap): step() with a graph.  rgb (H,W,3), depth (H,W), K / pose (4,4);
    prev = (points (M,3), colors (M,3), ccounts (M,) or (M,1)): the tensors that stand for the map before the step in the caller's
    graph (their VALUES are the resident rows; None: the map is a constant).  -> points, normals, colors (M',3), ccounts (M'): tensors of
    their own, copied out of the live rows; forward values and the resident state are those of step(), bit for bit.  points / colors /
    ccounts carry the gradient to depth, rgb and prev; the normals carry none.  pose_gradient (the chain gradient): the points also
    carry the gradient to a pose that requires grad, through Vg = R V + t; off, such a pose is a constant, as it is for the association
    either way.
    normal_gradient: prev takes a fourth tensor, the normals (M,3) of the map before the step, and the returned normals are an output
    of the same autograd function: they carry the gradient to the depth (through ng and alpha), to prev's normals and ccounts and,
    with pose_gradient, to the rotation of the pose.  Off: today's launches, and normals without a graph."""
    M0 = self.M
    pose_var = pose if pose_gradient else pose.detach()
    pose = pose.detach()
    if prev is None:
        prev = (self.points[:M0], self.colors[:M0], self.ccounts[:M0]) + ((self.normals[:M0],) if normal_gradient else ())
    if len(prev) != (4 if normal_gradient else 3):
        raise ValueError(f"prev: expected {4 if normal_gradient else 3} tensors (points, colors, ccounts"
                         f"{', normals' if normal_gradient else ''}), got {len(prev)}")
    prev_points, prev_colors, prev_ccounts = prev[:3]
    maps = vertex_normal_maps(depth.reshape(1, self.H, self.W), K.reshape(1, 4, 4), pose_var.reshape(1, 4, 4), self.sigma, alpha_grad=True,
                              normal_grad=normal_gradient)
    detached = {k: v.detach() for k, v in maps.items()}
    if normal_gradient:
        P, C, cc, N = _FuseStep.apply(maps["Vg"][0], rgb, maps["alpha"][0], prev_points, prev_colors, prev_ccounts.reshape(-1), self,
                                      detached, depth.detach(), K, pose, maps["ng"][0], prev[3])
        return P, N, C, cc
    P, C, cc = _FuseStep.apply(maps["Vg"][0], rgb, maps["alpha"][0], prev_points, prev_colors, prev_ccounts.reshape(-1), self, detached,
                               depth.detach(), K, pose)
    return P, self.normals[:self.M].clone(), C, cc
