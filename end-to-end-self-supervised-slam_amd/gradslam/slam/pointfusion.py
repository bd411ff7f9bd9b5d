import torch

from ..structures import Pointclouds
from .icpslam import ICPSLAM


def frame_as_pointcloud(frame, alpha_grad=False, pose_grad=False, normal_grad=False):
    """All valid-depth pixels of a 1-frame RGBDImages as a Pointclouds (row-major order), differentiable wrt
    depth through the global vertex map (alpha_grad: and through the confidences in features_list; pose_grad: and wrt a pose that
    requires grad; normal_grad: the normals are attached too).  This is what PointFusion.step returns for an EMPTY map (online_adaption.py:461-469) and what ICPSLAM's
    aggregation appends."""
    B, L, H, W = frame.shape
    if L != 1:
        raise ValueError(f"Expected a frame with sequence length 1. Got {L}.")
    if alpha_grad or pose_grad or normal_grad:
        m = frame._maps(alpha_grad=alpha_grad, pose_grad=pose_grad, normal_grad=normal_grad)
    else:
        m = frame._maps()
    pts, nrm, col, feat = [], [], [], []
    for b in range(B):
        keep = m["valid"][b, 0, ..., 0] if m["valid"].dim() == 5 else m["valid"][b, 0]
        pts.append(m["Vg"][b, 0][keep])
        nrm.append(m["ng"][b, 0][keep])
        col.append(frame.rgb_image[b, 0][keep])
        feat.append(m["alpha"][b, 0][keep].reshape(-1, 1))
    return Pointclouds(pts, nrm, col, feat, device=frame.device)


class PointFusion(ICPSLAM):
    """PointFusion map update (gradslam PointFusion = ICPSLAM + update_map_fusion).

    The global map lives in a resident e2ehip.FusionMap (capacity-sized HBM arrays, appended in place); the
    returned Pointclouds exposes zero-copy views of its live rows.  `map_capacity` points are reserved on
    first use (default: 64 frames' worth).

    map_gradient (default False): the map update is differentiable (FusionMap.step_differentiable; the rule is stated in
    include/e2eslam.h).  Points, colours and confidences of the returned cloud then carry a gradient to the live frame's depth and
    rgb and, through the incoming cloud's lists, to the frames fused before; they are tensors of their own instead of views.  The
    association, the poses and the intrinsics are constants, the normals carry no gradient.  Taken only while grad mode is on and the
    live depth, the live rgb or one of the incoming lists requires grad; otherwise, and with the switch off, the step is the plain one.

    chain_gradient (default False): the two halves are one graph, as in the reference (train_depth.py:360-397).  The localisation takes
    the map (the incoming cloud's points and normals lists) and the previous frame's pose as variables, and the map step takes the live
    pose as one (the association still sees a constant), so a pose carries the gradient to the depth of every earlier frame through
    whatever graph map_gradient gave the map, and the fused cloud moves with the estimated poses.  Values do not change.

    normal_gradient (default False): the normals of the returned cloud carry a gradient as well: to the live depth through the
    finite-difference normal map (e2e_normal_maps_bwd) and, in a differentiable map step, through the confidence-weighted fusion to the
    incoming cloud's normals and confidences (e2e_pf_fuse_normals_bwd).  Something has to read that graph: with chain_gradient the
    point-to-plane residual of every later localisation does; with map_gradient as well it reaches the fused rows, otherwise only the
    rows of the first frame.  Values do not change."""

    def __init__(self, *, odom="gradicp", dist_th=0.05, angle_th=20, sigma=0.6, dsratio=4, numiters=20, damp=1e-8, dist_thresh=None,
                 lambda_max=2.0, B=1.0, B2=1.0, nu=200.0, device=None, map_capacity=None, map_gradient=False, chain_gradient=False,
                 normal_gradient=False):
        super().__init__(odom=odom, dsratio=dsratio, numiters=numiters, damp=damp, dist_thresh=dist_thresh, lambda_max=lambda_max,
                         B=B, B2=B2, nu=nu, device=device)
        self.chain_gradient = bool(chain_gradient)
        if not isinstance(dist_th, (float, int)):
            raise TypeError(f"Distance threshold must be of type float or int; but was of type {type(dist_th)}.")
        if not isinstance(angle_th, (float, int)):
            raise TypeError(f"Angle threshold must be of type float or int; but was of type {type(angle_th)}.")
        if dist_th < 0:
            raise ValueError(f"Distance threshold must be non-negative: {dist_th}")
        if not 0 <= angle_th <= 90:
            raise ValueError(f"Angle threshold must be in [0, 90]: {angle_th}")
        self.dist_th, self.angle_th, self.sigma = dist_th, angle_th, sigma
        self.map_capacity = map_capacity
        self.map_gradient = bool(map_gradient)
        self.normal_gradient = bool(normal_gradient)

    def _map(self, pointclouds, live_frame, inplace=False):
        if len(pointclouds) > 1 or live_frame.shape[0] != 1:
            raise NotImplementedError("batch size 1 only (OPTIMIZATION.batch_size, configs/config.yaml:60)")
        _, _, H, W = live_frame.shape
        rgb, depth = live_frame.rgb_image[0, 0], live_frame.depth_image[0, 0, ..., 0]
        normals = self.normal_gradient and torch.is_grad_enabled()
        lists = [l[0] for l in (pointclouds.points_list, pointclouds.colors_list, pointclouds.features_list) +
                 ((pointclouds.normals_list,) if normals else ()) if l]
        chain = self.chain_gradient and torch.is_grad_enabled() and live_frame.poses.requires_grad       # the live pose is a variable
        with_graph = self.map_gradient and torch.is_grad_enabled() and (chain or any(t.requires_grad for t in [depth, rgb] + lists))
        if not pointclouds.has_points:
            # empty map: nothing to associate with -> the frame's valid pixels, still attached to the autograd
            # graph of the depth (the 3-D loss differentiates through this: online_adaption.py:461-469,638-645)
            attach = {"normal_grad": True} if normals and (chain or depth.requires_grad) else {}
            out = frame_as_pointcloud(live_frame, alpha_grad=with_graph, pose_grad=chain, **attach)
            return out
        fm = self._resident_map(pointclouds, live_frame)      # adopts an externally built cloud once
        if with_graph:
            P, Nn, C, cc = fm.step_differentiable(rgb, depth, live_frame.intrinsics[0, 0], live_frame.poses[0, 0],
                                                  prev=(pointclouds.points_list[0], pointclouds.colors_list[0], pointclouds.features_list[0]) +
                                                       ((pointclouds.normals_list[0],) if normals else ()),
                                                  pose_gradient=chain, **({"normal_gradient": True} if normals else {}))
            out = Pointclouds([P], [Nn], [C], [cc.reshape(-1, 1)], device=live_frame.device)
            out._fusion_maps = fm
            return out
        fm.step(live_frame.rgb_image[0, 0].detach(), live_frame.depth_image[0, 0, ..., 0].detach(),
                live_frame.intrinsics[0, 0], live_frame.poses[0, 0])
        P, Nn, C, cc = fm.live()
        out = Pointclouds([P], [Nn], [C], [cc.reshape(-1, 1)], device=live_frame.device)
        out._fusion_maps = fm
        return out
