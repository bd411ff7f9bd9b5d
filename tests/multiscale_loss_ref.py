"""Host-side half of tests/test_gpu_multiscale_loss.py: monodepth2's multi-scale image-space loss in float64 -- the reference pyramid of
tests/disp_pyramid_ref.py (every scale's disparity upsampled to the frames' size and converted to depth) feeding, per scale, the composition
of tests/warp_window_ref.py (oracle.warp_loss.backproject -> project -> F.grid_sample -> photometric of the masked images, the candidates and
their first minimum), then the mean over the scales.  Gradients: autograd to each scale's depth and to the poses, the depth gradients carried
on to the disparities by the reference adjoint of the pyramid.  Nothing touches a GPU.

Scenes: 32 x 64, the four scales 32 x 64 .. 4 x 8, K / inv_K / poses / tie noise of warp_window_ref.scene(B, 32, 64, 0), its frames
scaled into disjoint ranges; disparities rand * 0.35 + 0.12, which the limits (0.5, 10.0) turn into depths between 1 and 3, the range those
poses were made for.
Modes: the pair form (1, 0, 0) -- one source, no flags -- and the window form (2, 1, 1) -- two sources, min_reprojection + auto_masking.

Admission (the rule of tests/warp_pose_ref.py): the loss's gradients sum over EVERY pixel, so a case is admitted only if no pixel of any scale
has to be excluded -- each used source's kink set (warp_pose_ref.exclusions) and the near-ties of the selection, dilated by 1
(warp_window_ref.near_ties), are empty on all four scales.  At 4 x 2048 pixels a batch element a random scene has about ten such pixels
(a source index within the band of an integer above all), so every (scale, batch element) draws its disparity from a salt of its own, chosen
on the CPU as the first one that leaves nothing to exclude on that scale in the window form (which holds the pair form's set) with every
band DOUBLED (for B = 2 on the two elements together: the bands are the largest error over the batch) -- the float32 reference's error, hence every band, moves a little with the CPU's math library --;
tests/test_multiscale_loss_inputs.py holds the assembled cases to the rule."""
import functools

import torch

import disp_pyramid_ref as DP
import warp_contract_ref as R
import warp_pose_ref as P
import warp_window_ref as WW
from warp_contract_ref import F32, F64

SIZE = (32, 64)
SHAPES = ((32, 64), (16, 32), (8, 16), (4, 8))
LIMITS, SCALE = (0.5, 10.0), 1.0
PAD, USE_MASK = 1, 1
PAIR, WINDOW = (1, 0, 0), (2, 1, 1)
SCENE_SALT = 0
# the salt of every (scale, batch element)'s disparity draw, chosen on the CPU so that the admission rule holds (module docstring)
DISP_SALT = {1: ((7,), (0,), (63,), (29,)), 2: ((162, 11), (50, 9), (129, 16), (132, 9))}
CASES = [(B, mode) for B in (1, 2) for mode in (PAIR, WINDOW)]
FACTOR = 10                          # the new route may err ten times as much as the existing fp32 route does (profiles/disp_pyramid.txt)
EXISTING_WORST = 5.92e-05            # the largest max|x - r64| / max|r64| of the existing route over CASES and quantities, measured on an MI355X:
                                     # g_T of the first source, B = 2, window form (profiles/disp_pyramid.txt)


def disparity(B, k, b, salt):
    h, w = SHAPES[k]
    return torch.rand(1, 1, h, w, generator=R.gen("multiscale", B, k, b, salt)) * 0.35 + 0.12


@functools.lru_cache(maxsize=None)
def scene(B, disp_salt=None):
    """warp_window_ref.scene's intrinsics, poses and tie noise; frames whose values cannot meet (sources in [0, 0.4], the target in
    [0.6, 1]: the L1 term has no kink); one disparity draw per scale and batch element"""
    s = dict(WW.scene(B, *SIZE, SCENE_SALT))
    s["src"] = [t * 0.4 for t in s["src"]]
    s["tgt"] = s["tgt"] * 0.4 + 0.6
    salts = DISP_SALT[B] if disp_salt is None else disp_salt
    s["disps"] = {k: torch.cat([disparity(B, k, b, salts[k][b]) for b in range(B)]) for k in range(len(SHAPES))}
    return s


def element(s, b):
    """batch element b of a scene as a scene of its own"""
    cut = lambda t: t[b:b + 1]
    return {**s, "B": 1, "K": cut(s["K"]), "invK": cut(s["invK"]), "T": [cut(t) for t in s["T"]], "src": [cut(t) for t in s["src"]],
            "tgt": cut(s["tgt"]), "noise": cut(s["noise"])}


def scale_eval(s, depth, mode):
    """one scale: the scene with this scale's full-resolution depth (B,1,H,W) float64 as the target depth through warp_window_ref.maps /
    evaluate in float64 and float32 -> (the float64 evaluation, the pixels (B,H,W) the admission rule would exclude)"""
    r = {}
    for dt, d in ((F64, depth), (F32, depth.float())):
        sc = {**s, "depth": d[:, 0]}
        base = WW.maps(sc, PAD, USE_MASK, dt)
        r[dt] = (base, WW.evaluate(base, sc, mode, dt))
    ev = r[F64][1]
    excluded = torch.zeros(s["B"], *SIZE, dtype=torch.bool)
    for j in range(mode[0]):
        r64, r32 = ({key: r[dt][0][key][j] for key in ("grid", "m", "synth", "valid")} for dt in (F64, F32))
        excluded |= P.exclusions(s, r64, r32, PAD, USE_MASK)
    near, _ = WW.near_ties(ev["cands"], r[F32][1]["cands"].double())
    return ev, excluded | R.dilate(near, 1)


@functools.lru_cache(maxsize=None)
def case(B, mode):
    """-> dict(scene, loss, per_scale (S,), g_disp {k: (B,1,h,w)}, g_T [source] (B,4,4): of the mean over the scales, excluded: the number of
    pixels, over all scales, that the admission rule would exclude)"""
    s = scene(B)
    depth = DP.pyramid_depth(s["disps"], SIZE, *LIMITS, SCALE)                        # (4,B,1,H,W) float64
    out = dict(scene=s, mode=mode, g_T=[torch.zeros(B, 4, 4, dtype=F64) for _ in range(mode[0])], excluded=0)
    per_scale, g_depth = [], []
    for k in range(len(SHAPES)):
        ev, excluded = scale_eval(s, depth[k], mode)
        per_scale.append(ev["loss"])
        g_depth.append(ev["g_depth"].view(B, 1, *SIZE) / len(SHAPES))
        for j in range(mode[0]):
            out["g_T"][j] += ev["g_T"][j] / len(SHAPES)
        out["excluded"] += int(excluded.sum())
    out["per_scale"] = torch.stack(per_scale)
    out["loss"] = out["per_scale"].mean()
    out["g_disp"] = DP.pyramid_depth_bwd(torch.stack(g_depth), s["disps"], SIZE, *LIMITS, SCALE)
    return out
