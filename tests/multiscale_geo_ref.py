"""Host-side half of tests/test_gpu_warp_geo_groups_contracts.py and tests/test_gpu_multiscale_geometric.py: the geo pair over SCALE GROUPS
(e2e_warp_photo_geo_groups_fwd / _bwd) and ops.warp_photometric_multiscale(geometric=True).  Nothing touches a GPU;
tests/test_multiscale_geo_inputs.py proves what this docstring claims.

Grouped scenes.  A case is (group shape (B/G, H, W), G, S): G scenes warp_geo_ref.scene(B/G, H, W, salt) of one shape with the salts
SALTS[shape][:G], each given intrinsics of its own (warp_geo_ref's K depends on the shape alone), stacked scale-major along the batch: group g
is the batch items g B/G ... (g + 1) B/G - 1, with its own K, T, depth and source depths.  Padding border, mask on, mode MODE[S] (min-reprojection
and auto-masking: every candidate kind).

Shapes, the smallest at which the grouping can go wrong: (1,13,37) is ragged against the 8x32 tile with several tiles both ways; (2,9,33) has two
items per group, one row and one column past a tile, which catches a gate read from the neighbouring group or item.  G in 1..4 (3 is no power
of two), S in 1..2.

The salts are CHOSEN (search(), run once by hand) so that every group scene stays within warp_geo_ref's rules -- at most CAP_EXCLUDED of the
pixels excluded (the search asks for half of that, as the float32 reference moves a little with the CPU's math library) for either gradient, no pixel in a validity band, so every n_{s,g} is decided -- and so that per shape and source the float64
counts n_{s,g} of the four groups are pairwise distinct.  A gated case (G >= 2) sets geo_min_valid to the SMALLEST n_{0,g}: that group of source
0 is closed (the gate is strict) and every other group of source 0 is open.  ZERO is the one case with a group that has no valid projection at
all: its poses carry 100 units of sideways translation, which puts every projection far outside the frame, n = 0 for both sources.

Upstream: G_LOSS[:1 + S G], every slot different.  The float64 reference of group g is warp_geo_ref's composition on that group's scene with
g_loss = (G_LOSS[0] / G, G_LOSS[1 + s G + g] ...): loss_out[0] of the stacked call is the mean of the groups' losses.

ops.warp_photometric_multiscale(geometric=True): op_case(B, S) -- a 16x32 frame with disparities 16x32, 8x16, 4x8, 2x4 -- is the float64
composition tests/disp_pyramid_ref.py -> warp_geo_ref.maps per scale -> the means, differentiated with respect to every target disparity,
every source disparity and every pose.  The bound on the new route is FACTOR x EXISTING_WORST, the largest max|x - r64| / max|r64| that the
EXISTING per-scale route (F.interpolate, ops.depth_from_disp_range, one ops.warp_photometric_window(geometric=True) per scale) showed on the
same cases on the MI355X (profiles/multiscale_geo.txt), the margin profiles/slam_grad_contracts.txt took for two fp32 routes that sum in
different orders."""
import functools

import torch

import disp_pyramid_ref as DP
import warp_contract_ref as R
import warp_geo_ref as G
from warp_contract_ref import F32, F64

GROUP_SHAPES = [(1, 13, 37), (2, 9, 33)]
GROUPS, SOURCES = (1, 2, 3, 4), (1, 2)
PAD, MASK = 1, 1
MODE = {1: (1, 1, 1), 2: (2, 1, 1)}
SALTS = {(1, 13, 37): (2, 3, 4, 5), (2, 9, 33): (0, 1, 3, 5)}
CASES = [(shape, groups, S) for shape in GROUP_SHAPES for groups in GROUPS for S in SOURCES]
GATED = [c for c in CASES if c[1] >= 2]
ZERO = ((2, 9, 33), 3, 2)                                   # (shape, G, S); group ZERO_GROUP sees nothing
ZERO_GROUP = 1
G_LOSS = (1.3, 0.7, 1.9, 0.6, 1.1, 0.9, 1.7, 0.8, 1.4)
CAP_EXCLUDED = G.CAP_EXCLUDED


@functools.lru_cache(maxsize=None)
def group_scene(shape, salt, away=False):
    """warp_geo_ref.scene with intrinsics of its own; away: both poses get 100 units of translation along x, so nothing projects into the frame"""
    B, H, W = shape
    s = dict(G.scene(B, H, W, salt))
    s["K"], s["invK"] = R.intrinsics(B, H, W, "MG", salt)
    if away:
        s["T"] = [T.clone() for T in s["T"]]
        for T in s["T"]:
            T[:, 0, 3] += 100.0
    return s


def scenes(shape, groups, zero_group=None):
    return [group_scene(shape, SALTS[shape][g], away=(g == zero_group)) for g in range(groups)]


@functools.lru_cache(maxsize=None)
def _base(shape, salt, away):
    return _base_of(group_scene(shape, salt, away))


def _base_of(s):
    """warp_geo_ref.base_case on a scene of this module's"""
    shape = (s["B"], s["H"], s["W"])
    c = dict(scene=s, shape=shape, pad=PAD, use_mask=MASK, T=s["T"])
    for dt in (F64, F32):
        c[dt] = G.maps(s, PAD, dt, MASK, Ts=c["T"])
    c["photo"], c["geo"], c["src_excluded"] = [], [], []
    B, H, W = shape
    for k in range(2):
        r64, r32 = ({key: c[dt][key][k] for key in ("grid", "m", "synth", "valid", "wd", "id", "c2")} for dt in (F64, F32))
        c["photo"].append(G.photo_kinks(s, r64, r32, PAD, MASK))
        gk = G.geo_kinks(s, r64, r32, PAD)
        c["geo"].append(gk)
        c["src_excluded"].append(G.footprint(r64["grid"], H, W, PAD, gk["sign"] | gk["vband"]))
    return c


@functools.lru_cache(maxsize=None)
def group_case(shape, salt, S, geo_min_valid=0, g_loss=G.G_LOSS, away=False):
    """warp_geo_ref.geo_case on a group scene: the float64 and float32 references, the exclusion sets and the counts of one group"""
    b = _base(shape, salt, away)
    s, mode = b["scene"], MODE[S]
    case = dict(scene=s, shape=shape, pad=PAD, use_mask=MASK, mode=mode, base=b, g_loss=g_loss, geo_min_valid=geo_min_valid, n=b[F64]["n"][:S])
    for dt in (F64, F32):
        case[dt] = G.evaluate(b[dt], s, mode, dt, geo_min_valid, g_loss)
    return G._assemble(case, b, S)


def counts(shape, groups, S, zero_group=None):
    """n[s][g], the float64 references' valid projections"""
    return [[_base(shape, SALTS[shape][g], g == zero_group)[F64]["n"][s] for g in range(groups)] for s in range(S)]


def gate_of(case):
    """geo_min_valid of a gated case: the smallest n_{0,g}"""
    shape, groups, S = case
    return min(counts(shape, groups, S)[0])


def group_g_loss(groups, S, g):
    """the slice call's upstream for group g: g_loss[0] / G, then g_loss[1 + s G + g]"""
    return (G_LOSS[0] / groups,) + tuple(G_LOSS[1 + s * groups + g] for s in range(S))


def stacked(shape, groups, zero_group=None):
    """the G scenes stacked scale-major -> dict(B, H, W, depth, K, invK, T [2], src [2], tgt, dsrc [2], noise)"""
    ss = scenes(shape, groups, zero_group)
    cat = lambda key: torch.cat([s[key] for s in ss])
    out = dict(B=shape[0] * groups, H=shape[1], W=shape[2], depth=cat("depth"), K=cat("K"), invK=cat("invK"), tgt=cat("tgt"), noise=cat("noise"))
    for key in ("T", "src", "dsrc"):
        out[key] = [torch.cat([s[key][k] for s in ss]) for k in range(2)]
    return out


def survey(shape, salt):
    """what the choice of a salt looks at -> (largest excluded fraction over S, valid-band pixels, (n_0, n_1))"""
    worst, vb = 0.0, 0
    for S in SOURCES:
        c = group_case(shape, salt, S)
        worst = max(worst, G.excluded_fraction(c))
        vb += int(c["valid_band"].sum())
    return worst, vb, tuple(_base(shape, salt, False)[F64]["n"])


def search(shape, upto=40):
    """the first four salts whose scenes pass survey() with counts pairwise distinct per source (and the ZERO scene's rules with the second)"""
    got, n0, n1 = [], set(), set()
    for salt in range(upto):
        worst, vb, (a, b) = survey(shape, salt)
        if worst <= CAP_EXCLUDED / 2 and vb == 0 and a not in n0 and b not in n1 and a > 0 and b > 0:
            got.append(salt)
            n0.add(a)
            n1.add(b)
        if len(got) == 4:
            break
    return got


# ---------------------------------------------------------------------------------------------------------------------------------------
# ops.warp_photometric_multiscale(geometric=True)
# ---------------------------------------------------------------------------------------------------------------------------------------
SIZE = (16, 32)
SCALE_SHAPES = ((16, 32), (8, 16), (4, 8), (2, 4))
LIMITS, SCALE = (0.5, 10.0), 1.0                            # disparities rand * 0.35 + 0.12 -> depths between 1 and 3, the range the poses were made for
OP_CASES = [(B, S) for B in (1, 2) for S in (1, 2)]
OP_SALT = {1: 0, 2: 64}                                     # chosen (op_search) so that no pixel of any scale has to be excluded: the sums are whole
OP_MIN_VALID = 16                                           # low enough that every gate is open (tests/test_multiscale_geo_inputs.py)
OP_WEIGHTS = (0.5, 0.8)                                     # what is differentiated: loss + sum_s OP_WEIGHTS[s] geometric[s]
FACTOR = 10.0
EXISTING_WORST = 6.00e-06           # the largest max|x - r64| / max|r64| of the existing route over OP_CASES and quantities, measured on an MI355X:
                                    # the finest disparity of the first source, B = 2 (profiles/multiscale_geo.txt)


@functools.lru_cache(maxsize=None)
def op_scene(B, salt=None):
    """warp_geo_ref.scene at 16x32 with frames whose values cannot meet (multiscale_loss_ref.scene) and one disparity pyramid for the target
    and for each source: disps {k: (B,1,h,w)}, dsrc_disps [2] of the same"""
    salt = OP_SALT[B] if salt is None else salt
    s = dict(G.scene(B, *SIZE, salt))
    s["src"] = [t * 0.4 for t in s["src"]]
    s["tgt"] = s["tgt"] * 0.4 + 0.6
    g = R.gen("MGO", B, salt)
    draw = lambda: {k: torch.rand(B, 1, h, w, generator=g) * 0.35 + 0.12 for k, (h, w) in enumerate(SCALE_SHAPES)}
    s["disps"], s["dsrc_disps"] = draw(), [draw(), draw()]
    return s


@functools.lru_cache(maxsize=None)
def op_case(B, S, salt=None):
    """float64 -> dict(scene, loss = mean_g photometric_g, photo_per_scale (G,), geometric (S,) = mean_g G_{s,g}, per_scale (G,S), count (G,S),
    the gradients of loss + sum_s OP_WEIGHTS[s] geometric[s]: g_disp {k}, g_dsrc [s] {k}, g_T [s], and excluded: the number of pixels, over
    all scales, that warp_geo_ref's rules would exclude)"""
    s = op_scene(B, salt)
    nG, mode = len(SCALE_SHAPES), MODE[S]
    depth = DP.pyramid_depth(s["disps"], SIZE, *LIMITS, SCALE)                        # (G,B,1,H,W) float64
    dsd = [DP.pyramid_depth(p, SIZE, *LIMITS, SCALE) for p in s["dsrc_disps"]]
    gl = (1.0 / nG,) + tuple(w / nG for w in OP_WEIGHTS[:S])
    out = dict(scene=s, g_T=[torch.zeros(B, 4, 4, dtype=F64) for _ in range(S)], excluded=0)
    photo, per_scale, count, g_depth, g_ds = [], [], [], [], [[] for _ in range(S)]
    for k in range(nG):
        sc = {**s, "depth": depth[k][:, 0], "dsrc": [dsd[j][k][:, 0] for j in range(2)]}
        b = _base_of(sc)
        case = dict(scene=sc, shape=(B, *SIZE), pad=PAD, use_mask=MASK, mode=mode, base=b)
        for dt in (F64, F32):
            case[dt] = G.evaluate(b[dt], sc, mode, dt, OP_MIN_VALID, gl)
        G._assemble(case, b, S)
        out["excluded"] += int(case["grad_excluded"].sum()) + sum(int(x.sum()) for x in case["src_excluded"]) + int(case["valid_band"].sum())
        ev = case[F64]
        photo.append(ev["loss"])
        per_scale.append(torch.stack(ev["G"]))
        count.append(b[F64]["n"][:S])
        g_depth.append(ev["g_depth"].view(B, 1, *SIZE))
        for j in range(S):
            g_ds[j].append(ev["g_ds"][j].view(B, 1, *SIZE))
            out["g_T"][j] += ev["g_T"][j]
    out["photo_per_scale"], out["per_scale"], out["count"] = torch.stack(photo), torch.stack(per_scale), torch.tensor(count)
    out["loss"], out["geometric"] = out["photo_per_scale"].mean(), out["per_scale"].mean(0)
    out["g_disp"] = DP.pyramid_depth_bwd(torch.stack(g_depth), s["disps"], SIZE, *LIMITS, SCALE)
    out["g_dsrc"] = [DP.pyramid_depth_bwd(torch.stack(g_ds[j]), s["dsrc_disps"][j], SIZE, *LIMITS, SCALE) for j in range(S)]
    return out


def op_search(B, upto=200):
    """the first salt that leaves nothing to exclude on any scale with two sources (which holds the one-source set) and opens every gate"""
    for salt in range(upto):
        c = op_case(B, 2, salt)
        if c["excluded"] == 0 and int(c["count"].min()) > OP_MIN_VALID:
            return salt
    return None


