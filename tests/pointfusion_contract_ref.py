"""Host-side half of tests/test_gpu_map_contracts.py: a float64 (numpy) restatement of the PointFusion map step and of the RGB-D
unprojection, written from the semantics stated in oracle/pointfusion.py's docstrings and SURVEY.md Appendix A, in the NATURAL order of
the mathematics (matrix inverse, matrix products, u = fx x'/z' + cx, numpy's cross / norm) -- not in the order of the fp32 oracle or of
csrc/pointfusion.hip.  It is the comparand for the payloads, and the judge of which table rows a comparison may skip.  Nothing here
touches a GPU: tests/test_pointfusion_contract_ref.py proves on the CPU that every case skips what it may and contains what it claims.

MARGINS AND DECIDABILITY.  The index tables are discrete: a float64 reference and an fp32 evaluation can only be asked to agree on a
decision whose margin exceeds what fp32 rounding can move.  With every decision the reference returns its margin and the bound below;
a decision is DECIDABLE if margin > bound, or if it is EXACT: every intermediate value of the chain that feeds it is representable in
fp32 (dyadic inputs), in the natural order and in the order the oracle's docstring states, so that each IEEE fp32 operation returns the
true value and fp32 and float64 coincide bit for bit -- then even margin 0 (u = k + 0.5, z' = 0) is specified.  An exact tie between two
contenders of a pixel is decidable when the two map rows are bit-identical inputs (same point, same confidence: the same key whatever
the arithmetic) -- the smallest index wins.

Bounds (u32 = 2^-24 = half an fp32 ulp of 1; "a few ulp" = 8 u32 of the magnitudes that enter):
  camera coordinates  q = R^T (p - t):  dq = 8 u32 (max|p_i| + max|t_i|)                (three products, three sums, the inverse's -R^T t)
  front test z' > 0:                    dq
  pixel coordinate u = fx x'/z' + cx:   du = |fx| dq (1 + |x'/z'|) / |z'| + 8 u32 (|u| + |cx|)      (propagated dq + the chain's own ulps)
     -- the bound of the four window tests (u against -1e-3 and W - 0.999, whose fp32 roundings, 1e-10 and 4 u32 W, are inside it)
        and of the rounding test (u against the nearest half-integer)
  distance |Vg - p| < dist_th:          dd = sqrt(3) 8 u32 (max(|p_i|, |Vg_i|) + max|t_i|) + 4 u32 dist
  squared distance (the tie-break):     2 dist dd + dd^2
  normal of a pixel:                    dn = 4 dV (|dW V| + |dH V|) / |cross| + 8 u32,  dV = 8 u32 max|V_i| over the pixel and its two
                                        forward neighbours (cancellation in the differences, then the cross product's two terms)
  dot product ng . nm > dot_th:         dn |nm| + 8 u32
  confidence (1/(c + 1e-20), two roundings): relative gap in c above 8 u32, or bit-equal c

alpha = exp(-|V|^2 / (2 sigma^2 + 1e-7)) is a STORED fp32 quantity: the map's ccounts are fp32, and beyond |V| ~ 8.6 m the value is below
the smallest fp32 number, so the stored confidence is exactly 0 and the fuse step's where(c + a == 0, 1, c + a) branch is reachable.  The
reference therefore fuses with alpha rounded to fp32 (`alpha32`); it refuses (assert) depths whose alpha would be an fp32 subnormal,
because whether a subnormal is kept or flushed is a property of the exp implementation, not of the map step."""
import functools
import math

import numpy as np

F64, F32 = np.float64, np.float32
U32 = 2.0 ** -24
FEW = 8.0 * U32
DIST_TH = float(F32(0.05))                                   # the ABI takes floats: the thresholds are the fp32 values
DOT_TH = float(F32(math.cos(20.0 * math.pi / 180.0)))
SIGMA = 0.6
ALPHA_DEN = 2.0 * SIGMA ** 2 + 1e-7
FACTOR = 4.0                                                 # bound = FACTOR x the fp32 oracle's own error (summation order, contraction)


def ulp32(x):
    return float(np.spacing(F32(abs(float(x)))))


def bound(err_oracle, top):
    """the bound on max|gpu - float64| of one quantity: FACTOR x the fp32 oracle's largest error against the same float64 reference on the
    same inputs, never below 2 ulp of the quantity's largest magnitude"""
    return max(FACTOR * float(err_oracle), 2.0 * ulp32(top))


def _exact32(*arrays):
    """elementwise: every value is an fp32 number (so the fp32 operation that produces it is exact)"""
    ok = True
    for a in arrays:
        a = np.asarray(a, F64)
        with np.errstate(over="ignore", invalid="ignore"):
            ok = ok & (a.astype(F32).astype(F64) == a)
    return ok


# ---------------------------------------------------------------------------------------------------------------------------------------
# RGBDImages maps, batched: depth (B,H,W), K (B,4,4), pose (B,4,4) camera-to-world
# ---------------------------------------------------------------------------------------------------------------------------------------
def frame_maps(depth, K, pose, alpha_den=ALPHA_DEN):
    depth, K, pose = np.asarray(depth, F64), np.asarray(K, F64), np.asarray(pose, F64)
    B, H, W = depth.shape
    hs, ws = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    pix = np.stack([ws, hs, np.ones_like(ws)], -1)                              # (H,W,3) homogeneous pixel
    valid = depth != 0
    V, n, Vg, ng, rays = (np.zeros((B, H, W, 3)) for _ in range(5))
    dn = np.zeros((B, H, W))                                                    # the bound on |n32 - n| of every pixel
    for b in range(B):
        rays[b] = pix @ np.linalg.inv(K[b, :3, :3]).T
        V[b] = rays[b] * depth[b][..., None]                                    # 0 where depth is 0
        dh, dv = np.zeros((H, W, 3)), np.zeros((H, W, 3))
        dh[:, :-1] = V[b][:, 1:] - V[b][:, :-1]
        dv[:-1] = V[b][1:] - V[b][:-1]
        c = np.cross(dh, dv)
        nrm = np.linalg.norm(c, axis=-1)
        n[b] = c / np.where(nrm == 0, 1.0, nrm)[..., None] * valid[b][..., None]
        R, t = pose[b, :3, :3], pose[b, :3, 3]
        Vg[b] = (V[b] @ R.T + t) * valid[b][..., None]
        ng[b] = n[b] @ R.T
        vmax = np.abs(V[b]).max(-1)
        nb = vmax.copy()
        nb[:, :-1] = np.maximum(nb[:, :-1], vmax[:, 1:])
        nb[:-1] = np.maximum(nb[:-1], vmax[1:])
        with np.errstate(divide="ignore", invalid="ignore"):
            e = 4.0 * FEW * nb * (np.linalg.norm(dh, axis=-1) + np.linalg.norm(dv, axis=-1)) / nrm + FEW
        dn[b] = np.where(nrm == 0, 0.0, e)                                      # cross == 0 exactly (a missing neighbour): n = 0 on both sides
    s = (V * V).sum(-1)
    alpha = np.exp(-s / alpha_den)
    e = s / alpha_den
    assert not ((e > 86.0) & (e < 106.0)).any(), "a depth whose alpha is an fp32 subnormal: not a case of the map step"
    alpha32 = np.where(e >= 106.0, 0.0, alpha.astype(F32).astype(F64))
    return dict(valid=valid, V=V, n=n, Vg=Vg, ng=ng, alpha=alpha, alpha32=alpha32, dn=dn, rays=rays)


def vertex_maps_bwd(depth, K, pose, gV, gVg):
    """d/d depth of sum(gV . V) + sum(gVg . Vg); gV or gVg may be None"""
    depth, pose = np.asarray(depth, F64), np.asarray(pose, F64)
    rays = frame_maps(depth, K, pose)["rays"]
    g = np.zeros(depth.shape)
    if gV is not None:
        g += (np.asarray(gV, F64) * rays).sum(-1)
    if gVg is not None:
        g += (np.asarray(gVg, F64) * np.einsum("bij,bhwj->bhwi", pose[:, :3, :3], rays)).sum(-1)
    return g * (depth != 0)


def transform_points(p, T, transpose_rotation_only=False):
    p, T = np.asarray(p, F64), np.asarray(T, F64)
    return p @ T[:3, :3] if transpose_rotation_only else p @ T[:3, :3].T + T[:3, 3]


# ---------------------------------------------------------------------------------------------------------------------------------------
# fusionutils: one frame (H,W) against a map of M points
# ---------------------------------------------------------------------------------------------------------------------------------------
def _decided(conds):
    """conds: [(value, margin, bound)] of an AND of tests -> decidable: every test decidably true, or one decidably false"""
    all_true, any_false = True, False
    for val, margin, bnd in conds:
        with np.errstate(invalid="ignore"):
            clear = margin > bnd
        all_true = all_true & (val & clear)
        any_false = any_false | (~val & clear)
    return all_true | any_false


def associate(points, normals, ccounts, K, pose, maps, dist_th=DIST_TH, dot_th=DOT_TH):
    """maps: frame_maps(...) of ONE image (arrays (H,W,...)).  -> dict with the three tables (int64 rows [n,h,w]), the margins and the
    undecidable sets: und_pt (M,) map points whose own decisions (front, window, rounding, distance, normal) are undecidable or that
    contend for an undecidable pixel; und_px (H*W,) pixels whose winner is undecidable."""
    p, nm, c = np.asarray(points, F64).reshape(-1, 3), np.asarray(normals, F64).reshape(-1, 3), np.asarray(ccounts, F64).reshape(-1)
    K, pose = np.asarray(K, F64), np.asarray(pose, F64)
    H, W = maps["valid"].shape
    M, N = p.shape[0], H * W
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R, t = pose[:3, :3], pose[:3, 3]
    empty = np.zeros((0, 3), np.int64)
    out = dict(M=M, H=H, W=W, active=empty, similar=empty, unique=empty, und_pt=np.zeros(M, bool), und_px=np.zeros(N, bool),
               counts=dict(ties=0, half=0, win_u_lo=0, win_u_hi=0, win_v_lo=0, win_v_hi=0, behind_in_range=0, z_zero=0, by_conf=0, by_dist=0),
               pix_of=np.full(M, -1, np.int64), winner_of_pix=np.full(N, -1, np.int64))
    if M == 0:
        return out
    q = (p - t) @ R                                                             # R^T (p - t)
    x, y, z = q.T
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, v = fx * x / z + cx, fy * y / z + cy
        dq = FEW * (np.abs(p).max(1) + np.abs(t).max())
        du = abs(fx) * dq * (1 + np.abs(x / z)) / np.abs(z) + FEW * (np.abs(u) + abs(cx))
        dv = abs(fy) * dq * (1 + np.abs(y / z)) / np.abs(z) + FEW * (np.abs(v) + abs(cy))
        # exactness of the chain, in both association orders: R^T (p - t) and R^T p - R^T t; fx x'/z' + cx and (fx x' + cx z')/z'
        prods = (p[:, None, :] * R.T[None]), (t[None, :] * R.T)                  # (M,3,3) terms R_ji p_j ; (3,3) terms R_ji t_j
        ex_q = _exact32(p - t, q).all(1)
        for a in (prods[0], prods[0][..., 0] + prods[0][..., 1], prods[0].sum(-1)):
            ex_q = ex_q & _exact32(a).reshape(M, -1).all(1)
        ex_q = ex_q & bool(_exact32(prods[1], prods[1][..., 0] + prods[1][..., 1], prods[1].sum(-1)).all())
        ex_uv = ex_q & (z != 0) & _exact32(fx * x, fx * x / z, u, cx * z, fx * x + cx * z, fy * y, fy * y / z, v, cy * z, fy * y + cy * z)
        front = z > 0
        u_hi, v_hi = W - 0.999, H - 0.999
        conds = [(front, np.abs(z), dq), (u > -1e-3, np.abs(u + 1e-3), du), (u < u_hi, np.abs(u - u_hi), du),
                 (v > -1e-3, np.abs(v + 1e-3), dv), (v < v_hi, np.abs(v - v_hi), dv)]
        active = conds[0][0] & conds[1][0] & conds[2][0] & conds[3][0] & conds[4][0]
        dec = _decided(conds) | ex_uv | (ex_q & ~front)
        half_u, half_v = np.abs(u - np.floor(u) - 0.5), np.abs(v - np.floor(v) - 0.5)
        dec_round = ((half_u > du) & (half_v > dv)) | ex_uv
    und = ~dec | (active & ~dec_round)
    cnt = out["counts"]
    with np.errstate(invalid="ignore"):
        cnt["win_u_lo"], cnt["win_u_hi"] = int((active & (u < 0)).sum()), int((active & (u > W - 1)).sum())
        cnt["win_v_lo"], cnt["win_v_hi"] = int((active & (v < 0)).sum()), int((active & (v > H - 1)).sum())
        cnt["behind_in_range"] = int(((z < 0) & (u > -1e-3) & (u < u_hi) & (v > -1e-3) & (v < v_hi)).sum())
        cnt["z_zero"] = int((z == 0).sum())
        cnt["half"] = int((active & ((half_u == 0) | (half_v == 0))).sum())
    ia = np.nonzero(active)[0]
    h = np.clip(np.rint(v[ia]), 0, H - 1).astype(np.int64)
    w = np.clip(np.rint(u[ia]), 0, W - 1).astype(np.int64)
    out["active"] = np.stack([ia, h, w], 1)
    pix = h * W + w
    out["pix_of"][ia] = pix
    # similar
    fp, fn = maps["Vg"].reshape(N, 3)[pix], maps["ng"].reshape(N, 3)[pix]
    d = fp - p[ia]
    dist = np.linalg.norm(d, axis=1)
    dot = (fn * nm[ia]).sum(1)
    dd = math.sqrt(3.0) * FEW * (np.maximum(np.abs(p[ia]).max(1), np.abs(fp).max(1)) + np.abs(t).max()) + 4 * U32 * dist
    ddot = maps["dn"].reshape(N)[pix] * np.linalg.norm(nm[ia], axis=1) + FEW
    keep = (dist < dist_th) & (dot > dot_th)
    und[ia] |= ~_decided([(dist < dist_th, np.abs(dist - dist_th), dd), (dot > dot_th, np.abs(dot - dot_th), ddot)])
    out["margins"] = dict(z=np.abs(z), u_lo=np.abs(u + 1e-3), u_hi=np.abs(u - u_hi), v_lo=np.abs(v + 1e-3), v_hi=np.abs(v - v_hi), half_u=half_u,
                          half_v=half_v, du=du, dv=dv, dq=dq, dist=np.abs(dist - dist_th), dd=dd, dot=np.abs(dot - dot_th), ddot=ddot)
    out["similar"] = out["active"][keep]
    und_px = out["und_px"]
    # an undecidable point may land on any pixel around its projection: those pixels' winners are undecidable with it
    # -- unless it is decidably too far from that pixel's vertex, or decidably off its normal, to contend there
    iu = np.nonzero(und & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e6) & (np.abs(v) < 1e6))[0]
    for fu in (np.floor, np.ceil):
        for fv in (np.floor, np.ceil):
            uu = np.where(half_u[iu] > du[iu], np.rint(u[iu]), fu(u[iu]))         # a coordinate whose rounding is decidable has one candidate
            vv = np.where(half_v[iu] > dv[iu], np.rint(v[iu]), fv(v[iu]))
            ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            pn, pp = iu[ok], (vv[ok] * W + uu[ok]).astype(np.int64)
            gp, gn = maps["Vg"].reshape(N, 3)[pp], maps["ng"].reshape(N, 3)[pp]
            di = np.linalg.norm(gp - p[pn], axis=1)
            ddi = math.sqrt(3.0) * FEW * (np.maximum(np.abs(p[pn]).max(1), np.abs(gp).max(1)) + np.abs(t).max()) + 4 * U32 * di
            do = (gn * nm[pn]).sum(1)
            ddo = maps["dn"].reshape(N)[pp] * np.linalg.norm(nm[pn], axis=1) + FEW
            und_px[pp[~((di - dist_th > ddi) | (dot_th - do > ddo))]] = True
    # unique: per pixel the lexicographic minimum of (-c, d2, n)
    sn, sp = ia[keep], pix[keep]
    if sn.size:
        d2 = dist[keep] ** 2
        dd2 = 2 * dist[keep] * dd[keep] + dd[keep] ** 2
        order = np.lexsort((sn, d2, -c[sn], sp))
        sn, sp, d2, dd2 = sn[order], sp[order], d2[order], dd2[order]
        first = np.ones(sn.size, bool)
        first[1:] = sp[1:] != sp[:-1]
        start = np.maximum.accumulate(np.where(first, np.arange(sn.size), 0))    # index of each run's winner
        bn = sn[start]
        cb, ck = c[bn], c[sn]
        c_equal = ck == cb
        c_clear = np.abs(cb - ck) > FEW * np.maximum(np.abs(cb), np.abs(ck))
        same_row = c_equal & (p[sn].astype(F32) == p[bn].astype(F32)).all(1) & (sp == sp[start])
        d_clear = c_equal & (np.abs(d2 - d2[start]) > dd2 + dd2[start])
        rival_ok = first | c_clear | d_clear | same_row
        und_px[sp[~rival_ok]] = True
        und_px[sp[und[sn]]] = True
        rivals = ~first
        tie_px = np.unique(sp[rivals & same_row])
        cnt["ties"] = int((~und_px[tie_px]).sum())
        second = np.zeros(sn.size, bool)
        second[1:] = first[:-1] & ~first[1:]
        cnt["by_conf"] = int((second & c_clear & ~c_equal).sum())
        cnt["by_dist"] = int((second & d_clear & ~same_row).sum())
        win = sn[first]
        wp = sp[first]
        out["unique"] = np.stack([win, wp // W, wp % W], 1)
        out["winner_of_pix"][wp] = win
        und[sn[und_px[sp]]] = True                                               # contenders of an undecidable pixel
    out["und_pt"] = und
    return out


def fuse_append(state, maps, rgb, assoc):
    """fuse_with_map in float64 (alpha as stored: fp32).  -> new state dict + `new_pix`: the pixel of every appended row."""
    M, H, W = assoc["M"], assoc["H"], assoc["W"]
    N = H * W
    a32 = maps["alpha32"].reshape(N)
    src = dict(points=maps["Vg"].reshape(N, 3), normals=maps["ng"].reshape(N, 3), colors=np.asarray(rgb, F64).reshape(N, 3))
    st = {k: np.asarray(state[k], F64).reshape((-1, 3) if k != "ccounts" else (-1,)) for k in ("points", "normals", "colors", "ccounts")}
    new_mask = maps["valid"].reshape(N).copy()
    out = {}
    uq = assoc["unique"]
    if M > 0 and uq.shape[0] > 0:
        n, pix = uq[:, 0], uq[:, 1] * W + uq[:, 2]
        a = np.zeros(M)
        a[n] = a32[pix]
        c = st["ccounts"]
        cn = c + a
        den = np.where(cn == 0, 1.0, cn)
        for k in ("points", "normals", "colors"):
            f = np.zeros((M, 3))
            f[n] = src[k][pix]
            out[k] = (c[:, None] * st[k] + a[:, None] * f) / den[:, None]
        out["ccounts"] = cn
        new_mask[pix] = False
        c0 = int(((c == 0) & (cn == 0)).sum())
    else:
        out = {k: v.copy() for k, v in st.items()}
        c0 = 0
    new_pix = np.nonzero(new_mask)[0]
    for k in ("points", "normals", "colors"):
        out[k] = np.concatenate([out[k], src[k][new_pix]], 0)
    out["ccounts"] = np.concatenate([out["ccounts"], a32[new_pix]], 0)
    out["new_pix"], out["c0_fused"] = new_pix, c0
    return out


def frame_append(maps, rgb):
    """the aggregation map step: every pixel with depth != 0 is one row, row-major"""
    N = maps["valid"].size
    pix = np.nonzero(maps["valid"].reshape(N))[0]
    return dict(points=maps["Vg"].reshape(N, 3)[pix], normals=maps["ng"].reshape(N, 3)[pix], colors=np.asarray(rgb, F64).reshape(N, 3)[pix],
                ccounts=maps["alpha32"].reshape(N)[pix], new_pix=pix)


def step(case):
    """the whole map step of a case -> dict(maps, assoc, after)"""
    maps = {k: v[0] for k, v in frame_maps(case["depth"][None], case["K"][None], case["pose"][None]).items()}
    st = case["state"]
    assoc = associate(st["points"], st["normals"], st["ccounts"], case["K"], case["pose"], maps)
    return dict(maps=maps, assoc=assoc, after=fuse_append(st, maps, case["rgb"], assoc))


# ---------------------------------------------------------------------------------------------------------------------------------------
# comparison of a candidate (the fp32 oracle on the CPU, the kernels on the GPU) with the reference, on the decidable set
# ---------------------------------------------------------------------------------------------------------------------------------------
def compare_tables(ref, got):
    """got: dict active / similar / unique of int64 rows.  Asserts equality outside the undecidable sets; -> (share of undecidable map
    points, share of undecidable pixels)."""
    a = ref["assoc"]
    W = a["W"]
    for name in ("active", "similar"):
        r, g = a[name], np.asarray(got[name]).reshape(-1, 3)
        r, g = r[~a["und_pt"][r[:, 0]]], g[~a["und_pt"][g[:, 0]]]
        assert r.shape == g.shape and np.array_equal(r, g), f"{name} table differs on the decidable set ({g.shape[0]} rows, {r.shape[0]} expected)"
    r, g = a["unique"], np.asarray(got["unique"]).reshape(-1, 3)
    r, g = r[~a["und_px"][r[:, 1] * W + r[:, 2]]], g[~a["und_px"][g[:, 1] * W + g[:, 2]]]
    assert r.shape == g.shape and np.array_equal(r, g), f"unique table differs on the decidable set ({g.shape[0]} rows, {r.shape[0]} expected)"
    if not a["und_pt"].any() and not a["und_px"].any():
        for name in ("active", "similar", "unique"):
            assert np.asarray(got[name]).reshape(-1, 3).shape[0] == a[name].shape[0], f"{name}: row count differs"
    return skipped(ref)


def skipped(ref):
    a = ref["assoc"]
    return (float(a["und_pt"].mean()) if a["M"] else 0.0, float(a["und_px"].mean()))


def state_errors(ref, got, got_unique, valid):
    """got: the map after the step (dict of arrays, all live rows); got_unique: the candidate's own unique table (which pixels IT matched).
    -> {quantity: (max|got - ref| over the decidable rows, max|ref| there)} for points / normals / colors / ccounts, fused and appended rows
    together.  Asserts that the candidate appended exactly its own unmatched valid pixels, and the reference's on the decidable pixels."""
    a, after = ref["assoc"], ref["after"]
    M, H, W = a["M"], a["H"], a["W"]
    N = H * W
    gu = np.asarray(got_unique).reshape(-1, 3)
    mask = np.asarray(valid).reshape(N).copy()
    mask[gu[:, 1] * W + gu[:, 2]] = False
    got_pix = np.nonzero(mask)[0]
    assert got["ccounts"].shape[0] == M + got_pix.size, f"{got['ccounts'].shape[0] - M} rows appended, {got_pix.size} unmatched valid pixels"
    ref_row_of_pix = np.full(N, -1, np.int64)
    ref_row_of_pix[after["new_pix"]] = M + np.arange(after["new_pix"].size)
    ok_px = ~a["und_px"][got_pix]
    assert (ref_row_of_pix[got_pix[ok_px]] >= 0).all() and ok_px.sum() == (~a["und_px"][after["new_pix"]]).sum(), "appended pixels differ on the decidable set"
    rows_got = np.concatenate([np.nonzero(~a["und_pt"])[0], M + np.nonzero(ok_px)[0]])
    rows_ref = np.concatenate([np.nonzero(~a["und_pt"])[0], ref_row_of_pix[got_pix[ok_px]]])
    out = {}
    for k in ("points", "normals", "colors", "ccounts"):
        g, r = np.asarray(got[k], F64)[rows_got], after[k][rows_ref]
        out[k] = (float(np.abs(g - r).max()) if r.size else 0.0, float(np.abs(r).max()) if r.size else 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def pose_of(rx=0.0, ry=0.0, rz=0.0, t=(0.0, 0.0, 0.0)):
    a, b, c = (math.radians(v) for v in (rx, ry, rz))
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rz @ Ry @ Rx, t
    return T.astype(F32)


def intrinsics(H, W):
    """the benchmark camera scaled to the frame, with a focal length of at least 96 pixels: a small frame is a narrow view, not a coarse
    one (at 2 m a pixel then covers 2 cm, so that a map point within half a pixel of a vertex is within dist_th of it)"""
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = max(481.2 * W / 640, 96.0), -max(480.0 * H / 480, 96.3), 319.5 * W / 640, 239.5 * H / 480
    return K.astype(F32)


def intrinsics_dyadic(H, W):
    K = np.eye(4, dtype=F32)
    K[0, 0] = K[1, 1] = 64.0
    K[0, 2], K[1, 2] = W // 2, H // 2
    return K


def scene(H, W, seed, holes=0.02):
    """a smooth surface at about 2 m whose depth changes by a quarter of a pixel's footprint from one pixel to the next, with 2 mm of noise
    (six degrees on a normal) and a few holes"""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    depth = 2.0 + 0.001 * max(H, W) * np.sin(xs / max(W, 2) * 5.0) * np.cos(ys / max(H, 2) * 4.0) + 0.002 * rng.random((H, W))
    depth[rng.random((H, W)) < holes] = 0.0
    return depth.astype(F32), rng.random((H, W, 3)).astype(F32)


def empty_state():
    return dict(points=np.zeros((0, 3), F32), normals=np.zeros((0, 3), F32), colors=np.zeros((0, 3), F32), ccounts=np.zeros(0, F32))


def state32(after, rows=None):
    return {k: np.ascontiguousarray(after[k][:rows], F32) for k in ("points", "normals", "colors", "ccounts")}


def _case(name, kind, H, W, K, pose, depth, rgb, state):
    return dict(name=name, kind=kind, H=H, W=W, K=np.asarray(K, F32), pose=np.asarray(pose, F32), depth=np.asarray(depth, F32),
                rgb=np.asarray(rgb, F32), state=state)


# seeds chosen (tests/test_pointfusion_contract_ref.py checks the outcome) so that every random case skips at most 1 % and is not trivial
RANDOM_CASES = {
    "16x24": (16, 24, None), "33x37": (33, 37, None), "33x37-M0": (33, 37, 0), "33x37-M1": (33, 37, 1), "33x37-M1023": (33, 37, 1023),
    "33x37-M1024": (33, 37, 1024), "33x37-M1025": (33, 37, 1025), "1x8": (1, 8, None), "8x1": (8, 1, None), "72x100": (72, 100, None),
}
SEED = {"16x24": 11, "33x37": 12, "1x8": 13, "8x1": 14, "72x100": 15}
CONSTRUCTED_CASES = ("ties", "rounding", "edges", "far_band_first", "far_band_second", "no_correspondence")
LARGE_M = 1_100_000
LARGE_SEED = 8


@functools.lru_cache(maxsize=None)
def random_case(name):
    """the map is two earlier frames of the same surface, appended one behind the other (first M rows of that), so that most pixels have
    two contenders of unrelated confidence and distance; the live frame sees it from a pose a few degrees away.  A frame of one row or
    one column keeps the pose: its window is 1e-3 pixels wide across, and only a revisit lands in it."""
    H, W, M = RANDOM_CASES[name]
    seed = SEED[name.split("-")[0]]
    K = intrinsics(H, W)
    line = min(H, W) == 1
    parts = []
    for k, pose in enumerate((pose_of(), pose_of() if line else pose_of(-0.4, 0.3, 0.2, (-0.01, 0.015, 0.01)))):
        d0, c0 = scene(H, W, seed + k, holes=0.0 if M is not None else 0.02)
        parts.append(state32(step(_case(name, "random", H, W, K, pose, d0, c0, empty_state()))["after"]))
    st = {k: np.concatenate([parts[0][k], parts[1][k]])[:M] for k in parts[0]}
    assert M is None or st["ccounts"].shape[0] == M
    d1, _ = scene(H, W, seed)                                  # the same depth image from the moved camera: a nearby surface
    _, c1 = scene(H, W, seed + 100)
    return _case(name, "random", H, W, K, pose_of() if line else pose_of(0.5, 1.0, 0.3, (0.02, 0.01, -0.015)), d1, c1, st)


@functools.lru_cache(maxsize=None)
def large_case():
    """LARGE_M map points against a 16 x 24 frame: more than 1024 count blocks of 1024, so the block-count scan carries.  Most points are
    scattered through a 40 m box (outside the view or behind the camera); 3000 lie on the frame's surface, spread over the whole index
    range, the first in block 0 and the last in the last block."""
    H, W = 16, 24
    rng = np.random.default_rng(LARGE_SEED)
    K, pose = intrinsics(H, W), pose_of(2.0, -3.0, 1.0, (0.1, -0.05, 0.2))
    depth, rgb = scene(H, W, 21)
    m = {k: v[0] for k, v in frame_maps(depth[None], K[None], pose[None]).items()}
    pts = rng.uniform(-20, 20, (LARGE_M, 3))
    nrm = rng.standard_normal((LARGE_M, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    on = np.sort(rng.choice(LARGE_M, 3000, replace=False))
    on[0], on[-1] = 0, LARGE_M - 1
    pix = rng.choice(np.nonzero(m["valid"].reshape(-1))[0], 3000)
    pts[on] = m["Vg"].reshape(-1, 3)[pix] + rng.uniform(-0.012, 0.012, (3000, 3))
    nrm[on] = m["ng"].reshape(-1, 3)[pix]
    st = dict(points=pts.astype(F32), normals=nrm.astype(F32), colors=rng.random((LARGE_M, 3)).astype(F32),
              ccounts=rng.uniform(0.001, 2.0, LARGE_M).astype(F32))
    return _case("large", "random", H, W, K, pose, depth, rgb, st)


def _flat(H, W, d=2.0):
    return np.full((H, W), d, F32), np.random.default_rng(H * W).integers(0, 256, (H, W, 3)).astype(F32) / 256.0      # dyadic colours


def _point_at(u, v, zc, K, t, dz=0.0):
    """the world point (identity rotation, translation t) that projects to pixel coordinates (u, v) at camera depth zc (+ dz along the ray's z)"""
    return [(u - float(K[0, 2])) * zc / float(K[0, 0]) + t[0], (v - float(K[1, 2])) * zc / float(K[1, 1]) + t[1], zc + dz + t[2]]


@functools.lru_cache(maxsize=None)
def constructed_case(name):
    """fx = fy = 64, integer cx / cy, rotations with entries 0 / +-1, dyadic translations and depths: every projection is exact in fp32"""
    H, W = 16, 24
    K = intrinsics_dyadic(H, W)
    t = (0.5, -0.25, 0.125)
    pose = pose_of(t=t)
    depth, rgb = _flat(H, W)
    base = state32(step(_case(name, "constructed", H, W, K, pose, depth, rgb, empty_state()))["after"])       # the frame itself as a map
    up = np.array([0.0, 0.0, 1.0], F32)

    def with_points(rows, conf, st=None):
        st = empty_state() if st is None else st
        k = len(rows)
        return dict(points=np.concatenate([st["points"], np.asarray(rows, F32).reshape(k, 3)]), normals=np.concatenate([st["normals"], np.tile(up, (k, 1))]),
                    colors=np.concatenate([st["colors"], np.full((k, 3), 0.5, F32)]), ccounts=np.concatenate([st["ccounts"], np.asarray(conf, F32)]))

    if name == "ties":
        # a revisited place: the map is its own state twice -> every pixel with a normal has two bit-identical contenders, the lower index
        # wins.  Pixel (5,7): A (c 0.9, 1/32 m away) beats B (c 0.2, 1/128 m away) and the two copies: confidence first.  Pixel (9,12):
        # C (c 0.5, 1/32) loses to D (c 0.5, 1/64) although C has the lower index: then distance.
        st = {k: np.concatenate([base[k], base[k]]) for k in base}
        rows = [_point_at(7, 5, 2.0, K, t, dz=1 / 32), _point_at(7, 5, 2.0, K, t, dz=1 / 128), _point_at(12, 9, 2.0, K, t, dz=1 / 32), _point_at(12, 9, 2.0, K, t, dz=-1 / 64)]
        return _case(name, "constructed", H, W, K, pose, depth, rgb, with_points(rows, [0.9, 0.2, 0.5, 0.5], st))
    if name == "rounding":
        # u = 4.5 -> 4, 5.5 -> 6, v = 6.5 -> 6, 7.5 -> 8, (6.5, 2.5) -> (6, 2): round-half-even, half a pixel (1/64 m) from the pixel's vertex
        uv = [(4.5, 3), (5.5, 3), (10, 6.5), (12, 7.5), (6.5, 2.5), (15.5, 9.5)]
        return _case(name, "constructed", H, W, K, pose, depth, rgb, with_points([_point_at(u, v, 2.0, K, t) for u, v in uv], [0.5] * len(uv)))
    if name == "edges":
        e, o = 2.0 ** -11, 2.0 ** -9                            # inside the 1e-3 windows, and just outside them
        uv = [(-e, 4), (W - 1 + e, 5), (6, -e), (7, H - 1 + e), (-e, -e), (W - 1 + e, H - 1 + e),          # in the four windows
              (-o, 4), (W - 1 + o, 5), (6, -o), (7, H - 1 + o),                                            # a little further: outside
              (3, 3), (20, 12)]                                                                            # ordinary
        rows = [_point_at(u, v, 2.0, K, t) for u, v in uv]
        rows += [_point_at(u, v, -2.0, K, t) for u, v in ((3, 3), (11.5, 7.5), (20, 12))]                  # behind the camera, u and v in range
        rows += [[0.25 + t[0], 0.5 + t[1], t[2]], [t[0], t[1], t[2]]]                                      # z' == 0 (u = +-inf), and the camera centre (0/0)
        return _case(name, "constructed", H, W, K, pose, depth, rgb, with_points(rows, [0.5] * len(rows)))
    if name in ("far_band_first", "far_band_second"):
        d = depth.copy()
        d[H // 2:] = 9.5                                       # alpha = exp(-90 / 0.72) = 0 in fp32
        first = _case("far_band_first", "constructed", H, W, K, pose, d, rgb, empty_state())
        if name == "far_band_first":
            return first
        return _case(name, "constructed", H, W, K, pose, d, rgb, state32(step(first)["after"]))            # the same view again: every point meets itself
    if name == "no_correspondence":
        turned = np.eye(4, dtype=F32)
        turned[0, 0] = turned[2, 2] = -1.0                      # half a turn about y: the whole map is behind the camera
        turned[:3, 3] = t
        return _case(name, "constructed", H, W, K, turned, depth, rgb, base)
    raise KeyError(name)


def get_case(name):
    if name == "large":
        return large_case()
    return constructed_case(name) if name in CONSTRUCTED_CASES else random_case(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    return step(get_case(name))


@functools.lru_cache(maxsize=None)
def oracle(name):
    """the fp32 CPU oracle (oracle/pointfusion.py) on the same inputs -> (state after, tables) as numpy"""
    import torch
    from oracle import pointfusion as opf
    c = get_case(name)
    st = {k: torch.from_numpy(v) for k, v in c["state"].items()}
    after, tab = opf.pointfusion_step(st, torch.from_numpy(c["rgb"]), torch.from_numpy(c["depth"]), torch.from_numpy(c["K"]), torch.from_numpy(c["pose"]))
    maps = {k: v.numpy() for k, v in tab["maps"].items()}
    maps["alpha"] = opf.fusion_alpha(tab["maps"]["V"], SIGMA).numpy()
    return ({k: v.numpy() for k, v in after.items()}, {k: tab[k].numpy() for k in ("active", "similar", "unique")}, maps)
