// loss_terms.hip -- the image-space part of a refinement step WITH the loss terms the recommended configuration leaves off
// (online_adaption.py:421-439 geometric consistency, :486-511 auto-masking / minimum reprojection, :600-610 smoothness on the
// mean-normalised disparity), as launches over resident buffers with constant arguments, so that a flagged configuration rides
// in the captured step graph like the default one (e2ehip/stepplan.py).
//
//   e2e_warp_photo_terms_lossgrad   k_terms_prepare (zero d/d depth_src + count the valid projections)
//                                   -> k_warp_photo_terms (loss sums + d/d depth_tgt + scatter into d/d depth_src)
//                                   -> k_reduce_terms (fixed-order sums -> the five loss values)
//   e2e_smoothness_norm_lossgrad    k_sm_sum -> k_sm_grad -> k_sm_apply (mean, normalise, loss + gradient ACCUMULATED into d/d disp)
//
// k_warp_photo_terms runs the tile scheme of k_warp_photo_lossgrad (warp_photo_fused.hip; constants in lossgrad_tile.h: 256 threads =
// 32x16 pixels, two rows per thread, 36x20 warped positions in LDS, SSIM statistics on 34x18, 3x3 fold-back of (G1,G2,G3)) with three
// operands per position instead of two: {synth*m, src*m, tgt*m}.  The identity map photometric(src*m, tgt*m) of auto-masking needs no
// gradient (m is piecewise constant); its VALUE at every q of the 34x18 region decides whether the reprojection map's gradient at q
// survives the per-pixel minimum.
// The default configuration never comes here: warp_photo_fused.hip is untouched.
// LDS: 9 x 720 + 10 x 612 floats = 50.4 KB per workgroup (3 workgroups per CU by LDS).
// fp contraction is ON (FMA), as in warp_photo_fused.hip: tolerance for this path is 1e-4 relative.
#include "e2e_common.h"
#pragma clang fp contract(fast)
#include "lossgrad_tile.h"

#define TNT 256            // block size of the pre-pass, the reduction and the smoothness kernels (their sums add exactly four waves)

// c = d * (M [x,y,1]) + p4 : rows of M (9) then p4 (3), from the device matrices (same arithmetic as warp_photo_fused.hip phase 0)
__device__ __forceinline__ void terms_geometry(const float* __restrict__ K, const float* __restrict__ invK, const float* __restrict__ T, int b, int tid,
                                               float* sgeo) {
    if (tid < 12) {
        const float* Kb = K + b * 16; const float* Tb = T + b * 16; const float* Ib = invK + b * 16;
        const int r = (tid < 9) ? tid / 3 : tid - 9;
        float P[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) P[j] = fmaf(Kb[r * 4 + 0], Tb[0 * 4 + j], fmaf(Kb[r * 4 + 1], Tb[1 * 4 + j], fmaf(Kb[r * 4 + 2], Tb[2 * 4 + j], Kb[r * 4 + 3] * Tb[3 * 4 + j])));
        if (tid < 9) {
            const int cidx = tid % 3;
            sgeo[tid] = fmaf(P[0], Ib[0 * 4 + cidx], fmaf(P[1], Ib[1 * 4 + cidx], P[2] * Ib[2 * 4 + cidx]));
        } else {
            sgeo[tid] = P[3];
        }
    }
}

struct TProj {
    float r0, r1, r2, c2, rz, u, v;
    float inb;             // 0 <= u <= W-1 and 0 <= v <= H-1  <=>  max(|gx|,|gy|) <= 1 (view_synthesis.py:70-71)
};

// the ONE projection both the counting pre-pass and the main kernel evaluate: every operation is written out (fmaf, IEEE divide),
// so the two kernels take identical in-bounds decisions
__device__ __forceinline__ TProj terms_project(const float* geo, float x, float y, float d, int W, int H) {
    TProj p;
    p.r0 = fmaf(geo[0], x, fmaf(geo[1], y, geo[2]));
    p.r1 = fmaf(geo[3], x, fmaf(geo[4], y, geo[5]));
    p.r2 = fmaf(geo[6], x, fmaf(geo[7], y, geo[8]));
    const float c0 = fmaf(d, p.r0, geo[9]), c1 = fmaf(d, p.r1, geo[10]);
    p.c2 = fmaf(d, p.r2, geo[11]);
    p.rz = 1.f / (p.c2 + 1e-7f);
    p.u = c0 * p.rz;
    p.v = c1 * p.rz;
    p.inb = (p.u >= 0.f && p.u <= (float)(W - 1) && p.v >= 0.f && p.v <= (float)(H - 1)) ? 1.f : 0.f;
    return p;
}

struct TSamp {             // bilinear footprint with every index clamped into the image (flags say which taps count)
    int x0, x1, y0, y1;
    bool bx0, bx1, by0, by1;
    float tx, ty, mx, my;   // fractions; d(ix)/d(u), d(iy)/d(v) (0 where the border clamp is active)
};

// F = float for the frame's taps; F = double for the geometric term's sample of depth_src, whose bilinear WEIGHTS are the gradient
// (d/d depth_src = g * weight): a coordinate of ~600 px carries 6e-5 px of fp32 rounding, i.e. 1e-4 of a weight
template <int PAD, typename F>
__device__ __forceinline__ TSamp terms_sample_setup(F ix, F iy, float mx, float my, int W, int H) {
    TSamp s;
    s.mx = mx; s.my = my;
    if (PAD == E2E_PAD_BORDER) {
        if (!(ix > (F)0)) { ix = (F)0; s.mx = 0.f; }
        if (ix >= (F)(W - 1)) { ix = (F)(W - 1); s.mx = 0.f; }
        if (!(iy > (F)0)) { iy = (F)0; s.my = 0.f; }
        if (iy >= (F)(H - 1)) { iy = (F)(H - 1); s.my = 0.f; }
    } else {   // non-finite / wild coordinates: every tap is out of bounds, keep the weights finite
        if (!(fabs(ix) < (F)1e9)) ix = (F)-2;
        if (!(fabs(iy) < (F)1e9)) iy = (F)-2;
    }
    const F fx0 = floor(ix), fy0 = floor(iy);
    s.tx = (float)(ix - fx0); s.ty = (float)(iy - fy0);
    if (PAD == E2E_PAD_BORDER) {
        s.x0 = (int)fx0; s.y0 = (int)fy0;
        s.x1 = min(s.x0 + 1, W - 1); s.y1 = min(s.y0 + 1, H - 1);     // weight is 0 whenever the clamp bites
        s.bx0 = s.bx1 = s.by0 = s.by1 = true;
    } else {
        const int x0 = (int)fmin(fmax(fx0, (F)-2), (F)(W + 1)), y0 = (int)fmin(fmax(fy0, (F)-2), (F)(H + 1));
        s.bx0 = x0 >= 0 && x0 < W; s.bx1 = x0 + 1 >= 0 && x0 + 1 < W;
        s.by0 = y0 >= 0 && y0 < H; s.by1 = y0 + 1 >= 0 && y0 + 1 < H;
        s.x0 = min(max(x0, 0), W - 1); s.x1 = min(max(x0 + 1, 0), W - 1);
        s.y0 = min(max(y0, 0), H - 1); s.y1 = min(max(y0 + 1, 0), H - 1);
    }
    return s;
}

struct TTaps {             // what the adjoint needs about one of the thread's own pixels
    float nw[3], ne[3], sw[3], se[3];
    float tx, ty, mx, my;
    TProj p;
    float m;                // photometric mask (1 when use_mask == 0)
};

// ---- pre-pass: zero d/d depth_src (it receives a scatter) and count the in-bounds projections (losses.py:84-95 `mask.sum() > 10000`
// is a property of the whole frame: the count must exist before any gradient is scaled).  Integer atomics: order-independent.
__global__ __launch_bounds__(TNT) void k_terms_prepare(const float* __restrict__ depth, const float* __restrict__ K, const float* __restrict__ invK,
                                                        const float* __restrict__ T, int* __restrict__ count, float* __restrict__ g_ds, int H, int W) {
    __shared__ float sgeo[12];
    __shared__ float red[TNT / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int N = H * W;
    terms_geometry(K, invK, T, b, tid, sgeo);
    __syncthreads();
    float geo[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) geo[i] = sgeo[i];
    const int i = blockIdx.x * TNT + tid;
    float c = 0.f;
    if (i < N) {
        const int y = i / W, x = i - y * W;
        c = terms_project(geo, (float)x, (float)y, depth[(int64_t)b * N + i], W, H).inb;
        g_ds[(int64_t)b * N + i] = 0.f;
    }
    const float s = block_sum(c, red);
    if (tid == 0 && s > 0.f) atomicAdd(count, (int)s);
}

__global__ void k_terms_clear_count(int* count) { *count = 0; }

template <int PAD>
__global__ __launch_bounds__(TILE_NT) void k_warp_photo_terms(
    const float* __restrict__ depth, const float* __restrict__ d_s, const float* __restrict__ src, e2e_strides ss,
    const float* __restrict__ tgt, e2e_strides ts, const float* __restrict__ K, const float* __restrict__ invK,
    const float* __restrict__ T, int use_mask, int reg_kind, const float* __restrict__ ri_t, const float* __restrict__ ri_s,
    int terms, const float* __restrict__ noise, float w_photo, float w_reg, float w_geo, const int* __restrict__ valid_count,
    float* __restrict__ g_dt, float* g_ds, float* __restrict__ partials, int B, int H, int W) {
    constexpr int PPT = TILE_PPT, NE = TILE_NE;
    __shared__ float sx[3][3][TILE_NPOS];                       // [channel][synth*m | src*m | tgt*m]
    __shared__ float sg[9][TILE_NQ];
    __shared__ float sgate[TILE_NQ];
    __shared__ float sgeo[12];
    __shared__ double sgeo_d[12];                            // the same 12 numbers from the same inputs in double (geometric term only)
    __shared__ float red[TILE_NT / 64];
    const bool geo_on = (terms & E2E_TERM_GEOMETRIC) != 0, auto_on = (terms & E2E_TERM_AUTO_MASKING) != 0;
    const int b = blockIdx.z, tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int tid = threadIdx.y * TILE_W + threadIdx.x;
    const int64_t N = (int64_t)H * W;
    const float* dep = depth + b * N;
    const float* sb = src + b * ss.sb;
    const float* tb = tgt + b * ts.sb;

    terms_geometry(K, invK, T, b, tid, sgeo);
    if (geo_on && tid >= 64 && tid < 76) {
        const int t = tid - 64;
        const float* Kb = K + b * 16; const float* Tb = T + b * 16; const float* Ib = invK + b * 16;
        const int r = (t < 9) ? t / 3 : t - 9;
        double P[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            P[j] = (double)Kb[r * 4 + 0] * Tb[0 * 4 + j] + (double)Kb[r * 4 + 1] * Tb[1 * 4 + j] + (double)Kb[r * 4 + 2] * Tb[2 * 4 + j] + (double)Kb[r * 4 + 3] * Tb[3 * 4 + j];
        const int cidx = t % 3;
        sgeo_d[t] = (t < 9) ? P[0] * Ib[0 * 4 + cidx] + P[1] * Ib[1 * 4 + cidx] + P[2] * Ib[2 * 4 + cidx] : P[3];
    }
    __syncthreads();
    float geo[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) geo[i] = sgeo[i];
    const float sxw = (float)W / (float)(W - 1), syh = (float)H / (float)(H - 1);

    // ---- phase 1: warp tile + halo into LDS ------------------------------------------------------------------------------------
    TTaps kp[PPT];
    bool live[PPT];
    float dval[PPT];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
        int ly, lx;
        if (e < PPT) {
            ly = threadIdx.y * PPT + e + 2;
            lx = threadIdx.x + 2;
        } else {
            const int h = (tid < TILE_NHALO) ? tid : 0;
            if (h < 2 * TILE_XW) { ly = h / TILE_XW; lx = h % TILE_XW; }
            else if (h < 4 * TILE_XW) { ly = TILE_XH - 2 + (h - 2 * TILE_XW) / TILE_XW; lx = (h - 2 * TILE_XW) % TILE_XW; }
            else { const int k4 = h - 4 * TILE_XW; ly = 2 + (k4 >> 2); const int k = k4 & 3; lx = (k < 2) ? k : TILE_XW - 4 + k; }
        }
        const int gy = ty0 + ly - 2, gx = tx0 + lx - 2;
        const bool dom = gx >= -1 && gx <= W && gy >= -1 && gy <= H;
        // reflect, then clamp so that even unused slots address valid memory (their result is zeroed)
        const int qx = tile_clamped(gx, W), qy = tile_clamped(gy, H);
        const float d = dep[qy * W + qx];
        float tv[3], iv[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            tv[c] = tb[c * ts.sc + qy * ts.sh + qx * ts.sw];
            iv[c] = auto_on ? sb[c * ss.sc + qy * ss.sh + qx * ss.sw] : 0.f;
        }
        const TProj p = terms_project(geo, (float)qx, (float)qy, d, W, H);
        const float m = use_mask ? p.inb : 1.f;
        // geometric: the source FRAME is sampled with align_corners=True (ix = u; online_adaption.py:431-434, sic), otherwise with
        // align_corners=False of the /(W-1) grid (ix = u*W/(W-1) - 0.5)
        const TSamp s = geo_on ? terms_sample_setup<PAD, float>(p.u, p.v, 1.f, 1.f, W, H)
                               : terms_sample_setup<PAD, float>(fmaf(p.u, sxw, -0.5f), fmaf(p.v, syh, -0.5f), sxw, syh, W, H);
        float nw[3], ne[3], sw[3], se[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {                  // unconditional loads from clamped addresses, then select
            const float* pc = sb + c * ss.sc;
            const float a = pc[s.y0 * ss.sh + s.x0 * ss.sw], bq = pc[s.y0 * ss.sh + s.x1 * ss.sw];
            const float cq = pc[s.y1 * ss.sh + s.x0 * ss.sw], dq = pc[s.y1 * ss.sh + s.x1 * ss.sw];
            nw[c] = (s.by0 && s.bx0) ? a : 0.f;
            ne[c] = (s.by0 && s.bx1) ? bq : 0.f;
            sw[c] = (s.by1 && s.bx0) ? cq : 0.f;
            se[c] = (s.by1 && s.bx1) ? dq : 0.f;
        }
        const float w00 = (1.f - s.tx) * (1.f - s.ty), w01 = s.tx * (1.f - s.ty), w10 = (1.f - s.tx) * s.ty, w11 = s.tx * s.ty;
        const float mm = dom ? m : 0.f;               // outside the reflect domain: zeros
        if (e < PPT || tid < TILE_NHALO) {
            const int lpos = ly * TILE_XW + lx;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float sv = fmaf(nw[c], w00, fmaf(ne[c], w01, fmaf(sw[c], w10, se[c] * w11)));
                sx[c][0][lpos] = sv * mm;
                sx[c][1][lpos] = iv[c] * mm;
                sx[c][2][lpos] = tv[c] * mm;
            }
        }
        if (e < PPT) {
            live[e] = gx < W && gy < H;
            dval[e] = d;
            TTaps& k = kp[e];
#pragma unroll
            for (int c = 0; c < 3; ++c) { k.nw[c] = nw[c]; k.ne[c] = ne[c]; k.sw[c] = sw[c]; k.se[c] = se[c]; }
            k.tx = s.tx; k.ty = s.ty; k.mx = s.mx; k.my = s.my; k.p = p; k.m = m;
        }
    }
    __syncthreads();

    // ---- phase 2: per q of the 34x18 region: SSIM statistics of both maps, the minimum's choice, loss + (G1,G2,G3) ---------------
    const float kmean = 1.f / ((float)B * (float)H * (float)W);
    const float gup = w_photo * kmean * (0.85f / 3.f);      // upstream gradient on every ssim_c(q) that survives the minimum
    float lsum = 0.f;
#pragma unroll 1
    for (int i = tid; i < TILE_NQ; i += TILE_NT) {
        const int ly = i / TILE_GW, lx = i - ly * TILE_GW;
        const int qx = tx0 + lx - 1, qy = ty0 + ly - 1;
        const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
        const bool own = lx >= 1 && lx <= TILE_W && ly >= 1 && ly <= TILE_H;
        float Rq = 0.f, Aq = 0.f, G[9];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float s_x = 0.f, s_a = 0.f, s_y = 0.f, s_xx = 0.f, s_aa = 0.f, s_yy = 0.f, s_xy = 0.f, s_ay = 0.f;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int j = (ly + r) * TILE_XW + lx + k;
                    const float x = sx[c][0][j], y = sx[c][2][j];
                    s_x += x; s_y += y;
                    s_xx = fmaf(x, x, s_xx); s_yy = fmaf(y, y, s_yy); s_xy = fmaf(x, y, s_xy);
                    if (auto_on) {
                        const float a = sx[c][1][j];
                        s_a += a; s_aa = fmaf(a, a, s_aa); s_ay = fmaf(a, y, s_ay);
                    }
                }
            const int jc = (ly + 1) * TILE_XW + lx + 1;
            const float k9 = 1.f / 9.f, C1 = 1e-4f, C2 = 9e-4f;
            const float MY = s_y * k9, EYY = s_yy * k9, MYY = MY * MY, SIGY = EYY - MYY;
            {
                const float MX = s_x * k9, MXX = MX * MX, MXY = MX * MY;
                const float SIGX = s_xx * k9 - MXX, SIGXY = s_xy * k9 - MXY;
                const float A1 = 2.f * MXY + C1, A2 = 2.f * SIGXY + C2, B1 = MXX + MYY + C1, B2 = SIGX + SIGY + C2;
                const float INV = 1.f / (B1 * B2);
                const float S = A1 * A2 * INV;
                const float TT = 0.5f - 0.5f * S;               // (1 - S)/2
                const bool act = TT >= 0.f && TT <= 1.f;
                Rq += (0.85f / 3.f) * fminf(fmaxf(TT, 0.f), 1.f) + (0.15f / 3.f) * fabsf(sx[c][2][jc] - sx[c][0][jc]);
                // dS/dmu_x = 2 mu_y (A2 - A1)/(B1 B2) - 2 S mu_x (1/B1 - 1/B2) ; 1/B1 = B2*inv, 1/B2 = B1*inv
                const float GI = act ? -0.5f * gup * INV : 0.f;
                G[c * 3 + 0] = 2.f * GI * (MY * (A2 - A1) - S * MX * (B2 - B1));
                G[c * 3 + 1] = -(GI * S) * B1;
                G[c * 3 + 2] = 2.f * GI * A1;
            }
            if (auto_on) {
                const float MX = s_a * k9, MXX = MX * MX, MXY = MX * MY;
                const float SIGX = s_aa * k9 - MXX, SIGXY = s_ay * k9 - MXY;
                const float A1 = 2.f * MXY + C1, A2 = 2.f * SIGXY + C2, B1 = MXX + MYY + C1, B2 = SIGX + SIGY + C2;
                const float TT = 0.5f - 0.5f * (A1 * A2 / (B1 * B2));
                Aq += (0.85f / 3.f) * fminf(fmaxf(TT, 0.f), 1.f) + (0.15f / 3.f) * fabsf(sx[c][2][jc] - sx[c][1][jc]);
            }
        }
        if (auto_on && noise != nullptr && in) Aq += noise[qy * W + qx];      // "Break tie's" (:498): one plane for the whole batch
        // per-pixel minimum over (identity, reprojection): the FIRST minimal map takes the gradient, ties go to the identity map
        const bool gate = in && (!auto_on || Rq < Aq);
        const float val = (auto_on && !(Rq < Aq)) ? Aq : Rq;
        lsum += (in && own) ? val : 0.f;
#pragma unroll
        for (int j = 0; j < 9; ++j) sg[j][i] = gate ? G[j] : 0.f;
        sgate[i] = gate ? 1.f : 0.f;
    }
    __syncthreads();

    // ---- phase 3: adjoint per own pixel ------------------------------------------------------------------------------------------
    float rsum = 0.f, gsum = 0.f;
    const float gl1 = w_reg * kmean;
    const int cnt = geo_on ? *valid_count : 0;
    const bool geo_live = geo_on && cnt > 10000;                        // losses.py:84-95: below, the term is a constant 0
    const float ggeo = geo_live ? w_geo / (float)cnt : 0.f;
    {
        const int lxc = threadIdx.x, ly0 = threadIdx.y * PPT;          // tile-local
        const int px = tx0 + lxc;
        float wx[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int qx = px + k - 1;
            wx[k] = (qx < 0 || qx >= W) ? 0.f : refl_mult(px, qx, W);
        }
        float gsy[PPT][3];     // d loss / d synth per own pixel and channel
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float rs[3][PPT + 2];      // x-folded row sums of G1,G2,G3 for the PPT+2 rows the pixels touch
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < PPT + 2; ++r) {
                    const float* row = &sg[c * 3 + j][(ly0 + r) * TILE_GW + lxc];
                    rs[j][r] = fmaf(row[0], wx[0], fmaf(row[1], wx[1], row[2] * wx[2]));
                }
#pragma unroll
            for (int e = 0; e < PPT; ++e) {
                const int py = ty0 + ly0 + e;
                float a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int qy = py + k - 1;
                    const float wy = (qy < 0 || qy >= H) ? 0.f : refl_mult(py, qy, H);
                    a1 = fmaf(rs[0][e + k], wy, a1);
                    a2 = fmaf(rs[1][e + k], wy, a2);
                    a3 = fmaf(rs[2][e + k], wy, a3);
                }
                const int jc = (ly0 + e + 2) * TILE_XW + lxc + 2;
                const float cx = sx[c][0][jc], cy = sx[c][2][jc];
                float g = (a1 + 2.f * cx * a2 + cy * a3) * (1.f / 9.f);
                const float df = cy - cx;
                const float sgn = tile_sign(df);
                const float own_gate = sgate[(ly0 + e + 1) * TILE_GW + lxc + 1];
                g = fmaf(-w_photo * kmean * (0.15f / 3.f) * own_gate, sgn, g);
                gsy[e][c] = g * kp[e].m;                             // d/d synth = d/dx * mask
            }
        }
#pragma unroll
        for (int e = 0; e < PPT; ++e) {
            if (!live[e]) continue;
            const int py = ty0 + ly0 + e;
            const int64_t o = b * N + (int64_t)py * W + px;
            const TTaps& kq = kp[e];
            float gix = 0.f, giy = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gix = fmaf(gsy[e][c], fmaf(kq.ne[c] - kq.nw[c], 1.f - kq.ty, (kq.se[c] - kq.sw[c]) * kq.ty), gix);
                giy = fmaf(gsy[e][c], fmaf(kq.sw[c] - kq.nw[c], 1.f - kq.tx, (kq.se[c] - kq.ne[c]) * kq.tx), giy);
            }
            float gu = gix * kq.mx, gv = giy * kq.my;
            float gd_direct = 0.f;
            if (geo_on) {
                // losses.py:84-95: diff = clamp(|wd - id| / (wd + id), 0, 1) on the in-bounds pixels; wd = z of the projected point
                // (clamped at 1e-3, view_synthesis.py), id = depth_src sampled on the same grid with align_corners=False (sic)
                // the sampling position and z once more in double (see terms_sample_setup); validity stays the fp32 decision the count used
                const float* dsb = d_s + b * N;
                const double xd = (double)px, yd = (double)py, dd = (double)dval[e];
                const double C0 = dd * (sgeo_d[0] * xd + sgeo_d[1] * yd + sgeo_d[2]) + sgeo_d[9];
                const double C1 = dd * (sgeo_d[3] * xd + sgeo_d[4] * yd + sgeo_d[5]) + sgeo_d[10];
                const double C2 = dd * (sgeo_d[6] * xd + sgeo_d[7] * yd + sgeo_d[8]) + sgeo_d[11];
                const double RZ = 1.0 / (C2 + 1e-7);
                const TSamp s = terms_sample_setup<PAD, double>(C0 * RZ * ((double)W / (double)(W - 1)) - 0.5, C1 * RZ * ((double)H / (double)(H - 1)) - 0.5,
                                                                sxw, syh, W, H);
                const int i00 = s.y0 * W + s.x0, i01 = s.y0 * W + s.x1, i10 = s.y1 * W + s.x0, i11 = s.y1 * W + s.x1;
                const bool b00 = s.by0 && s.bx0, b01 = s.by0 && s.bx1, b10 = s.by1 && s.bx0, b11 = s.by1 && s.bx1;
                const float d00 = b00 ? dsb[i00] : 0.f, d01 = b01 ? dsb[i01] : 0.f, d10 = b10 ? dsb[i10] : 0.f, d11 = b11 ? dsb[i11] : 0.f;
                const float w00 = (1.f - s.tx) * (1.f - s.ty), w01 = s.tx * (1.f - s.ty), w10 = (1.f - s.tx) * s.ty, w11 = s.tx * s.ty;
                const float id = fmaf(d00, w00, fmaf(d01, w01, fmaf(d10, w10, d11 * w11)));
                const float wd = (float)fmax(C2, 1e-3);
                const float sum = wd + id, dif = wd - id, a = fabsf(dif);
                const float r = a / sum;
                const bool valid = kq.p.inb != 0.f;
                if (valid) gsum += fminf(fmaxf(r, 0.f), 1.f);
                if (valid && geo_live && r >= 0.f && r <= 1.f) {
                    const float sg1 = tile_sign(dif);
                    const float is = 1.f / sum;
                    const float g_wd = ggeo * (sg1 - r) * is, g_id = ggeo * (-sg1 - r) * is;
                    if (C2 >= 1e-3) gd_direct = g_wd * kq.p.r2;
                    gu = fmaf(g_id * s.mx, fmaf(d01 - d00, 1.f - s.ty, (d11 - d10) * s.ty), gu);
                    gv = fmaf(g_id * s.my, fmaf(d10 - d00, 1.f - s.tx, (d11 - d01) * s.tx), gv);
                    // d/d depth_src: bilinear scatter (float atomics, as e2e_grid_sample_bwd: not bitwise reproducible run to run)
                    float* gsb = g_ds + b * N;
                    if (b00) atomicAdd(&gsb[i00], g_id * w00);
                    if (b01) atomicAdd(&gsb[i01], g_id * w01);
                    if (b10) atomicAdd(&gsb[i10], g_id * w10);
                    if (b11) atomicAdd(&gsb[i11], g_id * w11);
                }
            }
            const float gc0 = gu * kq.p.rz, gc1 = gv * kq.p.rz, gc2 = -(gu * kq.p.u + gv * kq.p.v) * kq.p.rz;
            float gd = fmaf(gc0, kq.p.r0, fmaf(gc1, kq.p.r1, gc2 * kq.p.r2)) + gd_direct;
            if (reg_kind) {
                const float e0 = ri_t[o] - dval[e], e1 = ri_s[o] - d_s[o];
                float gs;
                if (reg_kind == 2) {
                    rsum += e0 * e0 + e1 * e1;
                    gd = fmaf(gl1, -2.f * e0, gd);
                    gs = gl1 * (-2.f * e1);
                } else {
                    rsum += fabsf(e0) + fabsf(e1);
                    gd += gl1 * ((e0 > 0.f) ? -1.f : ((e0 < 0.f) ? 1.f : 0.f));
                    gs = gl1 * ((e1 > 0.f) ? -1.f : ((e1 < 0.f) ? 1.f : 0.f));
                }
                if (geo_on) atomicAdd(&g_ds[o], gs);       // next to the scatter of other workgroups
                else g_ds[o] = gs;
            }
            g_dt[o] = gd;
        }
    }

    // ---- loss sums: per-workgroup partials, added in a fixed order by k_reduce_terms -------------------------------------------
    const int nblk = gridDim.x * gridDim.y * gridDim.z;
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const float s0 = block_sum(lsum, red);
    __syncthreads();
    const float s1 = block_sum(rsum, red);
    __syncthreads();
    const float s2 = block_sum(gsum, red);
    if (tid == 0) {
        partials[blk] = s0;
        partials[nblk + blk] = s1;
        partials[2 * nblk + blk] = s2;
    }
}

// out[0] photometric mean (after the minimum), out[1] regulariser, out[2] geometric term, out[4] number of valid projections;
// out[3] belongs to e2e_smoothness_norm_lossgrad
__global__ __launch_bounds__(TNT) void k_reduce_terms(const float* __restrict__ partials, int nblk, const int* __restrict__ count, int geo_on, double scale,
                                                      float* __restrict__ out) {
    __shared__ double sh[3][TNT / 64];
    const int tid = threadIdx.x;
    for (int s = 0; s < 3; ++s) {
        double acc = 0.0;
        for (int i = tid; i < nblk; i += TNT) acc += (double)partials[(int64_t)s * nblk + i];
        acc = wave_sum_d(acc);
        if ((tid & 63) == 0) sh[s][tid >> 6] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double v[3];
        for (int s = 0; s < 3; ++s) v[s] = ((sh[s][0] + sh[s][1]) + sh[s][2]) + sh[s][3];
        const int cnt = geo_on ? *count : 0;
        out[0] = (float)(v[0] * scale);
        out[1] = (float)(v[1] * scale);
        out[2] = (cnt > 10000) ? (float)(v[2] / (double)cnt) : 0.f;
        out[4] = (float)cnt;
    }
}

// ---- smoothness on the mean-normalised disparity ---------------------------------------------------------------------------------
#define SM_MAXB 256

// sum of nb (<= 256) per-workgroup partials, the same value in every thread of every workgroup (fixed order)
__device__ __forceinline__ double sm_parts_sum(const float* __restrict__ part, int nb, double* shd) {
    const int tid = threadIdx.x;
    double v = (tid < nb) ? (double)part[tid] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                       // shd may still be read from a previous call
    if ((tid & 63) == 0) shd[tid >> 6] = v;
    __syncthreads();
    return ((shd[0] + shd[1]) + shd[2]) + shd[3];
}

__global__ __launch_bounds__(TNT) void k_sm_sum(const float* __restrict__ disp, int N, float* __restrict__ part) {
    __shared__ float red[TNT / 64];
    float s = 0.f;
    for (int i = blockIdx.x * TNT + threadIdx.x; i < N; i += gridDim.x * TNT) s += disp[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__device__ __forceinline__ float sm_edge(const float* __restrict__ img, e2e_strides is, int y0, int x0, int y1, int x1) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) s += fabsf(img[c * is.sc + y0 * is.sh + x0 * is.sw] - img[c * is.sc + y1 * is.sh + x1 * is.sw]);
    return expf(-s * (1.f / 3.f));
}

// gn = d loss / d (normalised disparity) per pixel; partial sums of the loss and of sum_p gn[p] * disp[p] (the mean's own term)
__global__ __launch_bounds__(TNT) void k_sm_grad(const float* __restrict__ disp, const float* __restrict__ img, e2e_strides is, int H, int W,
                                                  const float* __restrict__ part_m, float* __restrict__ gn, float* __restrict__ part_ls) {
    __shared__ double shd[TNT / 64];
    __shared__ float red[TNT / 64];
    const int N = H * W, nb = gridDim.x;
    const float inv = 1.f / ((float)(sm_parts_sum(part_m, nb, shd) / (double)N) + 1e-7f);
    const float kx = 1.f / ((float)H * (float)(W - 1)), ky = 1.f / ((float)(H - 1) * (float)W);
    float ls = 0.f, ss = 0.f;
    for (int i = blockIdx.x * TNT + threadIdx.x; i < N; i += nb * TNT) {
        const int y = i / W, x = i - y * W;
        const float d0 = disp[i], n0 = d0 * inv;
        float g = 0.f;
        if (x < W - 1) {
            const float e = n0 - disp[i + 1] * inv, w = sm_edge(img, is, y, x, y, x + 1) * kx;
            ls = fmaf(fabsf(e), w, ls);
            g = fmaf(tile_sign(e), w, g);
        }
        if (x > 0) g = fmaf(-tile_sign(disp[i - 1] * inv - n0), sm_edge(img, is, y, x - 1, y, x) * kx, g);
        if (y < H - 1) {
            const float e = n0 - disp[i + W] * inv, w = sm_edge(img, is, y, x, y + 1, x) * ky;
            ls = fmaf(fabsf(e), w, ls);
            g = fmaf(tile_sign(e), w, g);
        }
        if (y > 0) g = fmaf(-tile_sign(disp[i - W] * inv - n0), sm_edge(img, is, y - 1, x, y, x) * ky, g);
        gn[i] = g;
        ss = fmaf(g, d0, ss);
    }
    const float s0 = block_sum(ls, red);
    __syncthreads();
    const float s1 = block_sum(ss, red);
    if (threadIdx.x == 0) {
        part_ls[blockIdx.x] = s0;
        part_ls[nb + blockIdx.x] = s1;
    }
}

// n = d / (m + eps), m = mean(d):  d loss / d d[p] = gn[p] / (m + eps) - sum_q gn[q] d[q] / (N (m + eps)^2)
__global__ __launch_bounds__(TNT) void k_sm_apply(const float* __restrict__ gn, const float* __restrict__ part_m, const float* __restrict__ part_ls, int N,
                                                   float weight, float* __restrict__ g_disp, float* __restrict__ loss_out) {
    __shared__ double shd[TNT / 64];
    const int nb = gridDim.x;
    const float inv = 1.f / ((float)(sm_parts_sum(part_m, nb, shd) / (double)N) + 1e-7f);
    const double L = sm_parts_sum(part_ls, nb, shd);
    const double S = sm_parts_sum(part_ls + nb, nb, shd);
    const float coef = (float)(S / (double)N) * inv * inv;
    for (int i = blockIdx.x * TNT + threadIdx.x; i < N; i += nb * TNT) g_disp[i] += weight * fmaf(gn[i], inv, -coef);
    if (blockIdx.x == 0 && threadIdx.x == 0) loss_out[0] = (float)L;
}

extern "C" {

static int terms_nblk(int B, int H, int W) { return e2e_ceil_div(W, TILE_W) * e2e_ceil_div(H, TILE_H) * B; }

int64_t e2e_warp_photo_terms_lossgrad_workspace_floats(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 3ll * terms_nblk(B, H, W) + 2;               // three partial sums per workgroup, then the count of valid projections
}

int e2e_warp_photo_terms_lossgrad(const float* depth_tgt, const float* depth_src, const float* src, e2e_strides ss, const float* tgt,
                                  e2e_strides ts, const float* K, const float* inv_K, const float* T, int use_mask, int padding_mode,
                                  int reg_kind, const float* reg_init_tgt, const float* reg_init_src, int terms, const float* tie_noise,
                                  float w_photo, float w_reg, float w_geometric, float* loss_out, float* g_depth_tgt, float* g_depth_src,
                                  float* workspace, int B, int H, int W, void* stream) {
    if (const int rc = lossgrad_check_args("e2e_warp_photo_terms_lossgrad", B, H, W,
                                           depth_tgt && src && tgt && K && inv_K && T && g_depth_tgt && workspace && loss_out, padding_mode,
                                           reg_kind, reg_init_tgt && reg_init_src && depth_src && g_depth_src))
        return rc;
    const int known = E2E_TERM_GEOMETRIC | E2E_TERM_AUTO_MASKING | E2E_TERM_MIN_REPROJECTION;
    E2E_REQUIRE((terms & ~known) == 0, E2E_ERR_ARG, "e2e_warp_photo_terms_lossgrad: unknown term bits 0x%x", terms);
    const int geo_on = (terms & E2E_TERM_GEOMETRIC) ? 1 : 0;
    E2E_REQUIRE(!geo_on || (depth_src && g_depth_src), E2E_ERR_ARG, "e2e_warp_photo_terms_lossgrad: the geometric term needs depth_src and g_depth_src");
    // the tie-break noise exists only where both maps AND min_reprojection are on (online_adaption.py:497-498)
    const bool noisy = (terms & E2E_TERM_AUTO_MASKING) && (terms & E2E_TERM_MIN_REPROJECTION);
    const float* noise = noisy ? tie_noise : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g(e2e_ceil_div(W, TILE_W), e2e_ceil_div(H, TILE_H), B);
    const int nblk = g.x * g.y * g.z;
    int* count = (int*)(workspace + 3ll * nblk);
    if (geo_on) {
        hipLaunchKernelGGL(k_terms_clear_count, dim3(1), dim3(1), 0, st, count);
        hipLaunchKernelGGL(k_terms_prepare, dim3(e2e_ceil_div((int64_t)H * W, TNT), B), dim3(TNT), 0, st, depth_tgt, K, inv_K, T, count, g_depth_src, H, W);
        E2E_LAUNCH_CHECK("e2e_warp_photo_terms_lossgrad(prepare)");
    }
#define TL_ARGS depth_tgt, depth_src, src, ss, tgt, ts, K, inv_K, T, use_mask, reg_kind, reg_init_tgt, reg_init_src, terms, noise, w_photo, w_reg, \
                w_geometric, count, g_depth_tgt, g_depth_src, workspace, B, H, W
    if (padding_mode == E2E_PADDING_BORDER) hipLaunchKernelGGL((k_warp_photo_terms<E2E_PAD_BORDER>), g, dim3(TILE_W, 8), 0, st, TL_ARGS);
    else hipLaunchKernelGGL((k_warp_photo_terms<E2E_PAD_ZEROS>), g, dim3(TILE_W, 8), 0, st, TL_ARGS);
#undef TL_ARGS
    E2E_LAUNCH_CHECK("e2e_warp_photo_terms_lossgrad");
    hipLaunchKernelGGL(k_reduce_terms, dim3(1), dim3(TNT), 0, st, workspace, nblk, count, geo_on, 1.0 / ((double)B * H * W), loss_out);
    E2E_LAUNCH_CHECK("e2e_warp_photo_terms_lossgrad(reduce)");
    return E2E_OK;
}

static int sm_blocks(int H, int W) {
    const int nb = e2e_ceil_div((int64_t)H * W, TNT);
    return nb < SM_MAXB ? nb : SM_MAXB;
}

int64_t e2e_smoothness_norm_lossgrad_workspace_floats(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return 3ll * SM_MAXB + (int64_t)H * W;
}

int e2e_smoothness_norm_lossgrad(const float* disp, const float* img, e2e_strides img_strides, float weight, float* loss_out, float* g_disp,
                                 float* workspace, int H, int W, void* stream) {
    E2E_REQUIRE(H > 1 && W > 1 && (int64_t)H * W * 3 < (1ll << 31), E2E_ERR_ARG, "e2e_smoothness_norm_lossgrad: bad dims H=%d W=%d", H, W);
    E2E_REQUIRE(disp && img && loss_out && g_disp && workspace, E2E_ERR_ARG, "e2e_smoothness_norm_lossgrad: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int nb = sm_blocks(H, W), N = H * W;
    float* part_m = workspace;
    float* part_ls = workspace + SM_MAXB;
    float* gn = workspace + 3 * SM_MAXB;
    hipLaunchKernelGGL(k_sm_sum, dim3(nb), dim3(TNT), 0, st, disp, N, part_m);
    hipLaunchKernelGGL(k_sm_grad, dim3(nb), dim3(TNT), 0, st, disp, img, img_strides, H, W, part_m, gn, part_ls);
    hipLaunchKernelGGL(k_sm_apply, dim3(nb), dim3(TNT), 0, st, gn, part_m, part_ls, N, weight, g_disp, loss_out);
    E2E_LAUNCH_CHECK("e2e_smoothness_norm_lossgrad");
    return E2E_OK;
}

}  // extern "C"
