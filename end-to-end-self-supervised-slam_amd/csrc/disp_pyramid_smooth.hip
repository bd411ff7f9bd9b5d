// disp_pyramid_smooth.hip -- monodepth2's edge-aware smoothness on every scale of the disparity pyramid, loss and gradient (gfx950).
//
// Per present scale K: loss_K = normalised_smoothness(dispK, img_K), img_K the box mean of the (H / hK) x (W / wK) blocks of img.  With
// m the mean of one plane, inv = 1 / (m + 1e-7) and n = d inv:  |n_p - n_q| = |inv| |d_p - d_q|, the sign of an edge does not depend on
// the mean, and sum_p gn_p d_p = sign(inv) * raw with raw = sum_edges k_e w_e |d_p - d_q| the plane's unnormalised loss sum.  So
//   k_dps_tiles   ONE pass over the raw disparities of every (scale, batch element) plane (grid z): per pixel the signed sum gn of its up
//                 to four weighted edges, staged in g_dispK itself; per tile the partial sums of d and of raw into the workspace;
//   k_dps_apply   adds the partial sums in a fixed order, scales the staged gradient in place
//                     g = weight (|inv| gn - raw |inv| inv / N)
//                 and writes loss_out[0 .. 4].
// Two launches whatever S and B are, no atomics, no per-pixel scratch plane; two calls give the same bits.
//
// k_dps_tiles: a workgroup of 256 lanes owns a DPS_TW x DPS_TH tile of coarse pixels and the edges that leave them to the right and
// below.  The gradient of the tile's first column and row also needs the edge that ARRIVES from the pixel before them; handing that
// contribution over from the neighbouring tile would take a scatter, so the tile carries a one-pixel halo on all four sides and forms
// those (DPS_TW + DPS_TH) edges itself, from the same operands in the same order as their owner (equal bits).  The box-averaged colour
// of tile + halo is formed once in LDS -- a wave takes one (channel, coarse row), its lanes walk the fine columns on consecutive
// addresses and add the fy fine rows top down, then one lane per coarse pixel adds its fx column sums left to right -- and every edge
// weight of the region is computed once, not once per endpoint.
#include "e2e_common.h"

#define DPS_SCALES 4
#define DPS_TW 32
#define DPS_TH 8
#define DPS_RW (DPS_TW + 2)                 // tile + halo
#define DPS_RH (DPS_TH + 2)
#define DPS_THREADS (DPS_TW * DPS_TH)       // 256: one lane per owned pixel
#define DPS_WAVES (DPS_THREADS / 64)
#define DPS_ROWBUF 512                      // floats of column sums a wave stages at a time
#define DPS_NEX (DPS_TH * (DPS_TW + 1))     // x-edges of the owned rows, the arriving one of column 0 included
#define DPS_NEY ((DPS_TH + 1) * DPS_TW)     // y-edges of the owned columns
#define DPS_APPLY_PX 1024                   // pixels a workgroup of k_dps_apply scales

struct DpsScale {
    const float* d;                         // (B,1,h,w)
    float* gd;                              // (B,1,h,w) or NULL (loss only)
    int h, w, fy, fx;                       // fy = H / h, fx = W / w
    int tiles_x, nt;                        // tiles a row, tiles a plane
    int slot;                               // K of dispK
    float kx, ky;                           // 1 / (B h (w - 1)), 1 / (B (h - 1) w)
    float nbox;                             // fy * fx
    float weight;
    int64_t part;                           // offset of this scale's partial sums in the workspace: plane b at part + 2 nt b
};
struct DpsParams {
    DpsScale s[DPS_SCALES];                 // the present scales, ascending, in the first S slots
};

__device__ __forceinline__ float dps_sign(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

__global__ __launch_bounds__(DPS_THREADS) void k_dps_tiles(DpsParams P, int B, const float* __restrict__ img, e2e_strides is,
                                                            float* __restrict__ ws) {
    const int z = blockIdx.z, si = z / B, b = z - si * B;
    const DpsScale& S = P.s[si];
    if ((int)blockIdx.x >= S.nt) return;                                        // uniform: a coarse plane needs fewer tiles than the grid has
    __shared__ float box[3][DPS_RH][DPS_RW];
    __shared__ float dsh[DPS_RH][DPS_RW];
    __shared__ float ex[DPS_RH][DPS_RW];                                        // ex[r][c]: the edge (r,c) -> (r,c+1), signed and weighted
    __shared__ float ey[DPS_RH][DPS_RW];                                        // ey[r][c]: the edge (r,c) -> (r+1,c)
    __shared__ float buf[DPS_WAVES][DPS_ROWBUF];
    __shared__ float red[DPS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int h = S.h, w = S.w, fy = S.fy, fx = S.fx;
    const int ty0 = (int)blockIdx.x / S.tiles_x, tx0 = (int)blockIdx.x - ty0 * S.tiles_x;
    const int y0 = ty0 * DPS_TH - 1, x0 = tx0 * DPS_TW - 1;                     // the coarse pixel of region entry (0,0)
    const float* d = S.d + (int64_t)b * h * w;

    for (int i = tid; i < DPS_RH * DPS_RW; i += DPS_THREADS) {
        const int ry = i / DPS_RW, rx = i - ry * DPS_RW, y = y0 + ry, x = x0 + rx;
        dsh[ry][rx] = (y >= 0 && y < h && x >= 0 && x < w) ? d[(int64_t)y * w + x] : 0.f;
    }

    // ---- the box-averaged colour of the region's columns that lie in the plane ----
    const int rx_lo = x0 < 0 ? 1 : 0, rx_hi = min(DPS_RW - 1, w - 1 - x0), ncols = rx_hi - rx_lo + 1;
    const int ncc = fx >= DPS_ROWBUF ? 1 : DPS_ROWBUF / fx;                     // coarse columns staged at a time
    const float* imb = img + (int64_t)b * is.sb;
    for (int it = 0; it * DPS_WAVES < 3 * DPS_RH; ++it) {
        const int combo = it * DPS_WAVES + wv, c = combo / DPS_RH, ry = combo - c * DPS_RH, y = y0 + ry;
        const bool live = combo < 3 * DPS_RH && y >= 0 && y < h;
        const float* row = imb + (int64_t)c * is.sc + (int64_t)y * fy * is.sh;
        for (int cc0 = 0; cc0 < ncols; cc0 += ncc) {
            const int nc = min(ncc, ncols - cc0);
            for (int p0 = 0; p0 < fx; p0 += DPS_ROWBUF) {                       // one pass unless a single box is wider than the buffer
                const int seg = min(fx - p0, DPS_ROWBUF), span = nc * seg;
                if (live) {
                    const float* col0 = row + ((int64_t)(x0 + rx_lo + cc0) * fx + p0) * is.sw;
                    for (int i0 = lane; i0 < span; i0 += 4 * 64) {              // consecutive lanes, consecutive fine columns; four
                        float s[4] = {0.f, 0.f, 0.f, 0.f};                      // columns a lane so that their loads are in flight together
                        for (int r = 0; r < fy; ++r)
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (i0 + 64 * u < span) s[u] += col0[(int64_t)(i0 + 64 * u) * is.sw + (int64_t)r * is.sh];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (i0 + 64 * u < span) buf[wv][i0 + 64 * u] = s[u];
                    }
                }
                __syncthreads();
                if (live && lane < nc) {
                    float s = 0.f;
                    for (int k = 0; k < seg; ++k) s += buf[wv][lane * seg + k];
                    float* o = &box[c][ry][rx_lo + cc0 + lane];
                    if (p0 > 0) s = *o + s;
                    *o = (p0 + DPS_ROWBUF >= fx) ? s / S.nbox : s;
                }
                __syncthreads();
            }
        }
    }

    // ---- every edge of the region once ----
    float ls = 0.f;
    for (int e = tid; e < DPS_NEX + DPS_NEY; e += DPS_THREADS) {
        const bool isx = e < DPS_NEX;
        int r, c;
        if (isx) {
            r = 1 + e / (DPS_TW + 1);
            c = e - (r - 1) * (DPS_TW + 1);
        } else {
            r = (e - DPS_NEX) / DPS_TW;
            c = 1 + (e - DPS_NEX) - r * DPS_TW;
        }
        const int r1 = isx ? r : r + 1, c1 = isx ? c + 1 : c;
        const int ya = y0 + r, xa = x0 + c, yb = y0 + r1, xb = x0 + c1;
        float val = 0.f;
        if (ya >= 0 && xa >= 0 && yb < h && xb < w) {
            const float s = (fabsf(box[0][r][c] - box[0][r1][c1]) + fabsf(box[1][r][c] - box[1][r1][c1])) + fabsf(box[2][r][c] - box[2][r1][c1]);
            const float wk = expf(-(s / 3.f)) * (isx ? S.kx : S.ky);
            const float dd = dsh[r][c] - dsh[r1][c1];                           // the sign of a difference of two fp32 numbers is exact
            val = wk * dps_sign(dd);
            if (r >= 1 && c >= 1) ls = fmaf(wk, fabsf(dd), ls);                 // the edges that LEAVE an owned pixel: each edge of the plane once
        }
        (isx ? ex : ey)[r][c] = val;
    }
    __syncthreads();

    const int ry = 1 + (tid >> 5), rx = 1 + (tid & (DPS_TW - 1)), y = y0 + ry, x = x0 + rx;
    float sd = 0.f;
    if (y < h && x < w) {
        sd = dsh[ry][rx];
        if (S.gd) S.gd[(int64_t)b * h * w + (int64_t)y * w + x] = ((ex[ry][rx] - ex[ry][rx - 1]) + ey[ry][rx]) - ey[ry - 1][rx];
    }
    const float s0 = block_sum(sd, red);
    __syncthreads();
    const float s1 = block_sum(ls, red);
    if (tid == 0) {
        float* part = ws + S.part + 2 * (int64_t)S.nt * b;
        part[blockIdx.x] = s0;
        part[S.nt + blockIdx.x] = s1;
    }
}

// sum of nb per-tile partials, by one wave, the same bits in every lane of every wave that asks (fixed order)
__device__ __forceinline__ double dps_parts_sum(const float* __restrict__ part, int nb) {
    double v = 0.0;
    for (int i = threadIdx.x & 63; i < nb; i += 64) v += (double)part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct DpsPlane {
    float ainv, coef;                       // |inv| and raw |inv| inv / N
    double loss;                            // |inv| raw
};
__device__ __forceinline__ DpsPlane dps_plane(const DpsScale& S, int b, const float* __restrict__ ws) {
    const float* part = ws + S.part + 2 * (int64_t)S.nt * b;
    const double N = (double)S.h * (double)S.w;
    const double sumd = dps_parts_sum(part, S.nt), raw = dps_parts_sum(part + S.nt, S.nt);
    const float inv = 1.f / ((float)(sumd / N) + 1e-7f);
    DpsPlane p;
    p.ainv = fabsf(inv);
    p.coef = (float)(raw / N) * p.ainv * inv;
    p.loss = (double)p.ainv * raw;
    return p;
}

__global__ __launch_bounds__(256) void k_dps_apply(DpsParams P, int S, int B, const float* __restrict__ ws, float* __restrict__ loss_out) {
    const int z = blockIdx.z, si = z / B, b = z - si * B;
    const DpsScale& Sc = P.s[si];
    const int64_t N = (int64_t)Sc.h * Sc.w, first = (int64_t)blockIdx.x * DPS_APPLY_PX;
    if (first >= N) return;                                                     // uniform; never the workgroup (0,0,0), which also writes the loss
    if (Sc.gd) {
        const DpsPlane p = dps_plane(Sc, b, ws);
        float* g = Sc.gd + (int64_t)b * N;
        const int64_t last = first + DPS_APPLY_PX < N ? first + DPS_APPLY_PX : N;
        for (int64_t i = first + threadIdx.x; i < last; i += 256) g[i] = Sc.weight * fmaf(g[i], p.ainv, -p.coef);
    }
    if (blockIdx.x == 0 && z == 0) {
        __shared__ double sh[4][DPS_SCALES];
        const int wv = threadIdx.x >> 6;
        double acc[DPS_SCALES] = {0.0, 0.0, 0.0, 0.0};
        for (int q = wv; q < S * B; q += 4) {                                   // wave wv: planes wv, wv + 4, ... in ascending order
            const int qs = q / B;
            const double l = dps_plane(P.s[qs], q - qs * B, ws).loss;
#pragma unroll
            for (int k = 0; k < DPS_SCALES; ++k) acc[k] += (k == qs) ? l : 0.0;
        }
        if ((threadIdx.x & 63) == 0)
#pragma unroll
            for (int k = 0; k < DPS_SCALES; ++k) sh[wv][k] = acc[k];
        __syncthreads();
        if (threadIdx.x == 0) {
            float out[DPS_SCALES] = {0.f, 0.f, 0.f, 0.f};
            double total = 0.0;
            for (int k = 0; k < S; ++k) {
                const double l = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
                out[P.s[k].slot] = (float)l;
                total += (double)P.s[k].weight * l;
            }
            for (int k = 0; k < DPS_SCALES; ++k) loss_out[k] = out[k];
            loss_out[DPS_SCALES] = (float)total;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
static inline int64_t dps_tiles(int h, int w) { return (int64_t)e2e_ceil_div(h, DPS_TH) * e2e_ceil_div(w, DPS_TW); }

// sum over the axes of (n - 1) |stride| fits an int64_t
static bool dps_extent_fits(e2e_strides s, int B, int H, int W) {
    const int64_t n[4] = {B, 3, H, W}, st[4] = {s.sb, s.sc, s.sh, s.sw};
    int64_t total = 0;
    for (int k = 0; k < 4; ++k) {
        if (st[k] == INT64_MIN) return false;
        int64_t term;
        if (__builtin_mul_overflow(n[k] - 1, st[k] < 0 ? -st[k] : st[k], &term) || __builtin_add_overflow(total, term, &total)) return false;
    }
    return true;
}

extern "C" {

int64_t e2e_disp_pyramid_smoothness_workspace_floats(int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3, int B) {
    const int hs[DPS_SCALES] = {h0, h1, h2, h3}, ws[DPS_SCALES] = {w0, w1, w2, w3};
    if (B < 1) return 0;
    int64_t tiles = 0;
    int S = 0;
    for (int k = 0; k < DPS_SCALES; ++k) {
        if (hs[k] == 0 && ws[k] == 0) continue;                                 // an absent scale
        if (hs[k] < 2 || ws[k] < 2) return 0;
        tiles += dps_tiles(hs[k], ws[k]);
        ++S;
    }
    if (S == 0 || (int64_t)S * B > 65535) return 0;
    return 2 * tiles * B;
}

int e2e_disp_pyramid_smoothness_lossgrad(const float* disp0, const float* disp1, const float* disp2, const float* disp3, int h0, int w0, int h1,
                                         int w1, int h2, int w2, int h3, int w3, const float* img, e2e_strides img_strides, int B, int H, int W,
                                         float weight0, float weight1, float weight2, float weight3, float* loss_out, float* g_disp0,
                                         float* g_disp1, float* g_disp2, float* g_disp3, float* workspace, void* stream) {
    const char* who = "e2e_disp_pyramid_smoothness_lossgrad";
    const float* disp[DPS_SCALES] = {disp0, disp1, disp2, disp3};
    float* g_disp[DPS_SCALES] = {g_disp0, g_disp1, g_disp2, g_disp3};
    const int hs[DPS_SCALES] = {h0, h1, h2, h3}, ws[DPS_SCALES] = {w0, w1, w2, w3};
    const float weights[DPS_SCALES] = {weight0, weight1, weight2, weight3};
    E2E_REQUIRE(img && loss_out && workspace, E2E_ERR_ARG, "%s: img, loss_out or workspace is NULL", who);
    E2E_REQUIRE(B > 0 && H > 0 && W > 0, E2E_ERR_ARG, "%s: bad argument (B < 1, H < 1 or W < 1)", who);
    E2E_REQUIRE(dps_extent_fits(img_strides, B, H, W), E2E_ERR_ARG, "%s: the strided extent of img does not fit 64 bits", who);
    DpsParams P;
    int S = 0, with_g = 0;
    int64_t part = 0, tiles_max = 1, apply_max = 1;
    for (int k = 0; k < DPS_SCALES; ++k) {
        if (!disp[k]) continue;
        const int h = hs[k], w = ws[k];
        E2E_REQUIRE(h >= 2 && w >= 2 && h <= H && w <= W, E2E_ERR_ARG, "%s: scale %d is %d x %d (needs 2 <= h <= H = %d and 2 <= w <= W = %d)", who,
                    k, h, w, H, W);
        E2E_REQUIRE(H % h == 0 && W % w == 0, E2E_ERR_ARG, "%s: scale %d: %d x %d does not divide the image %d x %d", who, k, h, w, H, W);
        DpsScale& s = P.s[S++];
        s.d = disp[k];
        s.gd = g_disp[k];
        with_g += g_disp[k] ? 1 : 0;
        s.h = h;
        s.w = w;
        s.fy = H / h;
        s.fx = W / w;
        s.tiles_x = e2e_ceil_div(w, DPS_TW);
        const int64_t nt = dps_tiles(h, w);
        E2E_REQUIRE(nt <= 0x7fffffffLL, E2E_ERR_ARG, "%s: scale %d: %lld tiles a plane exceed the grid", who, k, (long long)nt);
        s.nt = (int)nt;
        s.slot = k;
        s.kx = (float)(1.0 / ((double)B * h * (double)(w - 1)));
        s.ky = (float)(1.0 / ((double)B * (double)(h - 1) * w));
        s.nbox = (float)((double)s.fy * (double)s.fx);
        s.weight = weights[k];
        s.part = part;
        part += 2 * nt * B;
        tiles_max = nt > tiles_max ? nt : tiles_max;
        const int64_t na = ((int64_t)h * w + DPS_APPLY_PX - 1) / DPS_APPLY_PX;
        apply_max = na > apply_max ? na : apply_max;
    }
    E2E_REQUIRE(S > 0, E2E_ERR_ARG, "%s: no scale present (disp0 .. disp3 are all NULL)", who);
    E2E_REQUIRE(with_g == 0 || with_g == S, E2E_ERR_ARG, "%s: %d of %d present scales have a g_disp (every one, or none for the loss alone)", who,
                with_g, S);
    E2E_REQUIRE((int64_t)S * B <= 65535, E2E_ERR_ARG, "%s: scales x B = %lld exceeds 65535", who, (long long)S * B);
    if (with_g == 0)
        for (int k = 0; k < S; ++k) P.s[k].gd = nullptr;
    for (int k = S; k < DPS_SCALES; ++k) P.s[k] = P.s[0];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dps_tiles, dim3((unsigned)tiles_max, 1, S * B), dim3(DPS_THREADS), 0, st, P, B, img, img_strides, workspace);
    E2E_LAUNCH_CHECK("e2e_disp_pyramid_smoothness_lossgrad(tiles)");
    const dim3 ga = with_g ? dim3((unsigned)apply_max, 1, S * B) : dim3(1, 1, 1);
    hipLaunchKernelGGL(k_dps_apply, ga, dim3(256), 0, st, P, S, B, workspace, loss_out);
    E2E_LAUNCH_CHECK("e2e_disp_pyramid_smoothness_lossgrad");
    return E2E_OK;
}

}  // extern "C"
