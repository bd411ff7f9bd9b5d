// pointfusion_grad.hip -- the adjoint of the PointFusion map step (k_pf_fuse + k_pf_append of pointfusion.hip) for gfx950, and of the
// fusion confidence alpha = exp(-|V|^2 / alpha_den) with respect to the depth.  The differentiation rule is stated in
// include/e2eslam.h: the association, the validity mask, the append order, the pose and the intrinsics are constants.  The normals'
// side of the step (opt-in) is at the end: its own tape and its own backward, the points' rule with N for P; the adjoint of the normal
// map itself is in normal_maps_grad.hip.
//
// One pixel owns one map row and one map row is won by at most one pixel, so everything here is a gather over pixels (lane = pixel:
// the per-pixel arrays are read and written coalesced, the 12-byte map rows are gathered) plus one streaming pass over the rows of
// the previous map.  No atomics, no reductions: bitwise reproducible.
//
// The TAPE is what the backward needs of one step and the forward destroys (it fuses in place): per pixel the destination row and,
// for a fused pixel, the winner's confidence, point and colour before the step.  O(H*W) bytes whatever the size of the map.
#include "e2e_common.h"
#include "pf_workspace.h"

#define PFT_HDR_BYTES 64          // u32[16]: [0] = any_match of the step

struct PfTape {
    unsigned int* hdr;
    unsigned int* counts;         // appended pixels per CP_BLOCK pixels (scratch of the ordered scan)
    long long* row;               // [N] destination row: winner (< M_before), appended row (>= M_before), or -1
    float* c;                     // [N] winner's ccount before the step (0 unless fused)
    float* P;                     // [N,3] winner's point before the step
    float* C;                     // [N,3] winner's colour before the step
};
static inline int64_t pft_nb(int64_t N) { return (N + CP_BLOCK - 1) / CP_BLOCK; }
static inline int64_t pft_counts_bytes(int64_t N) { return ((pft_nb(N) + 15) & ~15ll) * 4; }
static inline PfTape pf_tape(void* tape, int64_t N) {
    PfTape t;
    char* p = (char*)tape;
    t.hdr = (unsigned int*)p; p += PFT_HDR_BYTES;
    t.counts = (unsigned int*)p; p += pft_counts_bytes(N);
    t.row = (long long*)p; p += 8 * N;
    t.c = (float*)p; p += 4 * N;
    t.P = (float*)p; p += 12 * N;
    t.C = (float*)p;
    return t;
}

// ---------------------------------------------------------------------------------------------
// tape.  The appended-row numbering is RECOMPUTED: the same ordered scan as k_pf_append's (predicate: no winner and depth != 0, in
// row-major pixel order), in the shape of k_fa_count / k_fa_append -- a count per CP_BLOCK pixels, then every workgroup sums the counts
// before it and ranks its own pixels with wave ballots.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PF_T) void k_pft_count(const float* __restrict__ depth, const unsigned int* __restrict__ pix_best, int64_t N,
                                                    const unsigned int* __restrict__ any_match, unsigned int* __restrict__ counts,
                                                    unsigned int* __restrict__ hdr) {
    __shared__ unsigned int sh[PF_T / 64];
    const int64_t base = (int64_t)blockIdx.x * CP_BLOCK + threadIdx.x;
    unsigned int c = 0;
#pragma unroll
    for (int r = 0; r < CP_ITEMS; ++r) {
        const int64_t i = base + r * PF_T;
        if (i < N && pix_best[i] == PF_NONE && depth[i] != 0.f) ++c;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    if (blockIdx.x == 0 && threadIdx.x < PFT_HDR_BYTES / 4) hdr[threadIdx.x] = threadIdx.x == 0 ? *any_match : 0u;
}

__global__ __launch_bounds__(PF_T) void k_pft_record(const float* __restrict__ pts, const float* __restrict__ col, const float* __restrict__ cc,
                                                     int64_t M, int64_t cap, const float* __restrict__ depth,
                                                     const unsigned int* __restrict__ pix_best, const unsigned int* __restrict__ counts,
                                                     int64_t N, long long* __restrict__ t_row, float* __restrict__ t_c,
                                                     float* __restrict__ t_P, float* __restrict__ t_C) {
    __shared__ unsigned int sh_before[PF_T / 64];
    __shared__ unsigned int sh_wave[CP_ITEMS * (PF_T / 64)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int before = 0;
    for (int j = threadIdx.x; j < (int)blockIdx.x; j += PF_T) before += counts[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_down(before, o, 64);
    if (lane == 0) sh_before[wave] = before;
    // round r, wave w, lane l = pixel blockIdx * CP_BLOCK + r * PF_T + w * 64 + l
    const int64_t base = (int64_t)blockIdx.x * CP_BLOCK + threadIdx.x;
    unsigned int best[CP_ITEMS], rank[CP_ITEMS];
    bool fresh[CP_ITEMS];
#pragma unroll
    for (int r = 0; r < CP_ITEMS; ++r) {
        const int64_t i = base + r * PF_T;
        best[r] = (i < N) ? pix_best[i] : PF_NONE;
        fresh[r] = i < N && best[r] == PF_NONE && depth[i] != 0.f;
        const unsigned long long m = __ballot(fresh[r]);
        rank[r] = (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) sh_wave[r * (PF_T / 64) + wave] = (unsigned int)__popcll(m);
    }
    __syncthreads();
    int64_t row = M + ((sh_before[0] + sh_before[1]) + (sh_before[2] + sh_before[3]));
#pragma unroll
    for (int r = 0; r < CP_ITEMS; ++r) {
        unsigned int woff = 0;
        for (int w = 0; w < wave; ++w) woff += sh_wave[r * (PF_T / 64) + w];
        const int64_t dst = row + woff + rank[r];
#pragma unroll
        for (int w = 0; w < PF_T / 64; ++w) row += sh_wave[r * (PF_T / 64) + w];
        const int64_t i = base + r * PF_T;
        if (i >= N) continue;
        long long out = -1;
        float c0 = 0.f, p[3] = {0.f, 0.f, 0.f}, k[3] = {0.f, 0.f, 0.f};
        if (best[r] != PF_NONE) {
            const int64_t n = (int64_t)best[r];
            if (n < M) {                                    // (the association only names live rows; a stale workspace must not read past them)
                out = n;
                c0 = cc[n];
#pragma unroll
                for (int j = 0; j < 3; ++j) { p[j] = pts[n * 3 + j]; k[j] = col[n * 3 + j]; }
            }
        } else if (fresh[r] && dst < cap) {
            out = dst;                                      // rows beyond the capacity are dropped by k_pf_append
        }
        t_row[i] = out;
        t_c[i] = c0;
#pragma unroll
        for (int j = 0; j < 3; ++j) { t_P[i * 3 + j] = p[j]; t_C[i * 3 + j] = k[j]; }
    }
}

// ---------------------------------------------------------------------------------------------
// backward.  Notation of include/e2eslam.h: a = alpha[q], winner's c / P / C before the step, s = c + a, den = s (1 where s == 0, as the
// forward divides).  With D = gP . (Vg - P) + gC . (rgb - C):  Vg - P' = c (Vg - P) / s and P - P' = -a (Vg - P) / s, so
//   g_alpha = gcc + c D / s^2 ,  g_prevcc = gcc - a D / s^2
// (the differences of nearby positions are taken before anything is scaled).  s == 0 (c = a = 0): X' = c X + a X_f exactly, so
//   g_alpha = gcc + gP . Vg + gC . rgb ,  g_prevcc = gcc + gP . P + gC . C  and every other factor is 0.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PF_T) void k_pf_fuse_bwd_rows(const float* __restrict__ gP, const float* __restrict__ gC, const float* __restrict__ gcc,
                                                           const float* __restrict__ cc_after, const unsigned int* __restrict__ hdr,
                                                           int64_t M_before, float* __restrict__ g_prevP, float* __restrict__ g_prevC,
                                                           float* __restrict__ g_prevcc) {
    // rows that won no pixel (the winners are overwritten by k_pf_fuse_bwd_pixels, which runs after this on the same stream): the
    // gradient passes through, except that a step in which anything matched sends a zero-confidence row's point and colour to 0.
    // For these rows cc_after is the confidence before the step (c + 0).
    const bool fused_any = hdr[0] != 0u;
    for (int64_t i = (int64_t)blockIdx.x * PF_T + threadIdx.x; i < M_before * 3; i += (int64_t)gridDim.x * PF_T) {
        const bool dead = fused_any && cc_after && cc_after[i / 3] == 0.f;     // (cc_after is NULL only when neither is asked for)
        if (g_prevP) g_prevP[i] = (gP && !dead) ? gP[i] : 0.f;
        if (g_prevC) g_prevC[i] = (gC && !dead) ? gC[i] : 0.f;
        if (g_prevcc && i < M_before) g_prevcc[i] = gcc ? gcc[i] : 0.f;
    }
}

__global__ __launch_bounds__(PF_T) void k_pf_fuse_bwd_pixels(const long long* __restrict__ t_row, const float* __restrict__ t_c,
                                                             const float* __restrict__ t_P, const float* __restrict__ t_C,
                                                             const float* __restrict__ Vg, const float* __restrict__ rgb,
                                                             const float* __restrict__ alpha, const float* __restrict__ gP,
                                                             const float* __restrict__ gC, const float* __restrict__ gcc, int64_t M_before,
                                                             int64_t M_after, int64_t N, float* __restrict__ g_Vg, float* __restrict__ g_rgb,
                                                             float* __restrict__ g_alpha, float* __restrict__ g_prevP,
                                                             float* __restrict__ g_prevC, float* __restrict__ g_prevcc) {
    for (int64_t q = (int64_t)blockIdx.x * PF_T + threadIdx.x; q < N; q += (int64_t)gridDim.x * PF_T) {
        const long long row = t_row[q];
        float gv[3] = {0.f, 0.f, 0.f}, gr[3] = {0.f, 0.f, 0.f}, ga = 0.f;
        if (row >= 0 && row < M_after) {
            float up[3], uc[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                up[j] = gP ? gP[row * 3 + j] : 0.f;
                uc[j] = gC ? gC[row * 3 + j] : 0.f;
            }
            const float ucc = gcc ? gcc[row] : 0.f;
            if (row >= M_before) {                          // appended: the row is the pixel
#pragma unroll
                for (int j = 0; j < 3; ++j) { gv[j] = up[j]; gr[j] = uc[j]; }
                ga = ucc;
            } else {                                        // fused into its winner
                const float a = alpha[q], c = t_c[q], s = c + a;
                float D = 0.f, Df = 0.f, Dm = 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float v = Vg[q * 3 + j], x = rgb[q * 3 + j], p = t_P[q * 3 + j], k = t_C[q * 3 + j];
                    D += up[j] * (v - p) + uc[j] * (x - k);
                    Df += up[j] * v + uc[j] * x;
                    Dm += up[j] * p + uc[j] * k;
                }
                float wf, wm, gprev_cc;                     // weights of the frame's and the map's value in the fused row
                if (s == 0.f) {
                    wf = 0.f; wm = 0.f;
                    ga = ucc + Df;
                    gprev_cc = ucc + Dm;
                } else {
                    wf = a / s; wm = c / s;
                    ga = ucc + wm * (D / s);
                    gprev_cc = ucc - wf * (D / s);
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gv[j] = wf * up[j];
                    gr[j] = wf * uc[j];
                    if (g_prevP) g_prevP[row * 3 + j] = wm * up[j];
                    if (g_prevC) g_prevC[row * 3 + j] = wm * uc[j];
                }
                if (g_prevcc) g_prevcc[row] = gprev_cc;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (g_Vg) g_Vg[q * 3 + j] = gv[j];
            if (g_rgb) g_rgb[q * 3 + j] = gr[j];
        }
        if (g_alpha) g_alpha[q] = ga;
    }
}

// alpha = exp(-(rx^2 + ry^2 + 1) d^2 / den) for a valid pixel (V = (rx, ry, 1) d):  d alpha / d depth = -2 (rx^2 + ry^2 + 1) d alpha / den.
// The forward's alpha is read back, not recomputed.  An invalid pixel (d == 0) gets 0, as the vertex maps give it.
__global__ __launch_bounds__(PF_T) void k_vertex_alpha_bwd(const float* __restrict__ depth, const float* __restrict__ K,
                                                           const float* __restrict__ alpha, const float* __restrict__ g_alpha, float alpha_den,
                                                           float* __restrict__ g_depth, int accumulate, int H, int W) {
    const int b = blockIdx.y;
    const int64_t N = (int64_t)H * W;
    const float* Kb = K + b * 16;
    const float fx = Kb[0], fy = Kb[5], cx = Kb[2], cy = Kb[6];
    const float kx = 1.0f / fx, ky = 1.0f / fy, kxc = -cx / fx, kyc = -cy / fy;     // as k_vertex_normal_maps
    for (int i = blockIdx.x * PF_T + threadIdx.x; i < N; i += gridDim.x * PF_T) {
        const int h = i / W, w = i - h * W;
        const float d = depth[b * N + i];
        float g = 0.f;
        if (d != 0.f) {
            const float rx = kx * (float)w + kxc, ry = ky * (float)h + kyc;
            g = g_alpha[b * N + i] * (-2.f * ((rx * rx + ry * ry) + 1.f) * d * alpha[b * N + i] / alpha_den);
        }
        g_depth[b * N + i] = accumulate ? g_depth[b * N + i] + g : g;
    }
}

// The normals' side of the map step.  N' = (c N + a Ng[q]) / s, not renormalised: the points' rule with N for P (D = gN . (Ng - N)).
// The normals tape holds the winner's normal before the step for every fused pixel; row / c come from the step's own tape.
__global__ __launch_bounds__(PF_T) void k_pft_record_normals(const long long* __restrict__ t_row, const float* __restrict__ nrm, int64_t M,
                                                             int64_t N, float* __restrict__ t_N) {
    for (int64_t q = (int64_t)blockIdx.x * PF_T + threadIdx.x; q < N; q += (int64_t)gridDim.x * PF_T) {
        const long long row = t_row[q];
        const bool fused = row >= 0 && row < M;
#pragma unroll
        for (int j = 0; j < 3; ++j) t_N[q * 3 + j] = fused ? nrm[row * 3 + j] : 0.f;
    }
}

__global__ __launch_bounds__(PF_T) void k_pf_fuse_normals_bwd_rows(const float* __restrict__ gN, const float* __restrict__ cc_after,
                                                                   const unsigned int* __restrict__ hdr, int64_t M_before,
                                                                   float* __restrict__ g_prevN, float* __restrict__ g_prevcc) {
    // as k_pf_fuse_bwd_rows: rows that won no pixel pass gN through (a zero-confidence row in a step where anything matched: 0) and
    // get nothing for their confidence; the winners are overwritten by the pixel pass.  g_prevcc is NULL here under accumulate.
    const bool fused_any = hdr[0] != 0u;
    for (int64_t i = (int64_t)blockIdx.x * PF_T + threadIdx.x; i < M_before * 3; i += (int64_t)gridDim.x * PF_T) {
        if (g_prevN) g_prevN[i] = (fused_any && cc_after[i / 3] == 0.f) ? 0.f : gN[i];
        if (g_prevcc && i < M_before) g_prevcc[i] = 0.f;
    }
}

__global__ __launch_bounds__(PF_T) void k_pf_fuse_normals_bwd_pixels(const long long* __restrict__ t_row, const float* __restrict__ t_c,
                                                                     const float* __restrict__ t_N, const float* __restrict__ Ng,
                                                                     const float* __restrict__ alpha, const float* __restrict__ gN,
                                                                     int64_t M_before, int64_t M_after, int64_t N, int accumulate,
                                                                     float* __restrict__ g_Ng, float* __restrict__ g_alpha,
                                                                     float* __restrict__ g_prevN, float* __restrict__ g_prevcc) {
    for (int64_t q = (int64_t)blockIdx.x * PF_T + threadIdx.x; q < N; q += (int64_t)gridDim.x * PF_T) {
        const long long row = t_row[q];
        float gn[3] = {0.f, 0.f, 0.f}, ga = 0.f;
        if (row >= 0 && row < M_after) {
            const float u[3] = {gN[row * 3], gN[row * 3 + 1], gN[row * 3 + 2]};
            if (row >= M_before) {                          // appended: the row is the pixel
#pragma unroll
                for (int j = 0; j < 3; ++j) gn[j] = u[j];
            } else {                                        // fused into its winner
                const float a = alpha[q], c = t_c[q], s = c + a;
                float D = 0.f, Df = 0.f, Dm = 0.f;
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float v = Ng[q * 3 + j], p = t_N[q * 3 + j];
                    D += u[j] * (v - p);
                    Df += u[j] * v;
                    Dm += u[j] * p;
                }
                float wf, wm, gprev_cc;
                if (s == 0.f) {
                    wf = 0.f; wm = 0.f;
                    ga = Df;
                    gprev_cc = Dm;
                } else {
                    wf = a / s; wm = c / s;
                    ga = wm * (D / s);
                    gprev_cc = -wf * (D / s);
                }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    gn[j] = wf * u[j];
                    if (g_prevN) g_prevN[row * 3 + j] = wm * u[j];
                }
                if (g_prevcc) g_prevcc[row] = accumulate ? g_prevcc[row] + gprev_cc : gprev_cc;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (g_Ng) g_Ng[q * 3 + j] = gn[j];
        if (g_alpha) g_alpha[q] = accumulate ? g_alpha[q] + ga : ga;
    }
}

static inline int pfg_grid(int64_t n, int cap = 2048) {
    int64_t g = (n + PF_T - 1) / PF_T;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

extern "C" {

int64_t e2e_pf_fuse_tape_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    const int64_t N = (int64_t)H * W;
    const int64_t b = PFT_HDR_BYTES + pft_counts_bytes(N) + (8 + 4 + 12 + 12) * N;
    return (b + 255) & ~255ll;
}

int e2e_pf_fuse_tape(const float* map_points, const float* map_colors, const float* map_ccounts, int64_t M, int64_t map_capacity,
                     const float* depth, void* workspace, int H, int W, void* tape, void* stream) {
    E2E_REQUIRE(M >= 0 && M <= map_capacity && M < (1ll << 32) - 1 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), E2E_ERR_ARG,
                "e2e_pf_fuse_tape: bad sizes M=%lld cap=%lld", (long long)M, (long long)map_capacity);
    E2E_REQUIRE(depth && workspace && tape && (M == 0 || (map_points && map_colors && map_ccounts)), E2E_ERR_ARG,
                "e2e_pf_fuse_tape: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const PfWs w = pf_ws(workspace, map_capacity, H, W);
    const int64_t N = (int64_t)H * W;
    const PfTape t = pf_tape(tape, N);
    const int nb = (int)pft_nb(N);
    hipLaunchKernelGGL(k_pft_count, dim3(nb), dim3(PF_T), 0, st, depth, (const unsigned int*)w.pix_best, N, (const unsigned int*)w.any_match,
                       t.counts, t.hdr);
    hipLaunchKernelGGL(k_pft_record, dim3(nb), dim3(PF_T), 0, st, map_points, map_colors, map_ccounts, M, map_capacity, depth,
                       (const unsigned int*)w.pix_best, (const unsigned int*)t.counts, N, t.row, t.c, t.P, t.C);
    E2E_LAUNCH_CHECK("e2e_pf_fuse_tape");
    return E2E_OK;
}

int e2e_pf_fuse_bwd(const void* tape, const float* Vg, const float* rgb, const float* alpha, const float* g_points, const float* g_colors,
                    const float* g_ccounts, const float* ccounts_after, int64_t M_before, int64_t M_after, float* g_Vg, float* g_rgb,
                    float* g_alpha, float* g_prev_points, float* g_prev_colors, float* g_prev_ccounts, int H, int W, void* stream) {
    E2E_REQUIRE(M_before >= 0 && M_after >= M_before && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), E2E_ERR_ARG,
                "e2e_pf_fuse_bwd: bad sizes M_before=%lld M_after=%lld", (long long)M_before, (long long)M_after);
    E2E_REQUIRE(tape && Vg && rgb && alpha, E2E_ERR_ARG, "e2e_pf_fuse_bwd: null pointer");
    E2E_REQUIRE(g_Vg || g_rgb || g_alpha || g_prev_points || g_prev_colors || g_prev_ccounts, E2E_ERR_ARG, "e2e_pf_fuse_bwd: no output");
    E2E_REQUIRE(ccounts_after || M_before == 0 || !(g_prev_points || g_prev_colors), E2E_ERR_ARG,
                "e2e_pf_fuse_bwd: ccounts_after is needed for the previous map's point / colour gradient");
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const PfTape t = pf_tape((void*)tape, N);
    if (M_before > 0 && (g_prev_points || g_prev_colors || g_prev_ccounts))
        hipLaunchKernelGGL(k_pf_fuse_bwd_rows, dim3(pfg_grid(M_before * 3, 8192)), dim3(PF_T), 0, st, g_points, g_colors, g_ccounts, ccounts_after,
                           (const unsigned int*)t.hdr, M_before, g_prev_points, g_prev_colors, g_prev_ccounts);
    hipLaunchKernelGGL(k_pf_fuse_bwd_pixels, dim3(pfg_grid(N)), dim3(PF_T), 0, st, (const long long*)t.row, (const float*)t.c, (const float*)t.P,
                       (const float*)t.C, Vg, rgb, alpha, g_points, g_colors, g_ccounts, M_before, M_after, N, g_Vg, g_rgb, g_alpha,
                       g_prev_points, g_prev_colors, g_prev_ccounts);
    E2E_LAUNCH_CHECK("e2e_pf_fuse_bwd");
    return E2E_OK;
}

int e2e_vertex_alpha_bwd(const float* depth, const float* K, const float* alpha, const float* g_alpha, float alpha_den, float* g_depth,
                         int accumulate, int B, int H, int W, void* stream) {
    E2E_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W * 3 < (1ll << 31), E2E_ERR_ARG, "e2e_vertex_alpha_bwd: bad dims");
    E2E_REQUIRE(depth && K && alpha && g_alpha && g_depth && alpha_den > 0.f, E2E_ERR_ARG, "e2e_vertex_alpha_bwd: bad argument");
    hipLaunchKernelGGL(k_vertex_alpha_bwd, dim3(pfg_grid((int64_t)H * W), B), dim3(PF_T), 0, (hipStream_t)stream, depth, K, alpha, g_alpha,
                       alpha_den, g_depth, accumulate, H, W);
    E2E_LAUNCH_CHECK("e2e_vertex_alpha_bwd");
    return E2E_OK;
}

int64_t e2e_pf_fuse_normals_tape_bytes(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (12 * (int64_t)H * W + 255) & ~255ll;
}

int e2e_pf_fuse_normals_tape(const void* tape, const float* map_normals, int64_t M, void* ntape, int H, int W, void* stream) {
    E2E_REQUIRE(M >= 0 && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), E2E_ERR_ARG, "e2e_pf_fuse_normals_tape: bad sizes M=%lld",
                (long long)M);
    E2E_REQUIRE(tape && ntape && (M == 0 || map_normals), E2E_ERR_ARG, "e2e_pf_fuse_normals_tape: null pointer");
    const int64_t N = (int64_t)H * W;
    const PfTape t = pf_tape((void*)tape, N);
    hipLaunchKernelGGL(k_pft_record_normals, dim3(pfg_grid(N)), dim3(PF_T), 0, (hipStream_t)stream, (const long long*)t.row, map_normals, M, N,
                       (float*)ntape);
    E2E_LAUNCH_CHECK("e2e_pf_fuse_normals_tape");
    return E2E_OK;
}

int e2e_pf_fuse_normals_bwd(const void* tape, const void* ntape, const float* Ng, const float* alpha, const float* g_normals,
                            const float* ccounts_after, int64_t M_before, int64_t M_after, float* g_Ng, float* g_prev_normals,
                            float* g_alpha, float* g_prev_ccounts, int accumulate, int H, int W, void* stream) {
    E2E_REQUIRE(M_before >= 0 && M_after >= M_before && H > 0 && W > 0 && (int64_t)H * W < (1ll << 31), E2E_ERR_ARG,
                "e2e_pf_fuse_normals_bwd: bad sizes M_before=%lld M_after=%lld", (long long)M_before, (long long)M_after);
    E2E_REQUIRE(tape && ntape && Ng && alpha && (g_normals || M_after == 0), E2E_ERR_ARG, "e2e_pf_fuse_normals_bwd: null pointer");
    E2E_REQUIRE(g_Ng || g_prev_normals || g_alpha || g_prev_ccounts, E2E_ERR_ARG, "e2e_pf_fuse_normals_bwd: no output");
    E2E_REQUIRE(ccounts_after || M_before == 0 || !g_prev_normals, E2E_ERR_ARG,
                "e2e_pf_fuse_normals_bwd: ccounts_after is needed for the previous map's normal gradient");
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)H * W;
    const PfTape t = pf_tape((void*)tape, N);
    float* rows_cc = accumulate ? nullptr : g_prev_ccounts;         // under accumulate the rows that won no pixel keep what they hold
    if (M_before > 0 && (g_prev_normals || rows_cc))
        hipLaunchKernelGGL(k_pf_fuse_normals_bwd_rows, dim3(pfg_grid(M_before * 3, 8192)), dim3(PF_T), 0, st, g_normals, ccounts_after,
                           (const unsigned int*)t.hdr, M_before, g_prev_normals, rows_cc);
    hipLaunchKernelGGL(k_pf_fuse_normals_bwd_pixels, dim3(pfg_grid(N)), dim3(PF_T), 0, st, (const long long*)t.row, (const float*)t.c,
                       (const float*)ntape, Ng, alpha, g_normals, M_before, M_after, N, accumulate != 0, g_Ng, g_alpha, g_prev_normals,
                       g_prev_ccounts);
    E2E_LAUNCH_CHECK("e2e_pf_fuse_normals_bwd");
    return E2E_OK;
}

}  // extern "C"
