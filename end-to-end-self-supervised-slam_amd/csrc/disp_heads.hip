// disp_heads.hip -- the multi-scale disparity heads of the monodepth2 decoder (networks.py:107-154): Conv3x3(reflect) Cin -> 1 with
// Cin = 16 / 32 / 64 / 128 (num_ch_dec[0..3]) + sigmoid, their backward with the activation's derivative folded in, and
// convert_disp_to_depth (training_utils.py:106-118) times the fixed depth scale (train_depth.py:302-312).  The contracts are stated in
// include/e2eslam.h; tests/test_gpu_disp_head_contracts.py holds every entry point of this file to a float64 reference.
//
// One output column cannot fill an MFMA tile: these are VALU / HBM-bound kernels in the shape of conv.hip's 16-channel head family
// (k_head_fwd, k_head_bwd_fused), generalised by a template on Cin.  Cin / 4 lanes serve one pixel, one float4 channel quad per lane, so a
// wave's load of one tap is whole contiguous pixel rows (Cin * 4 bytes each); at Cin = 128 a wave holds two pixels.  The weights are
// re-laid [tap][ci] in LDS (9 * 128 floats at most).  The lanes of a pixel are combined by a fixed __shfl_xor tree inside the wave; no
// sum in this file depends on arrival order (no atomics): two calls on the same inputs give the same bits.  Every pixel and element
// offset is 64-bit.
#include "e2e_common.h"

typedef float f4v __attribute__((ext_vector_type(4)));

enum { DH_ACT_NONE = 0, DH_ACT_DISP = 3, DH_ACT_SIGMOID = 4 };        // e2ehip.conv.ACT; 1 (ReLU) and 2 (ELU) are refused here
#define DH_PARTS 2048                                                  // most partial-sum rows of one backward call

__device__ __forceinline__ float dh_act(float v, int act) {
    if (act == DH_ACT_NONE) return v;
    const float s = 1.f / (1.f + expf(-v));
    return act == DH_ACT_SIGMOID ? s : 10.f * s + 0.01f;              // networks.py:152 / :290
}

// dz = dy * act'(u) at element i, act' recovered from the activation's OUTPUT y
__device__ __forceinline__ float dh_dz(const float* __restrict__ dy, const float* __restrict__ y, int64_t i, int act) {
    const float g = dy[i];
    if (act == DH_ACT_NONE) return g;
    const float v = y[i];
    if (act == DH_ACT_SIGMOID) return g * (v * (1.f - v));
    const float s = (v - 0.01f) / 10.f;
    return g * (10.f * (s * (1.f - s)));
}

template <int C>
__device__ __forceinline__ void dh_load_weights(float* sw, const float* __restrict__ w) {
    for (int i = threadIdx.x; i < 9 * C; i += 256) {                   // (ci,kh,kw) -> [tap][ci]
        const int ci = i / 9, tap = i - ci * 9;
        sw[tap * C + ci] = w[i];
    }
}

// 256 / (C / 4) pixels per workgroup and pass.  The trip count is the same for every lane of the workgroup (a pixel slot past the end
// recomputes the last pixel and does not store), so the shuffles inside the loop always see all 64 lanes.
template <int C>
__global__ __launch_bounds__(256) void k_disp_head_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ y, int B, int H, int W, int act) {
    constexpr int LPP = C / 4, PPW = 256 / LPP;
    __shared__ float sw[9 * C];
    dh_load_weights<C>(sw, w);
    __syncthreads();
    const int64_t N = (int64_t)B * H * W, HW = (int64_t)H * W;
    const int q = threadIdx.x & (LPP - 1), ps = threadIdx.x / LPP;
    for (int64_t n0 = (int64_t)blockIdx.x * PPW; n0 < N; n0 += (int64_t)gridDim.x * PPW) {
        const int64_t n = n0 + ps;
        const bool on = n < N;
        const int64_t nn = on ? n : N - 1;
        const int b = (int)(nn / HW);
        const int r = (int)(nn - (int64_t)b * HW), h = r / W, ww = r - h * W;
        float acc = 0.f;
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int ys = reflect1(h + kh - 1, H), xs = reflect1(ww + kw - 1, W);
                const f4v v = *(const f4v*)(x + (((int64_t)b * H + ys) * W + xs) * C + q * 4);
                const float* wt = &sw[(kh * 3 + kw) * C + q * 4];
                acc = fmaf(v[0], wt[0], fmaf(v[1], wt[1], fmaf(v[2], wt[2], fmaf(v[3], wt[3], acc))));
            }
#pragma unroll
        for (int o = 1; o < LPP; o <<= 1) acc += __shfl_xor(acc, o, 64);       // the quads of a pixel: fixed tree
        if (on && q == 0) y[n] = dh_act(acc + (bias ? bias[0] : 0.f), act);
    }
}

// dz summed over the outputs q that read input pixel (h, ww) of one image through tap (kh, kw) -- the gather conv.hip documents at
// head_dz_gather: along one axis the direct reader q = p - k + 1 and, for p one pixel away from a border only, the reader that reaches p
// through the reflection (p = 1: q = -k, `ra` = 0; p = n - 2: q = n - k + 1, `rb` = n + 1; -100: none; on a 3-pixel axis the middle pixel
// has both).  Fixed order: direct, then the reflected columns, rows, corners.  dz is formed from dy and y where it is read.
__device__ __forceinline__ float dh_dz_gather(const float* __restrict__ gy, const float* __restrict__ yy, int act, int h, int ww, int kh, int kw,
                                              int H, int W, int rya, int ryb, int rxa, int rxb) {
    const int qy0 = h - kh + 1, qx0 = ww - kw + 1, qya = rya - kh, qyb = ryb - kh, qxa = rxa - kw, qxb = rxb - kw;
    const bool y0 = qy0 >= 0 && qy0 < H, x0 = qx0 >= 0 && qx0 < W;
    const bool ya = qya >= 0 && qya < H, yb = qyb >= 0 && qyb < H, xa = qxa >= 0 && qxa < W, xb = qxb >= 0 && qxb < W;
    float g = (y0 && x0) ? dh_dz(gy, yy, (int64_t)qy0 * W + qx0, act) : 0.f;
    if (ya | yb | xa | xb) {                                                   // pixels next to a border only
        if (y0 && xa) g += dh_dz(gy, yy, (int64_t)qy0 * W + qxa, act);
        if (y0 && xb) g += dh_dz(gy, yy, (int64_t)qy0 * W + qxb, act);
        if (ya && x0) g += dh_dz(gy, yy, (int64_t)qya * W + qx0, act);
        if (yb && x0) g += dh_dz(gy, yy, (int64_t)qyb * W + qx0, act);
        if (ya && xa) g += dh_dz(gy, yy, (int64_t)qya * W + qxa, act);
        if (ya && xb) g += dh_dz(gy, yy, (int64_t)qya * W + qxb, act);
        if (yb && xa) g += dh_dz(gy, yy, (int64_t)qyb * W + qxa, act);
        if (yb && xb) g += dh_dz(gy, yy, (int64_t)qyb * W + qxb, act);
    }
    return g;
}

// d/dx, d/dw and d/dbias in one pass over the pixels.  Workgroup `blockIdx.x` of `gridDim.x` owns the contiguous pixel range
// [blockIdx.x * per, +per); a lane holds one channel quad of one pixel slot and
//   * (weights) multiplies its pixel's dz into the nine taps' quads and keeps 36 running sums (plus dz itself for the bias); after the
//     loop the pixel slots of a wave are folded by fixed xor-shuffles, the four waves through LDS in wave order, and the workgroup writes
//     ONE row of 9 C + 1 partial sums, [tap][ci] then the bias -- k_disp_head_wreduce adds the rows in a fixed order;
//   * (data) gathers the nine dz that read its pixel and stores dx = sum_tap dz_tap * w[tap][ci].
// No lane talks to another inside the loop, so its ragged end (ranges that are no multiple of the pixel slots) needs no care.
template <int C>
__global__ __launch_bounds__(256) void k_disp_head_bwd(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ x,
                                                       const float* __restrict__ w, float* __restrict__ dx, float* __restrict__ partials,
                                                       int B, int H, int W, int act, int want_w) {
    constexpr int LPP = C / 4, PPW = 256 / LPP, COLS = 9 * C + 1;
    __shared__ float red[4][COLS];
    __shared__ float sw[9 * C];
    if (dx) dh_load_weights<C>(sw, w);
    __syncthreads();
    const int64_t N = (int64_t)B * H * W, HW = (int64_t)H * W;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cq = threadIdx.x & (LPP - 1), ps = threadIdx.x / LPP;
    const int64_t per = (N + gridDim.x - 1) / gridDim.x;
    const int64_t n0 = (int64_t)blockIdx.x * per, n1 = (n0 + per < N) ? n0 + per : N;
    float acc[36];
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.f;
    float sb = 0.f;
    for (int64_t n = n0 + ps; n < n1; n += PPW) {
        const int b = (int)(n / HW);
        const int r = (int)(n - (int64_t)b * HW), h = r / W, ww = r - h * W;
        const float* gy = dy + (int64_t)b * HW;
        const float* yy = y + (int64_t)b * HW;
        if (partials) {
            const float g = dh_dz(gy, yy, r, act);
            if (want_w) {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int ys = reflect1(h + kh - 1, H), xs = reflect1(ww + kw - 1, W);
                        const f4v v = *(const f4v*)(x + (((int64_t)b * H + ys) * W + xs) * C + cq * 4);
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[(kh * 3 + kw) * 4 + c] = fmaf(g, v[c], acc[(kh * 3 + kw) * 4 + c]);
                    }
            }
            sb += g;
        }
        if (dx) {
            f4v da = {0.f, 0.f, 0.f, 0.f};
            const int rya = (h == 1) ? 0 : -100, ryb = (h == H - 2) ? H + 1 : -100;
            const int rxa = (ww == 1) ? 0 : -100, rxb = (ww == W - 2) ? W + 1 : -100;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const float* wt = &sw[(kh * 3 + kw) * C + cq * 4];
                    const float gg = dh_dz_gather(gy, yy, act, h, ww, kh, kw, H, W, rya, ryb, rxa, rxb);
#pragma unroll
                    for (int c = 0; c < 4; ++c) da[c] = fmaf(gg, wt[c], da[c]);
                }
            *(f4v*)(dx + n * C + cq * 4) = da;
        }
    }
    if (!partials) return;                                                     // uniform over the grid
#pragma unroll
    for (int k = 0; k < 36; ++k) {
        float v = acc[k];
#pragma unroll
        for (int o = LPP; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);          // the pixel slots of a wave
        acc[k] = v;
    }
#pragma unroll
    for (int o = LPP; o < 64; o <<= 1) sb += __shfl_xor(sb, o, 64);
    if (lane < LPP) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) red[wave][t * C + lane * 4 + c] = acc[t * 4 + c];
        if (lane == 0) red[wave][9 * C] = sb;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < COLS; i += 256)
        partials[(int64_t)blockIdx.x * COLS + i] = ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// one workgroup per column of the (9 C + 1)-vector: 256 threads add the partial rows (fixed assignment, fixed combine order)
__global__ __launch_bounds__(256) void k_disp_head_wreduce(const float* __restrict__ partials, int nparts, int C, float* __restrict__ dw,
                                                           float* __restrict__ dbias) {
    __shared__ float red[4];
    const int col = blockIdx.x, cols = 9 * C + 1;
    if (col == 9 * C ? !dbias : !dw) return;                                   // uniform over the workgroup
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partials[(int64_t)i * cols + col];
    const float t = block_sum(s, red);
    if (threadIdx.x == 0) {
        if (col == 9 * C) dbias[0] = t;
        else { const int tap = col / C, ci = col - tap * C; dw[ci * 9 + tap] = t; }          // (1,C,3,3)
    }
}

__global__ __launch_bounds__(256) void k_disp_range_depth_fwd(const float* __restrict__ disp, float lo, float span, float scale,
                                                              float* __restrict__ depth, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) depth[i] = scale / fmaf(span, disp[i], lo);
}

__global__ __launch_bounds__(256) void k_disp_range_depth_bwd(const float* __restrict__ g, const float* __restrict__ disp, float lo, float span,
                                                              float scale, float* __restrict__ g_disp, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float den = fmaf(span, disp[i], lo);
        g_disp[i] = -g[i] * (scale * span) / (den * den);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
static inline bool dh_channels_ok(int Cin) { return Cin == 16 || Cin == 32 || Cin == 64 || Cin == 128; }
static inline bool dh_act_ok(int act) { return act == DH_ACT_NONE || act == DH_ACT_DISP || act == DH_ACT_SIGMOID; }

// partial-sum rows (= workgroups) of a backward call: one per DH_PART_PIXELS pixels, at most DH_PARTS.  A row is 9 Cin + 1 floats written
// once and read once, against Cin floats of x per pixel: at 64 pixels a row the partial sums are a quarter of the traffic whatever Cin is
// (one row per workgroup PASS -- 8 pixels at Cin = 128 -- made them twice the activations; measured at B = 2: 33.3 -> 27.4 us for the
// 120 x 160 x 64 head, 27.7 -> 26.6 us for 60 x 80 x 128, the two larger heads unchanged -- DESIGN.md section 6).
#define DH_PART_PIXELS 64
static inline int dh_parts(int64_t N, int Cin) {
    const int64_t p = (N + DH_PART_PIXELS - 1) / DH_PART_PIXELS;
    return (int)(p < 1 ? 1 : (p > DH_PARTS ? DH_PARTS : p));
}

static inline int dh_egrid(int64_t n) { const int64_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

extern "C" {

int e2e_disp_head_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int act, void* stream) {
    E2E_REQUIRE(x && w && y && B > 0 && H >= 2 && W >= 2, E2E_ERR_ARG, "e2e_disp_head_fwd: bad argument (NULL x / w / y, or B < 1, H < 2, W < 2)");
    E2E_REQUIRE(dh_channels_ok(Cin), E2E_ERR_ARG, "e2e_disp_head_fwd: Cin = %d (the heads take 16, 32, 64 or 128 channels)", Cin);
    E2E_REQUIRE(dh_act_ok(act), E2E_ERR_ARG, "e2e_disp_head_fwd: act = %d (0 none, 3 disp, 4 sigmoid)", act);
    const int64_t N = (int64_t)B * H * W;
    const int64_t ppw = 256 / (Cin / 4), passes = (N + ppw - 1) / ppw;
    const dim3 grid((unsigned)(passes > 4096 ? 4096 : passes)), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (Cin) {
        case 16: hipLaunchKernelGGL(k_disp_head_fwd<16>, grid, block, 0, st, x, w, bias, y, B, H, W, act); break;
        case 32: hipLaunchKernelGGL(k_disp_head_fwd<32>, grid, block, 0, st, x, w, bias, y, B, H, W, act); break;
        case 64: hipLaunchKernelGGL(k_disp_head_fwd<64>, grid, block, 0, st, x, w, bias, y, B, H, W, act); break;
        default: hipLaunchKernelGGL(k_disp_head_fwd<128>, grid, block, 0, st, x, w, bias, y, B, H, W, act); break;
    }
    E2E_LAUNCH_CHECK("e2e_disp_head_fwd");
    return E2E_OK;
}

int64_t e2e_disp_head_workspace_floats(int B, int H, int W, int Cin) {
    if (B <= 0 || H <= 0 || W <= 0 || !dh_channels_ok(Cin)) return 0;
    return (int64_t)dh_parts((int64_t)B * H * W, Cin) * (9 * Cin + 1);
}

int e2e_disp_head_bwd(const float* dy, const float* y, const float* x, const float* w, float* dx, float* dw, float* dbias, float* workspace,
                      int B, int H, int W, int Cin, int act, void* stream) {
    E2E_REQUIRE(dy && y && x && w && workspace && B > 0 && H >= 2 && W >= 2, E2E_ERR_ARG,
                "e2e_disp_head_bwd: bad argument (NULL dy / y / x / w / workspace, or B < 1, H < 2, W < 2)");
    E2E_REQUIRE(dh_channels_ok(Cin), E2E_ERR_ARG, "e2e_disp_head_bwd: Cin = %d (the heads take 16, 32, 64 or 128 channels)", Cin);
    E2E_REQUIRE(dh_act_ok(act), E2E_ERR_ARG, "e2e_disp_head_bwd: act = %d (0 none, 3 disp, 4 sigmoid)", act);
    if (!dx && !dw && !dbias) return E2E_OK;
    const int parts = dh_parts((int64_t)B * H * W, Cin);
    float* partials = (dw || dbias) ? workspace : nullptr;
    const int want_w = dw ? 1 : 0;
    const dim3 grid(parts), block(256);
    hipStream_t st = (hipStream_t)stream;
    switch (Cin) {
        case 16: hipLaunchKernelGGL(k_disp_head_bwd<16>, grid, block, 0, st, dy, y, x, w, dx, partials, B, H, W, act, want_w); break;
        case 32: hipLaunchKernelGGL(k_disp_head_bwd<32>, grid, block, 0, st, dy, y, x, w, dx, partials, B, H, W, act, want_w); break;
        case 64: hipLaunchKernelGGL(k_disp_head_bwd<64>, grid, block, 0, st, dy, y, x, w, dx, partials, B, H, W, act, want_w); break;
        default: hipLaunchKernelGGL(k_disp_head_bwd<128>, grid, block, 0, st, dy, y, x, w, dx, partials, B, H, W, act, want_w); break;
    }
    if (partials) hipLaunchKernelGGL(k_disp_head_wreduce, dim3(9 * Cin + 1), block, 0, st, partials, parts, Cin, dw, dbias);
    E2E_LAUNCH_CHECK("e2e_disp_head_bwd");
    return E2E_OK;
}

int e2e_disp_range_depth_fwd(const float* disp, float min_depth, float max_depth, float scale, float* depth, int64_t n, void* stream) {
    E2E_REQUIRE(disp && depth && n > 0 && min_depth > 0.f && max_depth > min_depth, E2E_ERR_ARG,
                "e2e_disp_range_depth_fwd: bad argument (NULL pointer, n < 1, or not 0 < min_depth < max_depth)");
    const float lo = (float)(1.0 / (double)max_depth), span = (float)(1.0 / (double)min_depth - 1.0 / (double)max_depth);
    hipLaunchKernelGGL(k_disp_range_depth_fwd, dim3(dh_egrid(n)), dim3(256), 0, (hipStream_t)stream, disp, lo, span, scale, depth, n);
    E2E_LAUNCH_CHECK("e2e_disp_range_depth_fwd");
    return E2E_OK;
}

int e2e_disp_range_depth_bwd(const float* g_depth, const float* disp, float min_depth, float max_depth, float scale, float* g_disp, int64_t n,
                             void* stream) {
    E2E_REQUIRE(g_depth && disp && g_disp && n > 0 && min_depth > 0.f && max_depth > min_depth, E2E_ERR_ARG,
                "e2e_disp_range_depth_bwd: bad argument (NULL pointer, n < 1, or not 0 < min_depth < max_depth)");
    const float lo = (float)(1.0 / (double)max_depth), span = (float)(1.0 / (double)min_depth - 1.0 / (double)max_depth);
    hipLaunchKernelGGL(k_disp_range_depth_bwd, dim3(dh_egrid(n)), dim3(256), 0, (hipStream_t)stream, g_depth, disp, lo, span, scale, g_disp, n);
    E2E_LAUNCH_CHECK("e2e_disp_range_depth_bwd");
    return E2E_OK;
}

}  // extern "C"
