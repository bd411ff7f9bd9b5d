// disp_pyramid.hip -- the step from the monodepth2 disparity pyramid to full-resolution depths, and its adjoint (gfx950).
//
// Every scale's sigmoid disparity (B,1,h,w) is upsampled bilinearly to (H,W) with the half-pixel convention of
// F.interpolate(align_corners=False) and converted to depth as e2e_disp_range_depth_fwd does; up to four scales in ONE launch
// (grid z = scale * B + batch element).  The adjoint is a GATHER: a group of lanes of one wave owns a coarse pixel, walks the fine pixels
// of its footprint in a fixed order and adds the lanes' sums with a fixed shuffle tree -- no atomics, no workspace, equal bits call to
// call.  u is recomputed from the disparities in the backward; nothing is saved between the two calls.
//
// One device function (dp_axis) decides the stencil of a fine row / column for BOTH directions, so the weight the backward gives a
// (fine, coarse) pair is the weight the forward used, whatever fp32 did to the source coordinate.
#include "e2e_common.h"

#define DP_SCALES 4
#define DP_TILE_W 64                       // forward: a workgroup writes a 64 x 4 tile of one (scale, batch element) plane
#define DP_TILE_H 4
#define DP_MAX_SIDE (65535 * DP_TILE_H)    // grid.y = ceil(H / 4) fits the grid, and the footprint margin below holds (see dp_range)

struct DpScale {
    const float* d;                        // (B,1,h,w)
    float* gd;                             // (B,1,h,w), backward only
    int h, w;
    float ry, rx;                          // h / H, w / W: fine index -> coarse coordinate
    float fy, fx;                          // H / h, W / w: coarse index -> fine coordinate (footprint candidates)
    int lpp_shift;                         // backward: 2^lpp_shift lanes share a coarse pixel
};
struct DpParams {
    DpScale s[DP_SCALES];                  // the present scales, ascending, in the first S slots
};

struct DpAxis {
    int i0, i1;
    float w0, w1;
};

// the stencil of fine index y on an axis of n coarse samples: s = max((y + 0.5) r - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, n - 1)
__device__ __forceinline__ DpAxis dp_axis(int y, int n, float r) {
    const float s = fmaxf(fmaf((float)y + 0.5f, r, -0.5f), 0.f);
    const float f = floorf(s);
    DpAxis a;
    a.i0 = min((int)f, n - 1);
    a.i1 = min(a.i0 + 1, n - 1);
    a.w1 = s - f;
    a.w0 = 1.f - a.w1;
    return a;
}

__device__ __forceinline__ float dp_u(const float* __restrict__ d, int w, const DpAxis& ay, const DpAxis& ax) {
    const float* r0 = d + (int64_t)ay.i0 * w;
    const float* r1 = d + (int64_t)ay.i1 * w;
    return (ay.w0 * ax.w0) * r0[ax.i0] + (ay.w0 * ax.w1) * r0[ax.i1] + (ay.w1 * ax.w0) * r1[ax.i0] + (ay.w1 * ax.w1) * r1[ax.i1];
}

// the weight with which coarse index j enters the stencil a (both taps when i1 was clamped onto i0)
__device__ __forceinline__ float dp_weight_of(const DpAxis& a, int j) { return (a.i0 == j ? a.w0 : 0.f) + (a.i1 == j ? a.w1 : 0.f); }

// Fine indices that can touch coarse index j: s in [j - 1, j + 1) <=> y in [(j - 0.5) f - 0.5, (j + 1.5) f - 0.5), widened by one on
// either side (fp32 moves s by a few ulp of n, far less than the spacing r of two fine indices while the sides stay below DP_MAX_SIDE)
// and clipped to the axis.  j = 0 also owns everything whose s was clamped to 0, j = n - 1 everything up to the last fine index.
// dp_weight_of() then gives the candidates that do not touch j the weight 0: the range only has to be a superset.
__device__ __forceinline__ void dp_range(int j, int n, int N, float f, int& lo, int& hi) {
    lo = j == 0 ? 0 : max(0, (int)floorf(((float)j - 0.5f) * f - 0.5f) - 1);
    hi = j == n - 1 ? N - 1 : min(N - 1, (int)ceilf(((float)j + 1.5f) * f - 0.5f) + 1);
}

__global__ __launch_bounds__(256) void k_disp_pyramid_depth_fwd(DpParams P, int B, int H, int W, float lo, float span, float scale,
                                                                float* __restrict__ depth) {
    const int z = blockIdx.z, si = z / B, b = z - si * B;
    const int x = blockIdx.x * DP_TILE_W + (threadIdx.x & (DP_TILE_W - 1)), y = blockIdx.y * DP_TILE_H + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int h = P.s[si].h, w = P.s[si].w;
    const float* d = P.s[si].d + (int64_t)b * h * w;
    const float u = dp_u(d, w, dp_axis(y, h, P.s[si].ry), dp_axis(x, w, P.s[si].rx));
    depth[((int64_t)z * H + y) * W + x] = scale / fmaf(span, u, lo);
}

__global__ __launch_bounds__(256) void k_disp_pyramid_depth_bwd(DpParams P, int B, int H, int W, float lo, float span, float scale,
                                                                const float* __restrict__ g) {
    const int z = blockIdx.z, si = z / B, b = z - si * B;
    const int h = P.s[si].h, w = P.s[si].w, shift = P.s[si].lpp_shift, lpp = 1 << shift;
    const int64_t npx = (int64_t)h * w;
    if ((((int64_t)blockIdx.x * 256) >> shift) >= npx) return;                 // uniform: this scale needs fewer workgroups than the grid has
    const int64_t px = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> shift;
    const int lane = threadIdx.x & (lpp - 1);
    const bool live = px < npx;
    float acc = 0.f;
    if (live) {
        const float ry = P.s[si].ry, rx = P.s[si].rx;
        const float* d = P.s[si].d + (int64_t)b * npx;
        const float* gz = g + (int64_t)z * H * W;
        const int j = (int)(px / w), i = (int)(px - (int64_t)j * w);
        int ylo, yhi, xlo, xhi;
        dp_range(j, h, H, P.s[si].fy, ylo, yhi);
        dp_range(i, w, W, P.s[si].fx, xlo, xhi);
        const int nx = xhi - xlo + 1, n = (yhi - ylo + 1) * nx;
        for (int c = lane; c < n; c += lpp) {                                  // fixed order: candidate c of lane l is c = l + k lpp
            const int cy = c / nx, yy = ylo + cy, xx = xlo + (c - cy * nx);
            const DpAxis ay = dp_axis(yy, h, ry), ax = dp_axis(xx, w, rx);
            const float wgt = dp_weight_of(ay, j) * dp_weight_of(ax, i);
            if (wgt == 0.f) continue;
            const float den = fmaf(span, dp_u(d, w, ay, ax), lo);
            const float gu = -gz[(int64_t)yy * W + xx] * (scale * span) / (den * den);
            acc = fmaf(wgt, gu, acc);
        }
    }
    for (int o = lpp >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);      // the group's lanes, a fixed tree; every lane of the wave takes part
    if (live && lane == 0) P.s[si].gd[(int64_t)b * npx + px] = acc;
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
// lanes per coarse pixel: the footprint candidates (2 ceil(f) + 3 a side) at about eight a lane, a power of two from 1 to 64
static inline int dp_lpp_shift(int h, int w, int H, int W) {
    const int64_t n = (int64_t)(2 * ((H + h - 1) / h) + 3) * (2 * ((W + w - 1) / w) + 3);
    int s = 0;
    while (s < 6 && ((int64_t)8 << s) < n) ++s;
    return s;
}

// fills P with the present scales in ascending order; returns their number, or -1 with the error set
static int dp_collect(const char* who, const float* const* disp, float* const* g_disp, bool bwd, const int* hs, const int* ws, int B, int H,
                      int W, float min_depth, float max_depth, DpParams& P) {
    E2E_REQUIRE(B > 0 && H > 0 && W > 0 && H <= DP_MAX_SIDE && W <= DP_MAX_SIDE, -1,
                "%s: bad argument (B < 1, or H / W outside 1 .. %d)", who, DP_MAX_SIDE);
    E2E_REQUIRE(min_depth > 0.f && max_depth > min_depth, -1, "%s: not 0 < min_depth < max_depth", who);
    int S = 0;
    for (int k = 0; k < DP_SCALES; ++k) {
        if (!disp[k]) continue;
        E2E_REQUIRE(hs[k] > 0 && ws[k] > 0 && hs[k] <= H && ws[k] <= W, -1,
                    "%s: scale %d is %d x %d (needs 1 <= h <= H = %d and 1 <= w <= W = %d)", who, k, hs[k], ws[k], H, W);
        E2E_REQUIRE((int64_t)(2 * ((H + hs[k] - 1) / hs[k]) + 5) * (2 * ((W + ws[k] - 1) / ws[k]) + 5) <= 0x7fffffffLL, -1,
                    "%s: scale %d: the footprint of a coarse pixel exceeds 2^31 - 1 fine pixels", who, k);
        E2E_REQUIRE(!bwd || g_disp[k], -1, "%s: disp%d is given and g_disp%d is NULL", who, k, k);
        DpScale& s = P.s[S++];
        s.d = disp[k];
        s.gd = bwd ? g_disp[k] : nullptr;
        s.h = hs[k];
        s.w = ws[k];
        s.ry = (float)hs[k] / (float)H;
        s.rx = (float)ws[k] / (float)W;
        s.fy = (float)H / (float)hs[k];
        s.fx = (float)W / (float)ws[k];
        s.lpp_shift = dp_lpp_shift(hs[k], ws[k], H, W);
    }
    E2E_REQUIRE(S > 0, -1, "%s: no scale present (disp0 .. disp3 are all NULL)", who);
    E2E_REQUIRE((int64_t)S * B <= 65535, -1, "%s: scales x B = %lld exceeds 65535", who, (long long)S * B);
    for (int k = S; k < DP_SCALES; ++k) P.s[k] = P.s[0];
    return S;
}

extern "C" {

int e2e_disp_pyramid_depth_fwd(const float* disp0, const float* disp1, const float* disp2, const float* disp3, int h0, int w0, int h1, int w1,
                               int h2, int w2, int h3, int w3, int B, int H, int W, float min_depth, float max_depth, float scale,
                               float* depth, void* stream) {
    E2E_REQUIRE(depth, E2E_ERR_ARG, "e2e_disp_pyramid_depth_fwd: depth is NULL");
    const float* disp[DP_SCALES] = {disp0, disp1, disp2, disp3};
    const int hs[DP_SCALES] = {h0, h1, h2, h3}, ws[DP_SCALES] = {w0, w1, w2, w3};
    DpParams P;
    const int S = dp_collect("e2e_disp_pyramid_depth_fwd", disp, nullptr, false, hs, ws, B, H, W, min_depth, max_depth, P);
    if (S < 0) return E2E_ERR_ARG;
    const float lo = (float)(1.0 / (double)max_depth), span = (float)(1.0 / (double)min_depth - 1.0 / (double)max_depth);
    const dim3 grid(e2e_ceil_div(W, DP_TILE_W), e2e_ceil_div(H, DP_TILE_H), S * B);
    hipLaunchKernelGGL(k_disp_pyramid_depth_fwd, grid, dim3(256), 0, (hipStream_t)stream, P, B, H, W, lo, span, scale, depth);
    E2E_LAUNCH_CHECK("e2e_disp_pyramid_depth_fwd");
    return E2E_OK;
}

int e2e_disp_pyramid_depth_bwd(const float* g_depth, const float* disp0, const float* disp1, const float* disp2, const float* disp3, int h0,
                               int w0, int h1, int w1, int h2, int w2, int h3, int w3, int B, int H, int W, float min_depth, float max_depth,
                               float scale, float* g_disp0, float* g_disp1, float* g_disp2, float* g_disp3, void* stream) {
    E2E_REQUIRE(g_depth, E2E_ERR_ARG, "e2e_disp_pyramid_depth_bwd: g_depth is NULL");
    const float* disp[DP_SCALES] = {disp0, disp1, disp2, disp3};
    float* g_disp[DP_SCALES] = {g_disp0, g_disp1, g_disp2, g_disp3};
    const int hs[DP_SCALES] = {h0, h1, h2, h3}, ws[DP_SCALES] = {w0, w1, w2, w3};
    DpParams P;
    const int S = dp_collect("e2e_disp_pyramid_depth_bwd", disp, g_disp, true, hs, ws, B, H, W, min_depth, max_depth, P);
    if (S < 0) return E2E_ERR_ARG;
    const float lo = (float)(1.0 / (double)max_depth), span = (float)(1.0 / (double)min_depth - 1.0 / (double)max_depth);
    int64_t blocks = 1;
    for (int k = 0; k < S; ++k) {
        const int64_t need = (((int64_t)P.s[k].h * P.s[k].w << P.s[k].lpp_shift) + 255) / 256;
        blocks = need > blocks ? need : blocks;
    }
    E2E_REQUIRE(blocks <= 0x7fffffffLL, E2E_ERR_ARG, "e2e_disp_pyramid_depth_bwd: %lld workgroups a plane exceed the grid", (long long)blocks);
    const dim3 grid((unsigned)blocks, 1, S * B);
    hipLaunchKernelGGL(k_disp_pyramid_depth_bwd, grid, dim3(256), 0, (hipStream_t)stream, P, B, H, W, lo, span, scale, g_depth);
    E2E_LAUNCH_CHECK("e2e_disp_pyramid_depth_bwd");
    return E2E_OK;
}

}  // extern "C"
