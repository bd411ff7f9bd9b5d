// warp_photo_tile.h -- what the 32x8 warp-photometric family shares: the pair (warp_photo.hip), its pose gradient (warp_photo_pose.hip) and
// the three-frame window with and without the geometric-consistency term (warp_photo_window.hip: one kernel template pair for both).  Tile
// constants, the SSIM device functions, the three-channel sample, the pair's host argument checks, the layout of the backward workspaces,
// the one host path of the pair's three backwards (warp_photo_bwd_run) with its operand struct, and the host launchers of the second
// stages, each of which lives in one file and serves the others.
// The device functions were MOVED here as they stood: a function that already exists compiles to the same instructions wherever it is
// defined (profiles/warp_family_refactor.txt: 0 differing lines in every tile kernel).  Arithmetic that is written out in a kernel is not
// extracted into new functions: that does reorder the kernel (profiles/lossgrad_tile_refactor.txt §3).
// Host functions have C++ linkage and are not part of the C ABI.
#pragma once
#include "e2e_common.h"

constexpr int TW = 32, TH = 8, NTHREADS = TW * TH;     // one thread per pixel, 4 wave64 per workgroup
constexpr int FP_LD = TW + 2;                          // forward planes: tile + 1-px halo, 34 floats a row (lanes read consecutive words)
constexpr int BP_LD = TW + 4;                          // backward image planes: tile + 2-px halo
constexpr int BG_LD = TW + 2;                          // backward statistics planes: tile + 1-px halo
constexpr int WP_NSUM = 12;                            // a 3x4 block: sum gc X^T (3x3) | sum gc (3x1), row-major
constexpr int WP_NQ = 9;                               // a 3x3 block: sum gc (d pix)^T, row-major (the intrinsics mode only)
constexpr float SSIM_C1 = 1e-4f, SSIM_C2 = 9e-4f;      // 0.01**2, 0.03**2  losses.py:20-21

// what a launch of the backward tile kernels leaves: the depth gradient, the depth gradient and the 12 pose sums, or ONLY the 9 sums Q for inv_K
enum { WP_SUMS_NONE = 0, WP_SUMS_POSE = 1, WP_SUMS_INTRINSICS = 2 };

// ---------------------------------------------------------------------------------------------
// SSIM statistics on an LDS plane.  xs/ys point at the window's top-left element, `ld` = row pitch.
// Summation order = avg_pool2d's (rows outer, columns inner), then /9 -- losses.py:27-32.
// ---------------------------------------------------------------------------------------------
struct Stats {
    float mux, muy, sxx, syy, sxy;
};
__device__ __forceinline__ Stats window_stats(const float* xs, const float* ys, int ld) {
    float sx = 0.f, sy = 0.f, sxx = 0.f, syy = 0.f, sxy = 0.f;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const float a = xs[dy * ld + dx], b = ys[dy * ld + dx];
            sx += a;
            sy += b;
            sxx += a * a;
            syy += b * b;
            sxy += a * b;
        }
    Stats s;
    s.mux = sx / 9.f;
    s.muy = sy / 9.f;
    s.sxx = sxx / 9.f;
    s.syy = syy / 9.f;
    s.sxy = sxy / 9.f;
    return s;
}

__device__ __forceinline__ float ssim_value(const Stats& s) {
    const float sigx = s.sxx - s.mux * s.mux;
    const float sigy = s.syy - s.muy * s.muy;
    const float sigxy = s.sxy - s.mux * s.muy;
    const float n = (2.f * s.mux * s.muy + SSIM_C1) * (2.f * sigxy + SSIM_C2);
    const float d = (s.mux * s.mux + s.muy * s.muy + SSIM_C1) * (sigx + sigy + SSIM_C2);
    return fminf(fmaxf((1.f - n / d) / 2.f, 0.f), 1.f);
}

// d(ssim_c)/d(mux, sxx, sxy) scaled by the upstream gradient g of ssim_c  
__device__ __forceinline__ void ssim_partials(const Stats& s, float g, float& G1, float& G2, float& G3) {
    const float sigx = s.sxx - s.mux * s.mux;
    const float sigy = s.syy - s.muy * s.muy;
    const float sigxy = s.sxy - s.mux * s.muy;
    const float A1 = 2.f * s.mux * s.muy + SSIM_C1, A2 = 2.f * sigxy + SSIM_C2;
    const float B1 = s.mux * s.mux + s.muy * s.muy + SSIM_C1, B2 = sigx + sigy + SSIM_C2;
    const float S = (A1 * A2) / (B1 * B2);
    const float t = (1.f - S) / 2.f;
    const float gS = (t >= 0.f && t <= 1.f) ? -0.5f * g : 0.f;   // clamp passes grad on the closed interval
    const float inv = 1.f / (B1 * B2);
    G1 = gS * (2.f * s.muy * (A2 - A1) * inv - S * 2.f * s.mux * (1.f / B1 - 1.f / B2));
    G2 = gS * (-S / B2);
    G3 = gS * (2.f * A1 * inv);
}

// bilinear sample of three channels at one position
__device__ __forceinline__ void sample3(const float* __restrict__ base, const e2e_strides& s, const Bilin& bl, float* out) {
    const float* p = base + bl.y0 * s.sh + bl.x0 * s.sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* pc = p + c * s.sc;
        float acc = 0.f;
        if (bl.in_y0 & bl.in_x0) acc += pc[0] * bl.wnw;
        if (bl.in_y0 & bl.in_x1) acc += pc[s.sw] * bl.wne;
        if (bl.in_y1 & bl.in_x0) acc += pc[s.sh] * bl.wsw;
        if (bl.in_y1 & bl.in_x1) acc += pc[s.sh + s.sw] * bl.wse;
        out[c] = acc;
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static inline dim3 tile_grid(int B, int H, int W) { return dim3(e2e_ceil_div(W, TW), e2e_ceil_div(H, TH), B); }
static inline int64_t tile_count(int H, int W) { return (int64_t)e2e_ceil_div(W, TW) * e2e_ceil_div(H, TH); }     // tiles per batch element

// the argument checks of e2e_warp_photo_fwd and of the three backwards (`name` = the entry point; the messages are part of the interface)
static int warp_photo_check_args(const char* name, int B, int H, int W, bool pointers, int padding_mode, int reg_kind, bool reg_buffers) {
    E2E_REQUIRE(B > 0 && H > 1 && W > 1 && (int64_t)B * H * W < (1ll << 31), E2E_ERR_ARG, "%s: bad dims B=%d H=%d W=%d", name, B, H, W);
    E2E_REQUIRE(pointers, E2E_ERR_ARG, "%s: null pointer", name);
    E2E_REQUIRE(padding_mode == E2E_PADDING_BORDER || padding_mode == E2E_PADDING_ZEROS, E2E_ERR_ARG,
                "%s: padding_mode %d not supported (zeros|border)", name, padding_mode);
    E2E_REQUIRE(reg_kind >= 0 && reg_kind <= 2, E2E_ERR_ARG, "%s: reg_kind %d (0 none, 1 l1, 2 l2)", name, reg_kind);
    E2E_REQUIRE(!reg_kind || reg_buffers, E2E_ERR_ARG, "%s: regulariser buffers missing", name);
    return E2E_OK;
}

// E2E_LAUNCH_CHECK for a host path that serves several entry points: `stage` = "" or the "(stage)" that follows the entry point's name
static inline int warp_photo_launch_status(const char* name, const char* stage) {
    char what[96];                                     // the longest entry-point name with its stage has 49 characters
    snprintf(what, sizeof what, "%s%s", name, stage);
    E2E_LAUNCH_CHECK(what);
    return E2E_OK;
}

// The backward workspace of the whole family, for the *_workspace_bytes queries and the host paths alike, in 8-byte words: `fixed` words of
// fixed-point scratch (the geometric forms; 0 elsewhere), then the float64 pose sums [S][B][tiles][12], then, with WP_SUMS_INTRINSICS only,
// the float64 sums Q [S][B][tiles][9] (k_warp_photo_window_bwd finds this region by the same expression).  S = 1 for the pair.
struct WarpPhotoBwdWorkspace {
    int64_t partials, q_partials, words;               // where the two regions of sums begin, and the size
};
static inline WarpPhotoBwdWorkspace warp_photo_bwd_workspace(int64_t fixed, int sums, int S, int B, int H, int W) {
    const int64_t n = (int64_t)S * B * tile_count(H, W);
    return {fixed, fixed + n * WP_NSUM, fixed + n * WP_NSUM + (sums == WP_SUMS_INTRINSICS ? n * WP_NQ : 0)};
}

// what e2e_warp_photo_bwd, _bwd_pose and _bwd_intrinsics share, under the parameter names of include/e2eslam.h (host only: never a kernel
// argument -- that would change every kernarg layout, profiles/lossgrad_tile_refactor.txt)
struct WarpPhotoBwdArgs {
    const float *depth_tgt, *src;
    e2e_strides src_strides;
    const float* tgt;
    e2e_strides tgt_strides;
    const float *K, *inv_K, *T, *synth, *valid;
    int use_mask, padding_mode, reg_kind;
    const float *reg_init_tgt, *reg_init_src, *depth_src, *g_loss;
    float *g_depth_tgt, *g_depth_src;
    int B, H, W;
};

// The pair's backward, whole (warp_photo.hip, where k_warp_photo_bwd lives): the checks of the mode under the entry point's `name`, then the
// tile launch; WP_SUMS_POSE (g_T, workspace required) leaves partials[(b * tiles + tile) * 12 + r * 4 + j] and runs the pose final;
// WP_SUMS_INTRINSICS (g_K, g_inv_K, workspace required) adds a pass that stores only q_partials[(b * tiles + tile) * 9 + r * 3 + j] = sum gc_r d pix_j.
int warp_photo_bwd_run(const char* name, int sums, const WarpPhotoBwdArgs& a, float* g_T, float* g_K, float* g_inv_K, void* workspace,
                       hipStream_t stream);

// k_reduce_partials (warp_photo.hip): out[s] = scale * the fixed-order float64 sum of partials[s * nblk .. (s + 1) * nblk), s < nsets
void warp_photo_reduce_launch(const float* partials, int nblk, int nsets, float scale, float* out, hipStream_t stream);

// k_warp_photo_bwd_intrinsics_final (warp_photo_intrinsics.hip): g_K[b] and g_inv_K[b] from the fixed-order sums over the tiles of
// partials[((s * B + b) * tiles + tile) * 12 ..] and q_partials[((s * B + b) * tiles + tile) * 9 ..], the sources added in the order 0, 1;
// T is (S,B,4,4), K (B,4,4); S = 1 for the pair
void warp_photo_intrinsics_final_launch(const double* partials, const double* q_partials, int tiles, const float* K, const float* T, float* g_K,
                                        float* g_inv_K, int S, int B, hipStream_t stream);

// k_warp_photo_bwd_pose_final (warp_photo_pose.hip): g_T[(s * B + b) * 16 ..] = K_b^T times the fixed-order sum over the tiles of
// partials[((s * B + b) * tiles + tile) * 12 ..]; S = 1 for the pair
void warp_photo_pose_final_launch(const double* partials, int tiles, const float* K, float* g_T, int S, int B, hipStream_t stream);
