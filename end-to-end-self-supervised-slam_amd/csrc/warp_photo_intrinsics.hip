// warp_photo_intrinsics.hip -- the gradient with respect to the camera intrinsics K and inv_K: self-calibration through the photometric loss
// (a focal length that does not match the data is what the reference's scale_by_f / normalize_intrinsics / pretrained_focal exist for).
//
// The fused forms.  The per-pixel work is the tile kernels' (k_warp_photo_bwd<pad, WP_SUMS_INTRINSICS> of warp_photo.hip,
// k_warp_photo_window_bwd<pad, WP_SUMS_INTRINSICS, GEO> of warp_photo_window.hip): with c = P [X;1], P = (K T)[:3,:], X = d cam,
// cam = inv_K[:3,:3] pix, pix = (x, y, 1) and (gc0, gc1, gc2) the fp32 adjoint of c that reaches g_depth_tgt, they leave per workgroup
//     Pbar[i][j] = sum gc_i X_j (j < 3) | sum gc_i (j = 3)      the 12 pose sums, where e2e_warp_photo_bwd_pose leaves them
//     Q[i][j]    = sum gc_i d pix_j                             9 sums more, in a second region behind the first
// in float64.  K enters through rows 0..2 of K T only, inv_K through its upper-left 3x3 only, so
//     g_K[i][k]     = sum_s sum_{j<4} Pbar_s[i][j] T_s[k][j]     i < 3, k < 4; row 3 is 0
//     g_inv_K[r][j] = sum_s sum_{i<3} P_s[i][r] Q_s[i][j]        r, j < 3; row 3 and column 3 are 0
// with P_s formed in float64 from the fp32 K and T_s and the sources added in the order 0, 1.  Pbar comes from the pose instantiation's own
// launch, Q from a second pass of the tile kernel that stores nothing else (why two passes: the comment of k_warp_photo_bwd).  Here: the
// second stage that folds the workgroups' sums in a fixed order and applies the two formulas, and the pair's entry point, which fills the
// operand struct and calls the pair's one backward path (warp_photo_bwd_run, warp_photo.hip).
// k_warp_photo_bwd_pose_final runs unchanged on the first region, so g_T has the bits of e2e_warp_photo_bwd_pose.
//
// The operator forms.  e2e_project3d_bwd_k (the K half of Project3D's adjoint, next to e2e_project3d_bwd_t) and e2e_backproject_bwd_invk
// (the inv_K half of BackprojectDepth's): per-workgroup float64 partial sums, then one wave per sum.
// No atomics anywhere: bitwise reproducible run to run.
#include "e2e_common.h"
#include "warp_photo_tile.h"

namespace {

constexpr int IN_NW = 16;                                // waves of the fused second stage
constexpr int IN_NALL = WP_NSUM + WP_NQ;                 // 21 sums per source
constexpr int IN_MAX_S = 2;
constexpr int OP_T = 256, OP_MAX_PARTS = 256;            // the operator forms: threads per workgroup, workgroups per batch element at most

// one workgroup per batch element.  Wave w folds the sums w, w + 16, ... of (source, sum): lane l adds the tiles l, l + 64, ... in order, then
// a fixed shuffle tree.  Then 16 threads write g_K[b] and 16 write g_inv_K[b], all 16 entries of each.
__global__ __launch_bounds__(IN_NW * 64) void k_warp_photo_bwd_intrinsics_final(const double* __restrict__ partials, const double* __restrict__ q_partials,
                                                                                int tiles, const float* __restrict__ K, const float* __restrict__ T,
                                                                                float* __restrict__ g_K, float* __restrict__ g_inv_K, int S, int B) {
    __shared__ double sums[IN_MAX_S][IN_NALL];
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = w; k < S * IN_NALL; k += IN_NW) {       // wave-uniform
        const int s = k / IN_NALL, q = k % IN_NALL;
        const int64_t sb = (int64_t)s * B + b;
        const double* p = q < WP_NSUM ? partials + sb * tiles * WP_NSUM + q : q_partials + sb * tiles * WP_NQ + (q - WP_NSUM);
        const int ld = q < WP_NSUM ? WP_NSUM : WP_NQ;
        double a = 0.0;
        for (int i = lane; i < tiles; i += 64) a += p[(int64_t)i * ld];
        a = wave_sum_d(a);
        if (lane == 0) sums[s][q] = a;
    }
    __syncthreads();
    if (threadIdx.x < 16) {                              // g_K[i][k] = sum_s sum_j Pbar_s[i][j] T_s[k][j]
        const int i = threadIdx.x >> 2, k = threadIdx.x & 3;
        double v = 0.0;
        if (i < 3)
            for (int s = 0; s < S; ++s)
                for (int j = 0; j < 4; ++j) v += sums[s][i * 4 + j] * (double)T[((int64_t)s * B + b) * 16 + k * 4 + j];
        g_K[b * 16 + threadIdx.x] = (float)v;
    } else if (threadIdx.x >= 64 && threadIdx.x < 80) {  // g_inv_K[r][j] = sum_s sum_i P_s[i][r] Q_s[i][j]
        const int e = threadIdx.x - 64, r = e >> 2, j = e & 3;
        double v = 0.0;
        if (r < 3 && j < 3)
            for (int s = 0; s < S; ++s)
                for (int i = 0; i < 3; ++i) {
                    double P = 0.0;                      // P_s[i][r] = sum_k K[i][k] T_s[k][r]
                    for (int k = 0; k < 4; ++k) P += (double)K[b * 16 + i * 4 + k] * (double)T[((int64_t)s * B + b) * 16 + k * 4 + r];
                    v += P * sums[s][WP_NSUM + i * 3 + j];
                }
        g_inv_K[b * 16 + e] = (float)v;
    }
}

// the workgroup's NS float64 sums, the four waves in order -> out[NS]; every thread of the OP_T-thread workgroup calls it
template <int NS>
__device__ __forceinline__ void op_block_partials(const double* acc, double* __restrict__ out) {
    __shared__ double sh[NS][OP_T / 64];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double v = wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NS; ++k) out[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
    }
}

// Project3D's adjoint of the projected point, exactly as k_project3d_bwd (warp_photo.hip) forms it; Pbar = sum gc p^T over the workgroup's
// pixels -> partials[(b * parts + part) * 12 + r * 4 + j]
__global__ __launch_bounds__(OP_T) void k_project3d_bwd_K_partials(const float* __restrict__ pts, const float* __restrict__ K, const float* __restrict__ T,
                                                                   const float* __restrict__ ggrid, const float* __restrict__ gz, int H, int W,
                                                                   double* __restrict__ partials) {
    const int N = H * W;
    const int b = blockIdx.y;
    float P[12];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) s = fmaf(K[b * 16 + i * 4 + k], T[b * 16 + k * 4 + j], s);
            P[i * 4 + j] = s;
        }
    double acc[WP_NSUM];
#pragma unroll
    for (int k = 0; k < WP_NSUM; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * OP_T + threadIdx.x; i < N; i += gridDim.x * OP_T) {
        const float* p = pts + (int64_t)b * 4 * N + i;
        const float pv[4] = {p[0], p[N], p[(int64_t)2 * N], p[(int64_t)3 * N]};
        float c[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            c[r] = fmaf(P[r * 4 + 0], pv[0], fmaf(P[r * 4 + 1], pv[1], fmaf(P[r * 4 + 2], pv[2], P[r * 4 + 3] * pv[3])));
        const float z = c[2] + 1e-7f;
        const float u = c[0] / z, v = c[1] / z;
        const int64_t o = (int64_t)b * N + i;
        const float gu = ggrid[o * 2 + 0] * 2.f / (float)(W - 1);
        const float gv = ggrid[o * 2 + 1] * 2.f / (float)(H - 1);
        float gc[3];
        gc[0] = gu / z;
        gc[1] = gv / z;
        gc[2] = -(gu * u + gv * v) / z;
        if (gz && c[2] > 1e-3f) gc[2] += gz[o];     // clamp(min=1e-3) passes gradient above the bound
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[r * 4 + j] += (double)gc[r] * (double)pv[j];
    }
    op_block_partials<WP_NSUM>(acc, partials + ((int64_t)b * gridDim.x + blockIdx.x) * WP_NSUM);
}

// wave w of workgroup b folds sum w of batch element b; then g_K[i][k] = sum_j Pbar[i][j] T[k][j], row 3 zero
__global__ __launch_bounds__(WP_NSUM * 64) void k_project3d_bwd_K_final(const double* __restrict__ partials, int nparts, const float* __restrict__ T,
                                                                        float* __restrict__ g_K) {
    __shared__ double Pb[WP_NSUM];
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int i = lane; i < nparts; i += 64) s += partials[((int64_t)b * nparts + i) * WP_NSUM + w];
    s = wave_sum_d(s);
    if (lane == 0) Pb[w] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int i = threadIdx.x >> 2, k = threadIdx.x & 3;
        double v = 0.0;
        if (i < 3)
            for (int j = 0; j < 4; ++j) v += Pb[i * 4 + j] * (double)T[b * 16 + k * 4 + j];
        g_K[b * 16 + threadIdx.x] = (float)v;
    }
}

// BackprojectDepth: cam_r = depth (inv_K[r][:3] . pix), so g_inv_K[r][j] = sum g_cam[r] depth pix_j -> partials[(b * parts + part) * 9 + r * 3 + j]
__global__ __launch_bounds__(OP_T) void k_backproject_bwd_invK_partials(const float* __restrict__ gcam, const float* __restrict__ depth, int H, int W,
                                                                        double* __restrict__ partials) {
    const int N = H * W;
    const int b = blockIdx.y;
    double acc[WP_NQ];
#pragma unroll
    for (int k = 0; k < WP_NQ; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * OP_T + threadIdx.x; i < N; i += gridDim.x * OP_T) {
        const double pix[3] = {(double)(i % W), (double)(i / W), 1.0};
        const double d = (double)depth[(int64_t)b * N + i];
        const float* g = gcam + (int64_t)b * 4 * N + i;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double gd = (double)g[(int64_t)r * N] * d;
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[r * 3 + j] += gd * pix[j];
        }
    }
    op_block_partials<WP_NQ>(acc, partials + ((int64_t)b * gridDim.x + blockIdx.x) * WP_NQ);
}

__global__ __launch_bounds__(WP_NQ * 64) void k_backproject_bwd_invK_final(const double* __restrict__ partials, int nparts, float* __restrict__ g_inv_K) {
    __shared__ double Qb[WP_NQ];
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int i = lane; i < nparts; i += 64) s += partials[((int64_t)b * nparts + i) * WP_NQ + w];
    s = wave_sum_d(s);
    if (lane == 0) Qb[w] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int r = threadIdx.x >> 2, j = threadIdx.x & 3;
        g_inv_K[b * 16 + threadIdx.x] = (r < 3 && j < 3) ? (float)Qb[r * 3 + j] : 0.f;
    }
}

inline int op_parts(int64_t n) {
    const int64_t g = (n + OP_T - 1) / OP_T;
    return (int)(g > OP_MAX_PARTS ? OP_MAX_PARTS : g);
}

}  // namespace

void warp_photo_intrinsics_final_launch(const double* partials, const double* q_partials, int tiles, const float* K, const float* T, float* g_K,
                                        float* g_inv_K, int S, int B, hipStream_t stream) {
    hipLaunchKernelGGL(k_warp_photo_bwd_intrinsics_final, dim3(B), dim3(IN_NW * 64), 0, stream, partials, q_partials, tiles, K, T, g_K, g_inv_K, S, B);
}

extern "C" {

int64_t e2e_warp_photo_bwd_intrinsics_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return warp_photo_bwd_workspace(0, WP_SUMS_INTRINSICS, 1, B, H, W).words * 8;
}

int e2e_warp_photo_bwd_intrinsics(const float* depth_tgt, const float* src, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                                  const float* K, const float* inv_K, const float* T, const float* synth, const float* valid, int use_mask,
                                  int padding_mode, int reg_kind, const float* reg_init_tgt, const float* reg_init_src, const float* depth_src,
                                  const float* g_loss, float* g_depth_tgt, float* g_depth_src, float* g_T, float* g_K, float* g_inv_K,
                                  void* workspace, int B, int H, int W, void* stream) {
    const WarpPhotoBwdArgs a{depth_tgt, src, src_strides, tgt, tgt_strides, K, inv_K, T, synth, valid, use_mask, padding_mode, reg_kind,
                             reg_init_tgt, reg_init_src, depth_src, g_loss, g_depth_tgt, g_depth_src, B, H, W};
    return warp_photo_bwd_run("e2e_warp_photo_bwd_intrinsics", WP_SUMS_INTRINSICS, a, g_T, g_K, g_inv_K, workspace, (hipStream_t)stream);
}

int64_t e2e_project3d_bwd_k_workspace_bytes(int B) { return B > 0 ? (int64_t)B * OP_MAX_PARTS * WP_NSUM * 8 : 0; }

int e2e_project3d_bwd_k(const float* points, const float* K, const float* T, const float* g_grid, const float* g_z, float* g_K, void* workspace,
                        int B, int H, int W, void* stream) {
    E2E_REQUIRE(B > 0 && H > 1 && W > 1 && (int64_t)B * H * W < (1ll << 31), E2E_ERR_ARG, "e2e_project3d_bwd_k: bad dims B=%d H=%d W=%d", B, H, W);
    E2E_REQUIRE(B <= 65535, E2E_ERR_ARG, "e2e_project3d_bwd_k: B=%d exceeds the grid", B);
    E2E_REQUIRE(points && K && T && g_grid && g_K && workspace, E2E_ERR_ARG, "e2e_project3d_bwd_k: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int parts = op_parts((int64_t)H * W);
    hipLaunchKernelGGL(k_project3d_bwd_K_partials, dim3(parts, B), dim3(OP_T), 0, st, points, K, T, g_grid, g_z, H, W, (double*)workspace);
    hipLaunchKernelGGL(k_project3d_bwd_K_final, dim3(B), dim3(WP_NSUM * 64), 0, st, (const double*)workspace, parts, T, g_K);
    E2E_LAUNCH_CHECK("e2e_project3d_bwd_k");
    return E2E_OK;
}

int64_t e2e_backproject_bwd_invk_workspace_bytes(int B) { return B > 0 ? (int64_t)B * OP_MAX_PARTS * WP_NQ * 8 : 0; }

int e2e_backproject_bwd_invk(const float* g_cam, const float* depth, float* g_inv_K, void* workspace, int B, int H, int W, void* stream) {
    E2E_REQUIRE(B > 0 && H > 1 && W > 1 && (int64_t)B * H * W < (1ll << 31), E2E_ERR_ARG, "e2e_backproject_bwd_invk: bad dims B=%d H=%d W=%d", B, H,
                W);
    E2E_REQUIRE(B <= 65535, E2E_ERR_ARG, "e2e_backproject_bwd_invk: B=%d exceeds the grid", B);
    E2E_REQUIRE(g_cam && depth && g_inv_K && workspace, E2E_ERR_ARG, "e2e_backproject_bwd_invk: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int parts = op_parts((int64_t)H * W);
    hipLaunchKernelGGL(k_backproject_bwd_invK_partials, dim3(parts, B), dim3(OP_T), 0, st, g_cam, depth, H, W, (double*)workspace);
    hipLaunchKernelGGL(k_backproject_bwd_invK_final, dim3(B), dim3(WP_NQ * 64), 0, st, (const double*)workspace, parts, g_inv_K);
    E2E_LAUNCH_CHECK("e2e_backproject_bwd_invk");
    return E2E_OK;
}

}  // extern "C"
