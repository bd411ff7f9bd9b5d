// warp_photo_pose.hip -- the fused warp-photometric backward with the gradient with respect to the relative pose T (DATA.use_gt_pose: False:
// the photometric loss is differentiated through the pose, train_depth.py:381-382, :395).  The per-pixel work is k_warp_photo_bwd<pad, POSE>
// of warp_photo.hip, which already forms the adjoint (gc0, gc1, gc2) of the projected point on its way to g_depth_tgt; with POSE it also
// leaves Pbar = sum gc X^T | sum gc per workgroup as 12 float64 sums.  Here: the entry point, which fills the operand struct and calls the
// pair's one backward path (warp_photo_bwd_run, warp_photo.hip), and the second stage that folds the workgroups' sums per batch element in
// a fixed order and applies K^T, as k_project3d_bwd_T_final (pose_grad.hip) does for the operator.
// The three-frame window, with or without the geometric-consistency term (k_warp_photo_window_bwd<pad, POSE, GEO> of warp_photo_window.hip),
// runs the same second stage with one grid row per source.
// No atomics anywhere: bitwise reproducible run to run.
#include "e2e_common.h"
#include "warp_photo_tile.h"

// grid (B, S): wave w of workgroup (b, s) folds sum w of source s and batch element b: lane l adds the tiles l, l + 64, ... in order, then a
// fixed shuffle tree; then g_T[k][j] = sum_{i<3} K[i][k] Pbar[i][j], k = 0..3 (T enters through P = (K T)[:3,:] only).  K is per batch element.
__global__ __launch_bounds__(WP_NSUM * 64) void k_warp_photo_bwd_pose_final(const double* __restrict__ partials, int tiles, const float* __restrict__ K,
                                                                            float* __restrict__ g_T) {
    __shared__ double Pb[WP_NSUM];
    const int b = blockIdx.x, sb = blockIdx.y * gridDim.x + b, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int i = lane; i < tiles; i += 64) s += partials[((int64_t)sb * tiles + i) * WP_NSUM + w];
    s = wave_sum_d(s);
    if (lane == 0) Pb[w] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int k = threadIdx.x >> 2, j = threadIdx.x & 3;
        double v = 0.0;
        for (int i = 0; i < 3; ++i) v += (double)K[b * 16 + i * 4 + k] * Pb[i * 4 + j];
        g_T[sb * 16 + threadIdx.x] = (float)v;
    }
}

void warp_photo_pose_final_launch(const double* partials, int tiles, const float* K, float* g_T, int S, int B, hipStream_t stream) {
    hipLaunchKernelGGL(k_warp_photo_bwd_pose_final, dim3(B, S), dim3(WP_NSUM * 64), 0, stream, partials, tiles, K, g_T);
}

extern "C" {

int64_t e2e_warp_photo_bwd_pose_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return warp_photo_bwd_workspace(0, WP_SUMS_POSE, 1, B, H, W).words * 8;
}

int e2e_warp_photo_bwd_pose(const float* depth_tgt, const float* src, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                            const float* K, const float* inv_K, const float* T, const float* synth, const float* valid, int use_mask,
                            int padding_mode, int reg_kind, const float* reg_init_tgt, const float* reg_init_src, const float* depth_src,
                            const float* g_loss, float* g_depth_tgt, float* g_depth_src, float* g_T, void* workspace, int B, int H, int W,
                            void* stream) {
    const WarpPhotoBwdArgs a{depth_tgt, src, src_strides, tgt, tgt_strides, K, inv_K, T, synth, valid, use_mask, padding_mode, reg_kind,
                             reg_init_tgt, reg_init_src, depth_src, g_loss, g_depth_tgt, g_depth_src, B, H, W};
    return warp_photo_bwd_run("e2e_warp_photo_bwd_pose", WP_SUMS_POSE, a, g_T, nullptr, nullptr, workspace, (hipStream_t)stream);
}

}  // extern "C"
