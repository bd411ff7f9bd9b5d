// normal_maps_grad.hip -- the adjoint of the normal map of k_vertex_normal_maps (pointfusion.hip) with respect to the depth, for gfx950.
// The differentiation rule is stated in include/e2eslam.h (e2e_normal_maps_bwd).
#include "e2e_common.h"
#include "pf_workspace.h"

// ---------------------------------------------------------------------------------------------
// normals.  The adjoint of k_vertex_normal_maps's normal expressions with respect to the depth (rule in include/e2eslam.h), as a gather:
// the thread of pixel j collects what reaches V_j from its three contributors -- j itself (-(g_dh + g_dv)), (h, w-1) whose right
// neighbour it is (g_dh) and (h-1, w) whose lower neighbour it is (g_dv) -- recomputing each contributor's cross-product adjoint from
// its three depths and its gn.  Float64 per pixel, rounded once on the store: 1 / nrm and V_{p+1} - V_p cancel digits in float32.
// No implicit FMA: a b - b a must be exactly 0 where the forward's is (dh == dv, or a zero difference), or 1 / nrm of a rounding
// residue would follow.  Hence a file of its own, built with -ffp-contract=off like pointfusion.hip (csrc/build.py).
// ---------------------------------------------------------------------------------------------
struct NmGeom {
    double kx, kxc, ky, kyc;
    double R[9];
    int H, W;
};

__device__ __forceinline__ void nm_vertex(const NmGeom& G, float d, int h, int w, double* V) {
    const double dd = (double)d;                            // (d == 0 gives the zero row of the forward)
    V[0] = (G.kx * (double)w + G.kxc) * dd;
    V[1] = (G.ky * (double)h + G.kyc) * dd;
    V[2] = dd;
}

// g_dh, g_dv of pixel p = (h, w) (index i of its image): 0 for an invalid pixel, and 0 for the difference that the forward holds at
// the constant 0 (last column / last row).
__device__ __forceinline__ void nm_cross_adjoint(const NmGeom& G, const float* __restrict__ dep, const float* __restrict__ gNm,
                                                 const float* __restrict__ gNg, int h, int w, int i, double* gdh, double* gdv) {
    gdh[0] = gdh[1] = gdh[2] = 0.0;
    gdv[0] = gdv[1] = gdv[2] = 0.0;
    const float d = dep[i];
    if (d == 0.f) return;
    const bool has_r = w + 1 < G.W, has_d = h + 1 < G.H;
    if (!has_r && !has_d) return;
    double v0[3], v1[3], dh[3] = {0.0, 0.0, 0.0}, dv[3] = {0.0, 0.0, 0.0};
    nm_vertex(G, d, h, w, v0);
    if (has_r) {
        nm_vertex(G, dep[i + 1], h, w + 1, v1);
#pragma unroll
        for (int c = 0; c < 3; ++c) dh[c] = v1[c] - v0[c];
    }
    if (has_d) {
        nm_vertex(G, dep[i + G.W], h + 1, w, v1);
#pragma unroll
        for (int c = 0; c < 3; ++c) dv[c] = v1[c] - v0[c];
    }
    double gn[3] = {0.0, 0.0, 0.0};
    if (gNm) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gn[c] = (double)gNm[(int64_t)i * 3 + c];
    }
    if (gNg) {                                              // Ng = R n: gn += R^T g_Ng
        const double g0 = (double)gNg[(int64_t)i * 3], g1 = (double)gNg[(int64_t)i * 3 + 1], g2 = (double)gNg[(int64_t)i * 3 + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) gn[c] += (G.R[c] * g0 + G.R[3 + c] * g1) + G.R[6 + c] * g2;
    }
    double cr[3];
    cr[0] = dh[1] * dv[2] - dh[2] * dv[1];
    cr[1] = dh[2] * dv[0] - dh[0] * dv[2];
    cr[2] = dh[0] * dv[1] - dh[1] * dv[0];
    const double nrm = sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2]);
    double gc[3];
    if (nrm != 0.0) {
        const double nh[3] = {cr[0] / nrm, cr[1] / nrm, cr[2] / nrm};
        const double t = (nh[0] * gn[0] + nh[1] * gn[1]) + nh[2] * gn[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) gc[c] = (gn[c] - nh[c] * t) / nrm;
    } else {                                                // the forward divides by the constant 1 there
#pragma unroll
        for (int c = 0; c < 3; ++c) gc[c] = gn[c];
    }
    if (has_r) {                                            // g_dh = dv x gc
        gdh[0] = dv[1] * gc[2] - dv[2] * gc[1];
        gdh[1] = dv[2] * gc[0] - dv[0] * gc[2];
        gdh[2] = dv[0] * gc[1] - dv[1] * gc[0];
    }
    if (has_d) {                                            // g_dv = gc x dh
        gdv[0] = gc[1] * dh[2] - gc[2] * dh[1];
        gdv[1] = gc[2] * dh[0] - gc[0] * dh[2];
        gdv[2] = gc[0] * dh[1] - gc[1] * dh[0];
    }
}

__global__ __launch_bounds__(PF_T) void k_normal_maps_bwd(const float* __restrict__ depth, const float* __restrict__ K,
                                                          const float* __restrict__ pose, const float* __restrict__ gNm,
                                                          const float* __restrict__ gNg, float* __restrict__ g_depth, int accumulate,
                                                          int H, int W) {
    const int b = blockIdx.y;
    const int N = H * W;
    const float* Kb = K + b * 16;
    const float fx = Kb[0], fy = Kb[5], cx = Kb[2], cy = Kb[6];
    const float kx = 1.0f / fx, ky = 1.0f / fy, kxc = -cx / fx, kyc = -cy / fy;     // as k_vertex_normal_maps: fp32, then widened
    NmGeom G;
    G.kx = kx; G.kxc = kxc; G.ky = ky; G.kyc = kyc; G.H = H; G.W = W;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G.R[r * 3 + c] = (double)pose[b * 16 + r * 4 + c];
    const float* dep = depth + (int64_t)b * N;
    const float* gm = gNm ? gNm + (int64_t)b * N * 3 : nullptr;
    const float* gg = gNg ? gNg + (int64_t)b * N * 3 : nullptr;
    float* out = g_depth + (int64_t)b * N;
    for (int j = blockIdx.x * PF_T + threadIdx.x; j < N; j += gridDim.x * PF_T) {
        const int h = j / W, w = j - h * W;
        const float d = dep[j];
        if (d == 0.f) {                                     // vf_j = 0: exactly 0, or the prior value
            if (!accumulate) out[j] = 0.f;
            continue;
        }
        double gV[3], a[3], c[3];
        nm_cross_adjoint(G, dep, gm, gg, h, w, j, a, c);
#pragma unroll
        for (int k = 0; k < 3; ++k) gV[k] = -(a[k] + c[k]);
        if (w > 0) {
            nm_cross_adjoint(G, dep, gm, gg, h, w - 1, j - 1, a, c);
#pragma unroll
            for (int k = 0; k < 3; ++k) gV[k] += a[k];
        }
        if (h > 0) {
            nm_cross_adjoint(G, dep, gm, gg, h - 1, w, j - W, a, c);
#pragma unroll
            for (int k = 0; k < 3; ++k) gV[k] += c[k];
        }
        const double g = ((G.kx * (double)w + G.kxc) * gV[0] + (G.ky * (double)h + G.kyc) * gV[1]) + gV[2];
        out[j] = accumulate ? (float)((double)out[j] + g) : (float)g;
    }
}

extern "C" {

int e2e_normal_maps_bwd(const float* depth, const float* K, const float* pose, const float* g_Nm, const float* g_Ng, float* g_depth,
                        int accumulate, int B, int H, int W, void* stream) {
    E2E_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)B * H * W * 3 < (1ll << 31), E2E_ERR_ARG, "e2e_normal_maps_bwd: bad dims");
    E2E_REQUIRE(depth && K && pose && g_depth, E2E_ERR_ARG, "e2e_normal_maps_bwd: null pointer");
    E2E_REQUIRE(g_Nm || g_Ng, E2E_ERR_ARG, "e2e_normal_maps_bwd: no gradient given (g_Nm and g_Ng are both NULL)");
    const int64_t blocks = ((int64_t)H * W + PF_T - 1) / PF_T;
    const int grid = (int)(blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(k_normal_maps_bwd, dim3(grid, B), dim3(PF_T), 0, (hipStream_t)stream, depth, K, pose, g_Nm, g_Ng,
                       g_depth, accumulate != 0, H, W);
    E2E_LAUNCH_CHECK("e2e_normal_maps_bwd");
    return E2E_OK;
}

}  // extern "C"
