// pose_grad.hip -- the per-point halves of the ADJOINT of the odometry (differentiable ICP / GradICP) and of the two
// operators that consume a pose (Project3D, transform_pointcloud) with respect to the 4x4 transform.  The reference differentiates the
// photometric loss through the pose into the live frame's depth (train_depth.py:381-382, :395 with DATA.use_gt_pose: False); the 6x6
// algebra of that adjoint is float64 on the host (e2ehip/icp.py), as the forward's is.
// Sums are float64 with a fixed order (per-thread -> wave shuffle -> per-workgroup partials -> one wave per sum), no atomics: bitwise
// reproducible run to run.
#include "e2e_common.h"

#define PG_T 256
#define PG_MAX_PARTS 256
#define PG_NSUM 12           // a 3x4 block: sum g p^T (3x3) | sum g (3x1), row-major

// ---------------------------------------------------------------------------------------------
// adjoint of k_icp_partials (icp.hip) wrt the source points.  adj[0..20]: adjoints of the packed upper triangle of A^T A, adj[21..26]:
// of A^T b, adj[27]: of sum b^2.  With M = U + U^T (U the upper-triangular unpacking of adj[0..20]; the diagonal counts twice because
// a_r a_r has both factors), Abar = M A + b gbar, bbar = gbar . A + 2 ebar b, and A = [n, s x n], b = n . (t - s):
//   sbar = -bbar n + n x Abar[3:6].
// Rows the forward skipped (dists >= thresh^2) and rows whose index is outside [0, n_tgt) get zero and read nothing of the target.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PG_T) void k_icp_ne_bwd(const float* __restrict__ src, const float* __restrict__ tgt, const float* __restrict__ tgt_n,
                                                     int64_t n_tgt, const long long* __restrict__ idx, const float* __restrict__ dists,
                                                     float thresh_sq, const double* __restrict__ adj, int64_t n, float* __restrict__ g_src,
                                                     int accumulate) {
    __shared__ double M[36], gb[6], eb;
    if (threadIdx.x < 36) {
        const int r = threadIdx.x / 6, c = threadIdx.x % 6;
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const int k = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);          // packed index of (lo, hi), lo <= hi
        M[threadIdx.x] = (r == c ? 2.0 : 1.0) * adj[k];
    } else if (threadIdx.x < 42) {
        gb[threadIdx.x - 36] = adj[21 + threadIdx.x - 36];
    } else if (threadIdx.x == 42) {
        eb = adj[27];
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PG_T) {
        double sb[3] = {0.0, 0.0, 0.0};
        const long long j = idx[i];
        const bool keep = (thresh_sq < 0.f || dists[i] < thresh_sq) && j >= 0 && j < n_tgt;
        if (keep) {
            const double s[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
            const double t[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
            const double nn[3] = {tgt_n[j * 3], tgt_n[j * 3 + 1], tgt_n[j * 3 + 2]};
            const double a[6] = {nn[0], nn[1], nn[2], s[1] * nn[2] - s[2] * nn[1], s[2] * nn[0] - s[0] * nn[2], s[0] * nn[1] - s[1] * nn[0]};
            const double b = nn[0] * (t[0] - s[0]) + nn[1] * (t[1] - s[1]) + nn[2] * (t[2] - s[2]);
            double bb = 2.0 * eb * b, aw[3];
#pragma unroll
            for (int r = 0; r < 6; ++r) bb += gb[r] * a[r];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double v = b * gb[3 + r];
#pragma unroll
                for (int c = 0; c < 6; ++c) v += M[(3 + r) * 6 + c] * a[c];
                aw[r] = v;
            }
            sb[0] = -bb * nn[0] + (nn[1] * aw[2] - nn[2] * aw[1]);
            sb[1] = -bb * nn[1] + (nn[2] * aw[0] - nn[0] * aw[2]);
            sb[2] = -bb * nn[2] + (nn[0] * aw[1] - nn[1] * aw[0]);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) g_src[i * 3 + r] = accumulate ? (float)((double)g_src[i * 3 + r] + sb[r]) : (float)sb[r];
    }
}

// ---------------------------------------------------------------------------------------------
// 12 float64 sums per workgroup, then a fixed-order second stage
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pg_block_partials(const double* acc, double* __restrict__ partial_row) {
    __shared__ double sh[PG_NSUM][PG_T / 64];
#pragma unroll
    for (int k = 0; k < PG_NSUM; ++k) {
        const double v = wave_sum_d(acc[k]);
        if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < PG_NSUM) partial_row[threadIdx.x] = ((sh[threadIdx.x][0] + sh[threadIdx.x][1]) + sh[threadIdx.x][2]) + sh[threadIdx.x][3];
}

// out = R p + t:  d/dT[:3, :] of sum(g . out) = [sum g p^T | sum g]
__global__ __launch_bounds__(PG_T) void k_transform_bwd_T_partials(const float* __restrict__ g, const float* __restrict__ p, int64_t n,
                                                                   double* __restrict__ partials) {
    double acc[PG_NSUM];
#pragma unroll
    for (int k = 0; k < PG_NSUM; ++k) acc[k] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PG_T) {
        const double gi[3] = {g[i * 3], g[i * 3 + 1], g[i * 3 + 2]};
        const double pi[3] = {p[i * 3], p[i * 3 + 1], p[i * 3 + 2]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[r * 4 + c] += gi[r] * pi[c];
            acc[r * 4 + 3] += gi[r];
        }
    }
    pg_block_partials(acc, partials + (int64_t)blockIdx.x * PG_NSUM);
}

// one wave per sum: lane l adds the partials l, l + 64, ... in order, then a fixed shuffle tree (as k_icp_final)
__global__ __launch_bounds__(64) void k_pg_final(const double* __restrict__ partials, int nparts, double* __restrict__ out) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += partials[(int64_t)i * PG_NSUM + k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) out[k] = s;
}

// Project3D (view_synthesis.py:54-78): c = P p with P = (K T)[:3, :], z = c2 + 1e-7, grid = ((c0/z)/(W-1) - .5) 2, ((c1/z)/(H-1) - .5) 2,
// z_out = clamp(c2, 1e-3).  Pbar = sum_i cbar_i p_i^T with cbar exactly as k_project3d_bwd (warp_photo.hip) forms it.
__global__ __launch_bounds__(PG_T) void k_project3d_bwd_T_partials(const float* __restrict__ pts, const float* __restrict__ K, const float* __restrict__ T,
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
    double acc[PG_NSUM];
#pragma unroll
    for (int k = 0; k < PG_NSUM; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * PG_T + threadIdx.x; i < N; i += gridDim.x * PG_T) {
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
    pg_block_partials(acc, partials + ((int64_t)b * gridDim.x + blockIdx.x) * PG_NSUM);
}

// wave w of workgroup b folds sum w of batch b; then Tbar[k][j] = sum_{i<3} K[i][k] Pbar[i][j]
__global__ __launch_bounds__(PG_NSUM * 64) void k_project3d_bwd_T_final(const double* __restrict__ partials, int nparts, const float* __restrict__ K,
                                                                        float* __restrict__ g_T) {
    __shared__ double Pb[PG_NSUM];
    const int b = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double s = 0.0;
    for (int i = lane; i < nparts; i += 64) s += partials[((int64_t)b * nparts + i) * PG_NSUM + w];
    s = wave_sum_d(s);
    if (lane == 0) Pb[w] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        const int k = threadIdx.x >> 2, j = threadIdx.x & 3;
        double v = 0.0;
        for (int i = 0; i < 3; ++i) v += (double)K[b * 16 + i * 4 + k] * Pb[i * 4 + j];
        g_T[b * 16 + threadIdx.x] = (float)v;
    }
}

static inline int pg_parts(int64_t n) {
    int64_t g = (n + PG_T - 1) / PG_T;
    return (int)(g > PG_MAX_PARTS ? PG_MAX_PARTS : g);
}

extern "C" {

int e2e_icp_normal_equations_bwd(const float* src, const float* tgt, const float* tgt_normals, int64_t n_tgt, const long long* idx,
                                 const float* dists, float dist_thresh, const double* adj28, int64_t n, float* g_src, int accumulate,
                                 void* stream) {
    E2E_REQUIRE(src && tgt && tgt_normals && idx && adj28 && g_src && n > 0 && n_tgt > 0, E2E_ERR_ARG, "e2e_icp_normal_equations_bwd: bad argument");
    E2E_REQUIRE(dist_thresh < 0.f || dists, E2E_ERR_ARG, "e2e_icp_normal_equations_bwd: a distance threshold needs the distances");
    hipLaunchKernelGGL(k_icp_ne_bwd, dim3(pg_parts(n)), dim3(PG_T), 0, (hipStream_t)stream, src, tgt, tgt_normals, n_tgt, idx, dists,
                       dist_thresh < 0.f ? -1.f : dist_thresh * dist_thresh, adj28, n, g_src, accumulate);
    E2E_LAUNCH_CHECK("e2e_icp_normal_equations_bwd");
    return E2E_OK;
}

int64_t e2e_transform_points_bwd_t_workspace_bytes(void) { return (int64_t)PG_MAX_PARTS * PG_NSUM * 8; }

int e2e_transform_points_bwd_t(const float* g, const float* points, int64_t n, double* out12, void* workspace, void* stream) {
    E2E_REQUIRE(g && points && out12 && workspace && n > 0, E2E_ERR_ARG, "e2e_transform_points_bwd_t: bad argument");
    hipStream_t st = (hipStream_t)stream;
    const int parts = pg_parts(n);
    hipLaunchKernelGGL(k_transform_bwd_T_partials, dim3(parts), dim3(PG_T), 0, st, g, points, n, (double*)workspace);
    hipLaunchKernelGGL(k_pg_final, dim3(PG_NSUM), dim3(64), 0, st, (const double*)workspace, parts, out12);
    E2E_LAUNCH_CHECK("e2e_transform_points_bwd_t");
    return E2E_OK;
}

int64_t e2e_project3d_bwd_t_workspace_bytes(int B) { return B > 0 ? (int64_t)B * PG_MAX_PARTS * PG_NSUM * 8 : 0; }

int e2e_project3d_bwd_t(const float* points, const float* K, const float* T, const float* g_grid, const float* g_z, float* g_T,
                        void* workspace, int B, int H, int W, void* stream) {
    E2E_REQUIRE(B > 0 && H > 1 && W > 1 && (int64_t)B * H * W < (1ll << 31), E2E_ERR_ARG, "e2e_project3d_bwd_t: bad dims B=%d H=%d W=%d", B, H, W);
    E2E_REQUIRE(B <= 65535, E2E_ERR_ARG, "e2e_project3d_bwd_t: B=%d exceeds the grid", B);
    E2E_REQUIRE(points && K && T && g_grid && g_T && workspace, E2E_ERR_ARG, "e2e_project3d_bwd_t: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int parts = pg_parts((int64_t)H * W);
    hipLaunchKernelGGL(k_project3d_bwd_T_partials, dim3(parts, B), dim3(PG_T), 0, st, points, K, T, g_grid, g_z, H, W, (double*)workspace);
    hipLaunchKernelGGL(k_project3d_bwd_T_final, dim3(B), dim3(PG_NSUM * 64), 0, st, (const double*)workspace, parts, K, g_T);
    E2E_LAUNCH_CHECK("e2e_project3d_bwd_t");
    return E2E_OK;
}

}  // extern "C"
