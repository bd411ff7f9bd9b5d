// pose_grad.hip -- the per-point halves of the ADJOINT of the odometry (differentiable ICP / GradICP) and of the two
// operators that consume a pose (Project3D, transform_pointcloud) with respect to the 4x4 transform.  The reference differentiates the
// photometric loss through the pose into the live frame's depth (train_depth.py:381-382, :395 with DATA.use_gt_pose: False); the 6x6
// algebra of that adjoint is float64 on the host (e2ehip/icp.py), as the forward's is.
// Sums are float64 with a fixed order (per-thread -> wave shuffle -> per-workgroup partials -> one wave per sum; for the target-side
// scatter one owner per destination over its source rows in ascending index), no float atomics: bitwise reproducible run to run.
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
// adjoint of k_icp_partials wrt the TARGET points and normals (the chain gradient: the map is a variable of the localisation).  Same
// notation; for target row j, over the kept source rows i with idx[i] == j:
//   tbar_j = sum_i bbar_i n_j            nbar_j = sum_i bbar_i (t_j - s_i) + Abar_i[0:3] + Abar_i[3:6] x s_i
// Several sources share a target: the neighbour list is inverted per call (count, exclusive scan, fill) and ONE owner per target adds
// its rows in ascending source index in float64 and rounds once -- no float atomics, independent of arrival order, bitwise reproducible.
// The fill goes through an integer cursor, which leaves a segment in arbitrary order: the owner restores the order before it sums (a
// thread sorts a short segment in place; a wave ranks a long one into a second list, then lane l adds the rows l, l + 64, ... of the
// sorted segment and a fixed shuffle tree adds the lanes).  Every pass is O(n) or O(n_tgt).
// ---------------------------------------------------------------------------------------------
#define NT_ITEMS 16
#define NT_TILE (PG_T * NT_ITEMS)      // targets per workgroup of the scan
#define NT_LONG 64                     // a segment longer than this goes to a wave

__device__ __forceinline__ void pg_load_adj(const double* __restrict__ adj, double* M, double* gb, double* eb) {
    if (threadIdx.x < 36) {
        const int r = threadIdx.x / 6, c = threadIdx.x % 6;
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const int k = lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
        M[threadIdx.x] = (r == c ? 2.0 : 1.0) * adj[k];
    } else if (threadIdx.x < 42) {
        gb[threadIdx.x - 36] = adj[21 + threadIdx.x - 36];
    } else if (threadIdx.x == 42) {
        *eb = adj[27];
    }
    __syncthreads();
}

__device__ __forceinline__ bool pg_keep(const long long* __restrict__ idx, const float* __restrict__ dists, float thresh_sq, int64_t n_tgt,
                                        int64_t i, long long* j) {
    *j = idx[i];
    return (thresh_sq < 0.f || dists[i] < thresh_sq) && *j >= 0 && *j < n_tgt;
}

// one kept row's terms: acc[0] += bbar, acc[1..3] += bbar (t - s) + Abar[0:3] + Abar[3:6] x s
__device__ __forceinline__ void pg_tgt_row(const double* M, const double* gb, double eb, const float* __restrict__ src, int64_t i, const double* t,
                                           const double* nn, double* acc) {
    const double s[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
    const double a[6] = {nn[0], nn[1], nn[2], s[1] * nn[2] - s[2] * nn[1], s[2] * nn[0] - s[0] * nn[2], s[0] * nn[1] - s[1] * nn[0]};
    const double b = nn[0] * (t[0] - s[0]) + nn[1] * (t[1] - s[1]) + nn[2] * (t[2] - s[2]);
    double bb = 2.0 * eb * b, aw[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) bb += gb[r] * a[r];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double v = b * gb[r];
#pragma unroll
        for (int c = 0; c < 6; ++c) v += M[r * 6 + c] * a[c];
        aw[r] = v;
    }
    const double row[4] = {bb, bb * (t[0] - s[0]) + aw[0] + (aw[4] * s[2] - aw[5] * s[1]), bb * (t[1] - s[1]) + aw[1] + (aw[5] * s[0] - aw[3] * s[2]),
                           bb * (t[2] - s[2]) + aw[2] + (aw[3] * s[1] - aw[4] * s[0])};
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += row[r];
}

__device__ __forceinline__ void pg_tgt_store(const double* acc, const double* nn, int64_t j, float* __restrict__ g_tgt, float* __restrict__ g_tgt_n,
                                             int accumulate) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (g_tgt) g_tgt[j * 3 + r] = accumulate ? (float)((double)g_tgt[j * 3 + r] + acc[0] * nn[r]) : (float)(acc[0] * nn[r]);
        if (g_tgt_n) g_tgt_n[j * 3 + r] = accumulate ? (float)((double)g_tgt_n[j * 3 + r] + acc[1 + r]) : (float)acc[1 + r];
    }
}

__global__ __launch_bounds__(PG_T) void k_nt_count(const long long* __restrict__ idx, const float* __restrict__ dists, float thresh_sq, int64_t n_tgt,
                                                   int64_t n, int* __restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PG_T) {
        long long j;
        if (pg_keep(idx, dists, thresh_sq, n_tgt, i, &j)) atomicAdd(cnt + j, 1);
    }
}

// exclusive scan of one value per thread over the workgroup (PG_T threads); *total: the workgroup's sum
__device__ __forceinline__ int nt_block_scan(int v, int* total) {
    __shared__ int wt[PG_T / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) wt[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < PG_T / 64; ++k) {
        if (k < w) base += wt[k];
        tot += wt[k];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// per tile of NT_TILE targets: loc[j] = the kept rows of the tile's targets before j, tile_sum[tile] = the tile's rows; cnt is zeroed
// (it becomes the fill's cursor and ends as the count again)
__global__ __launch_bounds__(PG_T) void k_nt_local_scan(int* __restrict__ cnt, int* __restrict__ loc, int* __restrict__ tile_sum, int64_t n_tgt) {
    __shared__ int tile[NT_TILE];
    const int64_t base = (int64_t)blockIdx.x * NT_TILE;
    for (int k = threadIdx.x; k < NT_TILE; k += PG_T) {
        int v = 0;
        if (base + k < n_tgt) {
            v = cnt[base + k];
            cnt[base + k] = 0;
        }
        tile[k] = v;
    }
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int k = 0; k < NT_ITEMS; ++k) s += tile[threadIdx.x * NT_ITEMS + k];
    int tot;
    int ex = nt_block_scan(s, &tot);
#pragma unroll
    for (int k = 0; k < NT_ITEMS; ++k) {
        const int v = tile[threadIdx.x * NT_ITEMS + k];
        tile[threadIdx.x * NT_ITEMS + k] = ex;
        ex += v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NT_TILE; k += PG_T)
        if (base + k < n_tgt) loc[base + k] = tile[k];
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// one workgroup: tile_sum -> its exclusive scan, in place
__global__ __launch_bounds__(PG_T) void k_nt_scan_tiles(int* __restrict__ tile_sum, int tiles) {
    int carry = 0;
    for (int b0 = 0; b0 < tiles; b0 += PG_T) {
        const int i = b0 + threadIdx.x;
        int tot;
        const int ex = nt_block_scan(i < tiles ? tile_sum[i] : 0, &tot);
        if (i < tiles) tile_sum[i] = carry + ex;
        carry += tot;
    }
}

__global__ __launch_bounds__(PG_T) void k_nt_fill(const long long* __restrict__ idx, const float* __restrict__ dists, float thresh_sq, int64_t n_tgt,
                                                  int64_t n, const int* __restrict__ loc, const int* __restrict__ tile_sum, int* __restrict__ cursor,
                                                  int* __restrict__ list) {
    for (int64_t i = (int64_t)blockIdx.x * PG_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PG_T) {
        long long j;
        if (pg_keep(idx, dists, thresh_sq, n_tgt, i, &j)) list[loc[j] + tile_sum[j / NT_TILE] + atomicAdd(cursor + j, 1)] = (int)i;
    }
}

// one thread per target: nothing to add, or a short segment (sorted in place, added in ascending source index), or a long one (queued)
__global__ __launch_bounds__(PG_T) void k_nt_sum_short(const float* __restrict__ src, const float* __restrict__ tgt, const float* __restrict__ tgt_n,
                                                       int64_t n_tgt, const double* __restrict__ adj, const int* __restrict__ loc,
                                                       const int* __restrict__ tile_sum, const int* __restrict__ cnt, int* __restrict__ list,
                                                       int* __restrict__ long_list, int* __restrict__ long_count, float* __restrict__ g_tgt,
                                                       float* __restrict__ g_tgt_n, int accumulate) {
    __shared__ double M[36], gb[6], eb;
    pg_load_adj(adj, M, gb, &eb);
    for (int64_t j = (int64_t)blockIdx.x * PG_T + threadIdx.x; j < n_tgt; j += (int64_t)gridDim.x * PG_T) {
        const int len = cnt[j];
        if (len > NT_LONG) {
            long_list[atomicAdd(long_count, 1)] = (int)j;
            continue;
        }
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        const double nn[3] = {tgt_n[j * 3], tgt_n[j * 3 + 1], tgt_n[j * 3 + 2]};
        if (len == 0) {
            if (!accumulate) pg_tgt_store(acc, nn, j, g_tgt, g_tgt_n, 0);
            continue;
        }
        int* seg = list + loc[j] + tile_sum[j / NT_TILE];
        for (int p = 1; p < len; ++p) {                       // insertion sort: this thread owns the segment
            const int v = seg[p];
            int q = p - 1;
            while (q >= 0 && seg[q] > v) {
                seg[q + 1] = seg[q];
                --q;
            }
            seg[q + 1] = v;
        }
        const double t[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
        for (int p = 0; p < len; ++p) pg_tgt_row(M, gb, eb, src, seg[p], t, nn, acc);
        pg_tgt_store(acc, nn, j, g_tgt, g_tgt_n, accumulate);
    }
}

// one wave per queued target (workgroups of one wave, so the barrier below is the wave's)
__global__ __launch_bounds__(64) void k_nt_sum_long(const float* __restrict__ src, const float* __restrict__ tgt, const float* __restrict__ tgt_n,
                                                    const double* __restrict__ adj, const int* __restrict__ loc, const int* __restrict__ tile_sum,
                                                    const int* __restrict__ cnt, const int* __restrict__ list, int* __restrict__ sorted,
                                                    const int* __restrict__ long_list, const int* __restrict__ long_count, float* __restrict__ g_tgt,
                                                    float* __restrict__ g_tgt_n, int accumulate) {
    __shared__ double M[36], gb[6], eb;
    pg_load_adj(adj, M, gb, &eb);
    const int count = *long_count;
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        const int64_t j = long_list[k];
        const int len = cnt[j], start = loc[j] + tile_sum[j / NT_TILE];
        for (int p = threadIdx.x; p < len; p += 64) {          // source indices are distinct: the rank is the sorted position
            const int v = list[start + p];
            int rank = 0;
            for (int q = 0; q < len; ++q) rank += list[start + q] < v;
            sorted[start + rank] = v;
        }
        __syncthreads();
        const double t[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
        const double nn[3] = {tgt_n[j * 3], tgt_n[j * 3 + 1], tgt_n[j * 3 + 2]};
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int p = threadIdx.x; p < len; p += 64) pg_tgt_row(M, gb, eb, src, sorted[start + p], t, nn, acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = wave_sum_d(acc[r]);
        if (threadIdx.x == 0) pg_tgt_store(acc, nn, j, g_tgt, g_tgt_n, accumulate);
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

// workspace (ints): cnt[n_tgt] long_count[1] | loc[n_tgt] | tile_sum[tiles] | list[n] | sorted[n] | long_list[n / NT_LONG + 1]
static inline int64_t nt_tiles(int64_t n_tgt) { return (n_tgt + NT_TILE - 1) / NT_TILE; }

int64_t e2e_icp_normal_equations_bwd_tgt_workspace_bytes(int64_t n, int64_t n_tgt) {
    if (n <= 0 || n_tgt <= 0 || n >= (1ll << 31) || n_tgt >= (1ll << 31)) return 0;
    return 4 * (2 * n_tgt + 1 + nt_tiles(n_tgt) + 2 * n + n / NT_LONG + 1);
}

int e2e_icp_normal_equations_bwd_tgt(const float* src, const float* tgt, const float* tgt_normals, int64_t n_tgt, const long long* idx,
                                     const float* dists, float dist_thresh, const double* adj28, int64_t n, float* g_tgt, float* g_tgt_normals,
                                     int accumulate, void* workspace, void* stream) {
    E2E_REQUIRE(src && tgt && tgt_normals && idx && adj28 && workspace && n > 0 && n_tgt > 0 && n < (1ll << 31) && n_tgt < (1ll << 31), E2E_ERR_ARG,
                "e2e_icp_normal_equations_bwd_tgt: bad argument");
    E2E_REQUIRE(g_tgt || g_tgt_normals, E2E_ERR_ARG, "e2e_icp_normal_equations_bwd_tgt: neither output is wanted");
    E2E_REQUIRE(dist_thresh < 0.f || dists, E2E_ERR_ARG, "e2e_icp_normal_equations_bwd_tgt: a distance threshold needs the distances");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (int)nt_tiles(n_tgt);
    int* cnt = (int*)workspace;
    int* long_count = cnt + n_tgt;
    int* loc = long_count + 1;
    int* tile_sum = loc + n_tgt;
    int* list = tile_sum + tiles;
    int* sorted = list + n;
    int* long_list = sorted + n;
    const float tsq = dist_thresh < 0.f ? -1.f : dist_thresh * dist_thresh;
    const int64_t tblocks = (n_tgt + PG_T - 1) / PG_T, longs = n / NT_LONG + 1;
    if (hipMemsetAsync(cnt, 0, (size_t)(n_tgt + 1) * 4, st) != hipSuccess) {
        e2e_set_error("e2e_icp_normal_equations_bwd_tgt: clearing the counts failed");
        return E2E_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(k_nt_count, dim3(pg_parts(n)), dim3(PG_T), 0, st, idx, dists, tsq, n_tgt, n, cnt);
    hipLaunchKernelGGL(k_nt_local_scan, dim3(tiles), dim3(PG_T), 0, st, cnt, loc, tile_sum, n_tgt);
    hipLaunchKernelGGL(k_nt_scan_tiles, dim3(1), dim3(PG_T), 0, st, tile_sum, tiles);
    hipLaunchKernelGGL(k_nt_fill, dim3(pg_parts(n)), dim3(PG_T), 0, st, idx, dists, tsq, n_tgt, n, (const int*)loc, (const int*)tile_sum, cnt, list);
    hipLaunchKernelGGL(k_nt_sum_short, dim3((unsigned)(tblocks > 4096 ? 4096 : tblocks)), dim3(PG_T), 0, st, src, tgt, tgt_normals, n_tgt, adj28,
                       (const int*)loc, (const int*)tile_sum, (const int*)cnt, list, long_list, long_count, g_tgt, g_tgt_normals, accumulate);
    hipLaunchKernelGGL(k_nt_sum_long, dim3((unsigned)(longs > 256 ? 256 : longs)), dim3(64), 0, st, src, tgt, tgt_normals, adj28, (const int*)loc,
                       (const int*)tile_sum, (const int*)cnt, (const int*)list, sorted, (const int*)long_list, (const int*)long_count, g_tgt,
                       g_tgt_normals, accumulate);
    E2E_LAUNCH_CHECK("e2e_icp_normal_equations_bwd_tgt");
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
