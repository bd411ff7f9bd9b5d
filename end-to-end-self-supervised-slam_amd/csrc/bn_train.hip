// bn_train.hip -- train-mode BatchNorm2d of the ResNet body (networks.py:_ConvBN.run with bn.training): batch statistics over the
// P = B*H*W pixels of an NHWC tensor, the running-average update with nn.BatchNorm2d's own momentum rules (momentum=None: cumulative
// average over num_batches_tracked, read and advanced on the device), the normalisation with the residual add and the ReLU folded in,
// and the backward of all of it.  The contracts are stated in include/e2eslam.h; tests/test_gpu_bn_train_contracts.py holds every
// entry point of this file to the float64 reference of tests/bn_train_ref.py.
//
// Thread mapping (all five streaming kernels): a thread owns FOUR consecutive channels and moves them as one float4.  A workgroup of 256
// threads is QW = min(C/4, 64) channel quads wide and ROWS = 256 / QW pixel rows high, so a wave's load is 1 KiB contiguous for
// C >= 256 and whole pixel rows below that (four 256-byte rows at C = 64).  blockIdx.y walks the channel blocks of 4 QW channels,
// blockIdx.x the S "slices": slice s takes pixel rows s*ROWS + r, then strides by S*ROWS, so a thread's fp32 chain is P / (S*ROWS)
// long (about 8; it grows only past the 1024-slice cap, which the largest layer of a 480 x 640 frame pair just reaches).  S depends on
// (P, C) only.
//
// Statistics: each thread accumulates sum(z - K) and sum((z - K)^2) about the channel's first pixel K = z[0,c] -- never raw moments,
// whose fp32 cancellation is ruinous once |mean| >> std -- the rows of a workgroup are folded by a fixed tree in LDS, every slice
// writes one row of partial sums, and the finalise launch (one workgroup per 8 channels) adds the slices in float64 in a fixed order.
// The backward's sums (g and g * xhat, the ReLU mask taken from y, xhat recomputed from z) go the same way.  The count of batches is
// advanced by the FIRST launch of a forward and read by the second: no workgroup of the finalise launch races another for it.  No
// atomics, no host read: two calls on the same inputs give the same bits.  Every element offset is 64-bit.
#include "e2e_common.h"

typedef float f4v __attribute__((ext_vector_type(4)));

#define BT_MAX_SLICES 1024
#define BT_ROWS_PER_THREAD 8
#define BT_FIN_CH 8                                                    // a finalise workgroup: 8 channels x 32 slice lanes
#define BT_FIN_LANES 32

struct BtGeom {
    int qw, rows, ncb, S;                                              // quads per workgroup row, pixel rows, channel blocks, slices
};

static inline BtGeom bt_geom(int64_t P, int C) {
    BtGeom g;
    const int quads = C / 4;
    g.qw = quads < 64 ? quads : 64;
    g.rows = 256 / g.qw;
    g.ncb = (quads + g.qw - 1) / g.qw;
    const int64_t per = (int64_t)g.rows * BT_ROWS_PER_THREAD, s = (P + per - 1) / per;
    g.S = (int)(s < 1 ? 1 : (s > BT_MAX_SLICES ? BT_MAX_SLICES : s));
    return g;
}

// per-channel vectors carry no alignment promise (a parameter may be a slice of a flat bucket): four scalar loads
__device__ __forceinline__ f4v bt_ld4(const float* __restrict__ p, int c) { return f4v{p[c], p[c + 1], p[c + 2], p[c + 3]}; }
__device__ __forceinline__ f4v bt_ld4_or(const float* __restrict__ p, int c, float dflt) { return p ? bt_ld4(p, c) : f4v{dflt, dflt, dflt, dflt}; }

// where this thread sits: channel c (first of its quad), pixel row `row` of the workgroup; false: the thread only keeps the barriers
__device__ __forceinline__ bool bt_place(int C, int qw, int rows, int& c, int& row) {
    row = threadIdx.x / qw;
    const int q = blockIdx.y * qw + (threadIdx.x - row * qw);
    c = q * 4;
    return row < rows && c < C;
}

// fold the pixel rows of the workgroup (entries tid = row * qw + quad lane) in a fixed tree; the result is in row 0
__device__ __forceinline__ void bt_fold_rows(f4v* sa, f4v* sb, int qw, int rows, int row, f4v a, f4v b) {
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    int o = 1;
    while (o < rows) o <<= 1;
    for (o >>= 1; o > 0; o >>= 1) {
        __syncthreads();
        if (row < o && row + o < rows) {
            sa[threadIdx.x] += sa[threadIdx.x + o * qw];
            sb[threadIdx.x] += sb[threadIdx.x + o * qw];
        }
    }
}

// partial row of slice s: [s][0][C] then [s][1][C]
__device__ __forceinline__ void bt_store_partial(float* __restrict__ partials, int C, int c, f4v a, f4v b) {
    float* pa = partials + ((int64_t)blockIdx.x * 2) * C + c;
    *(f4v*)pa = a;
    *(f4v*)(pa + C) = b;
}

__global__ __launch_bounds__(256) void k_bn_train_stats(const float* __restrict__ z, float* __restrict__ partials, int64_t* __restrict__ nbt,
                                                        int64_t P, int C, int qw, int rows) {
    __shared__ f4v sa[256], sb[256];
    if (nbt && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) nbt[0] += 1;       // read by the finalise launch: 1 / count
    int c, row;
    const bool on = bt_place(C, qw, rows, c, row);
    f4v s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (on) {
        const f4v K = *(const f4v*)(z + c);                            // the channel's first pixel
#pragma unroll 4
        for (int64_t p = (int64_t)blockIdx.x * rows + row; p < P; p += (int64_t)gridDim.x * rows) {
            const f4v d = *(const f4v*)(z + p * C + c) - K;
            s1 += d;
            s2 += d * d;
        }
    }
    bt_fold_rows(sa, sb, qw, rows, row, s1, s2);
    if (on && row == 0) bt_store_partial(partials, C, c, sa[threadIdx.x], sb[threadIdx.x]);
}

// The S partial rows of 8 channels -> two float64 sums per channel, valid in threads 0..7 of the workgroup.  256 threads = 8 channels x 32
// slice lanes; fixed assignment (lane j adds slices j, j + 32, ... in that order) and fixed combine order (an xor tree over the 8 lanes
// of a wave, then the four waves in wave order).
__device__ __forceinline__ void bt_merge(const float* __restrict__ partials, int S, int C, int c, double (*sh)[4][BT_FIN_CH], double& t1, double& t2) {
    const int j = threadIdx.x / BT_FIN_CH, cl = threadIdx.x % BT_FIN_CH, wave = threadIdx.x >> 6;
    double a1 = 0.0, a2 = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int s = j; s < S; s += BT_FIN_LANES) {
            a1 += (double)partials[((int64_t)s * 2) * C + c];
            a2 += (double)partials[((int64_t)s * 2 + 1) * C + c];
        }
    }
#pragma unroll
    for (int o = BT_FIN_CH; o < 64; o <<= 1) {
        a1 += __shfl_xor(a1, o, 64);
        a2 += __shfl_xor(a2, o, 64);
    }
    if ((threadIdx.x & 63) < BT_FIN_CH) {
        sh[0][wave][cl] = a1;
        sh[1][wave][cl] = a2;
    }
    __syncthreads();
    t1 = t2 = 0.0;
    if (threadIdx.x < BT_FIN_CH) {
        t1 = ((sh[0][0][cl] + sh[0][1][cl]) + sh[0][2][cl]) + sh[0][3][cl];
        t2 = ((sh[1][0][cl] + sh[1][1][cl]) + sh[1][2][cl]) + sh[1][3][cl];
    }
}

// one workgroup per 8 channels.  The count of batches was advanced by k_bn_train_stats, one launch earlier: every workgroup here reads
// the same, already incremented value.
__global__ __launch_bounds__(256) void k_bn_train_fwd_finalise(const float* __restrict__ z, const float* __restrict__ partials,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               float momentum, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                               const int64_t* __restrict__ nbt, float* __restrict__ save_mean,
                                                               float* __restrict__ save_rstd, float* __restrict__ scale, float* __restrict__ shift,
                                                               int64_t P, int C, int S) {
    __shared__ double sh[2][4][BT_FIN_CH];
    const int c = blockIdx.x * BT_FIN_CH + threadIdx.x % BT_FIN_CH;
    double s1, s2;
    bt_merge(partials, S, C, c, sh, s1, s2);
    if (threadIdx.x >= BT_FIN_CH || c >= C) return;
    const double n = (double)P, m = s1 / n;
    const double mean = (double)z[c] + m;
    double var = s2 / n - m * m;                                       // float64, about K: |m| is a few standard deviations at most
    var = var > 0.0 ? var : 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    save_mean[c] = (float)mean;
    save_rstd[c] = (float)rstd;
    const float sc = (float)((gamma ? (double)gamma[c] : 1.0) * rstd);
    scale[c] = sc;
    shift[c] = (float)((beta ? (double)beta[c] : 0.0) - mean * (double)sc);
    if (running_mean) {
        const double f = momentum < 0.f ? 1.0 / (double)nbt[0] : (double)momentum;      // momentum=None: cumulative average
        running_mean[c] = (float)((1.0 - f) * (double)running_mean[c] + f * mean);
        running_var[c] = (float)((1.0 - f) * (double)running_var[c] + f * (var * (n / (n - 1.0))));
    }
}

__global__ __launch_bounds__(256) void k_bn_train_apply(const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ residual, int relu, float* __restrict__ y, int64_t P, int C,
                                                        int qw, int rows) {
    int c, row;
    if (!bt_place(C, qw, rows, c, row)) return;
    const f4v sc = bt_ld4(scale, c), sf = bt_ld4(shift, c);
#pragma unroll 4
    for (int64_t p = (int64_t)blockIdx.x * rows + row; p < P; p += (int64_t)gridDim.x * rows) {
        const int64_t i = p * C + c;
        f4v v = *(const f4v*)(z + i) * sc + sf;
        if (residual) v += *(const f4v*)(residual + i);
        if (relu)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = fmaxf(v[k], 0.f);
        *(f4v*)(y + i) = v;
    }
}

__device__ __forceinline__ f4v bt_masked(const float* __restrict__ dy, const float* __restrict__ y, int64_t i) {
    f4v g = *(const f4v*)(dy + i);
    if (y) {
        const f4v v = *(const f4v*)(y + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = v[k] > 0.f ? g[k] : 0.f;
    }
    return g;
}

__global__ __launch_bounds__(256) void k_bn_train_bwd_sums(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z,
                                                           const float* __restrict__ save_mean, const float* __restrict__ save_rstd,
                                                           float* __restrict__ partials, int64_t P, int C, int qw, int rows) {
    __shared__ f4v sa[256], sb[256];
    int c, row;
    const bool on = bt_place(C, qw, rows, c, row);
    f4v s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (on) {
        const f4v mean = bt_ld4(save_mean, c), rstd = bt_ld4(save_rstd, c);
#pragma unroll 4
        for (int64_t p = (int64_t)blockIdx.x * rows + row; p < P; p += (int64_t)gridDim.x * rows) {
            const int64_t i = p * C + c;
            const f4v g = bt_masked(dy, y, i);
            const f4v xhat = (*(const f4v*)(z + i) - mean) * rstd;
            s1 += g;
            s2 += g * xhat;
        }
    }
    bt_fold_rows(sa, sb, qw, rows, row, s1, s2);
    if (on && row == 0) bt_store_partial(partials, C, c, sa[threadIdx.x], sb[threadIdx.x]);
}

// totals (C floats of sum g, then C floats of sum g * xhat) for the elementwise pass; dbeta / dgamma where asked for
__global__ __launch_bounds__(256) void k_bn_train_bwd_finalise(const float* __restrict__ partials, float* __restrict__ totals,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, int C, int S) {
    __shared__ double sh[2][4][BT_FIN_CH];
    const int c = blockIdx.x * BT_FIN_CH + threadIdx.x % BT_FIN_CH;
    double s1, s2;
    bt_merge(partials, S, C, c, sh, s1, s2);
    if (threadIdx.x >= BT_FIN_CH || c >= C) return;
    const float db = (float)s1, dg = (float)s2;
    totals[c] = db;
    totals[C + c] = dg;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + db : db;
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + dg : dg;
}

// dz = gamma rstd (g - sum(g) / P - xhat sum(g xhat) / P), dresidual = g; totals NULL: dresidual only
__global__ __launch_bounds__(256) void k_bn_train_bwd_apply(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ z,
                                                            const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                                            const float* __restrict__ save_rstd, const float* __restrict__ totals,
                                                            float* __restrict__ dz, float* __restrict__ dresidual, int64_t P, int C, int qw, int rows) {
    int c, row;
    if (!bt_place(C, qw, rows, c, row)) return;
    f4v mean = {0.f, 0.f, 0.f, 0.f}, rstd = mean, a = mean, mb = mean, mg = mean;
    if (dz) {
        const float inv = 1.f / (float)P;
        mean = bt_ld4(save_mean, c);
        rstd = bt_ld4(save_rstd, c);
        a = bt_ld4_or(gamma, c, 1.f) * rstd;
        mb = bt_ld4(totals, c) * inv;
        mg = bt_ld4(totals, C + c) * inv;
    }
#pragma unroll 4
    for (int64_t p = (int64_t)blockIdx.x * rows + row; p < P; p += (int64_t)gridDim.x * rows) {
        const int64_t i = p * C + c;
        const f4v g = bt_masked(dy, y, i);
        if (dresidual) *(f4v*)(dresidual + i) = g;
        if (dz) {
            const f4v xhat = (*(const f4v*)(z + i) - mean) * rstd;
            *(f4v*)(dz + i) = a * ((g - mb) - xhat * mg);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
static inline bool bt_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }       // NULL passes

extern "C" {

int64_t e2e_bn_train_workspace_floats(int64_t P, int C) {
    if (P < 2 || C <= 0 || C % 4 != 0) return 0;
    return (int64_t)2 * bt_geom(P, C).S * C + 2 * (int64_t)C;
}

int e2e_bn_train_fwd(const float* z, const float* gamma, const float* beta, const float* residual, int relu, float eps, float momentum,
                     float* running_mean, float* running_var, int64_t* num_batches_tracked, float* y, float* save_mean, float* save_rstd,
                     int64_t P, int C, float* workspace, void* stream) {
    E2E_REQUIRE(z && y && workspace && save_mean && save_rstd, E2E_ERR_ARG, "e2e_bn_train_fwd: NULL z, y, save_mean, save_rstd or workspace");
    E2E_REQUIRE(P >= 2, E2E_ERR_ARG, "e2e_bn_train_fwd: P = %lld (batch statistics need more than one value per channel)", (long long)P);
    E2E_REQUIRE(C > 0 && C % 4 == 0, E2E_ERR_ARG, "e2e_bn_train_fwd: C = %d (a positive multiple of 4)", C);
    E2E_REQUIRE(eps > 0.f, E2E_ERR_ARG, "e2e_bn_train_fwd: eps = %g (must be positive)", (double)eps);
    const int given = (running_mean != nullptr) + (running_var != nullptr) + (num_batches_tracked != nullptr);
    E2E_REQUIRE(given == 0 || given == 3, E2E_ERR_ARG, "e2e_bn_train_fwd: running_mean, running_var and num_batches_tracked go together (all or none)");
    E2E_REQUIRE(bt_al16(z) && bt_al16(y) && bt_al16(residual) && bt_al16(workspace), E2E_ERR_ARG,
                "e2e_bn_train_fwd: z, y, residual and workspace must be 16-byte aligned");
    const BtGeom g = bt_geom(P, C);
    float* scale = workspace + (int64_t)2 * g.S * C;
    float* shift = scale + C;
    const dim3 grid(g.S, g.ncb), block(256);
    hipStream_t st = (hipStream_t)stream;
    const dim3 fin((C + BT_FIN_CH - 1) / BT_FIN_CH);
    hipLaunchKernelGGL(k_bn_train_stats, grid, block, 0, st, z, workspace, num_batches_tracked, P, C, g.qw, g.rows);
    hipLaunchKernelGGL(k_bn_train_fwd_finalise, fin, block, 0, st, z, (const float*)workspace, gamma, beta, eps, momentum, running_mean, running_var,
                       (const int64_t*)num_batches_tracked, save_mean, save_rstd, scale, shift, P, C, g.S);
    hipLaunchKernelGGL(k_bn_train_apply, grid, block, 0, st, z, (const float*)scale, (const float*)shift, residual, relu, y, P, C, g.qw, g.rows);
    E2E_LAUNCH_CHECK("e2e_bn_train_fwd");
    return E2E_OK;
}

int e2e_bn_train_bwd(const float* dy, const float* y, const float* z, const float* gamma, const float* save_mean, const float* save_rstd,
                     int64_t P, int C, float* dz, float* dresidual, float* dgamma, float* dbeta, int accumulate, float* workspace, void* stream) {
    E2E_REQUIRE(dy && z && save_mean && save_rstd && workspace, E2E_ERR_ARG, "e2e_bn_train_bwd: NULL dy, z, save_mean, save_rstd or workspace");
    E2E_REQUIRE(P >= 2, E2E_ERR_ARG, "e2e_bn_train_bwd: P = %lld (batch statistics need more than one value per channel)", (long long)P);
    E2E_REQUIRE(C > 0 && C % 4 == 0, E2E_ERR_ARG, "e2e_bn_train_bwd: C = %d (a positive multiple of 4)", C);
    E2E_REQUIRE(dz || dresidual || dgamma || dbeta, E2E_ERR_ARG, "e2e_bn_train_bwd: no output asked for (dz, dresidual, dgamma and dbeta all NULL)");
    E2E_REQUIRE(bt_al16(dy) && bt_al16(y) && bt_al16(z) && bt_al16(dz) && bt_al16(dresidual) && bt_al16(workspace), E2E_ERR_ARG,
                "e2e_bn_train_bwd: dy, y, z, dz, dresidual and workspace must be 16-byte aligned");
    const BtGeom g = bt_geom(P, C);
    float* totals = workspace + (int64_t)2 * g.S * C;
    const dim3 grid(g.S, g.ncb), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (dz || dgamma || dbeta) {
        hipLaunchKernelGGL(k_bn_train_bwd_sums, grid, block, 0, st, dy, y, z, save_mean, save_rstd, workspace, P, C, g.qw, g.rows);
        hipLaunchKernelGGL(k_bn_train_bwd_finalise, dim3((C + BT_FIN_CH - 1) / BT_FIN_CH), block, 0, st, (const float*)workspace, totals, dgamma,
                           dbeta, accumulate, C, g.S);
    }
    if (dz || dresidual)
        hipLaunchKernelGGL(k_bn_train_bwd_apply, grid, block, 0, st, dy, y, z, gamma, save_mean, save_rstd, (const float*)totals, dz, dresidual, P, C,
                           g.qw, g.rows);
    E2E_LAUNCH_CHECK("e2e_bn_train_bwd");
    return E2E_OK;
}

}  // extern "C"
