// warp_photo_window.hip -- the fused warp-photometric pair over a window of S = 1 or 2 source frames (DATA.frames: [0,-1,1], [0,-1], [0,1]) with
// the candidate / minimum logic of the reference's train_depth.py:621-662 (LOSS.auto_masking, LOSS.min_reprojection).  One tile launch forward
// (+ the fixed-order reduction of the workgroups' partial sums), one tile launch backward (+ a final kernel per source and batch element when
// the gradient with respect to the poses is asked for).
//
// Semantics.  For source s with its validity mask m_s (1 everywhere when use_mask == 0):
//     R_s = photometric(synth_s m_s, tgt m_s)                    the reprojection map
//     I_s = photometric(src_s m_s, tgt m_s)                      the identity map: src_s read at the target pixel
// Candidate list, in this order:
//     identity candidates, only with E2E_TERM_AUTO_MASKING:  with E2E_TERM_MIN_REPROJECTION  I_0 + n_0, ..., I_{S-1} + n_{S-1}  (n = tie_noise
//         (B,S,H,W); NULL: nothing is added), without it the one map mean_s I_s;
//     reprojection candidates:  with MIN_REPROJECTION  R_0, ..., R_{S-1},  without it the one map mean_s R_s.
// One candidate: the loss is its mean.  Several: the mean of the per-pixel minimum.  select (B,H,W) is the index of the FIRST minimal candidate;
// a NaN wins (the first one), as in torch.min and e2e_min_reprojection_lossgrad; select is 0 with one candidate.
// Gradient, nI = number of identity candidates:  select < nI: the pixel's loss has no gradient (frames and masks are constants);
// select - nI = r under MIN_REPROJECTION: the pixel's upstream g_loss / (B H W) goes to R_r alone; otherwise 1/S of it goes to each R_s.
// That per-pixel weight varies over the 3x3 SSIM footprint, so the statistics phase of the backward reads `select` with a 1-pixel halo.
// Everything else is e2e_warp_photo_fwd / _bwd_pose to the letter: z = c2 + 1e-7, align_corners=False, zero slope under an active border clamp,
// the mask is a constant, the g_T convention of e2e_project3d_bwd_t (bottom row included), float64 fixed-order sums and no atomics: two runs
// give the same bits.
//
// The small device functions (SSIM statistics, the three-channel bilinear sample), the tile constants and the two second stages
// (k_reduce_partials, k_warp_photo_bwd_pose_final) are the pair's, through warp_photo_tile.h: a function that is moved compiles to the
// instructions it had (profiles/warp_family_refactor.txt).  The tile kernels' phase bodies stay written out here and in warp_photo.hip:
// extracting written-out arithmetic into new functions does reorder a kernel (profiles/lossgrad_tile_refactor.txt §3).
#include "e2e_common.h"
#include "warp_photo_tile.h"

namespace {

constexpr int FP_N = (TH + 2) * FP_LD, BP_N = (TH + 4) * BP_LD, BG_N = (TH + 2) * BG_LD;     // floats per LDS plane
constexpr int MAX_S = 2;

// photometric value of the thread's pixel from two plane triples (x = prediction, y = target), w0 = the window's top-left element
__device__ __forceinline__ float photo_value(const float (*x)[FP_N], const float (*y)[FP_N], int w0) {
    const int ctr = w0 + FP_LD + 1;
    float sacc = 0.f, lacc = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const Stats s = window_stats(x[c] + w0, y[c] + w0, FP_LD);
        sacc += ssim_value(s);
        lacc += fabsf(y[c][ctr] - x[c][ctr]);
    }
    return 0.85f * (sacc / 3.f) + 0.15f * (lacc / 3.f);
}

// the running first-minimum over the candidate list: a NaN wins, and then nothing replaces it (torch.min)
struct FirstMin {
    float best;
    int idx, n;
    __device__ __forceinline__ void add(float v) {
        if (n == 0 || v < best || (v != v && best == best)) {
            best = v;
            idx = n;
        }
        ++n;
    }
};

// ---------------------------------------------------------------------------------------------
// forward: per source warp + mask into the LDS planes (lx = synth m, ly = tgt m, ls = src m at the target pixel), R_s and I_s of the own
// pixel into registers; a barrier, the next source over the same planes; then the candidates, select, pmap and one partial sum per workgroup
// ---------------------------------------------------------------------------------------------
template <int PAD>
__global__ __launch_bounds__(NTHREADS) void k_warp_photo_window_fwd(
    const float* __restrict__ depth, const float* __restrict__ src0, const float* __restrict__ src1, e2e_strides ss,
    const float* __restrict__ tgt, e2e_strides ts, const float* __restrict__ K, const float* __restrict__ invK,
    const float* __restrict__ T, const float* __restrict__ noise, float* __restrict__ synth, float* __restrict__ valid,
    int* __restrict__ select, float* __restrict__ pmap, int use_mask, int terms, float* __restrict__ partials, int S, int B, int H, int W) {
    __shared__ float lx[3][FP_N], ly[3][FP_N], ls[3][FP_N];
    __shared__ float red[NTHREADS / 64];
    const int b = blockIdx.z, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int tid = threadIdx.y * TW + threadIdx.x;
    const int64_t N = (int64_t)H * W;
    const bool automask = (terms & E2E_TERM_AUTO_MASKING) != 0, minrep = (terms & E2E_TERM_MIN_REPROJECTION) != 0;
    const float* dep = depth + b * N;
    const float* tb = tgt + b * ts.sb;
    const int px = tx0 + threadIdx.x, py = ty0 + threadIdx.y;
    const bool live = px < W && py < H;
    const int w0 = threadIdx.y * FP_LD + threadIdx.x;
    float Rv[MAX_S] = {0.f, 0.f}, Iv[MAX_S] = {0.f, 0.f};

#pragma unroll
    for (int s = 0; s < MAX_S; ++s) {
        if (s >= S) break;                               // S is a kernel argument: the whole workgroup leaves together
        const int64_t sbi = (int64_t)s * B + b;
        const Geom g = load_geom(K + b * 16, invK + b * 16, T + sbi * 16);
        const float* sb = (s ? src1 : src0) + b * ss.sb;
        if (s) __syncthreads();                          // every thread has taken source s-1's values out of the planes
        for (int i = tid; i < FP_N; i += NTHREADS) {
            const int l_y = i / FP_LD, l_x = i % FP_LD;
            const int gy = ty0 + l_y - 1, gx = tx0 + l_x - 1;
            float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
            if (gx >= -1 && gx <= W && gy >= -1 && gy <= H) {
                const int qx = reflect1(gx, W), qy = reflect1(gy, H);
                const Proj p = project_pixel(g, (float)qx, (float)qy, dep[(int64_t)qy * W + qx], W, H);
                float mx, my;
                const float ix = source_index<PAD, false>(p.gx, W, mx);
                const float iy = source_index<PAD, false>(p.gy, H, my);
                const Bilin bl = bilinear_setup(ix, iy, W, H);
                float sm[3];
                sample3(sb, ss, bl, sm);
                const float m = use_mask ? p.mask : 1.f;
                const float* tp = tb + qy * ts.sh + qx * ts.sw;
                const float* ip = sb + qy * ss.sh + qx * ss.sw;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xv[c] = sm[c] * m;
                    yv[c] = tp[c * ts.sc] * m;
                    if (automask) sv[c] = ip[c * ss.sc] * m;
                }
                if (qx == gx && qy == gy && l_x >= 1 && l_x <= TW && l_y >= 1 && l_y <= TH) {  // tile interior, real pixel
                    valid[sbi * N + (int64_t)qy * W + qx] = p.mask;
#pragma unroll
                    for (int c = 0; c < 3; ++c) synth[(sbi * 3 + c) * N + (int64_t)qy * W + qx] = sm[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lx[c][i] = xv[c];
                ly[c][i] = yv[c];
                ls[c][i] = sv[c];
            }
        }
        __syncthreads();
        if (live) {
            Rv[s] = photo_value(lx, ly, w0);
            if (automask) Iv[s] = photo_value(ls, ly, w0);
        }
    }

    float val = 0.f;
    if (live) {
        const int64_t pix = (int64_t)py * W + px;
        FirstMin f = {0.f, 0, 0};
        if (automask) {
            if (minrep) {
#pragma unroll
                for (int s = 0; s < MAX_S; ++s)
                    if (s < S) f.add(noise ? Iv[s] + noise[((int64_t)b * S + s) * N + pix] : Iv[s]);
            } else {
                f.add(S == 2 ? (Iv[0] + Iv[1]) / 2.f : Iv[0]);
            }
        }
        if (minrep) {
#pragma unroll
            for (int s = 0; s < MAX_S; ++s)
                if (s < S) f.add(Rv[s]);
        } else {
            f.add(S == 2 ? (Rv[0] + Rv[1]) / 2.f : Rv[0]);
        }
        val = f.best;
        select[b * N + pix] = f.idx;
        if (pmap) pmap[b * N + pix] = val;
    }
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const float s0 = block_sum(val, red);
    if (tid == 0) partials[blk] = s0;
}

// ---------------------------------------------------------------------------------------------
// backward: per source the photometric adjoint (3x3 box + reflect pad fold-back) with the per-pixel weight of that source's reprojection map,
// then the warp adjoint; g_depth_tgt accumulates in a register over the sources and is stored once.  POSE: per source the workgroup's 12
// float64 sums of gc_r X_j | gc_r in partials[((s B + b) tiles + tile) * 12 + r * 4 + j]; every thread takes part, dead pixels add zeros.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float source_weight(int sel, int s, int nI, bool minrep, float gl, float gl_mean) {
    if (sel < nI) return 0.f;                            // an identity candidate won: constants only
    if (minrep) return (sel - nI == s) ? gl : 0.f;
    return gl_mean;
}

template <int PAD, bool POSE>
__global__ __launch_bounds__(NTHREADS) void k_warp_photo_window_bwd(
    const float* __restrict__ depth, const float* __restrict__ src0, const float* __restrict__ src1, e2e_strides ss,
    const float* __restrict__ tgt, e2e_strides ts, const float* __restrict__ K, const float* __restrict__ invK,
    const float* __restrict__ T, const float* __restrict__ synth, const float* __restrict__ valid, const int* __restrict__ select,
    int use_mask, int terms, const float* __restrict__ g_loss, float* __restrict__ g_dt, double* __restrict__ partials, int S, int B, int H,
    int W) {
    __shared__ float lx[3][BP_N], ly[3][BP_N];
    __shared__ float lg[9][BG_N];
    __shared__ double sh[POSE ? WP_NSUM : 1][NTHREADS / 64];
    const int b = blockIdx.z, tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH;
    const int tid = threadIdx.y * TW + threadIdx.x;
    const int64_t N = (int64_t)H * W;
    const bool automask = (terms & E2E_TERM_AUTO_MASKING) != 0, minrep = (terms & E2E_TERM_MIN_REPROJECTION) != 0;
    const int nI = automask ? (minrep ? S : 1) : 0;
    const float kmean = 1.f / ((float)B * (float)H * (float)W);
    const float gl = g_loss[0] * kmean;                  // upstream on every element of the minimum map
    const float gl_mean = (S == 2) ? gl / 2.f : gl;      // ... and on each R_s under mean_s R_s
    const float* tb = tgt + b * ts.sb;
    const int* selb = select + b * N;
    const int px = tx0 + threadIdx.x, py = ty0 + threadIdx.y;
    const bool live = px < W && py < H;
    const int64_t pix = (int64_t)py * W + px;
    const int sel_own = live ? selb[pix] : 0;
    const float d = live ? depth[b * N + pix] : 0.f;
    float mult[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx, qy = py + dy;
            mult[(dy + 1) * 3 + dx + 1] = (!live || qx < 0 || qx >= W || qy < 0 || qy >= H) ? 0.f : refl_mult(px, qx, W) * refl_mult(py, qy, H);
        }
    float gd = 0.f;

#pragma unroll                                           // unrolled: the rolled loop takes 14 more VGPRs
    for (int s = 0; s < MAX_S; ++s) {
        if (s >= S) break;                               // S is a kernel argument: the whole workgroup leaves together
        const int64_t sbi = (int64_t)s * B + b;
        const float* syn = synth + sbi * 3 * N;
        const float* val = valid + sbi * N;
        if (s) __syncthreads();                          // source s-1's planes (and its pose sums) have been read
        for (int i = tid; i < BP_N; i += NTHREADS) {
            const int l_y = i / BP_LD, l_x = i % BP_LD;
            const int gy = ty0 + l_y - 2, gx = tx0 + l_x - 2;
            float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f};
            if (gx >= -1 && gx <= W && gy >= -1 && gy <= H) {
                const int qx = reflect1(gx, W), qy = reflect1(gy, H);
                const int64_t o = (int64_t)qy * W + qx;
                const float m = use_mask ? val[o] : 1.f;
                const float* tp = tb + qy * ts.sh + qx * ts.sw;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    xv[c] = syn[c * N + o] * m;
                    yv[c] = tp[c * ts.sc] * m;
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                lx[c][i] = xv[c];
                ly[c][i] = yv[c];
            }
        }
        __syncthreads();
        for (int i = tid; i < BG_N; i += NTHREADS) {
            const int l_y = i / BG_LD, l_x = i % BG_LD;
            const int qy = ty0 + l_y - 1, qx = tx0 + l_x - 1;
            const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const float wq = in ? source_weight(selb[(int64_t)qy * W + qx], s, nI, minrep, gl, gl_mean) : 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float G1 = 0.f, G2 = 0.f, G3 = 0.f;
                if (in) {
                    const Stats st = window_stats(lx[c] + l_y * BP_LD + l_x, ly[c] + l_y * BP_LD + l_x, BP_LD);
                    ssim_partials(st, wq * (0.85f / 3.f), G1, G2, G3);
                }
                lg[c * 3 + 0][i] = G1;
                lg[c * 3 + 1][i] = G2;
                lg[c * 3 + 2][i] = G3;
            }
        }
        __syncthreads();

        [[maybe_unused]] double acc[WP_NSUM];            // POSE only: this pixel's gc_r X_j | gc_r
#pragma unroll
        for (int k = 0; k < WP_NSUM; ++k) acc[k] = 0.0;
        if (live) {
            const float w_own = source_weight(sel_own, s, nI, minrep, gl, gl_mean);
            const int ctr = (threadIdx.y + 2) * BP_LD + threadIdx.x + 2;
            const float m = use_mask ? val[pix] : 1.f;
            float G[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int gi = (threadIdx.y + dy) * BG_LD + threadIdx.x + dx;
                        const float mm = mult[dy * 3 + dx];
                        s1 += mm * lg[c * 3 + 0][gi];
                        s2 += mm * lg[c * 3 + 1][gi];
                        s3 += mm * lg[c * 3 + 2][gi];
                    }
                const float xv = lx[c][ctr], yv = ly[c][ctr];
                float gx_ = (s1 + 2.f * xv * s2 + yv * s3) / 9.f;
                const float df = yv - xv;
                const float sg = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
                gx_ -= w_own * (0.15f / 3.f) * sg;
                G[c] = gx_ * m;                          // d/d synth = d/dx * mask
            }
            // warp adjoint: d synth / d grid (bilinear), grid -> (u,v) -> c -> depth
            const Geom g = load_geom(K + b * 16, invK + b * 16, T + sbi * 16);
            const Proj p = project_pixel(g, (float)px, (float)py, d, W, H);
            float mx, my;
            const float ix = source_index<PAD, false>(p.gx, W, mx);
            const float iy = source_index<PAD, false>(p.gy, H, my);
            const Bilin bl = bilinear_setup(ix, iy, W, H);
            const float* sp = (s ? src1 : src0) + b * ss.sb + bl.y0 * ss.sh + bl.x0 * ss.sw;
            float gix = 0.f, giy = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float* pc = sp + c * ss.sc;
                const float nw = (bl.in_y0 & bl.in_x0) ? pc[0] : 0.f;
                const float ne = (bl.in_y0 & bl.in_x1) ? pc[ss.sw] : 0.f;
                const float sw = (bl.in_y1 & bl.in_x0) ? pc[ss.sh] : 0.f;
                const float se = (bl.in_y1 & bl.in_x1) ? pc[ss.sh + ss.sw] : 0.f;
                gix += G[c] * ((ne - nw) * (1.f - bl.ty) + (se - sw) * bl.ty);
                giy += G[c] * ((sw - nw) * (1.f - bl.tx) + (se - ne) * bl.tx);
            }
            const float gu = (mx * gix) * 2.f / (float)(W - 1);
            const float gv = (my * giy) * 2.f / (float)(H - 1);
            const float gc0 = gu / p.z, gc1 = gv / p.z, gc2 = -(gu * p.u + gv * p.v) / p.z;
            gd += gc0 * p.r[0] + gc1 * p.r[1] + gc2 * p.r[2];
            if constexpr (POSE) {
                const float gc[3] = {gc0, gc1, gc2};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[r * 4 + j] = (double)gc[r] * (double)(d * p.cam[j]);
                    acc[r * 4 + 3] = (double)gc[r];
                }
            }
        }
        if constexpr (POSE) {  // every thread of the workgroup is here: wave shuffle, then the four waves in order through LDS
#pragma unroll
            for (int k = 0; k < WP_NSUM; ++k) {
                const double v = wave_sum_d(acc[k]);
                if ((tid & 63) == 0) sh[k][tid >> 6] = v;
            }
            __syncthreads();
            if (tid == 0) {
                const int64_t tiles = (int64_t)gridDim.x * gridDim.y;
                double* out = partials + (sbi * tiles + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * WP_NSUM;
#pragma unroll
                for (int k = 0; k < WP_NSUM; ++k) out[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
            }
        }
    }
    if (live) g_dt[b * N + pix] = gd;
}

// what both entry points refuse before they look at their own pointers
int check_window(const char* name, int S, int B, int H, int W, int padding_mode, int terms) {
    E2E_REQUIRE(S >= 1 && S <= MAX_S, E2E_ERR_ARG, "%s: S=%d source frames (1 or 2)", name, S);
    E2E_REQUIRE(B > 0 && B <= 65535 && H > 1 && W > 1 && (int64_t)B * H * W < (1ll << 31), E2E_ERR_ARG, "%s: bad dims B=%d H=%d W=%d", name,
                B, H, W);
    E2E_REQUIRE(padding_mode == E2E_PADDING_BORDER || padding_mode == E2E_PADDING_ZEROS, E2E_ERR_ARG,
                "%s: padding_mode %d not supported (zeros|border)", name, padding_mode);
    E2E_REQUIRE((terms & ~(E2E_TERM_AUTO_MASKING | E2E_TERM_MIN_REPROJECTION)) == 0, E2E_ERR_ARG,
                "%s: terms %d (E2E_TERM_AUTO_MASKING | E2E_TERM_MIN_REPROJECTION; the geometric term stays on the operators)", name, terms);
    return E2E_OK;
}

}  // namespace

extern "C" {

int64_t e2e_warp_photo_window_workspace_floats(int S, int B, int H, int W) {
    if (S < 1 || S > MAX_S || B <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)B * tile_count(H, W);
}

int e2e_warp_photo_window_fwd(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides, const float* tgt,
                              e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T, const float* tie_noise, float* synth,
                              float* valid, int* select, float* pmap, int use_mask, int padding_mode, int terms, float* loss_out,
                              float* workspace, int S, int B, int H, int W, void* stream) {
    const int rc = check_window("e2e_warp_photo_window_fwd", S, B, H, W, padding_mode, terms);
    if (rc != E2E_OK) return rc;
    E2E_REQUIRE(depth_tgt && src0 && (src1 || S == 1) && tgt && K && inv_K && T && synth && valid && select && loss_out && workspace, E2E_ERR_ARG,
                "e2e_warp_photo_window_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g = tile_grid(B, H, W);
    if (padding_mode == E2E_PADDING_BORDER)
        hipLaunchKernelGGL(k_warp_photo_window_fwd<E2E_PAD_BORDER>, g, dim3(TW, TH), 0, st, depth_tgt, src0, src1, src_strides, tgt, tgt_strides,
                           K, inv_K, T, tie_noise, synth, valid, select, pmap, use_mask, terms, workspace, S, B, H, W);
    else
        hipLaunchKernelGGL(k_warp_photo_window_fwd<E2E_PAD_ZEROS>, g, dim3(TW, TH), 0, st, depth_tgt, src0, src1, src_strides, tgt, tgt_strides,
                           K, inv_K, T, tie_noise, synth, valid, select, pmap, use_mask, terms, workspace, S, B, H, W);
    E2E_LAUNCH_CHECK("e2e_warp_photo_window_fwd");
    const float scale = (float)(1.0 / ((double)B * H * W));
    warp_photo_reduce_launch(workspace, (int)(g.x * g.y * g.z), 1, scale, loss_out, st);
    E2E_LAUNCH_CHECK("e2e_warp_photo_window_fwd(reduce)");
    return E2E_OK;
}

int64_t e2e_warp_photo_window_bwd_workspace_bytes(int S, int B, int H, int W) {
    if (S < 1 || S > MAX_S || B <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)S * B * tile_count(H, W) * WP_NSUM * 8;
}

int e2e_warp_photo_window_bwd(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides, const float* tgt,
                              e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T, const float* synth,
                              const float* valid, const int* select, int use_mask, int padding_mode, int terms, const float* g_loss,
                              float* g_depth_tgt, float* g_T, void* workspace, int S, int B, int H, int W, void* stream) {
    const int rc = check_window("e2e_warp_photo_window_bwd", S, B, H, W, padding_mode, terms);
    if (rc != E2E_OK) return rc;
    E2E_REQUIRE(depth_tgt && src0 && (src1 || S == 1) && tgt && K && inv_K && T && synth && valid && select && g_loss && g_depth_tgt, E2E_ERR_ARG,
                "e2e_warp_photo_window_bwd: null pointer");
    E2E_REQUIRE(!g_T || workspace, E2E_ERR_ARG, "e2e_warp_photo_window_bwd: g_T without workspace");
    hipStream_t st = (hipStream_t)stream;
    const dim3 g = tile_grid(B, H, W);
#define WINDOW_BWD(PADV, POSEV)                                                                                                            \
    hipLaunchKernelGGL((k_warp_photo_window_bwd<PADV, POSEV>), g, dim3(TW, TH), 0, st, depth_tgt, src0, src1, src_strides, tgt, tgt_strides, K, \
                       inv_K, T, synth, valid, select, use_mask, terms, g_loss, g_depth_tgt, (double*)workspace, S, B, H, W)
    if (padding_mode == E2E_PADDING_BORDER) {
        if (g_T) WINDOW_BWD(E2E_PAD_BORDER, true);
        else WINDOW_BWD(E2E_PAD_BORDER, false);
    } else {
        if (g_T) WINDOW_BWD(E2E_PAD_ZEROS, true);
        else WINDOW_BWD(E2E_PAD_ZEROS, false);
    }
#undef WINDOW_BWD
    E2E_LAUNCH_CHECK("e2e_warp_photo_window_bwd");
    if (g_T) {
        warp_photo_pose_final_launch((const double*)workspace, (int)tile_count(H, W), K, g_T, S, B, st);
        E2E_LAUNCH_CHECK("e2e_warp_photo_window_bwd(final)");
    }
    return E2E_OK;
}

}  // extern "C"
