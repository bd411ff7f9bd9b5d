// warp_photo_window.hip -- the fused warp-photometric pair over a window of S = 1 or 2 source frames (DATA.frames: [0,-1,1], [0,-1], [0,1]) with
// the candidate / minimum logic of the reference's train_depth.py:621-662 (LOSS.auto_masking, LOSS.min_reprojection), and the same window WITH
// the geometric-consistency term of the reference's LOSS.geometric branch (train_depth.py:558-576, view_synthesis.py:54-78, losses.py:84-95).
// ONE forward template <PAD, GEO> and ONE backward template <PAD, SUMS, GEO> (SUMS: no sums, the pose sums, those and the intrinsics') serve e2e_warp_photo_window_* (GEO = false) and
// e2e_warp_photo_geo_* (GEO = true): the text is the geometric kernel's, and the compile-time constant GEO deletes the geometric pieces
// from the window's instantiation (profiles/warp_window_geo_merge.txt).  One tile launch forward (+ the fixed-order reduction of the workgroups'
// partial sums), one tile launch backward (+ a final kernel per source and batch element when the gradient with respect to the poses is
// asked for).  On the host the eight entry points fill one operand struct and share ONE forward path (window_fwd<GEO>) and ONE backward path
// (window_bwd<GEO>, without or with the intrinsics); the workspace layouts are stated once, for the size queries and the paths alike.
//
// Semantics of the window.  For source s with its validity mask m_s (1 everywhere when use_mask == 0):
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
// Semantics with the geometric term (GEO).  The photometric side is the window's to the letter (candidates, order, select, pmap, NaN rule,
// tie_noise, the g_T convention), with ONE difference: under LOSS.geometric the reference samples the source image with align_corners=True
// (sic), so synth and its adjoint use that index.
//
// The geometric term of source s, per target pixel with c = d M [x,y,1]^T + p4 and the grid of z = c2 + 1e-7:
//     wd = max(c2, 1e-3);   id = bilinear sample of depth_src_s on the same grid with align_corners=False (same padding mode);
//     diff = clamp(|wd - id| / (wd + id), 0, 1);   n_s = sum(valid_s) over the batch;   G_s = sum(diff valid_s) / n_s if n_s > geo_min_valid, else 0.
// valid_s = max|grid| <= 1 whatever use_mask says.  The piece is per pixel: no halo and no LDS plane.  n_s is an integer sum of the fp32
// validity decision (per-workgroup int partials, added by k_geo_final); the diff sums are float per workgroup in the fixed order of
// block_sum, then float64 in a fixed order.
//
// Backward of g_loss[0] loss[0] + sum_s g_loss[1+s] G_s.  The geometric adjoint of a valid pixel, only when the gate of s is open
// (geo_count[s] > geo_min_valid, read on the device):  e = g_loss[1+s] / n_s,  sg = sign(wd - id) (0 at 0), the clamp passes on [0,1];
//     d/dwd = e sg 2 id / (wd + id)^2, reaching c2 where c2 >= 1e-3;     d/did = -e sg 2 wd / (wd + id)^2, which goes
//     (i) to the four taps of depth_src_s (e2e_grid_sample_bwd's g_input conventions) and (ii) to the sampling position (its g_grid
//     conventions: align_corners=False scaling, zero slope under an active border clamp) and from there through z into gc.
// Both add into the gc of the photometric adjoint, so g_depth_tgt = gc . r and the 12 float64 pose sums carry the term.  A closed gate -- or
// an upstream g_loss[1+s] of exactly 0 -- skips the piece: g_depth_tgt and g_T then have the bits of the photometric part alone and
// g_depth_src[s] is all zero.
//
// Scale groups (e2e_warp_photo_geo_groups_fwd / _bwd: monodepth2's disparity pyramid, the scales stacked along the batch).  The batch is G
// groups of B / G items, group g the items g B / G ... (g + 1) B / G - 1, and ONLY the term's reduction and gate are per group: n_{s,g}, G_{s,g}
// and the upstream g_loss[1 + s G + g] live in slot [s G + g].  The forward tile kernel is untouched: its partials are batch-major, so
// k_geo_final sums a group's run of blocks exactly as it sums a whole call's, and group g comes out with the bits of a call on its slice.
// The backward tile kernel reads its item's slot.  The other entry points are the G = 1 case of the same two kernels.
//
// (i) is a data-dependent scatter.  It is made order-independent as in e2e_grid_sample_bwd_exact: 2^-48 fixed-point int64 atomic adds into
// workspace zeroed by the call, then a conversion pass that writes all of g_depth_src; a contribution that is not finite or not below 4096
// is not added and turns that source's plane into NaN (one poison word per source).  Size: 4 taps x 8 B per valid pixel, 19.7 MB at
// 480x640 with S = 2, about 15 us at the chip-wide atomic rate of 1.3 TB/s -- below the tile kernel's own time, and spread over rows as
// the sampling positions are.  Two runs give the same bits on every output.
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
constexpr double FX_ONE = 281474976710656.0;                                                  // 2^48

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

// the four taps of a one-channel (H,W) plane at one position, zeros outside
struct Taps {
    float nw, ne, sw, se;
};
__device__ __forceinline__ Taps load_taps(const float* __restrict__ plane, int W, const Bilin& bl) {
    const float* p = plane + (int64_t)bl.y0 * W + bl.x0;
    Taps t;
    t.nw = (bl.in_y0 & bl.in_x0) ? p[0] : 0.f;
    t.ne = (bl.in_y0 & bl.in_x1) ? p[1] : 0.f;
    t.sw = (bl.in_y1 & bl.in_x0) ? p[W] : 0.f;
    t.se = (bl.in_y1 & bl.in_x1) ? p[W + 1] : 0.f;
    return t;
}

// the workgroup's integer sum, valid in thread 0; `scratch` holds NTHREADS / 64 ints and is this call's alone
__device__ __forceinline__ int block_sum_i(int v, int* scratch) {
    const int tid = threadIdx.y * TW + threadIdx.x;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) scratch[tid >> 6] = v;
    __syncthreads();
    return tid == 0 ? ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3] : 0;
}

// ---------------------------------------------------------------------------------------------
// forward: per source warp + mask into the LDS planes (lx = synth m, ly = tgt m, ls = src m at the target pixel), R_s and I_s of the own
// pixel into registers; a barrier, the next source over the same planes; then the candidates, select, pmap and one partial sum per workgroup.
// GEO: the image index is align_corners=True; the thread that projects a real tile-interior pixel for the planes also takes that pixel's
// depth sample and adds diff | 1 to its own sums of source s.  Without GEO dsrc0 / dsrc1 / gpart / cpart are not read (the window passes NULL).
// ---------------------------------------------------------------------------------------------
template <int PAD, bool GEO>
__global__ __launch_bounds__(NTHREADS) void k_warp_photo_window_fwd(
    const float* __restrict__ depth, const float* __restrict__ dsrc0, const float* __restrict__ dsrc1, const float* __restrict__ src0,
    const float* __restrict__ src1, e2e_strides ss, const float* __restrict__ tgt, e2e_strides ts, const float* __restrict__ K,
    const float* __restrict__ invK, const float* __restrict__ T, const float* __restrict__ noise, float* __restrict__ synth,
    float* __restrict__ valid, int* __restrict__ select, float* __restrict__ pmap, int use_mask, int terms, float* __restrict__ partials,
    float* __restrict__ gpart, int* __restrict__ cpart, int S, int B, int H, int W) {
    __shared__ float lx[3][FP_N], ly[3][FP_N], ls[3][FP_N];
    __shared__ float red[GEO ? 1 + MAX_S : 1][NTHREADS / 64];
    __shared__ int redi[GEO ? MAX_S : 1][NTHREADS / 64];
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
    float gsum[MAX_S] = {0.f, 0.f};
    int gcnt[MAX_S] = {0, 0};

#pragma unroll
    for (int s = 0; s < MAX_S; ++s) {
        if (s >= S) break;                               // S is a kernel argument: the whole workgroup leaves together
        const int64_t sbi = (int64_t)s * B + b;
        const Geom g = load_geom(K + b * 16, invK + b * 16, T + sbi * 16);
        const float* sb = (s ? src1 : src0) + b * ss.sb;
        const float* dsb = (s ? dsrc1 : dsrc0) + b * N;
        if (s) __syncthreads();                          // every thread has taken source s-1's values out of the planes
        for (int i = tid; i < FP_N; i += NTHREADS) {
            const int l_y = i / FP_LD, l_x = i % FP_LD;
            const int gy = ty0 + l_y - 1, gx = tx0 + l_x - 1;
            float xv[3] = {0.f, 0.f, 0.f}, yv[3] = {0.f, 0.f, 0.f}, sv[3] = {0.f, 0.f, 0.f};
            if (gx >= -1 && gx <= W && gy >= -1 && gy <= H) {
                const int qx = reflect1(gx, W), qy = reflect1(gy, H);
                const float dq = dep[(int64_t)qy * W + qx];
                const Proj p = project_pixel(g, (float)qx, (float)qy, dq, W, H);
                float mx, my;
                const float ix = source_index<PAD, GEO>(p.gx, W, mx);       // GEO: align_corners=True for the image (train_depth.py:570)
                const float iy = source_index<PAD, GEO>(p.gy, H, my);
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
                    if (GEO && p.mask != 0.f) {          // the geometric term of this pixel: the depth sample with align_corners=False
                        const float c2 = fmaf(dq, p.r[2], g.P[11]);
                        const float wd = fmaxf(c2, 1e-3f);
                        float mdx, mdy;
                        const float idx_ = source_index<PAD, false>(p.gx, W, mdx);
                        const float idy_ = source_index<PAD, false>(p.gy, H, mdy);
                        const Bilin bd = bilinear_setup(idx_, idy_, W, H);
                        const Taps t = load_taps(dsb, W, bd);
                        const float id = ((t.nw * bd.wnw + t.ne * bd.wne) + t.sw * bd.wsw) + t.se * bd.wse;
                        const float r = fabsf(wd - id) / (wd + id);
                        gsum[s] += (r != r) ? r : fminf(fmaxf(r, 0.f), 1.f);      // torch.clamp keeps a NaN
                        gcnt[s] += 1;
                    }
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
    const int nblk = gridDim.x * gridDim.y * gridDim.z;
    const float s0 = block_sum(val, red[0]);
    if (tid == 0) partials[blk] = s0;
#pragma unroll
    for (int s = 0; s < MAX_S; ++s) {
        if (!GEO || s >= S) break;
        const float gs = block_sum(gsum[s], red[1 + s]);
        const int gn = block_sum_i(gcnt[s], redi[s]);
        if (tid == 0) {
            gpart[(int64_t)s * nblk + blk] = gs;
            cpart[(int64_t)s * nblk + blk] = gn;
        }
    }
}

// one wave per source and scale group (grid (S, G); G = 1: the whole call): lane l adds the group's workgroup partials l, l + 64, ... counted
// from the group's first block, in order, then a fixed shuffle tree; the count is an integer sum.  The tile kernel numbers its blocks
// batch-major, so group g owns the nblk / G blocks from g nblk / G on, and its sum is the sum a call on that group's slice would form.
__global__ __launch_bounds__(64) void k_geo_final(const float* __restrict__ gpart, const int* __restrict__ cpart, int nblk, int geo_min_valid,
                                                  int* __restrict__ geo_count, float* __restrict__ loss_out) {
    const int s = blockIdx.x, g = blockIdx.y, G = gridDim.y, lane = threadIdx.x;
    const int per_group = nblk / G;
    const int64_t first = (int64_t)s * nblk + (int64_t)g * per_group;
    double a = 0.0;
    long long n = 0;
    for (int i = lane; i < per_group; i += 64) {
        a += (double)gpart[first + i];
        n += cpart[first + i];
    }
    a = wave_sum_d(a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if (lane == 0) {
        geo_count[s * G + g] = (int)n;
        loss_out[1 + s * G + g] = (n > (long long)geo_min_valid) ? (float)(a / (double)n) : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// backward: per source the photometric adjoint (3x3 box + reflect pad fold-back) with the per-pixel weight of that source's reprojection map,
// then the warp adjoint; g_depth_tgt accumulates in a register over the sources and is stored once.  POSE: per source the workgroup's 12
// float64 sums of gc_r X_j | gc_r in partials[((s B + b) tiles + tile) * 12 + r * 4 + j]; every thread takes part, dead pixels add zeros.
// SUMS = WP_SUMS_INTRINSICS: a pass of its own (see k_warp_photo_bwd, warp_photo.hip, for why) that stores ONLY the 9 sums of gc_r d pix_j,
// in a second region behind the pose sums, [((s B + b) tiles + tile) * 9 + r * 3 + j]: no depth gradient, no depth scatter, no pose sums.
// GEO: the image index is align_corners=True, and per source the geometric adjoint of the own pixel is added.  Without GEO dsrc0 / dsrc1 /
// geo_count / geo_min_valid / fx and g_loss[1..] are not read (the window passes NULL and 0).
// group_items = B / G, the batch items per scale group: item b reads the count and the upstream of slot s G + b / group_items.  Every entry
// point but the grouped pair passes B (one group, slot s).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float source_weight(int sel, int s, int nI, bool minrep, float gl, float gl_mean) {
    if (sel < nI) return 0.f;                            // an identity candidate won: constants only
    if (minrep) return (sel - nI == s) ? gl : 0.f;
    return gl_mean;
}

// one tap of the depth scatter: a 2^-48 fixed-point integer add, or the source's poison word (the range rule of e2e_grid_sample_bwd_exact)
__device__ __forceinline__ void scatter_tap(unsigned long long* dst, unsigned long long* poison, float v) {
    if (fabsf(v) < 4096.f) atomicAdd(dst, (unsigned long long)__double2ll_rn((double)v * FX_ONE));
    else atomicOr(poison, 1ull);
}

template <int PAD, int SUMS, bool GEO>
__global__ __launch_bounds__(NTHREADS) void k_warp_photo_window_bwd(
    const float* __restrict__ depth, const float* __restrict__ dsrc0, const float* __restrict__ dsrc1, const float* __restrict__ src0,
    const float* __restrict__ src1, e2e_strides ss, const float* __restrict__ tgt, e2e_strides ts, const float* __restrict__ K,
    const float* __restrict__ invK, const float* __restrict__ T, const float* __restrict__ synth, const float* __restrict__ valid,
    const int* __restrict__ select, const int* __restrict__ geo_count, int use_mask, int terms, int geo_min_valid,
    const float* __restrict__ g_loss, float* __restrict__ g_dt, unsigned long long* __restrict__ fx, double* __restrict__ partials, int S,
    int B, int H, int W, int group_items) {
    constexpr bool POSE = SUMS != WP_SUMS_NONE, INTR = SUMS == WP_SUMS_INTRINSICS;
    __shared__ float lx[3][BP_N], ly[3][BP_N];
    __shared__ float lg[9][BG_N];
    __shared__ double sh[POSE ? (INTR ? WP_NQ : WP_NSUM) : 1][NTHREADS / 64];
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
        const int slot = GEO ? s * (B / group_items) + b / group_items : 0;      // [s G + g] of this item's scale group; group_items = B: s
        const int ns = GEO ? geo_count[slot] : 0;
        const float e = (GEO && ns > geo_min_valid && ns > 0) ? g_loss[1 + slot] / (float)ns : 0.f;   // 0: the gate is closed, the piece is skipped
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
            const float vown = (GEO || use_mask) ? val[pix] : 1.f;
            const float m = use_mask ? vown : 1.f;
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
            // warp adjoint: d synth / d grid (bilinear, align_corners = GEO), grid -> (u,v) -> c -> depth
            const Geom g = load_geom(K + b * 16, invK + b * 16, T + sbi * 16);
            const Proj p = project_pixel(g, (float)px, (float)py, d, W, H);
            float mx, my;
            const float ix = source_index<PAD, GEO>(p.gx, W, mx);
            const float iy = source_index<PAD, GEO>(p.gy, H, my);
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
            float gu = (mx * gix) * 2.f / (float)(W - 1);
            float gv = (my * giy) * 2.f / (float)(H - 1);
            float gwd = 0.f;                             // the geometric adjoint on c2 through wd
            const bool geo = GEO && e != 0.f && vown != 0.f;
            if (geo) {
                const float c2 = fmaf(d, p.r[2], g.P[11]);
                const float wd = fmaxf(c2, 1e-3f);
                float mdx, mdy;
                const float idx_ = source_index<PAD, false>(p.gx, W, mdx);
                const float idy_ = source_index<PAD, false>(p.gy, H, mdy);
                const Bilin bd = bilinear_setup(idx_, idy_, W, H);
                const Taps t = load_taps((s ? dsrc1 : dsrc0) + b * N, W, bd);
                const float id = ((t.nw * bd.wnw + t.ne * bd.wne) + t.sw * bd.wsw) + t.se * bd.wse;
                const float df = wd - id, sum = wd + id;
                const float r = fabsf(df) / sum;
                const float sg = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
                const float k = (r >= 0.f && r <= 1.f) ? e * sg * 2.f / (sum * sum) : 0.f;     // the clamp passes on the closed interval
                const float gid = -k * wd;
                if (c2 >= 1e-3f) gwd = k * id;
                unsigned long long* dst = fx + sbi * N + (int64_t)bd.y0 * W + bd.x0;
                unsigned long long* poison = fx + (int64_t)S * B * N + s;
                if constexpr (!INTR) {                  // the Q pass adds nothing to the depth scatter: the pose pass has done it
                    if (bd.in_y0 & bd.in_x0) scatter_tap(dst, poison, gid * bd.wnw);
                    if (bd.in_y0 & bd.in_x1) scatter_tap(dst + 1, poison, gid * bd.wne);
                    if (bd.in_y1 & bd.in_x0) scatter_tap(dst + W, poison, gid * bd.wsw);
                    if (bd.in_y1 & bd.in_x1) scatter_tap(dst + W + 1, poison, gid * bd.wse);
                }
                const float gdx = gid * ((t.ne - t.nw) * (1.f - bd.ty) + (t.se - t.sw) * bd.ty);
                const float gdy = gid * ((t.sw - t.nw) * (1.f - bd.tx) + (t.se - t.ne) * bd.tx);
                gu += (mdx * gdx) * 2.f / (float)(W - 1);
                gv += (mdy * gdy) * 2.f / (float)(H - 1);
            }
            const float gc0 = gu / p.z, gc1 = gv / p.z;
            float gc2 = -(gu * p.u + gv * p.v) / p.z;
            if (geo) gc2 += gwd;
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
        if constexpr (POSE && !INTR) {  // every thread of the workgroup is here: wave shuffle, then the four waves in order through LDS
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
        if constexpr (INTR) {  // the Q pass: the same reduction for Q[r][j] = sum gc_r d pix_j, element by element (three live doubles)
            const double dd = (double)d;
            const double gcd[3] = {acc[3] * dd, acc[7] * dd, acc[11] * dd};     // acc[r][3] = (double)gc_r; a pixel outside the image has 0
            const double pixd[3] = {(double)px, (double)py, 1.0};               // exact
#pragma unroll
            for (int k = 0; k < WP_NQ; ++k) {
                const double v = wave_sum_d(gcd[k / 3] * pixd[k % 3]);
                if ((tid & 63) == 0) sh[k][tid >> 6] = v;
            }
            __syncthreads();
            if (tid == 0) {  // the second region, [S][B][tiles][9], behind the pose sums
                const int64_t tiles = (int64_t)gridDim.x * gridDim.y;
                double* q = partials + (int64_t)S * B * tiles * WP_NSUM + (sbi * tiles + (int64_t)blockIdx.y * gridDim.x + blockIdx.x) * WP_NQ;
#pragma unroll
                for (int k = 0; k < WP_NQ; ++k) q[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
            }
        }
    }
    if constexpr (INTR) return;                          // the Q pass stores no depth gradient: the pose pass has written it
    if (live) g_dt[b * N + pix] = gd;
}

// g_depth_src (S, B H W) from the fixed-point sums; a source whose poison word is set becomes NaN
__global__ void k_geo_fixed48_to_float(const long long* __restrict__ fx, float* __restrict__ out, int64_t per_source, int S) {
    const int64_t n = per_source * S;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool poisoned = fx[n + i / per_source] != 0;
        out[i] = poisoned ? __uint_as_float(0x7FC00000u) : (float)((double)fx[i] * (1.0 / FX_ONE));
    }
}

// ---- host: what the six entry points share, under the parameter names of include/e2eslam.h; the plain window leaves the geometric operands
// NULL / 0.  Never a kernel argument (that would change every kernarg layout, profiles/lossgrad_tile_refactor.txt).
struct WindowArgs {
    const float *depth_tgt, *depth_src0, *depth_src1, *src0, *src1;
    e2e_strides src_strides;
    const float* tgt;
    e2e_strides tgt_strides;
    const float *K, *inv_K, *T;
    int use_mask, padding_mode, terms, geo_min_valid;
    int S, B, H, W;
    int groups = 1;                                      // scale groups of the batch (the grouped geo pair sets it; see check_groups)
};
// the rest of each direction's list; an entry point sets by name what it has, the others stay NULL (the forward writes what the backward reads)
struct WindowFwdArgs : WindowArgs {
    const float* tie_noise;
    float *synth, *valid, *pmap, *loss_out, *workspace;
    int *select, *geo_count;
};
struct WindowBwdArgs : WindowArgs {
    const float *synth, *valid, *g_loss;
    const int *select, *geo_count;
    float *g_depth_tgt, *g_depth_src, *g_T, *g_K, *g_inv_K;
    void* workspace;
};

// what every entry point refuses before it looks at its own pointers (`name` = the entry point, geo = its geometric form; the messages are
// part of the interface)
int check_window(const char* name, bool geo, const WindowArgs& a) {
    E2E_REQUIRE(a.S >= 1 && a.S <= MAX_S, E2E_ERR_ARG, "%s: S=%d source frames (1 or 2)", name, a.S);
    E2E_REQUIRE(a.B > 0 && a.B <= 65535 && a.H > 1 && a.W > 1 && (int64_t)a.B * a.H * a.W < (1ll << 31), E2E_ERR_ARG,
                "%s: bad dims B=%d H=%d W=%d", name, a.B, a.H, a.W);
    E2E_REQUIRE(a.padding_mode == E2E_PADDING_BORDER || a.padding_mode == E2E_PADDING_ZEROS, E2E_ERR_ARG,
                "%s: padding_mode %d not supported (zeros|border)", name, a.padding_mode);
    E2E_REQUIRE((a.terms & ~(E2E_TERM_AUTO_MASKING | E2E_TERM_MIN_REPROJECTION)) == 0, E2E_ERR_ARG,
                "%s: terms %d (E2E_TERM_AUTO_MASKING | E2E_TERM_MIN_REPROJECTION; the geometric term %s)", name, a.terms,
                geo ? "is always on here" : "stays on the operators");
    E2E_REQUIRE(!geo || a.geo_min_valid >= 0, E2E_ERR_ARG, "%s: geo_min_valid %d is negative", name, a.geo_min_valid);
    return E2E_OK;
}

// the grouped geo pair's own refusals, after everything the geo pair refuses: the batch is `groups` scale groups of B / groups items each,
// group g the items g B / groups ... (g + 1) B / groups - 1.  The other entry points have one group and pass.
constexpr int MAX_GROUPS = 4;                            // PYRAMID_SCALES of e2e_disp_pyramid_depth_fwd
int check_groups(const char* name, const WindowArgs& a) {
    E2E_REQUIRE(a.groups >= 1 && a.groups <= MAX_GROUPS, E2E_ERR_ARG, "%s: groups=%d scale groups (1 to %d)", name, a.groups, MAX_GROUPS);
    E2E_REQUIRE(a.B % a.groups == 0, E2E_ERR_ARG, "%s: B=%d is not a multiple of groups=%d", name, a.B, a.groups);
    return E2E_OK;
}

bool bad_query(int S, int B, int H, int W) { return S < 1 || S > MAX_S || B <= 0 || H <= 0 || W <= 0; }     // every size query answers 0

// The forward workspace, for the two queries and the forward path alike, in floats: the loss partials [nblk], then with the geometric term the
// diff sums [S][nblk] (floats) and the validity counts [S][nblk] (ints)
struct FwdWorkspace {
    int64_t nblk, gpart, cpart, floats;
};
FwdWorkspace fwd_workspace(bool geo, int S, int B, int H, int W) {
    const int64_t nblk = (int64_t)B * tile_count(H, W);
    return {nblk, nblk, nblk * (1 + S), geo ? nblk * (1 + 2 * S) : nblk};
}

// the backward workspace: with the geometric term the fixed-point sums and one poison word per source come first, zeroed by the call
WarpPhotoBwdWorkspace bwd_workspace(bool geo, bool intrinsics, int S, int B, int H, int W) {
    return warp_photo_bwd_workspace(geo ? (int64_t)S * B * H * W + S : 0, intrinsics ? WP_SUMS_INTRINSICS : WP_SUMS_POSE, S, B, H, W);
}

// the PAD x SUMS instantiation of the backward tile kernel
template <bool GEO>
auto bwd_kernel(bool border, int sums) {
    if (border) {
        if (sums == WP_SUMS_INTRINSICS) return k_warp_photo_window_bwd<E2E_PAD_BORDER, WP_SUMS_INTRINSICS, GEO>;
        if (sums == WP_SUMS_POSE) return k_warp_photo_window_bwd<E2E_PAD_BORDER, WP_SUMS_POSE, GEO>;
        return k_warp_photo_window_bwd<E2E_PAD_BORDER, WP_SUMS_NONE, GEO>;
    }
    if (sums == WP_SUMS_INTRINSICS) return k_warp_photo_window_bwd<E2E_PAD_ZEROS, WP_SUMS_INTRINSICS, GEO>;
    if (sums == WP_SUMS_POSE) return k_warp_photo_window_bwd<E2E_PAD_ZEROS, WP_SUMS_POSE, GEO>;
    return k_warp_photo_window_bwd<E2E_PAD_ZEROS, WP_SUMS_NONE, GEO>;
}

// the forward of the window and of its geometric form: the tile launch, the reduction of the loss partials, with GEO the geometric term's final
template <bool GEO>
int window_fwd(const char* name, const WindowFwdArgs& a, hipStream_t st) {
    if (const int rc = check_window(name, GEO, a)) return rc;
    E2E_REQUIRE(a.depth_tgt && a.src0 && (a.src1 || a.S == 1) && a.tgt && a.K && a.inv_K && a.T && a.synth && a.valid && a.select && a.loss_out &&
                    a.workspace && (!GEO || (a.depth_src0 && (a.depth_src1 || a.S == 1) && a.geo_count)),
                E2E_ERR_ARG, "%s: null pointer", name);
    if (const int rc = check_groups(name, a)) return rc;
    const FwdWorkspace ws = fwd_workspace(GEO, a.S, a.B, a.H, a.W);
    float* gpart = GEO ? a.workspace + ws.gpart : nullptr;
    int* cpart = GEO ? (int*)(a.workspace + ws.cpart) : nullptr;
    const auto kernel = a.padding_mode == E2E_PADDING_BORDER ? k_warp_photo_window_fwd<E2E_PAD_BORDER, GEO> : k_warp_photo_window_fwd<E2E_PAD_ZEROS, GEO>;
    hipLaunchKernelGGL(kernel, tile_grid(a.B, a.H, a.W), dim3(TW, TH), 0, st, a.depth_tgt, a.depth_src0, a.depth_src1, a.src0, a.src1, a.src_strides,
                       a.tgt, a.tgt_strides, a.K, a.inv_K, a.T, a.tie_noise, a.synth, a.valid, a.select, a.pmap, a.use_mask, a.terms, a.workspace,
                       gpart, cpart, a.S, a.B, a.H, a.W);
    if (const int rc = warp_photo_launch_status(name, "")) return rc;
    const float scale = (float)(1.0 / ((double)a.B * a.H * a.W));
    warp_photo_reduce_launch(a.workspace, (int)ws.nblk, 1, scale, a.loss_out, st);
    if (const int rc = warp_photo_launch_status(name, "(reduce)")) return rc;
    if constexpr (GEO) {
        hipLaunchKernelGGL(k_geo_final, dim3(a.S, a.groups), dim3(64), 0, st, gpart, cpart, (int)ws.nblk, a.geo_min_valid, a.geo_count, a.loss_out);
        if (const int rc = warp_photo_launch_status(name, "(geometric)")) return rc;
    }
    return E2E_OK;
}

// The backward of the window and of its geometric form, without or with the gradient with respect to the intrinsics.  With it: the tile launch
// with the pose sums (the existing instantiation: the depth gradients and Pbar keep their bits), the tile launch in its third mode (the Q pass:
// 9 sums per workgroup and source into the region behind), then k_warp_photo_bwd_intrinsics_final; k_warp_photo_bwd_pose_final runs unchanged
// on the pose sums whenever g_T is asked for.
template <bool GEO>
int window_bwd(const char* name, bool intrinsics, const WindowBwdArgs& a, hipStream_t st) {
    if (const int rc = check_window(name, GEO, a)) return rc;
    // line 1: what all four need; line 2: the two geometric forms; line 3: the two intrinsics forms.  Those three always require workspace, so
    // only e2e_warp_photo_window_bwd can reach the second message.
    E2E_REQUIRE(a.depth_tgt && a.src0 && (a.src1 || a.S == 1) && a.tgt && a.K && a.inv_K && a.T && a.synth && a.valid && a.select && a.g_loss && a.g_depth_tgt &&
                    (!GEO || (a.depth_src0 && (a.depth_src1 || a.S == 1) && a.geo_count && a.g_depth_src && a.workspace)) &&
                    (!intrinsics || (a.g_K && a.g_inv_K && a.workspace)),
                E2E_ERR_ARG, "%s: null pointer", name);
    E2E_REQUIRE(!a.g_T || a.workspace, E2E_ERR_ARG, "%s: g_T without workspace", name);
    if (const int rc = check_groups(name, a)) return rc;
    const WarpPhotoBwdWorkspace ws = bwd_workspace(GEO, intrinsics, a.S, a.B, a.H, a.W);
    const int tiles = (int)tile_count(a.H, a.W);
    unsigned long long* fx = GEO ? (unsigned long long*)a.workspace : nullptr;
    double* partials = (double*)a.workspace + ws.partials;       // written only with the pose sums
    if constexpr (GEO)
        E2E_REQUIRE(hipMemsetAsync(fx, 0, (size_t)ws.partials * 8, st) == hipSuccess, E2E_ERR_LAUNCH,
                    "%s: hipMemsetAsync of the fixed-point scratch failed", name);
    const auto tile_pass = [&](int sums) {
        hipLaunchKernelGGL(bwd_kernel<GEO>(a.padding_mode == E2E_PADDING_BORDER, sums), tile_grid(a.B, a.H, a.W), dim3(TW, TH), 0, st, a.depth_tgt,
                           a.depth_src0, a.depth_src1, a.src0, a.src1, a.src_strides, a.tgt, a.tgt_strides, a.K, a.inv_K, a.T, a.synth, a.valid,
                           a.select, a.geo_count, a.use_mask, a.terms, a.geo_min_valid, a.g_loss, a.g_depth_tgt, fx, partials, a.S, a.B, a.H, a.W,
                           a.B / a.groups);
    };
    tile_pass(a.g_T || intrinsics ? WP_SUMS_POSE : WP_SUMS_NONE);
    if (intrinsics) tile_pass(WP_SUMS_INTRINSICS);                  // the Q pass, always second
    if (const int rc = warp_photo_launch_status(name, "")) return rc;
    if constexpr (GEO) {
        const int64_t per_source = (int64_t)a.B * a.H * a.W, n = per_source * a.S;
        hipLaunchKernelGGL(k_geo_fixed48_to_float, dim3((unsigned)((n + 255) / 256 > 4096 ? 4096 : (n + 255) / 256)), dim3(256), 0, st,
                           (const long long*)fx, a.g_depth_src, per_source, a.S);
        if (const int rc = warp_photo_launch_status(name, "(depth_src)")) return rc;
    }
    if (a.g_T) {
        warp_photo_pose_final_launch(partials, tiles, a.K, a.g_T, a.S, a.B, st);
        if (const int rc = warp_photo_launch_status(name, intrinsics ? "(pose)" : "(final)")) return rc;
    }
    if (intrinsics) {
        warp_photo_intrinsics_final_launch(partials, (double*)a.workspace + ws.q_partials, tiles, a.K, a.T, a.g_K, a.g_inv_K, a.S, a.B, st);
        if (const int rc = warp_photo_launch_status(name, "(final)")) return rc;
    }
    return E2E_OK;
}

}  // namespace

extern "C" {

int64_t e2e_warp_photo_window_workspace_floats(int S, int B, int H, int W) {
    return bad_query(S, B, H, W) ? 0 : fwd_workspace(false, S, B, H, W).floats;
}

int e2e_warp_photo_window_fwd(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides, const float* tgt,
                              e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T, const float* tie_noise, float* synth,
                              float* valid, int* select, float* pmap, int use_mask, int padding_mode, int terms, float* loss_out,
                              float* workspace, int S, int B, int H, int W, void* stream) {
    WindowFwdArgs a{{depth_tgt, nullptr, nullptr, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms, 0, S, B, H, W}};
    a.tie_noise = tie_noise; a.synth = synth; a.valid = valid; a.select = select; a.pmap = pmap; a.loss_out = loss_out; a.workspace = workspace;
    return window_fwd<false>("e2e_warp_photo_window_fwd", a, (hipStream_t)stream);
}

int64_t e2e_warp_photo_window_bwd_workspace_bytes(int S, int B, int H, int W) {
    return bad_query(S, B, H, W) ? 0 : bwd_workspace(false, false, S, B, H, W).words * 8;
}

int e2e_warp_photo_window_bwd(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides, const float* tgt,
                              e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T, const float* synth,
                              const float* valid, const int* select, int use_mask, int padding_mode, int terms, const float* g_loss,
                              float* g_depth_tgt, float* g_T, void* workspace, int S, int B, int H, int W, void* stream) {
    WindowBwdArgs a{{depth_tgt, nullptr, nullptr, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms, 0, S, B, H, W}};
    a.synth = synth; a.valid = valid; a.select = select; a.g_loss = g_loss; a.g_depth_tgt = g_depth_tgt; a.g_T = g_T; a.workspace = workspace;
    return window_bwd<false>("e2e_warp_photo_window_bwd", false, a, (hipStream_t)stream);
}

int64_t e2e_warp_photo_geo_workspace_floats(int S, int B, int H, int W) {
    return bad_query(S, B, H, W) ? 0 : fwd_workspace(true, S, B, H, W).floats;
}

int e2e_warp_photo_geo_fwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0, const float* src1,
                           e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T,
                           const float* tie_noise, float* synth, float* valid, int* select, float* pmap, int* geo_count, int use_mask,
                           int padding_mode, int terms, int geo_min_valid, float* loss_out, float* workspace, int S, int B, int H, int W,
                           void* stream) {
    WindowFwdArgs a{{depth_tgt, depth_src0, depth_src1, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms,
                      geo_min_valid, S, B, H, W}};
    a.tie_noise = tie_noise; a.synth = synth; a.valid = valid; a.select = select; a.pmap = pmap; a.loss_out = loss_out; a.workspace = workspace;
    a.geo_count = geo_count;
    return window_fwd<true>("e2e_warp_photo_geo_fwd", a, (hipStream_t)stream);
}

int64_t e2e_warp_photo_geo_bwd_workspace_bytes(int S, int B, int H, int W) {
    return bad_query(S, B, H, W) ? 0 : bwd_workspace(true, false, S, B, H, W).words * 8;
}

int e2e_warp_photo_geo_bwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0, const float* src1,
                           e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T,
                           const float* synth, const float* valid, const int* select, const int* geo_count, int use_mask, int padding_mode,
                           int terms, int geo_min_valid, const float* g_loss, float* g_depth_tgt, float* g_depth_src, float* g_T,
                           void* workspace, int S, int B, int H, int W, void* stream) {
    WindowBwdArgs a{{depth_tgt, depth_src0, depth_src1, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms,
                      geo_min_valid, S, B, H, W}};
    a.synth = synth; a.valid = valid; a.select = select; a.g_loss = g_loss; a.g_depth_tgt = g_depth_tgt; a.g_T = g_T; a.workspace = workspace;
    a.geo_count = geo_count; a.g_depth_src = g_depth_src;
    return window_bwd<true>("e2e_warp_photo_geo_bwd", false, a, (hipStream_t)stream);
}

int e2e_warp_photo_geo_groups_fwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0, const float* src1,
                                  e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                                  const float* T, const float* tie_noise, float* synth, float* valid, int* select, float* pmap, int* geo_count,
                                  int use_mask, int padding_mode, int terms, int geo_min_valid, float* loss_out, float* workspace, int S,
                                  int groups, int B, int H, int W, void* stream) {
    WindowFwdArgs a{{depth_tgt, depth_src0, depth_src1, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms,
                      geo_min_valid, S, B, H, W, groups}};
    a.tie_noise = tie_noise; a.synth = synth; a.valid = valid; a.select = select; a.pmap = pmap; a.loss_out = loss_out; a.workspace = workspace;
    a.geo_count = geo_count;
    return window_fwd<true>("e2e_warp_photo_geo_groups_fwd", a, (hipStream_t)stream);
}

int e2e_warp_photo_geo_groups_bwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0, const float* src1,
                                  e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                                  const float* T, const float* synth, const float* valid, const int* select, const int* geo_count, int use_mask,
                                  int padding_mode, int terms, int geo_min_valid, const float* g_loss, float* g_depth_tgt, float* g_depth_src,
                                  float* g_T, void* workspace, int S, int groups, int B, int H, int W, void* stream) {
    WindowBwdArgs a{{depth_tgt, depth_src0, depth_src1, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms,
                      geo_min_valid, S, B, H, W, groups}};
    a.synth = synth; a.valid = valid; a.select = select; a.g_loss = g_loss; a.g_depth_tgt = g_depth_tgt; a.g_T = g_T; a.workspace = workspace;
    a.geo_count = geo_count; a.g_depth_src = g_depth_src;
    return window_bwd<true>("e2e_warp_photo_geo_groups_bwd", false, a, (hipStream_t)stream);
}

int64_t e2e_warp_photo_window_bwd_intrinsics_workspace_bytes(int S, int B, int H, int W) {
    return bad_query(S, B, H, W) ? 0 : bwd_workspace(false, true, S, B, H, W).words * 8;
}

int e2e_warp_photo_window_bwd_intrinsics(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides, const float* tgt,
                                         e2e_strides tgt_strides, const float* K, const float* inv_K, const float* T, const float* synth,
                                         const float* valid, const int* select, int use_mask, int padding_mode, int terms, const float* g_loss,
                                         float* g_depth_tgt, float* g_T, float* g_K, float* g_inv_K, void* workspace, int S, int B, int H, int W,
                                         void* stream) {
    WindowBwdArgs a{{depth_tgt, nullptr, nullptr, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms, 0, S, B, H, W}};
    a.synth = synth; a.valid = valid; a.select = select; a.g_loss = g_loss; a.g_depth_tgt = g_depth_tgt; a.g_T = g_T; a.workspace = workspace;
    a.g_K = g_K; a.g_inv_K = g_inv_K;
    return window_bwd<false>("e2e_warp_photo_window_bwd_intrinsics", true, a, (hipStream_t)stream);
}

int64_t e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes(int S, int B, int H, int W) {
    return bad_query(S, B, H, W) ? 0 : bwd_workspace(true, true, S, B, H, W).words * 8;
}

int e2e_warp_photo_geo_bwd_intrinsics(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0,
                                      const float* src1, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides, const float* K,
                                      const float* inv_K, const float* T, const float* synth, const float* valid, const int* select,
                                      const int* geo_count, int use_mask, int padding_mode, int terms, int geo_min_valid, const float* g_loss,
                                      float* g_depth_tgt, float* g_depth_src, float* g_T, float* g_K, float* g_inv_K, void* workspace, int S,
                                      int B, int H, int W, void* stream) {
    WindowBwdArgs a{{depth_tgt, depth_src0, depth_src1, src0, src1, src_strides, tgt, tgt_strides, K, inv_K, T, use_mask, padding_mode, terms,
                      geo_min_valid, S, B, H, W}};
    a.synth = synth; a.valid = valid; a.select = select; a.g_loss = g_loss; a.g_depth_tgt = g_depth_tgt; a.g_T = g_T; a.workspace = workspace;
    a.geo_count = geo_count; a.g_depth_src = g_depth_src; a.g_K = g_K; a.g_inv_K = g_inv_K;
    return window_bwd<true>("e2e_warp_photo_geo_bwd_intrinsics", true, a, (hipStream_t)stream);
}

}  // extern "C"
