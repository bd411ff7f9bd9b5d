/* e2eslam.h -- C ABI of libe2eslam_hip.so: the MI355X (gfx950) implementation of the
 * online-refinement hot path of ivanalberico/End-To-End-Self-Supervised-SLAM.
 *
 * The reference has no FFI layer: its boundary for this path is the Python import surface of
 * online_adaption.py:15-36 / train_depth.py:17-38.  These entry points are what a
 * ctypes binding of that surface calls; each one cites the reference interface it replaces.
 * The Python host side lives in end-to-end-self-supervised-slam_amd/ (same module / class /
 * function names as the reference); INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 (or int64 / int32 where stated) unless marked `host`;
 *  - the caller owns every buffer (torch allocator); the library allocates nothing;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); no call synchronises;
 *  - return value 0 = OK, negative = E2E_ERR_*; e2e_last_error() gives a thread-local message;
 *  - image tensors are addressed through ELEMENT strides (sb, sc, sh, sw) so that the
 *    reference's NHWC frame stack (online_adaption.py:215-220) and its permuted NCHW views
 *    (online_adaption.py:393-394) are read in place, without a layout copy;
 *  - results are deterministic run to run: no floating-point atomics on any parity output.
 *
 * This file IS the Python binding (e2ehip/_lib.py parses it when it loads the library).  Grammar it accepts: every prototype is
 * `ret e2e_name(type name, ...);` or `ret e2e_name(void);` with ret one of int, int64_t, long long, const char*, and each parameter an
 * int, int64_t, long long, float, double, an e2e_strides by value or a pointer (any pointee, optionally const), always with a name;
 * structs are `typedef struct tag { fields } tag;` over the same types.  Parameter names are what the package's keyword calls bind to
 * (L.call(name, Hs=..., stream=...)) and what e2ehip/profile.py accounts by, so renaming one is a change to the package.
 */
#ifndef E2ESLAM_H
#define E2ESLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E2E_OK 0
#define E2E_ERR_ARG (-1)      /* bad argument (null pointer, non-positive size, unknown enum) */
#define E2E_ERR_LAUNCH (-2)   /* HIP reported a launch error */
#define E2E_ERR_WORKSPACE (-3)/* caller-provided workspace too small */

#define E2E_PADDING_ZEROS 0   /* MODEL.padding_mode: zeros  (configs/config.yaml:35) */
#define E2E_PADDING_BORDER 1  /* MODEL.padding_mode: border */

/* element strides of a (B,C,H,W)-indexed fp32 image */
typedef struct e2e_strides {
    int64_t sb, sc, sh, sw;
} e2e_strides;

int e2e_version(void);
const char* e2e_last_error(void);

/* ------------------------------------------------------------------------------------------ */
/* View synthesis -- depth_estimation/view_synthesis.py                                         */
/* ------------------------------------------------------------------------------------------ */
/* Every entry point of this section, of the photometric loss and of the fused refinement step that takes an image size as (B,H,W) needs
 * H >= 2 and W >= 2 (the grid is normalised by dividing by W-1 and H-1, and the 1-pixel reflection pad needs a second pixel): an axis of
 * length 1 is refused with E2E_ERR_ARG.  e2e_grid_sample_* take (Hi,Wi) and (Ho,Wo) instead and accept any positive sizes. */

/* BackprojectDepth.forward (view_synthesis.py:34-40): depth (B,H*W), inv_K (B,4,4)
 * -> cam_points (B,4,H*W) rows x,y,z,1. */
int e2e_backproject_fwd(const float* depth, const float* inv_K, float* cam_points,
                        int B, int H, int W, void* stream);
/* its autograd: g_cam (B,4,H*W) -> g_depth (B,H*W). */
int e2e_backproject_bwd(const float* g_cam, const float* inv_K, float* g_depth,
                        int B, int H, int W, void* stream);

/* Project3D.forward (view_synthesis.py:54-78): points (B,4,H*W), K, T (B,4,4)
 * -> grid (B,H,W,2) normalised with /(W-1),/(H-1); valid (B,H,W) = max|grid|<=1 as 0/1 float;
 * z_out (B,H,W) = clamp(c2, 1e-3) when non-NULL (geometric=True, view_synthesis.py:73-76). */
int e2e_project3d_fwd(const float* points, const float* K, const float* T, float* grid, float* valid,
                      float* z_out, int B, int H, int W, void* stream);
/* autograd of the above: g_grid (B,H,W,2), g_z (B,H,W) or NULL -> g_points (B,4,H*W). */
int e2e_project3d_bwd(const float* points, const float* K, const float* T, const float* g_grid,
                      const float* g_z, float* g_points, int B, int H, int W, void* stream);
/* the same adjoint with respect to T (entry-point names are lower case throughout this header, hence _bwd_t):
 * g_T (B,4,4) = d/dT of sum(g_grid . grid) + sum(g_z . z_out).  T enters through P = (K T)[:3,:] only, with the forward's eps, /(W-1), /(H-1) and clamp(1e-3) conventions (no gradient through z_out at or below the
 * clamp).  The per-pixel terms are the fp32 expressions of e2e_project3d_bwd; their sums are float64 in a fixed order (per-workgroup
 * partials, then one wave per sum; no atomics).  workspace: e2e_project3d_bwd_t_workspace_bytes(B) bytes. */
int64_t e2e_project3d_bwd_t_workspace_bytes(int B);
int e2e_project3d_bwd_t(const float* points, const float* K, const float* T, const float* g_grid,
                        const float* g_z, float* g_T, void* workspace, int B, int H, int W, void* stream);
/* ... and with respect to K, by the same convention: g_K (B,4,4) = d/dK of sum(g_grid . grid) + sum(g_z . z_out).  K enters through rows
 * 0..2 of K T only: with Pbar = sum cbar p^T (3x4; cbar the fp32 expressions of e2e_project3d_bwd, its clamp(1e-3) rule for g_z included;
 * float64 sums in a fixed order, no atomics), g_K[:3,:] = Pbar T^T and row 3 is 0.  workspace: e2e_project3d_bwd_k_workspace_bytes(B) bytes. */
int64_t e2e_project3d_bwd_k_workspace_bytes(int B);
int e2e_project3d_bwd_k(const float* points, const float* K, const float* T, const float* g_grid, const float* g_z,
                        float* g_K, void* workspace, int B, int H, int W, void* stream);
/* the adjoint of e2e_backproject_fwd with respect to inv_K: depth (B,H*W), g_cam (B,4,H*W) -> g_inv_K (B,4,4) with
 * g_inv_K[r][j] = sum g_cam[r] depth pix_j for r, j < 3, pix = (x, y, 1); row 3 and column 3 are 0 (the forward reads inv_K[:3,:3] only).
 * float64 sums in a fixed order, no atomics.  workspace: e2e_backproject_bwd_invk_workspace_bytes(B) bytes. */
int64_t e2e_backproject_bwd_invk_workspace_bytes(int B);
int e2e_backproject_bwd_invk(const float* g_cam, const float* depth, float* g_inv_K, void* workspace, int B, int H, int W,
                             void* stream);

/* F.grid_sample(input, grid, mode="bilinear", padding_mode, align_corners) as called at
 * online_adaption.py:431-439,450-453.  input (B,C,Hi,Wi) via strides, grid (B,Ho,Wo,2) contiguous,
 * out (B,C,Ho,Wo) contiguous. */
int e2e_grid_sample_fwd(const float* input, e2e_strides in_strides, const float* grid, float* out,
                        int B, int C, int Hi, int Wi, int Ho, int Wo, int padding_mode,
                        int align_corners, void* stream);
/* g_out (B,C,Ho,Wo) contiguous -> g_grid (B,Ho,Wo,2); if g_input != NULL it must be a ZEROED
 * contiguous (B,C,Hi,Wi) buffer that receives the scatter-add (only the geometric branch,
 * online_adaption.py:436-439, needs it; this one output uses float atomics). */
int e2e_grid_sample_bwd(const float* input, e2e_strides in_strides, const float* grid,
                        const float* g_out, float* g_grid, float* g_input, int B, int C, int Hi,
                        int Wi, int Ho, int Wo, int padding_mode, int align_corners, void* stream);
/* The same with a BITWISE REPRODUCIBLE gradient with respect to the sampled image: the bilinear adjoint is a data-dependent scatter; its
 * contributions are accumulated as 2^-48 fixed-point integers (integer adds commute: no dependence on arrival order; resolution 3.6e-15)
 * in g_input_fixed (B*C*Hi*Wi + 1 int64 of scratch, zeroed here) and converted to g_input (B,C,Hi,Wi) afterwards.  Range: every
 * contribution |g_out * weight| < 4096 and every sum < 32768; a contribution that is not finite or not below 4096 is refused and raises
 * the scratch's last word, and g_input then comes back as NaN everywhere (never a wrapped or saturated finite value). */
int e2e_grid_sample_bwd_exact(const float* input, e2e_strides in_strides, const float* grid, const float* g_out,
                              float* g_grid, long long* g_input_fixed, float* g_input, int B, int C, int Hi, int Wi,
                              int Ho, int Wo, int padding_mode, int align_corners, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Photometric loss -- loss/losses.py                                                           */
/* ------------------------------------------------------------------------------------------ */

/* SSIM.forward (losses.py:23-37) and photometric_loss (losses.py:97-117) in one pass.
 * x = prediction, y = target, both (B,C,H,W) via strides.
 * ssim_out (B,C,H,W) contiguous or NULL; pmap_out (B,1,H,W) contiguous or NULL
 * (pmap = 0.85*mean_c ssim + 0.15*mean_c |y-x|). */
int e2e_photometric_fwd(const float* x, e2e_strides xs, const float* y, e2e_strides ys,
                        float* ssim_out, float* pmap_out, int B, int C, int H, int W, void* stream);
/* Gradient wrt x.  g_pmap (B,1,H,W) or NULL, g_ssim (B,C,H,W) or NULL (both contiguous; the two
 * contributions add) -> g_x (B,C,H,W) contiguous.  Gradient wrt y: call with x and y swapped
 * (SSIM is symmetric; the L1 term's sign flips with the swap, as it must). */
int e2e_photometric_bwd(const float* x, e2e_strides xs, const float* y, e2e_strides ys,
                        const float* g_pmap, const float* g_ssim, float* g_x, int B, int C, int H,
                        int W, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Fused refinement-step kernels (what the build's own driver launches)                         */
/* ------------------------------------------------------------------------------------------ */

/* Number of floats of workspace the fused forward needs for (B,H,W). */
int64_t e2e_warp_photo_workspace_floats(int B, int H, int W);

/* Forward of one refinement step's image-space part, ONE launch (+ a 1-block reduction):
 *   backproject -> project -> grid_sample(src) -> mask -> masked SSIM+L1 -> mean   [+ depth reg.]
 * reference: online_adaption.py:412-455 (novel_view_synthesis), :544-564, :482-511, :612-623.
 *   depth_tgt (B,H,W)   target depth (after median scaling)
 *   src, tgt            source / target frame, (B,3,H,W) via strides (NHWC memory is fine)
 *   K, inv_K, T         (B,4,4)
 *   synth (B,3,H,W), valid (B,H,W)   outputs kept for the backward
 *   pmap (B,H,W) or NULL             per-pixel loss map
 *   use_mask            LOSS.photometric_mask
 *   reg_kind            0 = no depth regulariser, 1 = l1, 2 = l2 (losses.py:134-148); when != 0:
 *     reg_init_tgt, reg_init_src (B,H,W)  initial depths (online_adaption.py:284-285)
 *     depth_src (B,H,W)                    refined depth of the source frame
 *   loss_out[0] = photometric mean, loss_out[1] = mean-reg(tgt) + mean-reg(src)
 *   workspace: e2e_warp_photo_workspace_floats floats. */
int e2e_warp_photo_fwd(const float* depth_tgt, const float* src, e2e_strides src_strides,
                       const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                       const float* T, float* synth, float* valid, float* pmap, int use_mask,
                       int padding_mode, int reg_kind, const float* reg_init_tgt,
                       const float* reg_init_src, const float* depth_src, float* loss_out,
                       float* workspace, int B, int H, int W, void* stream);

/* Backward of the above, ONE launch.
 *   g_loss (device, 2 floats): upstream gradients of loss_out[0] and loss_out[1]
 *   g_depth_tgt (B,H,W) = d/d(depth_tgt) of g_loss[0]*photometric + g_loss[1]*reg
 *   g_depth_src (B,H,W) = d/d(depth_src) of g_loss[1]*reg   (written only when reg_kind != 0;
 *   the warp reads the TARGET depth only: online_adaption.py:419). */
int e2e_warp_photo_bwd(const float* depth_tgt, const float* src, e2e_strides src_strides,
                       const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                       const float* T, const float* synth, const float* valid, int use_mask,
                       int padding_mode, int reg_kind, const float* reg_init_tgt,
                       const float* reg_init_src, const float* depth_src, const float* g_loss,
                       float* g_depth_tgt, float* g_depth_src, int B, int H, int W, void* stream);

/* The same backward with the gradient with respect to the relative pose (DATA.use_gt_pose: False, train_depth.py:381-382, :395: the
 * photometric loss is differentiated through T).  Two launches: the kernel of e2e_warp_photo_bwd with one reduction more, and a final
 * kernel of one workgroup per batch element.
 *   g_depth_tgt, g_depth_src   bit-identical to what e2e_warp_photo_bwd writes for the same arguments;
 *   g_T (B,4,4) = d/dT of g_loss[0]*photometric (the regulariser does not depend on T).  T enters through P = (K T)[:3,:] only; the
 *     validity mask is a constant (in the reference it is a comparison cast to float); the forward's conventions hold: z = c2 + 1e-7,
 *     /(W-1) and /(H-1), align_corners=False, with border padding zero slope where the clamp is active, with zero padding the
 *     out-of-range taps are zero.
 *   Per pixel, with X = d * inv_K[:3,:3] [x,y,1]^T (fp32, the forward's own d * cam) and (gc0, gc1, gc2) the very fp32 adjoint of the
 *     projected point that reaches g_depth_tgt:  Pbar[r][j] += gc_r X_j (j < 3),  Pbar[r][3] += gc_r;  then
 *     g_T[k][j] = sum_{i<3} K[i][k] Pbar[i][j] for k = 0..3 -- the convention of e2e_project3d_bwd_t, its bottom row included.
 *   The sums are float64 in a fixed order: wave shuffle, the four waves of a workgroup through LDS, 12 doubles per workgroup (32x8
 *     pixels) in `workspace`, then one wave per sum over the workgroups of a batch element (lane l adds l, l + 64, ... in order, then a
 *     shuffle tree) and K^T.  No atomics: two runs give the same bits.
 *   workspace: e2e_warp_photo_bwd_pose_workspace_bytes(B,H,W) bytes = 96 B ceil(H/8) ceil(W/32) (0 for a non-positive size), all written.
 *   A refused call (NULL g_T or workspace or any pointer e2e_warp_photo_bwd needs, bad dimensions, padding_mode or reg_kind) returns
 *     E2E_ERR_ARG before any launch and writes nothing. */
int64_t e2e_warp_photo_bwd_pose_workspace_bytes(int B, int H, int W);
int e2e_warp_photo_bwd_pose(const float* depth_tgt, const float* src, e2e_strides src_strides,
                            const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                            const float* T, const float* synth, const float* valid, int use_mask,
                            int padding_mode, int reg_kind, const float* reg_init_tgt,
                            const float* reg_init_src, const float* depth_src, const float* g_loss,
                            float* g_depth_tgt, float* g_depth_src, float* g_T, void* workspace, int B,
                            int H, int W, void* stream);

/* The same backward with the gradient with respect to the camera intrinsics as well (self-calibration through the photometric loss; the
 * reference carries scale_by_f, normalize_intrinsics and utils/pretrained_focal.py because the focal length may not match the data).
 * Four launches (three without g_T): the kernel of e2e_warp_photo_bwd_pose itself (depth gradients and pose sums: its bits), a second
 * pass of the same tile kernel that stores only the nine sums Q below, the final kernel of e2e_warp_photo_bwd_pose when g_T is asked for,
 * and a final kernel of one workgroup per batch element for the intrinsics.
 *   RULE.  The conventions are those of e2e_warp_photo_bwd_pose: z = c2 + 1e-7, /(W-1) and /(H-1), the validity mask a constant, zero slope
 *     under an active border clamp.  Per batch element and source s:  P_s = (K T_s)[:3,:],  pix = (x, y, 1),  cam = inv_K[:3,:3] pix,
 *     X = d cam,  c = P_s [X;1].  K enters through rows 0..2 of K T only and inv_K through its upper-left 3x3 only.  With (gc0, gc1, gc2)
 *     the very fp32 adjoint of c that reaches g_depth_tgt, in float64:
 *       Pbar_s[i][j] = sum gc_i X_j (j < 3),  Pbar_s[i][3] = sum gc_i      the pose sums, in the place and layout they have there;
 *       Q_s[i][j]    = sum gc_i d pix_j  (i, j < 3)                        from the same fp32 gc and d, pix exact; pixels outside add 0;
 *       g_K[i][k]     = sum_s sum_{j<4} Pbar_s[i][j] T_s[k][j]   for i < 3, k < 4;   row 3 is 0;
 *       g_inv_K[r][j] = sum_s sum_{i<3} P_s[i][r] Q_s[i][j]      for r, j < 3;       row 3 and column 3 are 0;
 *     P_s is formed in float64 from the fp32 K and T_s, the sources are added in the order s = 0, 1, and all 16 entries of both outputs
 *     are written.  (The pair has the one source s = 0.)  Under the geometric term gc2 carries that term's adjoint, so the same formulas
 *     hold for e2e_warp_photo_geo_bwd_intrinsics.
 *   g_K, g_inv_K (B,4,4)       both required;
 *   g_T (B,4,4) or NULL        NULL: the pose final stage is not launched; otherwise bit-identical to e2e_warp_photo_bwd_pose's;
 *   g_depth_tgt, g_depth_src   bit-identical to what e2e_warp_photo_bwd writes for the same arguments.
 *   The sums are float64 in the fixed order of e2e_warp_photo_bwd_pose (wave shuffle, the four waves through LDS, per workgroup 12 doubles
 *     in [B][tiles][12] and 9 in a second region [B][tiles][9] behind them); the final kernel folds the tiles per sum (lane l adds
 *     l, l + 64, ... in order, then a shuffle tree).  No atomics: two runs give the same bits.
 *   workspace: e2e_warp_photo_bwd_intrinsics_workspace_bytes(B,H,W) bytes = 8 x 21 B ceil(H/8) ceil(W/32) (0 for a non-positive size).
 *   A refused call (NULL g_K, g_inv_K or workspace or any pointer e2e_warp_photo_bwd needs, bad dimensions, padding_mode or reg_kind)
 *     returns E2E_ERR_ARG before any launch and writes nothing. */
int64_t e2e_warp_photo_bwd_intrinsics_workspace_bytes(int B, int H, int W);
int e2e_warp_photo_bwd_intrinsics(const float* depth_tgt, const float* src, e2e_strides src_strides,
                                  const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                                  const float* T, const float* synth, const float* valid, int use_mask,
                                  int padding_mode, int reg_kind, const float* reg_init_tgt,
                                  const float* reg_init_src, const float* depth_src, const float* g_loss,
                                  float* g_depth_tgt, float* g_depth_src, float* g_T, float* g_K, float* g_inv_K,
                                  void* workspace, int B, int H, int W, void* stream);

/* The step the build's driver actually launches: loss AND gradient in ONE pass (the gradient of a
 * mean does not depend on its value, so forward and backward of the image-space part collapse;
 * synth / valid / the loss map never reach HBM).  Same semantics as e2e_warp_photo_fwd followed by
 * e2e_warp_photo_bwd with upstream gradients (w_photo, w_reg):
 *   loss_out[0] = photometric mean, loss_out[1] = regulariser (unweighted);
 *   g_depth_tgt = d(w_photo*loss0 + w_reg*loss1)/d(depth_tgt), g_depth_src likewise (reg_kind != 0).
 * workspace: e2e_warp_photo_lossgrad_workspace_floats floats (per-workgroup partial sums; a
 * second-stage kernel adds them in a fixed order => bitwise reproducible loss).  loss_out == NULL
 * skips that second launch (gradients only).
 *   e2e_warp_photo_lossgrad_workspace_floats(B,H,W) = 2 B ceil(W/32) ceil(H/8), rounded up to even, + 2 x 8 x 129 floats (the
 *     per-workgroup partial sums, then the chained form's 8 slot sets of 129 64-bit words); 0 for a non-positive size.  No launch
 *     writes behind it.
 *   loss_out[1] = 0 when reg_kind == 0 (the second-stage kernel and the chained form's finalisation both write it); g_depth_src is
 *     not written then.
 *   A refused call (a required pointer NULL -- loss_out is not required --, B <= 0, H or W < 2, a padding_mode or reg_kind outside
 *     its range, a regulariser buffer or g_depth_src missing with reg_kind != 0; for the chained form and its flush also what their
 *     comment rules out) returns E2E_ERR_ARG before any launch and writes nothing: outputs, loss and workspace stay as they were. */
int64_t e2e_warp_photo_lossgrad_workspace_floats(int B, int H, int W);
int e2e_warp_photo_lossgrad(const float* depth_tgt, const float* src, e2e_strides src_strides,
                            const float* tgt, e2e_strides tgt_strides, const float* K,
                            const float* inv_K, const float* T, int use_mask, int padding_mode,
                            int reg_kind, const float* reg_init_tgt, const float* reg_init_src,
                            const float* depth_src, float w_photo, float w_reg, float* loss_out,
                            float* g_depth_tgt, float* g_depth_src, float* workspace, int B, int H,
                            int W, void* stream);

/* Same launch for ONE keyframe pair (B = 1) when the caller already holds the pair's geometry on the HOST (poses are
 * dataset inputs): geometry12_host = rows of M = (K T)[:3,:3] inv(K)[:3,:3] (9 floats) followed by p4 = (K T)[:3,3]
 * (3 floats), so that c = d * M [x,y,1]^T + p4.  The 12 numbers travel as kernel arguments: no device round trip and no
 * workgroup barrier before the first loads. */
int e2e_warp_photo_lossgrad_hostgeo(const float* depth_tgt, const float* src, e2e_strides src_strides,
                                    const float* tgt, e2e_strides tgt_strides,
                                    const float* geometry12_host, int use_mask, int padding_mode,
                                    int reg_kind, const float* reg_init_tgt, const float* reg_init_src,
                                    const float* depth_src, float w_photo, float w_reg, float* loss_out,
                                    float* g_depth_tgt, float* g_depth_src, float* workspace, int H,
                                    int W, void* stream);

/* Chained form: ONE kernel per step.  Each workgroup adds its partial loss sums (as 2^-36 fixed
 * point: the integer total does not depend on arrival order, so the result is bitwise reproducible)
 * into slot set `set_cur` of the workspace, and the launch also turns the complete slot set
 * `set_prev` of the PREVIOUS launch into that launch's loss (loss_prev_out[0..1]) and clears it
 * (set_prev < 0: nothing to finalise).  Sets are 0..7 and must alternate; the last launch of a chain
 * is finished by e2e_warp_photo_lossgrad_chain_flush.  geometry12_host non-NULL (B == 1) replaces
 * K / inv_K / T as in e2e_warp_photo_lossgrad_hostgeo.  The workspace (same size function) must be
 * zero-filled once before the first chained launch.  A per-workgroup sum that is negative, not
 * finite or above 2.6e8 / #workgroups turns the loss into NaN (the gradients are unaffected): both
 * numbers of that step's loss, and the flag is cleared with the set.  Refused: set_cur outside 0..7,
 * set_prev above 7 or equal to set_cur, set_prev >= 0 without loss_prev_out, host geometry with
 * B != 1; for the flush a NULL workspace or loss_out or a set outside 0..7.  reg_kind must not change
 * along a chain: a launch (and the flush) finalises set_prev with the sum count of its OWN reg_kind,
 * so a step's regulariser sum is reported only if the call that finalises it has a regulariser too
 * (the slots are cleared either way). */
int e2e_warp_photo_lossgrad_chain(const float* depth_tgt, const float* src, e2e_strides src_strides,
                                  const float* tgt, e2e_strides tgt_strides, const float* K,
                                  const float* inv_K, const float* T, const float* geometry12_host,
                                  int use_mask, int padding_mode, int reg_kind, const float* reg_init_tgt,
                                  const float* reg_init_src, const float* depth_src, float w_photo,
                                  float w_reg, int set_cur, int set_prev, float* loss_prev_out,
                                  float* g_depth_tgt, float* g_depth_src, float* workspace, int B, int H,
                                  int W, void* stream);
int e2e_warp_photo_lossgrad_chain_flush(float* workspace, int set, int reg_kind, float* loss_out, int B,
                                        int H, int W, void* stream);

/* The same step WITH the loss terms the recommended configuration leaves off (online_adaption.py:421-439, :486-511; the
 * operator-by-operator form is SLAM.compute_flagged_losses), still loss AND gradient together, every launch argument
 * constant (capturable).  e2e_warp_photo_lossgrad itself is not involved: the default configuration's code path is unchanged.
 *   terms   bit set of E2E_TERM_*:
 *     GEOMETRIC        src is sampled with align_corners=True, depth_src with align_corners=False on the same grid (sic);
 *                      diff = clamp(|wd - id| / (wd + id), 0, 1), wd = max(z, 1e-3) of the projected point, id = the sample of
 *                      depth_src; term = sum(diff * valid) / sum(valid) if sum(valid) > 10000 over the whole batch, else 0
 *                      with zero gradient (losses.py:84-95).  The count is taken by a pre-pass and stays on the device.
 *                      Gradients reach depth_tgt (through wd and through the sampling position) and depth_src (scatter).
 *     AUTO_MASKING     identity map photometric(src*m, tgt*m) concatenated BEFORE the reprojection map, per-pixel minimum;
 *                      the first minimal map takes the gradient (ties: the identity map, which has none).
 *     MIN_REPROJECTION no effect with one source frame, except that together with AUTO_MASKING the plane
 *                      tie_noise (1,1,H,W) -- NULL: none -- is added to the identity map (online_adaption.py:498).
 *   depth_src (B,H,W)  needed with GEOMETRIC or reg_kind != 0; g_depth_src likewise (then fully written: zeroed here first).
 *   loss_out[5] = {photometric mean after the minimum, regulariser (unweighted), geometric term (unweighted), untouched
 *                  (the slot of e2e_smoothness_norm_lossgrad), number of valid projections (0 without GEOMETRIC)}
 *   gradients are of w_photo*loss[0] + w_reg*loss[1] + w_geometric*loss[2].
 * Reproducibility: the loss values and g_depth_tgt are bitwise reproducible run to run (fixed-order sums, integer count).
 * With GEOMETRIC, g_depth_src is accumulated with float atomics like e2e_grid_sample_bwd's g_input: equal to rounding, not
 * bitwise.  Without GEOMETRIC it is a plain store per pixel and reproducible.
 * workspace: e2e_warp_photo_terms_lossgrad_workspace_floats floats, no initialisation needed. */
#define E2E_TERM_GEOMETRIC 1
#define E2E_TERM_AUTO_MASKING 2
#define E2E_TERM_MIN_REPROJECTION 4
int64_t e2e_warp_photo_terms_lossgrad_workspace_floats(int B, int H, int W);
int e2e_warp_photo_terms_lossgrad(const float* depth_tgt, const float* depth_src, const float* src,
                                  e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                                  const float* K, const float* inv_K, const float* T, int use_mask,
                                  int padding_mode, int reg_kind, const float* reg_init_tgt,
                                  const float* reg_init_src, int terms, const float* tie_noise, float w_photo,
                                  float w_reg, float w_geometric, float* loss_out, float* g_depth_tgt,
                                  float* g_depth_src, float* workspace, int B, int H, int W, void* stream);

/* The fused forward / backward pair over a WINDOW of S = 1 or 2 source frames (DATA.frames: [0,-1,1] is S = 2), with the candidate /
 * minimum logic of train_depth.py:621-662.  Forward: one tile launch over the sources + the fixed-order reduction; backward: one tile
 * launch over the sources, + one final kernel of S B workgroups when g_T is asked for.
 *   src0, src1          the source frames, (B,3,H,W) through the SAME strides (src1 may be NULL with S = 1); tgt likewise through its own
 *   T (S,B,4,4)         the relative pose of each source;  K, inv_K (B,4,4)
 *   terms               E2E_TERM_AUTO_MASKING | E2E_TERM_MIN_REPROJECTION (E2E_TERM_GEOMETRIC is refused: that term is e2e_warp_photo_geo_fwd / _bwd)
 *   For source s with its validity mask m_s (1 when use_mask == 0):
 *     R_s = photometric(synth_s m_s, tgt m_s);   I_s = photometric(src_s m_s, tgt m_s), src_s read at the target pixel.
 *   Candidates, in this order:  identity candidates, only with AUTO_MASKING -- with MIN_REPROJECTION  I_0 + n_0, ..., I_{S-1} + n_{S-1}
 *     (n = tie_noise (B,S,H,W); NULL: nothing added), without it the one map mean_s I_s;  then the reprojection candidates -- with
 *     MIN_REPROJECTION  R_0, ..., R_{S-1},  without it the one map mean_s R_s.
 *   loss_out[0] = the mean of the one candidate, or of the per-pixel minimum of several;  pmap (B,H,W) or NULL = that map;
 *   select (B,H,W) int32 = the index of the FIRST minimal candidate (a NaN wins, as in torch.min and e2e_min_reprojection_lossgrad); 0 with
 *     one candidate;  synth (S,B,3,H,W), valid (S,B,H,W): each source's sample and mask, kept for the backward.
 *   Gradient, nI = the number of identity candidates: select < nI -- none (frames and masks are constants); select - nI = r under
 *     MIN_REPROJECTION -- the pixel's g_loss[0] / (B H W) goes to R_r alone; otherwise 1/S of it to each R_s.  Per source the rest is
 *     e2e_warp_photo_bwd_pose's: z = c2 + 1e-7, align_corners=False, zero slope under an active border clamp, the mask a constant.
 *   g_depth_tgt (B,H,W): the sum over the sources, one store per pixel.
 *   g_T (S,B,4,4) or NULL (no pose sums; workspace may then be NULL, and g_depth_tgt has the same bits): the convention of
 *     e2e_project3d_bwd_t, bottom row included; float64 sums in the fixed order of e2e_warp_photo_bwd_pose.  No atomics anywhere: two runs
 *     give the same bits.
 *   workspace: forward e2e_warp_photo_window_workspace_floats(S,B,H,W) = B ceil(H/8) ceil(W/32) floats, backward
 *     e2e_warp_photo_window_bwd_workspace_bytes(S,B,H,W) = 96 S B ceil(H/8) ceil(W/32) bytes, both all written (0 for a non-positive size or
 *     an S outside 1..2).
 *   A refused call (S outside 1..2, src1 NULL with S = 2, H or W < 2, B <= 0 or > 65535, an unknown padding mode or term, a NULL required
 *     pointer -- tie_noise, pmap and g_T are not required; workspace is, except for the backward without g_T) returns E2E_ERR_ARG before
 *     any launch and writes nothing. */
int64_t e2e_warp_photo_window_workspace_floats(int S, int B, int H, int W);
int e2e_warp_photo_window_fwd(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides,
                              const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                              const float* T, const float* tie_noise, float* synth, float* valid, int* select,
                              float* pmap, int use_mask, int padding_mode, int terms, float* loss_out,
                              float* workspace, int S, int B, int H, int W, void* stream);
int64_t e2e_warp_photo_window_bwd_workspace_bytes(int S, int B, int H, int W);
int e2e_warp_photo_window_bwd(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides,
                              const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                              const float* T, const float* synth, const float* valid, const int* select, int use_mask,
                              int padding_mode, int terms, const float* g_loss, float* g_depth_tgt, float* g_T,
                              void* workspace, int S, int B, int H, int W, void* stream);

/* The window pair WITH the geometric-consistency term of LOSS.geometric (train_depth.py:558-576, view_synthesis.py:54-78, losses.py:84-95).
 * Everything of e2e_warp_photo_window_fwd / _bwd holds (candidates, order, select, pmap, the NaN rule, tie_noise, g_T), with one difference
 * on the photometric side: the source image is sampled with align_corners=True (sic, as the reference does under this flag), so synth
 * holds that sample and its adjoint uses that index; the identity maps still read the source at the target pixel.
 *   depth_src0, depth_src1 (B,H,W) contiguous: the depth of each source frame (depth_src1 may be NULL with S = 1)
 *   Per source s and target pixel, with c the projected point:  wd = max(c2, 1e-3);  id = the bilinear sample of depth_src_s on the same grid
 *     with align_corners=False and the same padding mode;  diff = clamp(|wd - id| / (wd + id), 0, 1);  valid_s = max|grid| <= 1 whatever use_mask.
 *   geo_count[s] int32 = n_s = the number of valid projections of source s over the batch (an exact integer count of the fp32 decision);
 *   loss_out[0] = the window's photometric loss;  loss_out[1 + s] = G_s = sum(diff valid_s) / n_s if n_s > geo_min_valid, else 0 (the
 *     reference's gate is geo_min_valid = 10000).  Fixed-order float64 second stages.
 *   Backward: gradients of g_loss[0] loss[0] + sum_s g_loss[1 + s] G_s.  Where the gate of s is open (geo_count[s] > geo_min_valid, read on
 *     the device) a valid pixel adds, with e = g_loss[1 + s] / n_s and sg = sign(wd - id) (0 at 0; the clamp passes on [0,1]):
 *     e sg 2 id / (wd + id)^2 to c2 where c2 >= 1e-3, and -e sg 2 wd / (wd + id)^2 to id, which goes to the four taps of depth_src_s
 *     (e2e_grid_sample_bwd's g_input conventions) and to the sampling position (its g_grid conventions, align_corners=False) and on through
 *     z = c2 + 1e-7.  All of it enters the same per-pixel adjoint as the photometric part, so g_depth_tgt and g_T carry the term.
 *     A closed gate, or g_loss[1 + s] == 0, skips the piece: g_depth_tgt and g_T have the bits of the photometric part, g_depth_src[s] is 0.
 *   g_depth_src (S,B,H,W): fully written.  The scatter is summed as 2^-48 fixed-point integers (order-independent, as in
 *     e2e_grid_sample_bwd_exact): a contribution that is not finite or not below 4096 turns that source's plane into NaN.
 *   Every output is bitwise reproducible run to run; g_T = NULL gives the same g_depth_tgt and g_depth_src bits.
 *   workspace: forward e2e_warp_photo_geo_workspace_floats = (1 + 2 S) B ceil(H/8) ceil(W/32) floats, all written; backward
 *     e2e_warp_photo_geo_bwd_workspace_bytes = 8 (S B H W + S) + 96 S B ceil(H/8) ceil(W/32) bytes: the fixed-point sums, zeroed by the call,
 *     then the pose sums, written only with g_T.  Both are needed (0 for a non-positive size or an S outside 1..2).
 *   A refused call (the window's refusals, a NULL depth_src0, a NULL depth_src1 with S = 2, a NULL geo_count, g_depth_src or workspace,
 *     geo_min_valid < 0, E2E_TERM_GEOMETRIC or an unknown bit in terms) returns E2E_ERR_ARG before any launch and writes nothing. */
int64_t e2e_warp_photo_geo_workspace_floats(int S, int B, int H, int W);
int e2e_warp_photo_geo_fwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0,
                           const float* src1, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                           const float* K, const float* inv_K, const float* T, const float* tie_noise, float* synth,
                           float* valid, int* select, float* pmap, int* geo_count, int use_mask, int padding_mode,
                           int terms, int geo_min_valid, float* loss_out, float* workspace, int S, int B, int H, int W,
                           void* stream);
int64_t e2e_warp_photo_geo_bwd_workspace_bytes(int S, int B, int H, int W);
int e2e_warp_photo_geo_bwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0,
                           const float* src1, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                           const float* K, const float* inv_K, const float* T, const float* synth, const float* valid,
                           const int* select, const int* geo_count, int use_mask, int padding_mode, int terms,
                           int geo_min_valid, const float* g_loss, float* g_depth_tgt, float* g_depth_src, float* g_T,
                           void* workspace, int S, int B, int H, int W, void* stream);

/* e2e_warp_photo_geo_fwd / _bwd over SCALE GROUPS of the batch: monodepth2's disparity pyramid with the scales stacked along the batch
 * (ops.warp_photometric_multiscale(geometric=True)), where the reference's gate and mean of the geometric term are per scale.
 *   B is the stacked batch, groups = G in 1..4 with B % G == 0; group g is the batch items g B/G ... (g + 1) B/G - 1 (scale-major).
 *   Everything of the geo pair holds per item and per source: the candidates, select, pmap, tie_noise, align_corners=True for the image
 *     and False for the depth sample, the fixed-point scatter into g_depth_src, g_T per stacked item, bitwise reproducibility.
 *   Only the geometric term's reduction and gate change.  geo_count int32 [S G] and loss_out float [1 + S G], indexed [s G + g] and
 *     [1 + s G + g]:  n_{s,g} = the valid projections of source s over group g;  G_{s,g} = sum(diff valid over group g) / n_{s,g} if
 *     n_{s,g} > geo_min_valid, else 0;  loss_out[0] stays the photometric mean over the whole stacked batch.  The second stage adds group g's
 *     workgroup partials in the order a call of e2e_warp_photo_geo_fwd on that group's slice adds them: geo_count[s G + g] and
 *     loss_out[1 + s G + g] have that call's bits, and so have synth, valid, select and pmap.
 *   Backward: g_loss float [1 + S G]; a valid pixel of item b in group g uses e = g_loss[1 + s G + g] / n_{s,g} under that group's gate.  A closed
 *     gate, n_{s,g} == 0 or g_loss[1 + s G + g] == 0 skips the piece for that group's items only: their g_depth_src planes are 0, their
 *     g_depth_tgt and g_T have the bits of the photometric part.  The poison word of the scatter stays one per source: a contribution out of
 *     range turns that source's g_depth_src into NaN for every group.
 *   groups = 1 is e2e_warp_photo_geo_fwd / _bwd bit for bit.  There is no intrinsics form.
 *   workspace: e2e_warp_photo_geo_workspace_floats and e2e_warp_photo_geo_bwd_workspace_bytes at the stacked B; the layouts are unchanged.
 *   A refused call (what the geo pair refuses, in its order; then groups outside 1..4; then B % groups != 0) returns E2E_ERR_ARG before any
 *     launch and writes nothing. */
int e2e_warp_photo_geo_groups_fwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0,
                                  const float* src1, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                                  const float* K, const float* inv_K, const float* T, const float* tie_noise, float* synth,
                                  float* valid, int* select, float* pmap, int* geo_count, int use_mask, int padding_mode,
                                  int terms, int geo_min_valid, float* loss_out, float* workspace, int S, int groups, int B, int H,
                                  int W, void* stream);
int e2e_warp_photo_geo_groups_bwd(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0,
                                  const float* src1, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                                  const float* K, const float* inv_K, const float* T, const float* synth, const float* valid,
                                  const int* select, const int* geo_count, int use_mask, int padding_mode, int terms,
                                  int geo_min_valid, const float* g_loss, float* g_depth_tgt, float* g_depth_src, float* g_T,
                                  void* workspace, int S, int groups, int B, int H, int W, void* stream);

/* e2e_warp_photo_window_bwd and e2e_warp_photo_geo_bwd with the gradient with respect to the intrinsics: the rule of
 * e2e_warp_photo_bwd_intrinsics with one (Pbar_s, Q_s) per source, added in the order s = 0, 1.
 *   g_K, g_inv_K (B,4,4)   both required;   g_T (S,B,4,4) or NULL: NULL skips the pose final stage, otherwise the bits of the form above;
 *   g_depth_tgt (and the geometric form's g_depth_src): bit-identical to what the form above writes for the same arguments.
 *   workspace (required): e2e_warp_photo_window_bwd_intrinsics_workspace_bytes = 8 x 21 S B ceil(H/8) ceil(W/32) bytes -- the pose sums
 *     [S][B][tiles][12] where e2e_warp_photo_window_bwd has them, then [S][B][tiles][9];  e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes =
 *     8 (S B H W + S) + 8 x 21 S B ceil(H/8) ceil(W/32): the fixed-point sums first.  0 for a non-positive size or an S outside 1..2.
 *   A refused call (what the form above refuses, or a NULL g_K, g_inv_K or workspace) returns E2E_ERR_ARG before any launch and writes
 *     nothing.  Bitwise reproducible run to run. */
int64_t e2e_warp_photo_window_bwd_intrinsics_workspace_bytes(int S, int B, int H, int W);
int e2e_warp_photo_window_bwd_intrinsics(const float* depth_tgt, const float* src0, const float* src1, e2e_strides src_strides,
                                         const float* tgt, e2e_strides tgt_strides, const float* K, const float* inv_K,
                                         const float* T, const float* synth, const float* valid, const int* select, int use_mask,
                                         int padding_mode, int terms, const float* g_loss, float* g_depth_tgt, float* g_T,
                                         float* g_K, float* g_inv_K, void* workspace, int S, int B, int H, int W, void* stream);
int64_t e2e_warp_photo_geo_bwd_intrinsics_workspace_bytes(int S, int B, int H, int W);
int e2e_warp_photo_geo_bwd_intrinsics(const float* depth_tgt, const float* depth_src0, const float* depth_src1, const float* src0,
                                      const float* src1, e2e_strides src_strides, const float* tgt, e2e_strides tgt_strides,
                                      const float* K, const float* inv_K, const float* T, const float* synth, const float* valid,
                                      const int* select, const int* geo_count, int use_mask, int padding_mode, int terms,
                                      int geo_min_valid, const float* g_loss, float* g_depth_tgt, float* g_depth_src, float* g_T,
                                      float* g_K, float* g_inv_K, void* workspace, int S, int B, int H, int W, void* stream);

/* online_adaption.py:600-610 + losses.py:119-132 for ONE frame: edge-aware first-order smoothness of
 * disp / (mean(disp) + 1e-7) with the edges of img (3,H,W through strides; the batch stride is not used), fused
 * mean -> normalise -> loss + gradient.  loss_out[0] = the term (unweighted);  g_disp (H,W) += weight * d(term)/d(disp),
 * the mean's own contribution included -- ACCUMULATED, so that it can follow e2e_depth_scale_bwd_at on the same buffer.
 * Fixed-order sums: bitwise reproducible.  workspace: e2e_smoothness_norm_lossgrad_workspace_floats floats. */
int64_t e2e_smoothness_norm_lossgrad_workspace_floats(int H, int W);
int e2e_smoothness_norm_lossgrad(const float* disp, const float* img, e2e_strides img_strides, float weight,
                                 float* loss_out, float* g_disp, float* workspace, int H, int W,
                                 void* stream);

/* ------------------------------------------------------------------------------------------ */
/* RGB-D unprojection and the PointFusion map step -- gradslam (un-vendored dependency; semantics */
/* per SURVEY.md Appendix A), reference call sites online_adaption.py:347-363, :461-469, :642      */
/* ------------------------------------------------------------------------------------------ */

/* gradslam RGBDImages.vertex_map / normal_map / global_vertex_map / global_normal_map and the
 * fusion confidence alpha = exp(-|V|^2 / alpha_den) (alpha_den = 2 sigma^2 + 1e-7) in one pass.
 * depth (B,H,W); K, pose (B,4,4); outputs channels-last (B,H,W,3) / alpha (B,H,W).
 * V, Nm, Ng, alpha may be NULL.  Invalid (zero) depth gives zero rows. */
int e2e_vertex_normal_maps(const float* depth, const float* K, const float* pose, float alpha_den,
                           float* V, float* Nm, float* Vg, float* Ng, float* alpha, int B, int H,
                           int W, void* stream);
/* d/d(depth) of sum(g_V . V) + sum(g_Vg . Vg); either gradient may be NULL.  The normal map is not
 * differentiated (nothing on the reference path takes its gradient). */
int e2e_vertex_maps_bwd(const float* depth, const float* K, const float* pose, const float* g_V,
                        const float* g_Vg, float* g_depth, int B, int H, int W, void* stream);

/* gradslam.geometry.geometryutils.transform_pointcloud (online_adaption.py:642): out = R p + t for
 * (n,3) points, T (4,4).  transpose_rotation_only=1 gives R^T p (its autograd wrt the points). */
int e2e_transform_points(const float* points, const float* T, float* out, int64_t n,
                         int transpose_rotation_only, void* stream);
/* its autograd wrt T: g (n,3), points (n,3) -> out12 (device float64, a row-major 3x4 block) = [sum_i g_i p_i^T | sum_i g_i], the top
 * three rows of d/dT (the bottom row of T does not enter).  Float64 sums in a fixed order, no atomics.
 * workspace: e2e_transform_points_bwd_t_workspace_bytes() bytes. */
int64_t e2e_transform_points_bwd_t_workspace_bytes(void);
int e2e_transform_points_bwd_t(const float* g, const float* points, int64_t n, double* out12, void* workspace,
                               void* stream);

/* PointFusion map step (gradslam update_map_fusion) for ONE live frame against ONE resident map.
 * The map is four capacity-sized arrays (points/normals/colors (cap,3), ccounts (cap)) of which
 * the first M rows are live.  workspace: e2e_pf_workspace_bytes(cap, H, W) bytes.
 *
 * e2e_pf_associate = find_active_map_points + find_similar_map_points +
 *   find_best_unique_correspondences: per map point the pixel it projects to and its flags, per
 *   pixel the winning map point (max confidence, then min distance, then min index).
 * e2e_pf_table materialises one of the three index tables as int64 rows [n, h, w]
 *   (which = 0 active (ascending n), 1 similar (ascending n), 2 unique (ordered by pixel)); the row
 *   count goes to *count_out (device int64).  rows must hold min(M, H*W) resp. M rows.
 * e2e_pf_fuse_append = fuse_with_map: confidence-weighted merge of the matched points, then the
 *   frame's unmatched valid pixels are appended in row-major order; *new_count_out (device int64)
 *   receives the new live row count (rows beyond capacity are dropped -- size the map for the run). */
int64_t e2e_pf_workspace_bytes(int64_t map_capacity, int H, int W);
int e2e_pf_associate(const float* map_points, const float* map_normals, const float* map_ccounts,
                     int64_t M, const float* K, const float* pose, const float* Vg, const float* Ng,
                     float dist_th, float dot_th, void* workspace, int64_t map_capacity, int H, int W,
                     void* stream);
int e2e_pf_table(int which, int64_t M, void* workspace, int64_t map_capacity, int H, int W,
                 long long* rows, long long* count_out, void* stream);
int e2e_pf_fuse_append(float* map_points, float* map_normals, float* map_colors, float* map_ccounts,
                       int64_t M, int64_t map_capacity, const float* depth, const float* Vg,
                       const float* Ng, const float* rgb, const float* alpha, void* workspace, int H,
                       int W, long long* new_count_out, void* stream);

/* The same two steps on a map whose live size is DEVICE data (online_adaption.py:347-363 keeps the global
 * map on the device; gradslam reads its length on the host, which costs one synchronisation per keyframe).
 * map_count_dev: int64[3] in device memory = {M, scratch, sticky overflow flag}; e2e_pf_associate_dev
 * reads M, e2e_pf_fuse_append_dev reads M and writes the size after the append back to [0]
 * (clamped to map_capacity; [2] then holds the size that would have been needed, else stays 0).
 * Grids are sized by map_capacity, every argument is constant from keyframe to keyframe, the host reads
 * nothing: results equal e2e_pf_associate / e2e_pf_fuse_append called with the same M. */
int e2e_pf_associate_dev(const float* map_points, const float* map_normals, const float* map_ccounts,
                         const long long* map_count_dev, const float* K, const float* pose, const float* Vg,
                         const float* Ng, float dist_th, float dot_th, void* workspace, int64_t map_capacity,
                         int H, int W, void* stream);
/* Target cloud of the odometry: the map points the last e2e_pf_associate[_dev] found ACTIVE (find_active_map_points against
 * the previous frame, online_adaption.py:362 through PointFusion._localize), every dsratio-th of them in ascending map order
 * (gradslam downsample_pointclouds), gathered with their normals.  tgt_count_dev: int64[3] {targets written, active points,
 * sticky overflow flag (more targets than tgt_capacity)} -- device data like the map size. */
int e2e_pf_active_subsample_dev(const float* map_points, const float* map_normals, const long long* map_count_dev,
                                int64_t map_capacity, void* workspace, int H, int W, int dsratio, float* tgt,
                                float* tgt_normals, long long* tgt_count_dev, int64_t tgt_capacity, void* stream);
int e2e_pf_fuse_append_dev(float* map_points, float* map_normals, float* map_colors, float* map_ccounts,
                           long long* map_count_dev, int64_t map_capacity, const float* depth, const float* Vg,
                           const float* Ng, const float* rgb, const float* alpha, void* workspace, int H, int W,
                           void* stream);
/* Aggregation map step (MODEL.slam: ICPSLAM, online_adaption.py:110-124; gradslam ICPSLAM._map = update_map_aggregate, SURVEY.md
 * Appendix A) on the same resident map: every pixel of the live frame with depth != 0 becomes one row {global vertex, global normal,
 * colour, alpha} at map_count_dev[0], in row-major pixel order -- no association, no fusion.  depth (H,W), rgb (H,W,3), K / pose (4,4)
 * device fp32; alpha_den as for e2e_vertex_normal_maps.  Vertex, forward-difference normal and alpha are computed inside the kernel
 * that writes the rows (no per-pixel intermediate in memory), with the expressions of e2e_vertex_normal_maps: the rows are
 * bit-identical to e2e_vertex_normal_maps + e2e_pf_fuse_append_dev on a map where nothing matches.  Commit as
 * e2e_pf_fuse_append_dev: [0] = min(needed, map_capacity), [1] = needed, [2] = needed when it exceeded map_capacity; nothing is
 * written at or beyond map_capacity.  Three launches, all arguments constant between keyframes (capturable).
 * Size range: meant for camera frames.  Each of the ceil(H*W / 1024) workgroups sums the counts of the workgroups before it
 * (that is what keeps it at three launches with no workgroup waiting on another): H*W / 1024 squared / 2 four-byte reads out of L2 in
 * total -- 45 000 at 480x640, 8 M at 4096x4096; quadratic beyond that, where a scan launch between count and append would be due. */
int e2e_frame_append_dev(float* map_points, float* map_normals, float* map_colors, float* map_ccounts,
                         long long* map_count_dev, int64_t map_capacity, const float* depth, const float* rgb,
                         const float* K, const float* pose, float alpha_den, void* workspace, int H, int W, void* stream);

/* DIFFERENTIABLE MAP STEP (opt-in: gradslam.slam.PointFusion(map_gradient=True), E2E_MAP_GRAD=1 for train_depth.py).  gradslam exists so
 * that the fused map is differentiable with respect to the frames that built it (train_depth.py:378-385 takes the 3-D loss on the
 * reconstruction of the predicted depths; gradient_experiments.py:132-161 optimises pixels through slam/custom_slam.py's cloud).
 *
 * Differentiation rule.  CONSTANTS: the association (the active / similar / unique tables), the validity mask, the append order, the
 * pose and the intrinsics.  The normals are not differentiated: their rows come back without a gradient, as for e2e_vertex_maps_bwd.
 * DIFFERENTIATED: the step's output points, colors and ccounts, with respect to the live frame's depth and rgb and to the previous
 * map's points, colors and ccounts (which is what carries a gradient through a chain of steps back to earlier frames).
 * Take a pixel q with a = alpha[q].  It is appended as row r, or fused into its winner row n; c, P, C are the winner's values before the
 * step, s = c + a, P', C' the fused row (P' = (c P + a Vg[q]) / s: the arithmetic of the forward).  gP, gC, gcc: the gradients of the
 * step's outputs.
 *   appended:  g_Vg[q] = gP[r]        g_rgb[q] = gC[r]        g_alpha[q] = gcc[r]
 *   fused:     g_Vg[q] = (a/s) gP[n]  g_rgb[q] = (a/s) gC[n]  g_alpha[q] = gcc[n] + (gP[n].(Vg[q] - P') + gC[n].(rgb[q] - C')) / s
 *              g_prevP[n] = (c/s) gP[n]   g_prevC[n] = (c/s) gC[n]   g_prevcc[n] = gcc[n] + (gP[n].(P - P') + gC[n].(C - C')) / s
 *              (s == 0, where the forward divides by 1: g_alpha[q] = gcc[n] + gP[n].Vg[q] + gC[n].rgb[q], g_prevcc[n] = gcc[n] + gP[n].P +
 *              gC[n].C, the other four are 0)
 *   a map row that won no pixel passes its gradient through unchanged -- except that a zero-confidence row in a step where anything
 *   matched has its point and colour zeroed by the forward and gets 0 for them (its confidence gradient still passes through: c X /
 *   where(c == 0, 1, c) jumps at c = 0 and has no derivative there);
 *   invalid pixels and pixels dropped beyond the capacity get 0.
 * The frame side reaches the depth two ways: g_Vg through e2e_vertex_maps_bwd (Vg = R V + t), g_alpha through e2e_vertex_alpha_bwd.
 * One pixel owns one row and one row is won by at most one pixel: a gather over pixels, no atomics, bitwise reproducible.
 * The pose of the map step is a constant by default; with the chain gradient (FusionMap.step_differentiable(pose_gradient=True)) it is a
 * variable through Vg = R V + t: g_pose[:3] = [sum g_Vg V^T | sum g_Vg] over the valid pixels (e2e_transform_points_bwd_t), bottom row 0;
 * the association still sees it as a constant.  Not differentiated: the normals; single sequence only; the resident forms (e2e_*_dev)
 * have no tape.
 *
 * e2e_pf_fuse_tape runs BETWEEN e2e_pf_associate and e2e_pf_fuse_append on the same workspace and map (the forward fuses in place) and
 *   records per pixel what the backward needs: the destination row as int64 (winner n, appended row, or -1) and, for a fused pixel, the
 *   winner's ccount, point and colour before the step.  The appended-row numbering is RECOMPUTED with the same ordered scan as
 *   e2e_pf_fuse_append's (pixels with depth != 0 and no winner, row-major; rows at or beyond map_capacity are dropped: -1), not read from
 *   the workspace -- the forward's offsets do not exist yet when the tape is taken.  tape: e2e_pf_fuse_tape_bytes(H, W) bytes, O(H*W)
 *   whatever the size of the map.
 * e2e_pf_fuse_bwd: tape, the frame's Vg / rgb (H,W,3) and alpha (H,W), the step's output gradients g_points / g_colors (M_after,3) and
 *   g_ccounts (M_after) -- each may be NULL = zero -- and the map sizes before and after the step  ->  g_Vg, g_rgb (H,W,3), g_alpha (H,W),
 *   g_prev_points, g_prev_colors (M_before,3), g_prev_ccounts (M_before).  Every output may be NULL (not wanted), not all of them.
 *   ccounts_after: the ccounts after the step (at least M_before rows; for a row that won no pixel that is its confidence before the
 *   step); needed when g_prev_points or g_prev_colors is wanted and M_before > 0.  One streaming pass over the M_before rows (skipped
 *   when no g_prev_* is wanted), then one pass over the pixels.
 * e2e_vertex_alpha_bwd: g_depth (+)= g_alpha * d alpha / d depth with alpha = exp(-|V|^2 / alpha_den), V = Kinv [w, h, 1] depth:
 *   -2 |Kinv [w, h, 1]|^2 depth alpha / alpha_den for a valid pixel, 0 where depth == 0.  alpha: the forward's output.  accumulate = 1
 *   adds to g_depth (after e2e_vertex_maps_bwd on the same buffer), 0 overwrites it.  depth, alpha, g_alpha, g_depth (B,H,W); K (B,4,4). */
int64_t e2e_pf_fuse_tape_bytes(int H, int W);
int e2e_pf_fuse_tape(const float* map_points, const float* map_colors, const float* map_ccounts, int64_t M, int64_t map_capacity,
                     const float* depth, void* workspace, int H, int W, void* tape, void* stream);
int e2e_pf_fuse_bwd(const void* tape, const float* Vg, const float* rgb, const float* alpha, const float* g_points,
                    const float* g_colors, const float* g_ccounts, const float* ccounts_after, int64_t M_before, int64_t M_after,
                    float* g_Vg, float* g_rgb, float* g_alpha, float* g_prev_points, float* g_prev_colors, float* g_prev_ccounts,
                    int H, int W, void* stream);
int e2e_vertex_alpha_bwd(const float* depth, const float* K, const float* alpha, const float* g_alpha, float alpha_den,
                         float* g_depth, int accumulate, int B, int H, int W, void* stream);

/* THE NORMALS' GRADIENT (opt-in: gradslam.slam.PointFusion(normal_gradient=True), E2E_NORMAL_GRAD=1 for train_depth.py).  In the
 * reference's single graph every normal is a finite-difference function of three depths, is fused with the confidence weights and is
 * read by the point-to-plane residual of every later localisation (e2e_icp_normal_equations_bwd_tgt returns g_tgt_normals).  The three
 * entry points below carry that gradient to the depth; the blocks above keep their rule ("the normals are not differentiated") for the
 * entry points they declare.
 *
 * e2e_normal_maps_bwd: d/d(depth) of sum(g_Nm . Nm) + sum(g_Ng . Ng), the adjoint of e2e_vertex_normal_maps's own normal expressions.
 *   depth (B,H,W); K, pose (B,4,4); g_Nm, g_Ng (B,H,W,3) channels-last, either may be NULL, both NULL is refused; g_depth (B,H,W).
 *   accumulate = 1 adds to g_depth (after e2e_vertex_maps_bwd or e2e_vertex_alpha_bwd on the same buffer), 0 overwrites it.
 *   Rule.  CONSTANTS: the validity mask vf = (depth != 0), the pose, the intrinsics.  Per pixel p = (h,w): r_p = (kx w + kxc, ky h + kyc, 1),
 *   V_p = r_p d_p vf_p; dh_p = V_{h,w+1} - V_p (the constant 0 in the last column), dv_p = V_{h+1,w} - V_p (the constant 0 in the last
 *   row); c = dh x dv, nrm = |c|, n = (c / where(nrm == 0, 1, nrm)) vf_p, Ng = R n.  Adjoint:
 *     gn = (g_Nm[p] + R^T g_Ng[p]) vf_p
 *     gc = (gn - nh (nh . gn)) / nrm with nh = c / nrm where nrm != 0;  gc = gn where nrm == 0: the forward's divisor is the constant 1
 *          there (the where is taken on the norm, nothing is divided by 0), so the result is finite, never NaN
 *     g_dh = dv x gc,  g_dv = gc x dh
 *     p sends -(g_dh + g_dv) to V_p, g_dh to V_{h,w+1} when w+1 < W, g_dv to V_{h+1,w} when h+1 < H (a difference held at the constant
 *     0 sends nothing);  g_depth[j] = vf_j r_j . gV_j.
 *   A gather: the thread of pixel j collects its three contributors (j itself, (h,w-1) as a right neighbour, (h-1,w) as a lower
 *   neighbour) and recomputes their cross-product adjoints from seven depths and three gn.  No atomics; the result does not depend on
 *   the grid; bitwise reproducible.  Invalid pixels get exactly 0 (accumulate: keep their prior value).  The per-pixel arithmetic is
 *   float64, rounded once on the store (1 / nrm and V_{p+1} - V_p cancel digits in float32); the inverse intrinsics are the float32
 *   ones of the forward, widened.
 *   With a pose that requires grad, Ng = R n also gives g_pose[:3,:3] += sum_p g_Ng[p] n_p^T: e2e_transform_points_bwd_t(g = g_Ng,
 *   points = Nm), left 3x3 block only (the fourth column of that call is no gradient of anything here and is discarded).
 *
 * The normals' side of the map step.  The forward is N' = (c N + a Ng[q]) / s, s = c + a, NOT renormalised; constants as for the
 * DIFFERENTIABLE MAP STEP above.  The adjoint is the points' rule with N for P (gN: the gradient of the step's output normals):
 *   appended:  g_Ng[q] = gN[r]
 *   fused:     g_Ng[q] = (a/s) gN[n]     g_alpha[q] += gN[n].(Ng[q] - N') / s     g_prevN[n] = (c/s) gN[n]     g_prevcc[n] += gN[n].(N - N') / s
 *              (s == 0, where the forward divides by 1: g_alpha[q] += gN[n].Ng[q], g_prevcc[n] += gN[n].N, the other two are 0)
 *   a map row that won no pixel passes gN through and gets nothing for its confidence, except that a zero-confidence row in a step where
 *   anything matched gets 0, as for the points;  invalid pixels and rows dropped beyond the capacity get 0.
 * e2e_pf_fuse_normals_tape runs AFTER e2e_pf_fuse_tape and BEFORE e2e_pf_fuse_append: for every fused pixel (the winner's row number is
 *   already in `tape`) it records the winner's normal before the step, 0 for every other pixel.  ntape:
 *   e2e_pf_fuse_normals_tape_bytes(H, W) bytes, O(H*W) whatever the size of the map.  M: the live rows before the step.
 * e2e_pf_fuse_normals_bwd: both tapes, the frame's Ng (H,W,3) and alpha (H,W), g_normals (M_after,3), ccounts_after (as for
 *   e2e_pf_fuse_bwd; needed when g_prev_normals is wanted and M_before > 0)  ->  g_Ng (H,W,3), g_prev_normals (M_before,3), and the
 *   normals' contributions to g_alpha (H,W) and g_prev_ccounts (M_before).  One accumulate flag covers those two: 1 adds to what
 *   e2e_pf_fuse_bwd wrote into them, 0 overwrites.  Every output may be NULL (not wanted), not all of them.  One streaming pass over
 *   the M_before rows (skipped when it has nothing to write), then one pass over the pixels.  No atomics. */
int e2e_normal_maps_bwd(const float* depth, const float* K, const float* pose, const float* g_Nm, const float* g_Ng,
                        float* g_depth, int accumulate, int B, int H, int W, void* stream);
int64_t e2e_pf_fuse_normals_tape_bytes(int H, int W);
int e2e_pf_fuse_normals_tape(const void* tape, const float* map_normals, int64_t M, void* ntape, int H, int W, void* stream);
int e2e_pf_fuse_normals_bwd(const void* tape, const void* ntape, const float* Ng, const float* alpha, const float* g_normals,
                            const float* ccounts_after, int64_t M_before, int64_t M_after, float* g_Ng, float* g_prev_normals,
                            float* g_alpha, float* g_prev_ccounts, int accumulate, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* chamferdist.knn_points, K = 1, D = 3 (loss/losses.py:3,57)                                   */
/* ------------------------------------------------------------------------------------------ */

/* p1 (n1,3) queries, p2 (n2,3) references -> dists (n1) squared L2, idx (n1) int64 (first minimum
 * wins = smallest index among equal distances).  algorithm: 0 = auto, 1 = brute force (LDS-tiled,
 * fp32 VALU bound), 2 = exact uniform grid (counting-sort build + shell search with a provable
 * stopping rule + brute-force finish for the few unbounded queries).  Both give IDENTICAL results.
 * workspace: e2e_knn1_workspace_bytes(n1, n2) bytes. */
int64_t e2e_knn1_workspace_bytes(int64_t n1, int64_t n2);
int e2e_knn1_fwd(const float* p1, int64_t n1, const float* p2, int64_t n2, float* dists,
                 long long* idx, void* workspace, int algorithm, void* stream);
/* g_p1 = 2 g_dists (p1 - p2[idx]) */
int e2e_knn1_bwd(const float* g_dists, const float* p1, const float* p2, const long long* idx,
                 int64_t n1, float* g_p1, void* stream);
/* The other half of chamferdist's knn_points backward (un-vendored, SURVEY.md Appendix A: "d p2 = scatter of the negative"):
 *   g_p2[idx[i]] += -2 g_dists[i] (p1[i] - p2[idx[i]])        (n2,3)
 * reached by ChamferDistance(..., bidirectional=True) at train_depth.py:690-692, whose reverse term searches the
 * differentiable cloud.  Collisions are summed as 2^-48 fixed-point integers (order independent, bitwise reproducible);
 * scratch_fixed: 3*n2+1 int64, zeroed here.  A non-finite / >= 4096 contribution turns the whole result into NaN. */
int e2e_knn1_bwd_ref(const float* g_dists, const float* p1, const float* p2, const long long* idx,
                     int64_t n1, int64_t n2, long long* scratch_fixed, float* g_p2, void* stream);

/* Persistent index over one reference set: build once, query many times (ICP iterations, the
 * refinement steps of one keyframe all search the same map).  `index`: caller-owned buffer of
 * e2e_knn1_workspace_bytes(max_queries, n2) bytes; results are identical to e2e_knn1_fwd. */
int e2e_knn1_index_build(const float* p2, int64_t n2, int64_t max_queries, void* index, void* stream);
int e2e_knn1_index_query(const float* p1, int64_t n1, int64_t n2, int64_t max_queries, void* index,
                         float* dists, long long* idx, void* stream);
/* The index over a RESIDENT reference set (the global map of online_adaption.py:638-645) whose live size
 * is device data: *n2_dev points (0 < *n2_dev <= n2_capacity) are indexed, the host never reads the count.
 * `index`: e2e_knn1_index_capacity_bytes(max_queries, n2_capacity) bytes, allocated once for the run;
 * all launch arguments are constant between builds (the 3-D loss launches can sit in a captured hipGraph).
 * Results are identical to e2e_knn1_fwd on the first *n2_dev points. */
int64_t e2e_knn1_index_capacity_bytes(int64_t max_queries, int64_t n2_capacity);
int e2e_knn1_index_build_dev(const float* p2, const long long* n2_dev, int64_t n2_capacity, int64_t max_queries,
                             void* index, void* stream);
int e2e_knn1_index_query_dev(const float* p1, int64_t n1, int64_t n2_capacity, int64_t max_queries, void* index,
                             float* dists, long long* idx, void* stream);
/* The resident index at a caller-chosen resolution (cells per axis, 4 .. 256) for query sets the map-tuned rule does not fit:
 * frame-to-model odometry (PointFusion._localize behind online_adaption.py:362) asks 19 200 queries of a sparse target set,
 * possibly decimetres away while the pose is still wrong -- a coarse grid bounds the walk over empty cells.  Identical results
 * at any resolution.  ref_points / warm_idx: both NULL (cold search) or both set (candidates from an earlier search). */
int64_t e2e_knn1_index_capacity_bytes_res(int64_t max_queries, int64_t n2_capacity, int cells_per_axis);
int e2e_knn1_index_build_dev_res(const float* p2, const long long* n2_dev, int64_t n2_capacity, int64_t max_queries,
                                 void* index, int cells_per_axis, void* stream);
int e2e_knn1_index_query_dev_res(const float* p1, int64_t n1, const float* ref_points, const long long* warm_idx,
                                 int64_t n2_capacity, int64_t max_queries, void* index, int cells_per_axis,
                                 float* dists, long long* idx, void* stream);
/* The same query for queries that are the pixels of an image (row-major, `row_len` pixels per row, n1 a whole number of rows -- the
 * back-projected depth map of the 3-D loss, online_adaption.py:638-645): the lanes of a wave take 8 x 8 pixel tiles, whose points share
 * their grid cells, instead of 64 consecutive pixels of a row.  Results are identical; row_len = 0 (or sizes that are not multiples of 8)
 * falls back to the plain order. */
int e2e_knn1_index_query_dev_image(const float* p1, int64_t n1, int row_len, int64_t n2_capacity, int64_t max_queries, void* index,
                                   float* dists, long long* idx, void* stream);
/* ... with a WARM START: warm_idx[i] (NULL: none; may be the same buffer as idx) is the result of an earlier query for a point near
 * p1[i] against the same reference set -- the three refinement steps of a keyframe (online_adaption.py:259-327) query the same pixels with
 * slightly moved depths.  The candidate's distance bounds the search from the start; the result is still the exact nearest neighbour
 * (lowest index among ties), whatever the candidates are -- entries outside [0, live points) are ignored.  ref_points: the reference
 * points the index was built over (unsorted, rows of 3 floats). */
int e2e_knn1_index_query_dev_image_warm(const float* p1, int64_t n1, int row_len, const float* ref_points, const long long* warm_idx,
                                        int64_t n2_capacity, int64_t max_queries, void* index, float* dists, long long* idx, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* disp -> depth, median scaling, regulariser, metrics, optimiser                                */
/* ------------------------------------------------------------------------------------------ */

/* torch.median over all elements (online_adaption.py:295,343): the LOWER median (rank (n-1)/2) by
 * radix select; *value_out (device).  workspace: e2e_median_workspace_bytes() bytes; afterwards it
 * also holds the smallest index whose value equals the median and the number of elements that hold it (used by
 * the scale chain's autograd).  Values are ordered by their bit patterns: -0.0 sorts below +0.0, and a NaN is not propagated -- one
 * with the sign bit clear sorts above +inf, one with it set below -inf, so the result is NaN only when the rank falls among them
 * (torch.median returns NaN as soon as one is present; depths and disparities hold none). */
int64_t e2e_median_workspace_bytes(void);
int e2e_median_lower(const float* x, int64_t n, float* value_out, void* workspace, void* stream);

/* online_adaption.py:282,292-298 for the n = F*H*W elements of the stacked disparities:
 *   delta = 1/disp ; ratio = median_gt / median(delta) ; depth = ratio * delta.
 * median_gt, median_delta, ratio_out are device scalars.  The backward is the exact autograd chain,
 * including the term torch routes to the element that IS the median:
 *   g_delta = ratio*g + [delta_i == median] * (-(ratio/median_delta) * sum(g*delta)) / #{delta_j == median} ;
 *   g_disp = -delta^2 g_delta      (torch.median(x) differentiates as evenly_distribute_backward: the elements that HOLD
 *   the median value share its gradient equally -- one element unless values tie exactly).
 * workspace (shared by fwd and bwd of one step): e2e_depth_scale_workspace_bytes() bytes. */
int64_t e2e_depth_scale_workspace_bytes(void);
int e2e_depth_scale_fwd(const float* disp, const float* median_gt, float* delta, float* depth,
                        float* median_delta, float* ratio_out, void* workspace, int64_t n,
                        void* stream);
int e2e_depth_scale_bwd(const float* g_depth, const float* delta, const float* median_gt,
                        const float* median_delta, float* g_disp, void* workspace, int64_t n,
                        void* stream);
/* TEST INSTRUMENTATION, no counterpart in the reference; the refinement step itself calls e2e_depth_scale_bwd.  The same chain
 * with the elements that receive the median's gradient NAMED by the caller (device int32 indices into the n stacked
 * predictions, 1..64 of them, sharing the gradient equally; n_elements == 0: e2e_depth_scale_bwd).  Among 614 400 fp32 depths
 * the neighbours of the median lie ~1e-6 apart, closer than two correct evaluations of the network agree, so WHICH element
 * it is belongs to the evaluation, not to the algorithm -- the parity tests name the CPU evaluation's elements here and
 * compare everything else (online_adaption.py:295-298). */
int e2e_depth_scale_bwd_at(const float* g_depth, const float* delta, const float* median_gt,
                           const float* median_delta, const int* elements, int n_elements,
                           float* g_disp, void* workspace, int64_t n, void* stream);

/* The fixed-scale form of train_depth.py:331-345 (`depth = 1 / disp` then `depth *= ABLATION.scaling_depth`): delta = 1 / disp
 * (may be NULL), depth = delta * scale; backward g_disp = -(g_depth * scale) / disp^2. */
int e2e_depth_fixed_scale_fwd(const float* disp, float scale, float* delta, float* depth, int64_t n,
                              void* stream);
int e2e_depth_fixed_scale_bwd(const float* g_depth, const float* disp, float scale, float* g_disp,
                              int64_t n, void* stream);

/* depth_reguralizer (losses.py:134-148) as a stand-alone op: out = mean |a-b| (kind 1) or
 * mean (a-b)^2 (kind 2); backward wrt b with upstream device scalar g_out.
 * workspace: e2e_reduce_workspace_floats() floats. */
int64_t e2e_reduce_workspace_floats(void);
int e2e_mean_diff_fwd(const float* a, const float* b, int64_t n, int kind, float* out,
                      float* workspace, void* stream);
int e2e_mean_diff_bwd(const float* a, const float* b, const float* g_out, int64_t n, int kind,
                      float* g_b, void* stream);

/* depth_metrics / compute_depth_errors (losses.py:162-201): out7 = abs_rel, sq_rel, rmse, rmse_log,
 * a1, a2, a3 over the kept pixels (mask_zero_gt = 1 drops gt == 0: the "TUM" rule). */
int e2e_depth_metrics(const float* gt, const float* pred, int64_t n, int mask_zero_gt, float* out7,
                      float* workspace, void* stream);

/* torch.optim.Adam step (training_utils.py:23-25; amsgrad off, no weight decay) over ONE flat,
 * 16-byte-aligned fp32 buffer per state; `step` is the 1-based step count. */
int e2e_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int step, void* stream);
/* The data-parallel form (one sequence per GPU): `grad_sums` is the flat bucket after ONE all-reduce(SUM)
 * over the ranks, `participants` (device scalar, all-reduced as the bucket's extra tail element) the number of ranks that
 * took a refinement step; the update uses grad_sums / max(participants, 1), so every value <= 1 (0 included) leaves the
 * gradient as it is.  participants == 1: identical to e2e_adam_step, bit for bit. */
int e2e_adam_step_mean(float* params, const float* grad_sums, const float* participants, float* exp_avg,
                       float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2, float eps,
                       int step, void* stream);
/* The hipGraph-safe form: the step count lives on the device.  schedule (device, 8-byte aligned) holds for t = 1..len the
 * pair { lr / (1 - beta1^t), sqrt(1 - beta2^t) } exactly as the host computes it for e2e_adam_step (doubles rounded to
 * fp32); the launch uses entry step_counter[0] (1-based, clamped to [1, len]: a counter of 0 or less reads the first row, one
 * past len the last) and a second one-thread kernel advances the counter by exactly 1 whatever its value, so a captured step
 * replays through the bias corrections.  participants may be NULL (= 1).  Equal inputs give e2e_adam_step's bits. */
int e2e_adam_step_resident(float* params, const float* grad_sums, const float* participants, float* exp_avg,
                           float* exp_avg_sq, int64_t n, float beta1, float beta2, float eps,
                           const float* schedule, int schedule_len, int* step_counter, void* stream);

/* The other optimisers of define_optim (training_utils.py:26-47) over the same flat bucket, hipGraph-safe like the resident Adam
 * form: one flat, 16-byte-aligned fp32 buffer per array, g = grad_sums / max(participants[0], 1) (participants: device scalar or
 * NULL = 1), the learning rate READ FROM DEVICE MEMORY (`lr`, one float: a replayed launch sees a rate rewritten in place), and a
 * device step counter that a second one-thread kernel advances by exactly 1 behind the update (the update does not read it).  The
 * other hyper-parameters are doubles, rounded to fp32 once on the host as torch rounds the python scalars of its own updates.  No
 * atomics: equal inputs give equal bits.  g == 0 on a zero state leaves the parameter as it is (the padding between bucket slices).
 *   SGD (dampening 0, no nesterov):       d = g + weight_decay * p;  buf = momentum * buf + d;  p -= lr * buf
 *                                         (a zero buffer makes the first step buf = d, as torch's first step does)
 *   RMSprop (no momentum, not centred):   v = alpha * v + (1 - alpha) * g * g;  p -= lr * g / (sqrt(v) + eps)
 *   Adagrad (lr_decay 0):                 s += g * g;  p -= lr * g / (sqrt(s) + eps)
 * momentum, weight_decay >= 0; 0 <= alpha <= 1; eps > 0. */
int e2e_sgd_step_resident(float* params, const float* grad_sums, const float* participants, float* momentum_buffer,
                          int64_t n, const float* lr, double momentum, double weight_decay, int* step_counter,
                          void* stream);
int e2e_rmsprop_step_resident(float* params, const float* grad_sums, const float* participants, float* square_avg,
                              int64_t n, const float* lr, double alpha, double eps, int* step_counter, void* stream);
int e2e_adagrad_step_resident(float* params, const float* grad_sums, const float* participants, float* sum, int64_t n,
                              const float* lr, double eps, int* step_counter, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Depth network convolutions -- depth_estimation/networks.py:44-57,157-189,277-292             */
/* fp32 implicit GEMM on v_mfma_f32_32x32x2_f32, NHWC activations.                               */
/* ------------------------------------------------------------------------------------------ */
#define E2E_ACT_NONE 0
#define E2E_ACT_RELU 1
#define E2E_ACT_ELU 2
#define E2E_ACT_DISP 3   /* 10*sigmoid(x)+0.01 (networks.py:290) */

/* torch weight (Cout,Cin,KH,KW) -> w_fwd [(kh,kw,ci)][ld_fwd] and/or w_bwd [(kh,kw,co)][ld_bwd]
 * (k-major GEMM operands; the padding columns must have been zeroed by the caller). */
int e2e_conv_weight_layouts(const float* w, int Cout, int Cin, int KH, int KW, float* w_fwd,
                            int ld_fwd, float* w_bwd, int ld_bwd, void* stream);

/* The same for `nlayers` layers in one launch (all layouts go stale together after an optimiser
 * step).  `desc`: DEVICE array of 10 int64 per layer {w, w_fwd, w_bwd (addresses, 0 = skip), Cout,
 * Cin, KH, KW, ld_fwd, ld_bwd, 0}. */
int e2e_conv_weight_layouts_batched(const long long* desc, int nlayers, void* stream);
/* (descriptor slot 9, "reserved" in round 1: a float* per-output-channel factor folded into w_bwd only, or 0) */

/* out (B,Ho,Wo,Cout) = act( scale[c] * conv(x) + shift[c] (+ residual) ), x = the VIRTUAL input
 * cat( nearest_upsample(src0 (B,Hs/up,Ws/up,C1), up), src1 (B,Hs,Ws,Cin-C1) ) padded by `pad`
 * (pad_mode 0 zeros, 1 reflection) -- upsample, concat and padding are gather arithmetic, never
 * materialised (networks.py:283-287, :186-188).  scale/shift: folded eval-mode BatchNorm and/or
 * bias (either may be NULL).  Cin % 16 != 0 (the RGB stem) takes a scalar-gather path that also
 * applies (v - in_sub) * in_mul to the image (networks.py:50).
 * Any Cout > 0 with ld_fwd >= Cout, ld_fwd % 4 == 0; any of the four activations behind any operand combination.  Refused with
 * E2E_ERR_ARG: a NULL src0 / w_fwd / out; a non-positive B, Hs, Ws, Cin, Cout, KH or KW; up other than 1 or 2 (Hs, Ws multiples of
 * it); C1 outside 1 .. Cin, or C1 < Cin without src1; a stride other than 1 or 2; pad < 0 or a kernel larger than the padded input
 * (Hs + 2 pad < KH, Ws + 2 pad < KW); reflection with pad != 1 or Hs, Ws < 2; on the channel-quad path (Cin and a split C1 multiples of
 * 16) a kernel beyond 3 x 3; on the scalar path an upsample or a second source.  tests/test_gpu_conv_fwd_contracts.py holds all of it. */
int e2e_conv2d_fwd(const float* src0, const float* src1, int C1, int up, const float* w_fwd,
                   int ld_fwd, const float* scale, const float* shift, const float* residual,
                   float* out, int B, int Hs, int Ws, int Cin, int Cout, int KH, int KW, int stride,
                   int pad, int pad_mode, int act, float in_sub, float in_mul, float* workspace,
                   void* stream);
/* Layers with few output tiles (deep, small-spatial) split the reduction over workgroups and add the
 * slices in a fixed order.  workspace for e2e_conv2d_fwd (rows = B*Ho*Wo, cols = Cout, K = KH*KW*Cin)
 * and e2e_conv2d_bwd_data (rows = B*(Hs+2p)*(Ws+2p), cols = Cin, K = KH*KW*Cout); NULL disables it. */
int64_t e2e_conv2d_splitk_workspace_floats(int64_t rows, int cols, int K);
/* floats of workspace for e2e_conv2d_bwd_data* on an input-gradient domain of (B, Hd, Wd, cols) with K = KH * KW * Cout: the split-K
 * slabs of a stride-1 layer, or the per-(tap, parity class) slabs of the stride-2 class form (4 x 4 x the largest class). */
int64_t e2e_conv2d_bwd_data_workspace_floats(int B, int Hd, int Wd, int cols, int K, int stride);
/* The head of every convolution GEMM workspace (e2e_conv_workspace_flag_floats() floats) holds the hand-off flags of the stream-K
 * kernels: zero outside a launch (a launch clears what it raised), so the owner zeroes that region ONCE after allocating the buffer.
 * Its int32 word e2e_conv_streamk_error_index() is raised, and stays raised, if a workgroup ever timed out waiting for a partial tile
 * (a bounded spin instead of a GPU hang); read it wherever the host synchronises anyway. */
int e2e_conv_workspace_flag_floats(void);
int e2e_conv_streamk_error_index(void);
/* Tuned forms (tools/gemm_tune.py, tests/test_gpu_conv.py): the same operators with the GEMM decomposition given PER CALL -- the
 * library keeps no mutable tuning state.  tile_m x tile_n in {64x64, 128x64, 128x128, 128x32, 32x128, 32x64, 64x32, 32x32, 32x96, 64x96};
 * ksplit >= 1: K slices (split-K slabs + reduction launch); ksplit < 0: stream-K on -ksplit persistent workgroups (64 x 64 tiles:
 * equal shares of the flattened (tile, K chunk) space, partial tiles combined in-launch in K order); tile_m == 0: the built-in choice.
 * workspace: e2e_conv_tuned_workspace_floats(GEMM rows, GEMM columns) floats, flag region zeroed.
 * e2e_conv2d_bwd_weight_scaled_tuned: the implicit-GEMM backward-weight kernels with `target_workgroups` pixel slices x tiles;
 * workspace e2e_conv2d_wgrad_tuned_workspace_floats(...). */
int64_t e2e_conv_tuned_workspace_floats(int64_t rows, int cols);
int e2e_conv2d_fwd_tuned(const float* src0, const float* src1, int C1, int up, const float* w_fwd, int ld_fwd, const float* scale,
                         const float* shift, const float* residual, float* out, int B, int Hs, int Ws, int Cin, int Cout, int KH,
                         int KW, int stride, int pad, int pad_mode, int act, float in_sub, float in_mul, float* workspace, int tile_m,
                         int tile_n, int ksplit, void* stream);
int e2e_conv2d_bwd_data_fused_tuned(const float* da, const float* w_bwd, int ld_bwd, float* dxp, int B, int Hs, int Ws, int Cin, int Cout,
                                    int Ho, int Wo, int KH, int KW, int stride, int pad, int pad_mode, int accumulate, const float* x_in,
                                    int in_act, const float* pre_add, float* workspace, int tile_m, int tile_n, int ksplit, void* stream);
int64_t e2e_conv2d_wgrad_tuned_workspace_floats(int B, int Ho, int Wo, int Cin, int Cout, int KH, int KW, int has_bias, int target_workgroups);
int e2e_conv2d_bwd_weight_scaled_tuned(const float* da, const float* out_scale, const float* src0, const float* src1, int C1, int up,
                                       float* dw, float* dbias, float* workspace, int B, int Hs, int Ws, int Cin, int Cout, int Ho, int Wo,
                                       int KH, int KW, int stride, int pad, int pad_mode, int accumulate, float in_sub, float in_mul,
                                       int target_workgroups, void* stream);
/* host-only query of that choice: out3 (HOST pointer) = {bm, bn, K slices}. */
int e2e_conv_gemm_choice(int64_t rows, int cols, int K, int chunk_depth, int allow_split, int* out3_host);

/* dZ = dY * act'(Y) * scale[c]  (Y = the op's OUTPUT; scale may be NULL). */
int e2e_conv2d_act_bwd(const float* dy, const float* y, const float* scale, float* dz, int64_t n,
                       int C, int act, void* stream);
/* the same with dz += ... when accumulate != 0 (a tensor with several consumers, e.g. a BasicBlock's input that feeds
 * both the first convolution and the residual add: networks.py -> torchvision BasicBlock.forward). */
int e2e_conv2d_act_bwd_acc(const float* dy, const float* y, const float* scale, float* dz, int64_t n,
                           int C, int act, int accumulate, void* stream);

/* gradient wrt the virtual (padded when pad_mode == 1) input: dxp (B,Hs+2p,Ws+2p,Cin). 
 * workspace: e2e_conv2d_bwd_data_workspace_floats(B, Hs + 2 pp, Ws + 2 pp, Cin, KH * KW * Cout, stride) floats (NULL: no split). */
int e2e_conv2d_bwd_data(const float* dz, const float* w_bwd, int ld_bwd, float* dxp, int B, int Hs,
                        int Ws, int Cin, int Cout, int Ho, int Wo, int KH, int KW, int stride,
                        int pad, int pad_mode, float* workspace, void* stream);
/* the same with dxp += ... when accumulate != 0 (pad_mode 0 only: the padded domain of a reflection-padded layer is folded
 * by e2e_conv2d_gather_adjoint, which has its own accumulate flags). */
int e2e_conv2d_bwd_data_acc(const float* dz, const float* w_bwd, int ld_bwd, float* dxp, int B, int Hs,
                            int Ws, int Cin, int Cout, int Ho, int Wo, int KH, int KW, int stride,
                            int pad, int pad_mode, int accumulate, float* workspace, void* stream);
/* Backward-data for the launch plan of a whole network (e2ehip.netplan), which keeps d loss / d PRE-activation in every gradient
 * buffer: `da` is that gradient of this layer's output (no separate dY * act'(Y) pass; a folded BatchNorm scale is folded into
 * w_bwd by e2e_conv_weight_layouts_batched), and with in_act = 1 (ReLU) / 2 (ELU) the epilogue multiplies the result by
 * act'(.) of the tensor x_in (B,Hs,Ws,Cin) the forward convolution read, so dxp is already the pre-activation gradient of the
 * layer that produced x_in (pad_mode 0 only; reflection-padded layers apply it in e2e_conv2d_gather_adjoint_act).
 * pre_add (may be NULL; (B,Hs,Ws,Cin)): a second gradient with respect to the same tensor -- the residual branch of a BasicBlock
 * (networks.py / torchvision BasicBlock.forward `out += identity`) -- added before the act' factor:
 * dxp (+)= (dA * W^T + pre_add) * act'(x_in). */
int e2e_conv2d_bwd_data_fused(const float* da, const float* w_bwd, int ld_bwd, float* dxp, int B, int Hs,
                              int Ws, int Cin, int Cout, int Ho, int Wo, int KH, int KW, int stride,
                              int pad, int pad_mode, int accumulate, const float* x_in, int in_act,
                              const float* pre_add, float* workspace, void* stream);
/* adjoint of the gather: dxp -> d_src0 (B,Hs/up,Ws/up,C1) [, d_src1 (B,Hs,Ws,Cin-C1)]; every output
 * element sums its reflect-pad copies and its up x up readers in a fixed order (no atomics). */
int e2e_conv2d_gather_adjoint(const float* dxp, int B, int Hs, int Ws, int Cin, int C1, int up,
                              int padded, float* d_src0, float* d_src1, int accumulate0,
                              int accumulate1, void* stream);

/* the same, each destination multiplied by act'(.) of the tensor it is the gradient of (src0 (B,Hs/up,Ws/up,C1) with act0, src1
 * (B,Hs,Ws,Cin-C1) with act1; 0 none, 1 ReLU, 2 ELU -- derivative taken from the activation's output). */
int e2e_conv2d_gather_adjoint_act(const float* dxp, int B, int Hs, int Ws, int Cin, int C1, int up,
                                  int padded, float* d_src0, float* d_src1, int accumulate0,
                                  int accumulate1, const float* src0, int act0, const float* src1,
                                  int act1, void* stream);

/* dW (Cout,Cin,KH,KW) [and dbias (Cout) when non-NULL] = split-K GEMM over the output pixels with a
 * fixed-order slab reduction.  workspace: e2e_conv2d_wgrad_workspace_floats(...) floats. */
int64_t e2e_conv2d_wgrad_workspace_floats(int B, int Ho, int Wo, int Cin, int Cout, int KH, int KW,
                                          int has_bias);
int e2e_conv2d_bwd_weight(const float* dz, const float* src0, const float* src1, int C1, int up,
                          float* dw, float* dbias, float* workspace, int B, int Hs, int Ws, int Cin,
                          int Cout, int Ho, int Wo, int KH, int KW, int stride, int pad,
                          int pad_mode, int accumulate, float in_sub, float in_mul, void* stream);

/* the same on `da` = the gradient BEFORE a folded BatchNorm scale: dW[co] = out_scale[co] * sum_p da[p,co] x[p,...] (the scale is
 * applied once per output element in the slab reduction instead of once per pixel in a separate pass); out_scale may be NULL.
 * dbias[co] = sum_p da[p,co], without the scale: the forward is out_scale * conv + shift, and the bias travels in the shift. */
int e2e_conv2d_bwd_weight_scaled(const float* da, const float* out_scale, const float* src0,
                                 const float* src1, int C1, int up, float* dw, float* dbias,
                                 float* workspace, int B, int Hs, int Ws, int Cin, int Cout, int Ho,
                                 int Wo, int KH, int KW, int stride, int pad, int pad_mode,
                                 int accumulate, float in_sub, float in_mul, void* stream);

/* The slab reduction that ends a backward-weight call, as data (see e2e_conv2d_bwd_weight_scaled_deferred): the reference has no counterpart --
 * torch.autograd runs cuDNN's backward-filter per layer (loss.backward(), online_adaption.py:323) -- this is launch economy of the static plan. */
typedef struct e2e_wgrad_reduce_desc {
    const float* slabs;     /* S partial slabs [Mpad][Npad] */
    float* dw;              /* (Cout,Cin,KH,KW) */
    float* dbias;           /* (Cout) or NULL */
    const float* scale;     /* per-output-channel factor or NULL */
    int S, Mpad, Npad, Cout, Cin, KH, KW, has_bias, accumulate;
    int zl;                 /* 8 or 2: waves that share the slabs of one group of 64 quads (fixes the association of the sum) */
    long long first_item;   /* filled by e2e_wgrad_reduce_batch_prepare */
} e2e_wgrad_reduce_desc;
int e2e_conv2d_bwd_weight_scaled_deferred(const float* da, const float* out_scale, const float* src0,
                                          const float* src1, int C1, int up, float* dw, float* dbias,
                                          float* workspace, int B, int Hs, int Ws, int Cin, int Cout, int Ho,
                                          int Wo, int KH, int KW, int stride, int pad, int pad_mode,
                                          int accumulate, float in_sub, float in_mul,
                                          e2e_wgrad_reduce_desc* desc_out_host, void* stream);
/* A layer's backward-data (the arguments of e2e_conv2d_bwd_data_fused; accumulate = 0, x_in = pre_add = NULL, in_act = 0 give
 * e2e_conv2d_bwd_data) and its backward-weight (those of e2e_conv2d_bwd_weight_scaled_deferred) on the same gradient `da`, as ONE GEMM
 * launch where the decompositions both entry points choose allow it (wgrad_first: the backward-weight tiles come first in the grid),
 * otherwise as the two launch sequences.  Results are bit-identical to the two separate calls. */
int e2e_conv2d_bwd_pair_deferred(const float* da, const float* w_bwd, int ld_bwd, float* dxp, int B, int Hs,
                                 int Ws, int Cin, int Cout, int Ho, int Wo, int KH, int KW, int stride,
                                 int pad, int pad_mode, int accumulate, const float* x_in, int in_act,
                                 const float* pre_add, float* workspace, const float* out_scale,
                                 const float* src0, const float* src1, int C1, int up, float* dw,
                                 float* dbias, float* workspace_w, int accumulate_w, float in_sub,
                                 float in_mul, e2e_wgrad_reduce_desc* desc_out_host, int wgrad_first,
                                 void* stream);
/* e2e_conv2d_bwd_pair_deferred whose ONE launch also runs slab reductions that EARLIER backward-weight GEMMs on the stream left to do: the
 * work items [carry_first_item, carry_first_item + carry_items) of a prepared descriptor table in device memory, as a third part of the
 * grid (carry_place: 0 after both tile sets, 1 between them, 2 in front of them).  The items are bound by memory and fill the tail of a
 * launch bound by the matrix pipe; each does the arithmetic it does in e2e_wgrad_reduce_batched, so the results are bit-identical.  The
 * range must not include this layer's own descriptor, and the slabs it reads must be complete when the launch starts (stream order
 * guarantees that for earlier launches).  carry_items == 0 is e2e_conv2d_bwd_pair_deferred.  Where the two GEMMs do not pair
 * (e2e_conv2d_bwd_pair_is_one_launch == 0) the range runs as a reduction launch of its own after them. */
int e2e_conv2d_bwd_pair_carry(const float* da, const float* w_bwd, int ld_bwd, float* dxp, int B, int Hs,
                              int Ws, int Cin, int Cout, int Ho, int Wo, int KH, int KW, int stride,
                              int pad, int pad_mode, int accumulate, const float* x_in, int in_act,
                              const float* pre_add, float* workspace, const float* out_scale,
                              const float* src0, const float* src1, int C1, int up, float* dw,
                              float* dbias, float* workspace_w, int accumulate_w, float in_sub,
                              float in_mul, e2e_wgrad_reduce_desc* desc_out_host, int wgrad_first,
                              const e2e_wgrad_reduce_desc* carry_descs_dev, int carry_n,
                              long long carry_first_item, long long carry_items, int carry_place,
                              void* stream);
/* Host only: 1 where the two pair entry points run this layer's GEMMs as ONE launch (decided by the code the calls themselves use), 0 where
 * they run two launch sequences or refuse the arguments (a refusal sets e2e_last_error like the calls' own, although nothing failed).  The
 * has_* flags stand for the operands the decision looks at (non-NULL or not). */
int e2e_conv2d_bwd_pair_is_one_launch(int ld_bwd, int B, int Hs, int Ws, int Cin, int Cout, int Ho, int Wo,
                                      int KH, int KW, int stride, int pad, int pad_mode, int accumulate,
                                      int in_act, int has_pre_add, int has_workspace, int has_src1, int C1,
                                      int up, int has_bias);
/* Forward of a stage entry (the first BasicBlock of an encoder stage) on ONE block input x: conv1 -- out1 = act1(scale1 * conv(x, w1) +
 * shift1), KH x KW with `stride` / `pad`, zero padding, exactly e2e_conv2d_fwd with these operands and workspace1 -- and the downsample
 * branch -- z = conv(x, wd), 1 x 1, same stride, no padding (e2e_conv2d_fwd without a workspace); bn_scale / bn_shift / bn_rstd as
 * e2e_bn_fold gives them; y = z * bn_scale + bn_shift as e2e_affine_fwd gives it.  Where both GEMMs resolve to the 32 x 128 tile at
 * chunk depth 32 (e2e_conv2d_fwd_entry_pair_is_one_launch) all of it is ONE launch whose grid carries both tile sets, followed by conv1's
 * split-K epilogue when conv1 is split; otherwise the four launch sequences run one after the other.  Bit-identical to the separate
 * calls either way.  z is the tensor the BatchNorm's backward reads (e2e_affine_bwd). */
int e2e_conv2d_fwd_entry_pair(const float* x, const float* w1_fwd, int ld1, const float* scale1, const float* shift1,
                              float* out1, int act1, float* workspace1, const float* wd_fwd, int ldd,
                              const float* gamma, const float* beta, const float* running_mean,
                              const float* running_var, float eps, float* bn_scale, float* bn_shift, float* bn_rstd,
                              float* z, float* y, int B, int Hs, int Ws, int Cin, int Cout, int KH, int KW, int stride,
                              int pad, void* stream);
/* Host only: 1 where e2e_conv2d_fwd_entry_pair runs as ONE launch (decided by the code the call itself uses), 0 where it falls back to the
 * separate launches or refuses the arguments.  has_workspace1: conv1's workspace is non-NULL. */
int e2e_conv2d_fwd_entry_pair_is_one_launch(int ld1, int ldd, int has_workspace1, int B, int Hs, int Ws, int Cin,
                                            int Cout, int KH, int KW, int stride, int pad);
long long e2e_wgrad_reduce_batch_prepare(e2e_wgrad_reduce_desc* descs_host, int n);
int e2e_wgrad_reduce_batched(const e2e_wgrad_reduce_desc* descs_dev, int n, long long total_items, void* stream);
/* the work items [first_item, first_item + items) of a prepared table: the layers (or parts of layers) in that range and nothing else */
int e2e_wgrad_reduce_batched_range(const e2e_wgrad_reduce_desc* descs_dev, int n, long long first_item, long long items, void* stream);

/* Many device-to-device copies in one launch (launch economy of the static plan; the reference has no counterpart): n descriptors
 * {src, dst, bytes (a positive multiple of 16, both pointers 16-byte aligned), first_item} in device memory, prepared on the host. */
typedef struct e2e_copy_desc {
    const void* src;
    void* dst;
    long long bytes;
    long long first_item;   /* filled by e2e_copy_batch_prepare */
} e2e_copy_desc;
long long e2e_copy_batch_prepare(e2e_copy_desc* descs_host, int n);
int e2e_copy_batched(const e2e_copy_desc* descs_dev, int n, long long total_items, void* stream);

/* ResNet stem max-pool, nn.MaxPool2d(3, 2, 1) (networks.py:53 -> torchvision resnet.maxpool): x (B,H,W,C) NHWC ->
 * y (B,(H-1)/2+1,(W-1)/2+1,C).  The backward keeps no index tensor: every input element re-derives the first maximum
 * (ATen's scan order) of the <= 4 windows that contain it; accumulate != 0 adds to dx, mul_relu != 0 multiplies the
 * result by [x > 0] (the stem's ReLU, whose output x is).  C % 4 == 0. */
int e2e_maxpool3x3s2_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
int e2e_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C,
                         int accumulate, int mul_relu, void* stream);
/* The same pair with the position of each window's maximum kept in one byte per output element (argmax (B,Ho,Wo,C) uint8 = kh * 3 + kw
 * of the first maximum in ATen's scan order): the backward reads the <= 4 windows' bytes instead of re-scanning the input (the launch
 * plan's form; x is only read for mul_relu). */
int e2e_maxpool3x3s2_fwd_idx(const float* x, float* y, unsigned char* argmax, int B, int H, int W, int C, void* stream);
int e2e_maxpool3x3s2_bwd_idx(const float* x, const unsigned char* argmax, const float* dy, float* dx, int B, int H, int W, int C,
                             int accumulate, int mul_relu, void* stream);

/* eval-mode BatchNorm with a TRAINABLE affine (the reference freezes parameters whose name contains "bn",
 * online_adaption.py:182-184, so encoder.layerN.0.downsample.1 keeps training): scale = gamma / sqrt(var + eps),
 * shift = beta - mean * scale, rstd = 1 / sqrt(var + eps) (rstd may be NULL). */
int e2e_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                const float* running_var, float eps, float* scale, float* shift, float* rstd, int C,
                void* stream);
/* y[i] = relu?( z[i] * scale[i % C] + shift[i % C] + residual[i] ) over n NHWC elements (shift / residual may be NULL).
 * With C = 1 and no residual / relu this is Conv1x1(1, 1, bias) / ScaleLayer of the scale-learning experiments
 * (networks.py:191-215). */
int e2e_affine_fwd(const float* z, const float* scale, const float* shift, const float* residual, int relu,
                   float* y, int64_t n, int C, void* stream);
int64_t e2e_affine_bwd_workspace_floats(int C);
/* d gamma[c] = sum_p dy[p,c] (z[p,c] - mean[c]) rstd[c], d beta[c] = sum_p dy[p,c] over P pixels (mean / rstd NULL:
 * 0 / 1, required for C = 1); two-stage fixed-order reduction; accumulate != 0 adds to the outputs. */
int e2e_affine_bwd(const float* dy, const float* z, const float* mean, const float* rstd, int64_t P,
                   int C, float* dgamma, float* dbeta, int accumulate, float* workspace, void* stream);

/* Train-mode BatchNorm2d behind a convolution (csrc/bn_train.hip; networks.py's ResNet body when MODEL.refinement_mode is off and the
 * network stays in train mode, train_depth.py:246-247).  z, y, residual, dy, dz, dresidual are (P, C): P = B*H*W pixels of an NHWC
 * tensor, fp32, 16-byte aligned; C a multiple of 4; P >= 2 (batch statistics need a second value per channel).  Per-channel vectors
 * (C floats) carry no alignment requirement.  workspace: exactly e2e_bn_train_workspace_floats(P, C) floats, the same for both
 * directions (a number of partial-sum rows that depends on (P, C) only, times 2 C, plus 2 C; 0 for sizes that are refused).
 *
 * Forward, three launches (partial statistics about the channel's first pixel -- never raw moments --, a fixed-order float64 merge,
 * the normalisation); backward, three launches (partial sums, fixed-order merge, the elementwise pass; the merge pair is skipped
 * when only dresidual is asked for, the elementwise pass when neither dz nor dresidual is).  No atomics and no host read: two calls on
 * the same inputs give the same bits.  All element offsets are 64-bit.
 * Refused with E2E_ERR_ARG before any launch: a NULL z, y (forward), dy (backward), save_mean, save_rstd or workspace; P < 2; C <= 0 or
 * C % 4 != 0; eps <= 0; only some of running_mean / running_var / num_batches_tracked given; a backward whose dz, dresidual, dgamma and
 * dbeta are all NULL; a misaligned (P, C) tensor or workspace. */
int64_t e2e_bn_train_workspace_floats(int64_t P, int C);

/* y = relu?( (z - mean_B) * rstd_B * gamma + beta + residual? ); batch mean / BIASED variance over the P pixels;
 * running_mean = (1-f) running_mean + f mean_B, running_var likewise with the UNBIASED variance (P / (P-1));
 * *num_batches_tracked += 1 (int64, device); f = momentum, or 1 / (the incremented count) when momentum < 0
 * (nn.BatchNorm2d(momentum=None)).  running_* / num_batches_tracked may all be NULL (no update).
 * save_mean / save_rstd (C floats each) are what the backward needs.  gamma / beta NULL: 1 / 0. */
int e2e_bn_train_fwd(const float* z, const float* gamma, const float* beta, const float* residual, int relu,
                     float eps, float momentum, float* running_mean, float* running_var,
                     int64_t* num_batches_tracked, float* y, float* save_mean, float* save_rstd,
                     int64_t P, int C, float* workspace, void* stream);

/* g = dy * [y > 0] (y NULL: g = dy);  dbeta = sum_p g;  dgamma = sum_p g * xhat;
 * dz = gamma * rstd * (g - dbeta / P - xhat * dgamma / P);  dresidual = g (NULL: not wanted).
 * dz, dgamma, dbeta may each be NULL; accumulate != 0 adds to dgamma / dbeta (flat gradient bucket). */
int e2e_bn_train_bwd(const float* dy, const float* y, const float* z, const float* gamma,
                     const float* save_mean, const float* save_rstd, int64_t P, int C,
                     float* dz, float* dresidual, float* dgamma, float* dbeta, int accumulate,
                     float* workspace, void* stream);

/* upsample() of networks.py:218-221 [+ torch.cat with the skip tensor, :283-286]: x (B,h,w,C1), skip (B,2h,2w,C2) or
 * NULL -> y (B,2h,2w,C1+C2), all NHWC.  (Inside the decoder this is fused into the next convolution's gather.) */
int e2e_upsample2_concat(const float* x, const float* skip, float* y, int B, int h, int w, int C1,
                         int C2, void* stream);

/* The 1-channel disparity head: Conv3x3(reflect) 16 -> 1 (+ activation), networks.py:271-272,289-290.
 * x (B,H,W,16) NHWC, w (1,16,3,3), y (B,H,W).  Backward: dz = dY*act' (e2e_conv2d_act_bwd) ->
 * dx (B,H,W,16), dw (1,16,3,3), dbias (1); any of dx / dw may be NULL.
 * workspace: e2e_head_workspace_floats() floats. */
int e2e_head_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W,
                 int Cin, int act, void* stream);
int64_t e2e_head_workspace_floats(void);
int e2e_head_bwd(const float* dz, const float* x, const float* w, float* dx, float* dw, float* dbias,
                 float* workspace, int B, int H, int W, int Cin, void* stream);

/* e2e_head_bwd whose dx is multiplied by act'(x) (in_act 1 ReLU / 2 ELU, from the activation's output x): the pre-activation
 * gradient of the layer that produced x (launch plan form, see e2e_conv2d_bwd_data_fused).  With both dx and dw asked for, the two
 * gradients come out of ONE pass over x and dz (same partition and summation orders: bit-identical); the environment variable
 * E2E_HEAD_BWD_FUSED=0, read by every call, restores the two kernels. */
int e2e_head_bwd_act(const float* dz, const float* x, const float* w, float* dx, float* dw, float* dbias,
                     float* workspace, int B, int H, int W, int Cin, int in_act, void* stream);

/* The multi-scale disparity heads of the monodepth2 decoder (csrc/disp_heads.hip): Conv3x3(reflect) Cin -> 1 + activation at every
 * scale of DATA.scales, networks.py:134-135,151-152 (num_ch_dec[0..3] = 16, 32, 64, 128 input channels).
 *
 * e2e_disp_head_fwd: x (B,H,W,Cin) NHWC, w (1,Cin,3,3) as torch lays it out, bias (1) or NULL (no bias), y (B,H,W):
 *     y[b,h,w] = act( bias + sum_{ci,kh,kw} w[0,ci,kh,kw] * x[b, r(h+kh-1,H), r(w+kw-1,W), ci] ),
 * r the index map of ReflectionPad2d(1) (-1 -> 1, n -> n-2).  act: 0 none, 3 disp = 10*sigmoid(.)+0.01, 4 sigmoid.
 * Refused with E2E_ERR_ARG, nothing written: a NULL x, w or y; B < 1; H < 2 or W < 2 (the pad needs a second pixel); Cin other than
 * 16, 32, 64, 128; any other act (1 ReLU and 2 ELU of the other convolutions included).
 *
 * e2e_disp_head_bwd: dy (B,H,W) is the gradient of the ACTIVATED output and y (B,H,W) the forward's output; the kernels form
 *     dz = dy * act'(y):   act 0: dy;   act 4: dy * y (1 - y);   act 3: dy * 10 s (1 - s) with s = (y - 0.01) / 10
 * themselves (no activation-backward launch) and write, each only when its pointer is not NULL (a NULL one is neither computed nor
 * written):
 *     dx (B,H,W,Cin): dx[b,p,ci]     = sum over the (q, kh, kw) whose reflected tap position is p of dz[b,q] * w[0,ci,kh,kw]
 *     dw (1,Cin,3,3): dw[0,ci,kh,kw] = sum_{b,h,w} dz[b,h,w] * x[b, r(h+kh-1,H), r(w+kw-1,W), ci]
 *     dbias (1):      dbias[0]       = sum_{b,h,w} dz[b,h,w]
 * dw and dbias are per-workgroup partial sums (in workspace) added by a second kernel in a fixed order; no atomics anywhere: two calls
 * on the same inputs give the same bits.  workspace: exactly e2e_disp_head_workspace_floats(B, H, W, Cin) floats are used (a number of
 * partial rows capped by a constant and by the pixel count, times 9 Cin + 1; 0 for sizes the heads refuse); it is required even when
 * only dx is asked for.  All pixel and element offsets are 64-bit.  Refused with E2E_ERR_ARG, nothing written: a NULL dy, y, x, w or
 * workspace, and the forward's conditions on B, H, W, Cin and act. */
int e2e_disp_head_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int act, void* stream);
int64_t e2e_disp_head_workspace_floats(int B, int H, int W, int Cin);
int e2e_disp_head_bwd(const float* dy, const float* y, const float* x, const float* w, float* dx, float* dw, float* dbias,
                      float* workspace, int B, int H, int W, int Cin, int act, void* stream);

/* convert_disp_to_depth (utils/training_utils.py:106-118) times the fixed depth scale of train_depth.py:302-312, one launch each way:
 *     depth[i] = scale / (lo + (hi - lo) * disp[i]),   lo = 1 / max_depth, hi = 1 / min_depth,   i < n;
 *     g_disp[i] = -g_depth[i] * scale * (hi - lo) / (lo + (hi - lo) * disp[i])^2.
 * Refused with E2E_ERR_ARG, nothing written: a NULL pointer, n < 1, or not 0 < min_depth < max_depth. */
int e2e_disp_range_depth_fwd(const float* disp, float min_depth, float max_depth, float scale, float* depth, int64_t n, void* stream);
int e2e_disp_range_depth_bwd(const float* g_depth, const float* disp, float min_depth, float max_depth, float scale, float* g_disp,
                             int64_t n, void* stream);

/* The multi-scale photometric loss of monodepth2 (csrc/disp_pyramid.hip; LOSS.multiscale): every scale's disparity is upsampled
 * bilinearly to the input resolution and converted to depth, so that each scale is warped and compared at full resolution.  For a scale
 * with disparity d (B,1,h,w) and the full size (H,W), h <= H and w <= W -- F.interpolate(d, size=(H,W), mode="bilinear",
 * align_corners=False) followed by e2e_disp_range_depth_fwd:
 *     sy = max((y + 0.5) * h / H - 0.5, 0),  y0 = floor(sy),  y1 = min(y0 + 1, h - 1),  wy = sy - y0        (the same in x)
 *     u(y,x)     = (1-wy)(1-wx) d[y0,x0] + (1-wy) wx d[y0,x1] + wy (1-wx) d[y1,x0] + wy wx d[y1,x1]
 *     depth(y,x) = scale / (lo + (hi - lo) u),   lo = 1 / max_depth, hi = 1 / min_depth
 * and the adjoint, with u recomputed from d (nothing is saved between the two calls):
 *     g_u = -g_depth * scale * (hi - lo) / (lo + (hi - lo) u)^2
 *     g_d[j,i] = sum over every fine pixel (y,x) whose stencil touches (j,i) of its weight on (j,i) times g_u(y,x)
 * (row 0 also receives the fine rows whose sy was clamped to 0, row h-1 both weights of the fine rows whose y1 was clamped onto y0;
 * columns likewise).  The adjoint is a gather: the lanes that own a coarse pixel walk its footprint in a fixed order and are added by a
 * fixed tree; no atomics and no workspace, two calls give the same bits.  Both directions take one stencil function, so the adjoint's
 * weights are the forward's.
 *
 * Up to four scales in ONE launch each way: disp0 .. disp3 with their sizes h0,w0 .. h3,w3; a NULL disparity is an absent scale, and
 * its sizes (and g_disp) are not read.  depth and g_depth are (S,B,1,H,W) over the S present scales in ascending order; the grid's z
 * index is (scale, batch element).  Where h == H and w == W every weight is exactly 0 or 1, and that scale's depth and g_disp are
 * bit-equal to e2e_disp_range_depth_fwd / _bwd on the same input.
 * Refused with E2E_ERR_ARG before any launch, nothing written: a NULL depth / g_depth; no scale present; a present scale with h > H,
 * w > W or a non-positive size, or (backward) a NULL g_disp; B < 1, H < 1 or W < 1; not 0 < min_depth < max_depth; and the limits of
 * the launch geometry: H or W above 262140, S * B above 65535, a coarse pixel whose footprint exceeds 2^31 - 1 fine pixels. */
int e2e_disp_pyramid_depth_fwd(const float* disp0, const float* disp1, const float* disp2, const float* disp3, int h0, int w0, int h1, int w1,
                               int h2, int w2, int h3, int w3, int B, int H, int W, float min_depth, float max_depth, float scale,
                               float* depth, void* stream);
int e2e_disp_pyramid_depth_bwd(const float* g_depth, const float* disp0, const float* disp1, const float* disp2, const float* disp3, int h0,
                               int w0, int h1, int w1, int h2, int w2, int h3, int w3, int B, int H, int W, float min_depth, float max_depth,
                               float scale, float* g_disp0, float* g_disp1, float* g_disp2, float* g_disp3, void* stream);

/* The multi-scale edge-aware smoothness of monodepth2 (csrc/disp_pyramid_smooth.hip; LOSS.multiscale_smoothness): every scale's
 * mean-normalised disparity held against the colour image at that scale's own resolution, loss and gradient in one call.
 * Slots: dispK is (B,1,hK,wK) contiguous; a NULL dispK is an absent scale: its sizes, weight and g_dispK are not read and its g_dispK
 * buffer is not written.
 * Image: img is (B,3,H,W) read through img_strides (an NCHW view of NHWC memory works).  For slot K, fy = H / hK and fx = W / wK must be
 * integers >= 1 (they may differ); the image of scale K is the box mean of each fy x fx block per channel, F.avg_pool2d(img, (fy, fx)),
 * each box summed in a fixed order (the fy rows of a column top down, then the fx column sums left to right).  This box pyramid is
 * this project's definition: monodepth2's dataloader resizes the colour image with an antialiasing filter instead.
 * Loss, per present scale (losses.py:119-132 on the mean-normalised disparity of online_adaption.py:600-610):
 *     n = d / (m + 1e-7), m the mean of d over one image's plane
 *     loss_K = mean over B h (w-1) x-edges of |n(y,x) - n(y,x+1)| exp(-mean_c |img_K(c,y,x) - img_K(c,y,x+1)|)
 *            + mean over B (h-1) w y-edges of the same in y
 * loss_out[5]: loss_out[K] = loss_K, unweighted, 0 for an absent slot; loss_out[4] = sum_K weightK loss_K.  All five are always written.
 * Gradients: g_dispK = weightK d loss_K / d dispK, the mean's own contribution included; every element is written, nothing is
 * accumulated.  The subgradient of |.| at 0 is 0: a constant plane gives a loss of exactly 0 and a gradient of exactly 0 everywhere.
 * The sign of an edge is taken from the raw difference d(p) - d(q).  Either every present scale has its g_disp, or all four are NULL
 * (the loss alone; loss_out then has the bits of the call with gradients).
 * Two launches whatever S and B are (the grid's z index is (scale, batch element)); no atomics: per-tile partial sums go into
 * `workspace` (e2e_disp_pyramid_smoothness_workspace_floats floats: partial sums only, no per-pixel plane) and are added in a fixed
 * order, the per-pixel gradient is staged in g_dispK and scaled in place.  Two calls give the same bits.
 * Refused with E2E_ERR_ARG before any launch, nothing written: a NULL img, loss_out or workspace; no scale present; a present scale
 * with h < 2, w < 2, h > H, w > W, H % h != 0 or W % w != 0; some but not all present scales with a g_disp; B < 1, H < 1 or W < 1;
 * S * B above 65535; an image whose strided extent (sum over the axes of (n - 1) |stride|) does not fit the int64_t of e2e_strides.
 * The workspace query takes 0 x 0 for an absent scale and returns 0 for sizes the entry point refuses. */
int64_t e2e_disp_pyramid_smoothness_workspace_floats(int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3, int B);
int e2e_disp_pyramid_smoothness_lossgrad(const float* disp0, const float* disp1, const float* disp2, const float* disp3,
        int h0, int w0, int h1, int w1, int h2, int w2, int h3, int w3,
        const float* img, e2e_strides img_strides, int B, int H, int W,
        float weight0, float weight1, float weight2, float weight3,
        float* loss_out, float* g_disp0, float* g_disp1, float* g_disp2, float* g_disp3,
        float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Frame-to-model ICP odometry (gradslam odometry providers; MODEL.odom: icp | gradicp)          */
/* ------------------------------------------------------------------------------------------ */

/* One Gauss-Newton reduction of point-to-plane ICP: for every source point s_i (n,3) with nearest
 * target t_i = tgt[idx[i]] and normal n_i: A_i = [n_i, s_i x n_i], b_i = n_i . (t_i - s_i).
 * out29 (device, float64) = upper triangle of A^T A (21, row-major), A^T b (6), inlier count,
 * sum b_i^2.  Points with dists[i] >= dist_thresh^2 are skipped (dist_thresh < 0: keep all).
 * workspace: e2e_icp_workspace_bytes() bytes. */
int64_t e2e_icp_workspace_bytes(void);
int e2e_icp_normal_equations(const float* src, const float* tgt, const float* tgt_normals,
                             const long long* idx, const float* dists, float dist_thresh, int64_t n,
                             double* out29, void* workspace, void* stream);

/* THE ADJOINT OF THE ODOMETRY (differentiable ICP / GradICP; the reference back-propagates the photometric loss through the pose into
 * the live frame's depth, train_depth.py:381-382, :395).  The rule, for the whole iteration sequence:
 *   - by default it is taken with respect to the SOURCE points only: target points, target normals and prev_pose are constants.  The
 *     chain gradient (opt-in: point_to_plane_icp(target_gradient=True), PointFusion(chain_gradient=True), E2E_CHAIN_GRAD=1) also takes
 *     it with respect to the target points and normals (e2e_icp_normal_equations_bwd_tgt below) and to prev_pose (pose = T . prev_pose:
 *     T^T gbar_pose, float64 on the host);
 *   - the nearest-neighbour indices, the dist_thresh keep mask and the inlier counts of every search are held fixed;
 *   - the clipped region of GradICP's gate (|nu delta| >= 60) has zero derivative;
 *   - the fp32 roundings of the running transform and of the pose are passed straight through.
 * This entry point is the per-point part for ONE reduction: adj28 (device float64) holds the adjoints of the 21 packed A^T A entries,
 * of A^T b (6) and of sum b^2, in out29's order (the count has none).  With U the upper-triangular unpacking of adj28[0..20],
 * Abar_i = (U + U^T) A_i + b_i gbar, bbar_i = gbar . A_i + 2 ebar b_i:   g_src_i = -bbar_i n_i + n_i x Abar_i[3:6]   (n,3) fp32,
 * added to g_src when accumulate != 0.  A row the forward skipped contributes zero; so does a row whose idx is outside [0, n_tgt), which
 * reads nothing of the target.  Pointwise: nothing to reduce, bitwise reproducible.  The 6x6 part of the adjoint (solve, exp, damping
 * update, gate) is float64 on the host, as the forward's is (e2ehip/icp.py). */
int e2e_icp_normal_equations_bwd(const float* src, const float* tgt, const float* tgt_normals, int64_t n_tgt,
                                 const long long* idx, const float* dists, float dist_thresh, const double* adj28,
                                 int64_t n, float* g_src, int accumulate, void* stream);

/* The TARGET side of the same reduction's adjoint (the chain gradient: the map is a variable of the localisation).  Same arguments and
 * notation; for target row j, summed over the kept source rows i with idx[i] == j:
 *   g_tgt[j]         = sum_i  bbar_i n_j
 *   g_tgt_normals[j] = sum_i  bbar_i (t_j - s_i) + Abar_i[0:3] + Abar_i[3:6] x s_i            both (n_tgt,3) fp32.
 * A row the forward skipped contributes nothing; a row whose idx is outside [0, n_tgt) contributes nothing and reads nothing.  A target
 * that no kept row names gets 0 with accumulate == 0 and keeps its value with accumulate != 0; every other target gets
 * (float)sum, or (float)((double)old + sum).  g_tgt and g_tgt_normals may each be NULL (not wanted), not both.
 * Several sources share one target, so this is a scatter with collisions.  It is done without float atomics and without fixed-point
 * accumulation (adj28 has no bounded scale): the neighbour list is inverted per call (count the kept rows per target, exclusive scan,
 * fill), and one owner per target adds its segment in ascending source index in float64 and rounds once; a segment of more than 64
 * rows goes to a wave (lane l adds the rows l, l + 64, ... of the sorted segment, then a fixed shuffle tree).  Bitwise reproducible and
 * independent of arrival order; memory traffic O(n + n_tgt).  n and n_tgt below 2^31.
 * workspace: e2e_icp_normal_equations_bwd_tgt_workspace_bytes(n, n_tgt) bytes (0 for sizes out of range). */
int64_t e2e_icp_normal_equations_bwd_tgt_workspace_bytes(int64_t n, int64_t n_tgt);
int e2e_icp_normal_equations_bwd_tgt(const float* src, const float* tgt, const float* tgt_normals, int64_t n_tgt,
                                     const long long* idx, const float* dists, float dist_thresh, const double* adj28,
                                     int64_t n, float* g_tgt, float* g_tgt_normals, int accumulate,
                                     void* workspace, void* stream);

/* The rest of an odometry iteration ON THE DEVICE (gradslam odometry providers "icp" / "gradicp" behind PointFusion.step,
 * online_adaption.py:111-122,362; configs/config.yaml:30-35 ships odom: gradicp): solve (A^T A + lambda I) xi = A^T b, the
 * se(3) exponential, GradICP's smooth damping update and T <- exp(.) T, all float64, from the 29 sums of
 * e2e_icp_normal_equations -- so the numiters iterations of a keyframe are a fixed launch sequence without a host round trip.
 *   state   : e2e_icp_state_doubles() float64 (T, xi, lambda, trace ...), initialised by e2e_icp_state_init (T = I, lambda = damp)
 *   T32     : (4,4) float32, the running transform for e2e_transform_points(src -> cur)
 *   step32  : (4,4) float32, GradICP's trial step for e2e_transform_points(cur -> next)
 *   pose_out: (4,4) float32 = T . prev_pose after every update (may be NULL)
 * mode 0 "icp":     phase 0 = solve, T <- exp(xi) T.
 * mode 1 "gradicp": phase 0 = solve, step32 <- exp(xi), remember err / cnt;  phase 1 (out29 = the reduction at the trial pose):
 *                   delta = err' / cnt' - err / cnt ; lambda *= 1/lmax + (lmax - 1/lmax) / (1 + B exp(-B2 nu delta)) ;
 *                   T <- exp(xi / (1 + exp(clip(nu delta, +-60)))) T.
 * Fewer than 6 inliers stop the iteration for good (later updates leave T alone), as the host loop's `break`.
 * exp is Rodrigues' formula and the V matrix; below an angle of 1e-2 their coefficients come from the power series (the closed forms
 * cancel there), so exp(xi) is within 2e-14 max(1, |v|) of the true exponential at every angle (tests/test_icp_ref.py). */
int64_t e2e_icp_state_doubles(void);
int e2e_icp_state_init(double* state, float* T32, float* step32, const float* prev_pose, float* pose_out,
                       double damp, void* stream);
int e2e_icp_update(const double* out29, double* state, float* T32, float* step32, const float* prev_pose,
                   float* pose_out, int mode, int phase, double lambda_max, double B, double B2, double nu,
                   void* stream);
/* e2e_icp_normal_equations followed by e2e_icp_update as TWO launches (the update folds the per-workgroup partial sums itself). */
int e2e_icp_reduce_update(const float* src, const float* tgt, const float* tgt_normals, const long long* idx,
                          const float* dists, float dist_thresh, int64_t n, void* workspace, double* state, float* T32,
                          float* step32, const float* prev_pose, float* pose_out, int mode, int phase,
                          double lambda_max, double B, double B2, double nu, void* stream);
/* Source cloud of the odometry (gradslam downsample_rgbdimages): every dsratio-th pixel in both directions of the live
 * frame's world vertex map Vg (H,W,3), row-major -> src (ceil(H/ds) * ceil(W/ds), 3).  A selected pixel without depth sets
 * *status (device int32; the resident path serves network-predicted depths, which are positive everywhere). */
int e2e_icp_source_subsample(const float* Vg, const float* depth, int H, int W, int dsratio, float* src,
                             int* status, void* stream);

/* ------------------------------------------------------------------------------------------ */
/* Off-by-default losses: loss value(s) AND the gradient for a unit upstream  */
/* gradient in one pass each; workspace: e2e_aux_workspace_floats() floats.                      */
/* ------------------------------------------------------------------------------------------ */
int64_t e2e_aux_workspace_floats(void);

/* loss/losses.py:119-132 disparity_smoothness_loss.  disp (B,1,H,W) contiguous, img (B,C,H,W)
 * through element strides.  loss_out[0] = x term, loss_out[1] = y term (the loss is their sum);
 * g_disp (B,1,H,W) = d(sum)/d(disp) or NULL. */
int e2e_smoothness_lossgrad(const float* disp, const float* img, e2e_strides img_strides, int B, int C,
                            int H, int W, float* loss_out, float* g_disp, float* workspace,
                            void* stream);

/* loss/losses.py:84-95 geometric_consistency_loss on n elements (mask as float, already expanded).
 * stats_out3 = {loss, sum(mask), gradient normaliser}; the `sum(mask) > 10000` gate is evaluated
 * on the device (loss and gradients are 0 when it is closed).  g_* both NULL or both given. */
int e2e_geometric_consistency_lossgrad(const float* warped_depth, const float* interpolated_depth,
                                       const float* mask, int64_t n, float* stats_out3,
                                       float* g_warped, float* g_interpolated, float* workspace,
                                       void* stream);

/* loss/losses.py:151-160 depth_gt_loss: mean |prediction * mask - sparse_gt| over n elements. */
int e2e_masked_l1_lossgrad(const float* prediction, const float* sparse_gt, const float* sparse_mask,
                           int64_t n, float* loss_out, float* g_prediction, float* workspace,
                           void* stream);

/* train_depth.py:657-661: mean over (b,y,x) of min over the C stacked error maps (B,C,H,W); the
 * gradient goes to the first minimal channel.  A NaN wins the minimum like in torch.min (the first NaN channel takes the
 * gradient, the loss is NaN). */
int e2e_min_reprojection_lossgrad(const float* errors, int B, int C, int H, int W, float* loss_out,
                                  float* g_errors, float* workspace, void* stream);

/* train_depth.py's operator-by-operator loss assembly (the fused kernels cover the default flags; these serve min-reprojection /
 * auto-masking / smoothness):  out (B,C,H,W) = x (strided view) * mask (B,1,H,W) (:713-714);  channel mean of stacked error maps
 * (B,C,H,W) -> (B,1,H,W) (:630) and its adjoint (adjoint = 1: x (B,1,H,W) -> out (B,C,H,W) = x / C);  mean-normalised disparity
 * d / (mean_hw(d) + 1e-7) per image (:768-770) and, with g != NULL, its adjoint for the upstream gradient g (workspace: B * 130
 * floats). */
int e2e_mask_mul(const float* x, e2e_strides x_strides, const float* mask, int B, int C, int H, int W,
                 float* out, void* stream);
int e2e_channel_mean(const float* x, int B, int C, int H, int W, int adjoint, float* out, void* stream);
int e2e_mean_normalize(const float* d, const float* g, int B, int H, int W, float* out, float* workspace,
                       void* stream);

/* mean of values[i] over the elements whose gate[i] != 0, and weight x its gradient: the 3-D point loss
 * (online_adaption.py:638-645; loss/losses.py:57-63 `torch.mean(dists)`) over the valid-depth pixels without the
 * reference's boolean indexing (dynamic shape + host sync): gate = the depth map.  out3 = {mean, count, weight / count};
 * g_values (may be NULL) = weight * [gate != 0] / count.  Every gate that compares unequal to zero selects -- negative, tiny and
 * subnormal ones too; +0.0 and -0.0 do not.  An empty selection gives {NaN, 0, 0} and an all-zero gradient.
 * workspace: e2e_aux_workspace_floats() floats. */
int e2e_masked_mean_lossgrad(const float* values, const float* gate, int64_t n, float weight, float* out3,
                             float* g_values, float* workspace, void* stream);

/* train_depth.py:224-237 process_disparity: disp_pair (2,1,H,W) = net(img), net(flip(img)) ->
 * out (1,1,H,W); bwd: g_out (H,W) -> g_disp_pair (2,1,H,W).  With left = disp_pair[0], right = flip_w(disp_pair[1]),
 * middle = (left + right) / 2 and the ROW mask l(y) = 1 - clip(20 (y / (H - 1) - 0.05), 0, 1) (y / (H - 1) = 0 for H = 1; the
 * reference's meshgrid varies along rows, so its flipped mask r equals l):  out = l left + l right + (1 - 2 l) middle. */
int e2e_disp_blend_fwd(const float* disp_pair, int H, int W, float* out, void* stream);
int e2e_disp_blend_bwd(const float* g_out, int H, int W, float* g_disp_pair, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* E2ESLAM_H */
