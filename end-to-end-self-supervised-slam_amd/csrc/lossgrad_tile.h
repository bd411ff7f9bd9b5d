// lossgrad_tile.h -- what k_warp_photo_lossgrad (warp_photo_fused.hip) and k_warp_photo_terms (loss_terms.hip) share of their tile scheme:
// 256 threads own a 32x16 pixel tile, two rows per thread; phase 1 warps the tile + 2-px halo (36x20 positions) into LDS, phase 2 takes
// SSIM statistics on the tile + 1-px halo (34x18) and leaves (G1,G2,G3) in nine LDS planes, phase 3 folds them back per own pixel.
// The per-position arithmetic stays written out in each kernel: moving it into inlined functions reorders k_warp_photo_lossgrad's
// instructions and moves its register counts (profiles/lossgrad_tile_refactor.txt); the constants, the two
// one-line functions below, refl_mult (e2e_common.h) and the host checks do not.
// Include AFTER `#pragma clang fp contract(fast)`: both kernels are compiled with contraction on whatever the command line says.
#pragma once
#include "e2e_common.h"

constexpr int TILE_PPT = 2;     // image rows per thread (one row, 32x8 tiles, measured slower: profiles/r01_warp_photo_lossgrad_history.md)
constexpr int TILE_W = 32, TILE_H = 8 * TILE_PPT;                // own pixels
constexpr int TILE_XW = TILE_W + 4, TILE_XH = TILE_H + 4;        // warped positions: halo 2
constexpr int TILE_GW = TILE_W + 2, TILE_GH = TILE_H + 2;        // SSIM statistics: halo 1
constexpr int TILE_NT = 256;                                     // threads = dim3(TILE_W, 8)
constexpr int TILE_NPOS = TILE_XW * TILE_XH, TILE_NQ = TILE_GW * TILE_GH;
constexpr int TILE_NHALO = TILE_NPOS - TILE_W * TILE_H;          // 208 halo positions, one per thread tid < 208
constexpr int TILE_NE = TILE_PPT + 1;                            // warp evaluations per thread: own pixels, then a halo slot

// halo addressing: reflect, then clamp so that even unused slots address valid memory (their result is zeroed)
__device__ __forceinline__ int tile_clamped(int g, int n) { return min(max(reflect1(g, n), 0), n - 1); }

__device__ __forceinline__ float tile_sign(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

// ---- host: the argument checks both entry points share (`name` = the entry point; the messages are part of the interface) ---------
static int lossgrad_check_args(const char* name, int B, int H, int W, bool pointers, int padding_mode, int reg_kind, bool reg_buffers) {
    E2E_REQUIRE(B > 0 && H > 1 && W > 1 && (int64_t)B * H * W * 3 < (1ll << 31), E2E_ERR_ARG, "%s: bad dims B=%d H=%d W=%d", name, B, H, W);
    E2E_REQUIRE(pointers, E2E_ERR_ARG, "%s: null pointer", name);
    E2E_REQUIRE(padding_mode == E2E_PADDING_BORDER || padding_mode == E2E_PADDING_ZEROS, E2E_ERR_ARG,
                "%s: padding_mode %d not supported (zeros|border)", name, padding_mode);
    E2E_REQUIRE(reg_kind >= 0 && reg_kind <= 2, E2E_ERR_ARG, "%s: reg_kind %d (0 none, 1 l1, 2 l2)", name, reg_kind);
    E2E_REQUIRE(!reg_kind || reg_buffers, E2E_ERR_ARG, "%s: regulariser buffers missing", name);
    return E2E_OK;
}
