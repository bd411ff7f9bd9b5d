// warp_photo_pose.h -- what warp_photo.hip lends to warp_photo_pose.hip: the pose form of the fused backward kernel is an instantiation of
// k_warp_photo_bwd, so its launch stays in that file.  Host functions, C++ linkage, not part of the C ABI.
#pragma once
#include "e2e_common.h"

// 32x8 tiles (= workgroups of the fused backward) per batch element
int64_t warp_photo_bwd_tiles(int H, int W);

// k_warp_photo_bwd<pad, POSE = true>: the launch of e2e_warp_photo_bwd plus 12 float64 sums per workgroup in
// partials[(b * tiles + tile) * 12 + r * 4 + j].  Arguments are not checked here.
void warp_photo_bwd_pose_launch(const float* depth_tgt, const float* src, e2e_strides ss, const float* tgt, e2e_strides ts, const float* K,
                                const float* inv_K, const float* T, const float* synth, const float* valid, int use_mask, int padding_mode,
                                int reg_kind, const float* reg_init_tgt, const float* reg_init_src, const float* depth_src, const float* g_loss,
                                float* g_depth_tgt, float* g_depth_src, double* partials, int B, int H, int W, hipStream_t stream);
