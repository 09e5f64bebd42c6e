// Internal interface of the direct weight-gradient kernel (csrc/conv_wgrad_mfma.hip) and the tiling it shares with
// k_wgrad_s2_dma and k_wgrad_s2p, used by sr_conv2d_wgrad_mfma (csrc/conv_wgrad_dispatch.hip).
// U is the operand read through the tap window, V the one on the base grid (conv_wgrad_mfma.hip has the formula).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgrad_params.h"

// Patches of pw x ph pixels x pb samples, channel tiles of ut x vt, and the K (patch) range cut into `ks` slices of
// `pps` patches: the grid is tiles_u * tiles_v * ks workgroups.
struct SrWgradTiles {
    int pw, ph, pb, ut, vt;
    int tiles_x, tiles_y, tiles_b, tiles_u, tiles_v, ks, pps;
};
SrWgradTiles sr_wgrad_tiles(int stride, int B, int CU, int CV, int GH, int GW);
// 4-wave groups per workgroup, by patch type: each writes a partial slab of its own
constexpr int sr_wgrad_groups(int pb) { return pb == 1 ? 2 : 1; }
// floats of the partial slabs [ks * groups][ksize^2][UP][VP] (+ 4)
int64_t sr_wgrad_direct_floats(const SrWgradTiles& t, int ksize);
// the kernel argument of a call on these tiles (k_wgrad_s2_dma takes the same one)
WgradParams sr_wgrad_params(const float* U, const float* V, const float* uscale, const float* vscale, float* partial,
                            int64_t B, int CU, int CV, int UH, int UW, int GH, int GW, int d0, const SrWgradTiles& t);
// ksize 3 | 1, stride 1 | 2; launches nothing when p.B == 0
int sr_wgrad_direct_launch(const WgradParams& p, const SrWgradTiles& t, int ksize, int stride, hipStream_t st);
