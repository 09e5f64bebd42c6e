// Internal interface of the polyphase stride-2 3x3 weight gradient (csrc/conv_wgrad_s2_wino.hip): 25 instead of 36
// matrix products per 2x2 tile of the base grid, used by sr_conv2d_wgrad_mfma for the shapes k_wgrad_s2_dma serves: the
// same U window (sr_s2_window of wgrad_tile.h), the same patch order (sr_wgrad_patch) and the K slices of
// sr_wgrad_tiles (conv_wgrad_mfma.h), which the dispatch passes in as ks / pps.
// U is the windowed (2G + 1)-wide operand, V the G-wide one (conv_wgrad_mfma.hip has the formula).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wgrad_params.h"

// 3x3 stride 2 pad 0: GW % 16 == 0, GH % 4 == 0, CU % 32 == 0, CV % 128 == 0, windows inside U, byte offsets < 2^31
bool sr_wgrad_s2_wino_eligible(int64_t B, int64_t CU, int64_t CV, int64_t UH, int64_t UW, int64_t GH, int64_t GW, int d0);
// floats of `ks` slabs of 16 transform-domain positions [ks][16][CU][CV]
int64_t sr_wgrad_s2_wino_scratch_floats(int64_t ks, int64_t CU, int64_t CV);
// main launch: K slice s of `ks` covers the 16 x 4 patches [s * pps, (s + 1) * pps) of the direct plan's patch order
int sr_wgrad_s2_wino_launch(const float* U, const float* V, const float* uscale, const float* vscale, float* partial,
                            int64_t B, int64_t CU, int64_t CV, int64_t UH, int64_t UW, int64_t GH, int64_t GW, int ks,
                            int pps, hipStream_t st);
// finish: slices summed in slice order, 16 -> 9 positions, written in the layout of `out`
int sr_wgrad_s2_wino_finish(const WgradOut& out, const float* partial, int ks, int64_t CU, int64_t CV, hipStream_t st);
// Transposed convolution ((u, v) = (n, c)) whose K slices hold `sps` whole slices per sample, main launch with
// vscale = NULL: the finish of wgrad_style_finish.h — dwt [9][C = CV][N = CU] with the style iscale [B][CV] applied, and
// gis[b][c] = sum_{t,n} wt[t][c][n] * (weight gradient of sample b without the style).  wt [9][CV][ldw] is the forward
// weight, `part` sr_wgrad_style_part_floats(B, CU, CV, true) floats.  B <= 32.
int sr_wgrad_s2_wino_style_finish(float* dwt, float* gis, const float* partial, const float* iscale, const float* wt,
                                  int64_t ldw, int sps, int64_t B, int64_t CU, int64_t CV, float* part, hipStream_t st);
