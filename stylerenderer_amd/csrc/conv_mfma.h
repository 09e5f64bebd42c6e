// Internal interface of the direct implicit-GEMM kernel k_conv_mfma and its tap-split, strip and per-phase launchers
// (csrc/conv_mfma.hip), used by the dispatch plan and sr_conv2d_mfma_ex (csrc/conv_dispatch.hip).  Every launcher takes
// the call's ConvParams (buffers, extents, scratch in `partial` / `partial_floats`) by value and sets the geometry of
// its own launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_params.h"

// Scratch the direct kernel's split-K would use: ks * B * N * region for the largest region a launch may split — the
// whole output grid or, transposed, the phase grids and their border strips.  A wish, not a need: the launch drops
// to one slice when the slab does not fit.
int64_t sr_conv_direct_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                              int transposed);
// non-transposed 3x3 / 1x1, stride 1 / 2
int sr_conv_direct_launch(ConvParams p, int ksize, int stride, int pad, hipStream_t st);

// Transposed stride-2 3x3.  Tap-split form (nine shifted 1x1 convolutions in one launch + one reduction): whether a
// call of this size wants it, its K slices, its launch (ks / c_per_slice: sr_convt_taps_plan's; gemm: the
// flattened-pixel form, sr_convt_taps_gemm_eligible for this call's weights)
bool sr_convt_taps_wanted(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW);
void sr_convt_taps_plan(int IH, int IW, int B, int N, int C, int& ks, int& c_per_slice);
int sr_convt_taps_launch(ConvParams p, int ks, int c_per_slice, bool gemm, hipStream_t st);
// output row 2*IH and column 2*IW behind an interior kernel: two three-tap launches + one reduction
int64_t sr_convt_strip_floats(int64_t B, int64_t N, int64_t IH, int64_t IW);
int sr_convt_strips_launch(ConvParams p, hipStream_t st);
// the four output phases as per-phase launches; interior_done: an interior kernel has written the interior already
int sr_convt_phases_launch(ConvParams p, bool interior_done, hipStream_t st);
