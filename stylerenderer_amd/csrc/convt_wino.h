// Internal interface of the 25-product form of the stride-2 transposed 3x3 convolution (csrc/convt_wino.hip), used by
// sr_conv2d_mfma_ex for the forward of the up-sampling layers.  The kernel writes the interior of the map (rows < 2 IH,
// columns < 2 IW), as k_convt_fused does; output row 2 IH and column 2 IW stay with the strip launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// IW % 32 == 0, IH % 8 == 0, C % 8 == 0, C <= 2048, N % 64 == 0, 16-byte aligned input (NULL: assumed aligned)
bool sr_convt_wino_eligible(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t ldw, const void* in);
// wt: [9][C][ldw] raw taps; no scratch
int sr_convt_wino_launch(float* out, const float* in, const float* wt, int64_t ldw, const float* iscale,
                         const float* oscale, const float* obias, int64_t B, int64_t C, int64_t N, int64_t IH,
                         int64_t IW, hipStream_t st);
