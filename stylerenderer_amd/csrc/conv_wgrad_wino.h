// Internal interface of the Winograd weight gradient of the stride-1 3x3 pad-1 convolution (csrc/conv_wgrad_wino.hip),
// used by sr_conv2d_wgrad_mfma.  SR_WINOGRAD=0 (sr_winograd_enabled, conv_wino.h) keeps it out, as it does the forward
// kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// H % 2 == 0, W % 16 == 0, C % 64 == 0, N % 64 == 0, 0 < B <= 32, 16-byte aligned x / gy
bool sr_wgrad_wino_eligible(int64_t B, int64_t C, int64_t N, int64_t H, int64_t W, const void* x, const void* gy);
// eligible shapes only
int64_t sr_wgrad_wino_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t H, int64_t W);
int sr_wgrad_wino_launch(float* dwt, const float* x, const float* gy, const float* xscale, const float* gscale,
                         int64_t B, int64_t C, int64_t N, int64_t H, int64_t W, float* scratch, hipStream_t st);
