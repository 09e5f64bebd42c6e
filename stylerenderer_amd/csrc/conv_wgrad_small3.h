// Internal interface of the streaming weight gradient of the map heads' tiny 3x3 layers (csrc/conv_wgrad_small3.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// 3x3 stride 1 pad 1, not transposed, C <= 4 and N <= 4, SR_WGRAD_SMALL != 0: every call of such a shape
bool sr_wgrad_small3_eligible(int64_t C, int64_t N, int ksize, int stride, int pad, int transposed);
// one slab of 9 x 4 x 4 sums per pixel block (+ 4)
int64_t sr_wgrad_small3_floats(int64_t B, int64_t IH, int64_t IW);
// writes dwt [9][C][N] in the regular layout; B == 0 writes zeros
int sr_wgrad_small3_launch(float* dwt, const float* x, const float* gy, const float* xscale, const float* gscale, int64_t B,
                           int64_t C, int64_t N, int64_t IH, int64_t IW, float* scratch, hipStream_t st);
