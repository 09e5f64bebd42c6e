// Internal interface of the polyphase minimal-filtering stride-2 3x3 convolution (csrc/conv_s2_wino.hip), used by
// sr_conv2d_mfma_ex for the non-transposed stride-2 call: the data gradient of the up-sampling layers and the
// discriminator's down-sampling convolution.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// IH == 2 * OH + 1, IW == 2 * OW + 1, OW % 32 == 0, OH % 8 == 0, C % 4 == 0, N % 64 == 0, 16-byte aligned tensors
bool sr_conv_s2_wino_eligible(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                              const void* in, const void* out);
// workgroups of the launch (the kernel has no K slices: the caller keeps small launches on k_conv_mfma)
int64_t sr_conv_s2_wino_blocks(int64_t B, int64_t N, int64_t OH, int64_t OW);
// floats of transformed weights at the head of the call's scratch
int64_t sr_conv_s2_wino_scratch_floats(int64_t C, int64_t N);
int sr_conv_s2_wino_launch(float* out, const float* in, const float* wt, int64_t ldw, const float* iscale,
                           const float* oscale, const float* obias, int64_t B, int64_t C, int64_t N, int64_t IH,
                           int64_t IW, int64_t OH, int64_t OW, float* scratch, hipStream_t st);
