// Internal interface of the four-phases-in-one-workgroup kernel for the interior of the stride-2 transposed 3x3
// convolution (csrc/convt_fused.hip), used by sr_conv2d_mfma_ex (csrc/conv_dispatch.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_params.h"

// whole 32 x 4 patches, C % 8 == 0, C <= 2048, 16-byte aligned input, byte offsets below 2^31
bool sr_convt_fused_eligible(int64_t C, int64_t IH, int64_t IW, int64_t ldw, const void* in);
// workgroups of the launch without K slices (partial patches not counted: the plan asks before it asks `eligible`)
int64_t sr_convt_fused_blocks(int64_t B, int64_t N, int64_t IH, int64_t IW);
// K slices for a launch of `fused_blocks` workgroups: the smallest of 2 / 4 that gives >= 192 workgroups with whole
// chunks and >= 64 channels per slice, else 1 (also when the map is not whole patches)
int sr_convt_fused_slices(int64_t fused_blocks, int64_t C, int64_t IH, int64_t IW);
// p: the call's buffers and extents, wmap = identity; ks > 1: the K slices the plan chose (sr_convt_fused_slices), raw
// sums to p.partial and k_convt_fused_reduce behind the kernel
int sr_convt_fused_launch(ConvParams p, int ks, hipStream_t st);
