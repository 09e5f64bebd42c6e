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

// Style gradient from the per-sample slabs (wgrad_style_finish.h).  Whole K slices per sample of the plan — the chunks of
// a sample are a multiple of the plan's chunks per slice — or 0: a slice straddles two samples (or B > 32).
int sr_wgrad_wino_slices_per_sample(int64_t B, int64_t C, int64_t N, int64_t H, int64_t W);
// eligible shapes with sr_wgrad_wino_slices_per_sample > 0 only: dwt as sr_wgrad_wino_launch(xscale = iscale) and
// gis[b][c] = sum_{t,n} wt[t][c][n] * (weight gradient of sample b without the style).  wt [9][C][ldw] is the forward
// weight, `part` sr_wgrad_style_part_floats(B, C, N, false) floats, `scratch` as for sr_wgrad_wino_launch.
int sr_wgrad_wino_style_launch(float* dwt, float* gis, const float* x, const float* gy, const float* iscale,
                               const float* gscale, const float* wt, int64_t ldw, int64_t B, int64_t C, int64_t N, int64_t H,
                               int64_t W, float* scratch, float* part, hipStream_t st);
