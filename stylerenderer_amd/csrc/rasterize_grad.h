// Backward of the rasterizer (csrc/rasterize_grad.hip): k_dcoeff (API parity with rasterize_gpu_backward) and the fused
// gradient of the autograd Function, a deterministic two-phase gather.
#pragma once
#include "common.h"

// One gradient call after validation and flag decode.
template <typename R>
struct RasterGrad {
    long long b, nv, nf, h, w;
    bool repeat_f, perspective, chw, accumulate;
    const R* v;
    const R* tex;
    long long tex_c;
    const long long* tri;
    const int* win;
    const int* big;                           // gradient state the forward left (raster_layout.h: GradState)
    const R* grad_out;
    const int* adj_off;
    const int* adj;
    long long off_bs, adj_bs;
    const int* adj_slot;                      // cached inverse incidence table or NULL
    R* grad_v;
    R* grad_tex;
    R eps;                                    // >= 0
};

// ---- gradient of a pyramid (the same mesh at several resolutions, RasterLevels above) in four launches ------------------
// blockIdx.y (k_first_pix / k_grad_big / k_grad_pix) = level; k_grad_vert_levels sums the levels' per-vertex sums in table
// order — the value SR_RASTER_GRAD_ACC calls in that order produce, bit for bit (each level's sum is formed on its own,
// then added to the running total).  fp32, <= 4 attribute channels, vertex-major slots from the caller's inverse table.
struct GradLevels {
    int n;
    int res_h[SR_RASTER_MAX_LEVELS], res_w[SR_RASTER_MAX_LEVELS];
    const int* win[SR_RASTER_MAX_LEVELS];
    int* big[SR_RASTER_MAX_LEVELS];               // gradient state of the level (GradState)
    const float* grad_out[SR_RASTER_MAX_LEVELS];
    float* tg[SR_RASTER_MAX_LEVELS];                 // per-level scratch: corner slots (quad plane | tail planes) ...
    unsigned long long* valid[SR_RASTER_MAX_LEVELS]; // ... and the valid words behind them
};

template <typename R>
int raster_dcoeff_launch(long long b, long long n, long long h, long long w, bool perspective, const R* v,
                         const long long* index, R* dcoeff, R eps, hipStream_t st);
// `work` >= GradScratch<R>::bytes
template <typename R>
int raster_grad_launch(const RasterGrad<R>& c, void* work, hipStream_t st);
// c.h / c.w / win / big / grad_out come from the table; c.adj_slot != NULL, c.tex_c <= 4; max_pix as in the forward
int raster_grad_levels_launch(const GradLevels& t, const RasterGrad<float>& c, long long max_pix, hipStream_t st);
