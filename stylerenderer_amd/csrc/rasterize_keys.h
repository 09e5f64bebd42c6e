// Global-key forward of the rasterizer (csrc/rasterize_keys.hip): what the host entries in rasterize.hip hand over.
#pragma once
#include "common.h"

// One forward call after validation and flag decode: the arguments of either forward path.
template <typename R>
struct RasterForward {
    long long b, nv, nf, h, w;
    bool repeat_v, repeat_f, perspective, chw;
    const R* v;
    const long long* tri;
    long long* index;
    R* coeff;
    R* zbuf;
    R eps;                                    // >= 0
    const R* tex;
    long long tex_c;
    R* attr;
    int* win;
    int* big;                                 // gradient state (raster_layout.h: GradState) or NULL
};

// ---- the same mesh at several resolutions in three launches (GeneratorWithMap: one normal map per synthesis
// resolution, reference model.py:255-262 — seven calls of three launches each at 256^2, every one ~5 us at the training
// and inversion batch sizes).  blockIdx.y selects the level; its extents and buffers come from a table passed by value.
// The bodies are the single-level kernels' (same expressions, same order: same bits).
struct RasterLevels {
    int n;
    int res_h[SR_RASTER_MAX_LEVELS], res_w[SR_RASTER_MAX_LEVELS];
    unsigned long long* keys[SR_RASTER_MAX_LEVELS];
    int* big[SR_RASTER_MAX_LEVELS];              // gradient state of the level (or NULL)
    int* win[SR_RASTER_MAX_LEVELS];
    float* attr[SR_RASTER_MAX_LEVELS];
};

// fill, depth keys (fp64: depth maxima, then ids), resolve; `work` >= KeyScratch::bytes
template <typename R>
int raster_keys_launch(const RasterForward<R>& c, void* work, hipStream_t st);
// the same three passes for every level of `t` at once (fp32; c.h / c.w / outputs / state come from the table);
// max_pix = the largest b * h * w of the levels
int raster_keys_levels_launch(const RasterLevels& t, const RasterForward<float>& c, long long max_pix, hipStream_t st);
