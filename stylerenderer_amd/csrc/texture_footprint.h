// The per-pixel arithmetic of the texture look-up (definition: stylerenderer_amd/op/texture.py, _footprint), shared by the
// sampler (texture_sample.hip) and the tap-list builder (tap_plan.hip) so that there is one copy: the texels a pixel's
// four taps fall on and its two fractions, every step one float32 operation in the definition's order.  Files that
// include this are compiled without contraction (-ffp-contract=off).
#pragma once
#include "common.h"

constexpr float TS_FLT_MAX = 3.4028234663852886e38f;

// what one pixel needs to blend its C planes
struct Foot {
    int o00, o01, o10, o11;      // offsets into one plane of the texture: (ya, xa), (ya, xb), (yb, xa), (yb, xb)
    float fx, fy;
    bool live, inx, iny;
};

__device__ __forceinline__ Foot footprint(float u, float v, bool cover, int Th, int Tw) {
    Foot f;
    f.o00 = f.o01 = f.o10 = f.o11 = 0;
    f.fx = f.fy = 0.f;
    f.inx = f.iny = false;
    f.live = cover && fabsf(u) <= TS_FLT_MAX && fabsf(v) <= TS_FLT_MAX;   // (a NaN compares false)
    if (!f.live) return f;
    const float tw = (float)Tw, th = (float)Th;
    const float sx = u * tw - 0.5f, sy = (1.f - v) * th - 0.5f;
    f.inx = sx >= -1.f && sx <= tw;
    f.iny = sy >= -1.f && sy <= th;
    const float sxc = fminf(fmaxf(sx, -1.f), tw), syc = fminf(fmaxf(sy, -1.f), th);
    const float x0f = floorf(sxc), y0f = floorf(syc);
    f.fx = sxc - x0f;
    f.fy = syc - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;                               // in [-1, Tw] x [-1, Th]
    const int xa = min(max(x0, 0), Tw - 1), xb = min(max(x0 + 1, 0), Tw - 1);
    const int ya = min(max(y0, 0), Th - 1), yb = min(max(y0 + 1, 0), Th - 1);
    f.o00 = ya * Tw + xa;
    f.o01 = ya * Tw + xb;
    f.o10 = yb * Tw + xa;
    f.o11 = yb * Tw + xb;
    return f;
}
