// fp32 forward with LDS-staged triangle tiles (square images): csrc/rasterize_tiled.hip.
// The global-key path (rasterize_keys.hip) pays 8 B/pixel of key buffer (fill, atomics in L2, re-read) and walks
// bounding boxes one lane per triangle (lanes of a wave wait for the largest box).  The tiled path:
//   k_tile_bin     one lane per (sample, triangle): the SAME load + setup; accepted small triangles (box <= BIG_BOX
//                  pixels, hence <= 4 tiles) are appended to the list of every 32x32 screen tile their box touches
//                  (wave-aggregated counter atomics); large boxes, and entries beyond a tile's capacity, go to the
//                  sample's `wide` list that every tile of the sample scans;
//   k_tile_raster  one workgroup per (sample, tile): the depth keys of the tile live in LDS (8 KB, ds_max_u64).  List
//                  entries are set up 256 at a time into LDS records; the (triangle, pixel-of-clipped-box) pairs are
//                  enumerated by a block prefix sum so that EVERY lane shades one pixel per step whatever the box
//                  sizes are; then the tile is resolved from LDS and each output is written once.
// Same `tri_setup` / `shade` device functions, same packed key (max z, ties -> lowest id): same bits as the global
// path and the CPU loops.  No key buffer, no fill pass, no second kernel for the resolve.
// TILE and TILE_CAP shape the scratch and live with it in raster_layout.h.
#pragma once
#include "raster_layout.h"
#include "raster_math.h"
#include "rasterize_keys.h"

constexpr int REC_F = 13;           // floats per LDS triangle record: z0 z1 z2, e0..e8, area (+ 4 integer fields)
constexpr int BIN_LDS_TILES = 1024; // images of up to this many tiles bin through LDS counters (k_tile_bin_lds)

namespace {

// Device-only short forms of `tri_setup`, also taken by the gradient pass (k_grad_pix) on square images.
// The per-triangle work of these kernels is vector-ALU bound (k_depth_keys: ~1 100 VALU instructions, 80 us for 3.2 M
// lanes), so the tiled kernels use slimmer device-only forms of `tri_setup` — the SAME floating-point expressions in
// the same order (same bits), without what costs instructions and changes no result:
//   * float -> int64 conversion with x86 semantics is ~20 instructions of emulation, four times per triangle; the
//     bounding box only ever meets [0, res - 1], where a SATURATED 32-bit conversion compares identically (NaN and
//     values >= 2^63 behave as "very negative", like cvttss2si's INT64_MIN);
//   * the projection mode is a template parameter (no division code in the orthographic kernels);
//   * indices are 32-bit, the sample comes from blockIdx.y;
//   * the resolve step needs the edge constants only: no bounding box, no rejection tests.
__device__ __forceinline__ int sat_i32_x86(float f) {
    const int i = (int)f;                                   // v_cvt_i32_f32: saturates, NaN -> 0
    return (f >= 9223372036854775808.0f || f != f) ? (int)0x80000000 : i;
}

template <bool PERSP>
__device__ __forceinline__ bool screen3(Tri<float>& t, float fres, float eps) {
    if (!to_screen<float>(t.p0, t.p1, t.p2, fres, fres, PERSP, eps)) return false;
    if (!to_screen<float>(t.p3, t.p4, t.p5, fres, fres, PERSP, eps)) return false;
    return to_screen<float>(t.p6, t.p7, t.p8, fres, fres, PERSP, eps);
}

__device__ __forceinline__ bool bounds_i32(Tri<float>& t, int res) {
    float lo_u = t.p0, hi_u = t.p0, lo_v = t.p1, hi_v = t.p1;
    grow<float>(lo_u, hi_u, t.p3);
    grow<float>(lo_v, hi_v, t.p4);
    grow<float>(lo_u, hi_u, t.p6);
    grow<float>(lo_v, hi_v, t.p7);
    int x0 = sat_i32_x86(ceilf(lo_u)), x1 = sat_i32_x86(floorf(hi_u));
    int y0 = sat_i32_x86(ceilf(lo_v)), y1 = sat_i32_x86(floorf(hi_v));
    x0 = x0 < 0 ? 0 : x0;
    x1 = x1 > res - 1 ? res - 1 : x1;
    y0 = y0 < 0 ? 0 : y0;
    y1 = y1 > res - 1 ? res - 1 : y1;
    t.x0 = x0; t.x1 = x1; t.y0 = y0; t.y1 = y1;
    return x1 >= x0 && y1 >= y0;
}

// e0..e2 and the signed area sum (tri_setup's `det`)
__device__ __forceinline__ float edge_origin(Tri<float>& t) {
    float m0 = t.p3 * t.p7, m1 = t.p4 * t.p6;
    t.e0 = m0 - m1;
    m0 = t.p1 * t.p6; m1 = t.p0 * t.p7;
    t.e1 = m0 - m1;
    m0 = t.p0 * t.p4; m1 = t.p1 * t.p3;
    t.e2 = m0 - m1;
    float det = t.e0 + t.e1;
    det = det + t.e2;
    return det;
}

__device__ __forceinline__ void edge_slopes(Tri<float>& t, float det) {
    t.e3 = t.p4 - t.p7;
    t.e4 = t.p7 - t.p1;
    t.e5 = t.p1 - t.p4;
    t.e6 = t.p6 - t.p3;
    t.e7 = t.p0 - t.p6;
    t.e8 = t.p3 - t.p0;
    if (det < 0) {
        t.e0 = -t.e0; t.e1 = -t.e1; t.e2 = -t.e2;
        t.e3 = -t.e3; t.e4 = -t.e4; t.e5 = -t.e5;
        t.e6 = -t.e6; t.e7 = -t.e7; t.e8 = -t.e8;
        t.area = -det;
    } else {
        t.area = det;
    }
}

// accept / reject + bounding box (what the binning needs); on a square image of `res` pixels
template <bool PERSP>
__device__ __forceinline__ bool tri_bounds_fast(Tri<float>& t, int res, float eps) {
    if (!screen3<PERSP>(t, (float)res, eps)) return false;
    if (!bounds_i32(t, res)) return false;
    return !(edge_origin(t) > eps);
}

// the whole of tri_setup for a triangle that is known to be accepted
template <bool PERSP>
__device__ __forceinline__ void tri_setup_accepted(Tri<float>& t, int res, float eps, bool want_box) {
    screen3<PERSP>(t, (float)res, eps);
    if (want_box) bounds_i32(t, res);
    edge_slopes(t, edge_origin(t));
}

__device__ __forceinline__ bool load_tri32(Tri<float>& t, const float* __restrict__ vs,
                                           const long long* __restrict__ fs, unsigned ti, unsigned nv,
                                           unsigned& i0, unsigned& i1, unsigned& i2) {
    const long long a = fs[3 * (size_t)ti], bq = fs[3 * (size_t)ti + 1], c = fs[3 * (size_t)ti + 2];
    if ((unsigned long long)a >= nv || (unsigned long long)bq >= nv || (unsigned long long)c >= nv) return false;
    i0 = (unsigned)a; i1 = (unsigned)bq; i2 = (unsigned)c;
    load3<float>(vs + 3 * (size_t)i0, t.p0, t.p1, t.p2);
    load3<float>(vs + 3 * (size_t)i1, t.p3, t.p4, t.p5);
    load3<float>(vs + 3 * (size_t)i2, t.p6, t.p7, t.p8);
    return true;
}

}  // namespace

// The tiled path serves fp32 on square images (x and y ranges are swapped by the reference's call sites, SURVEY D8:
// on a non-square image pixel columns beyond the width alias into the next row, which only a global key buffer
// reproduces).  It pays when there are thousands of (sample, tile) workgroups with a few hundred triangles each —
// BASELINE config[3]: 64 samples x 64 tiles, ~400 accepted triangles per tile: 0.116 vs 0.129 ms.  With few tiles (low
// resolution under the same mesh: sub-pixel triangles that the global path rejects in a handful of instructions) or
// few samples (training: 4, inversion: 1) each workgroup walks a long list serially and the global-key path wins by
// 2-5x (scripts/raster_res_probe.py), so the choice is made per call.  SR_RASTER_TILED=1 forces the tiled path (tests),
// =0 the global-key path.  fp32 only: fp64 never asks.
bool raster_tiled_ok(long long b, long long nf, long long h, long long w);
// zero + bin + raster; c.h == c.w; `work` >= TileScratch::words * 4 bytes
int raster_tiled_launch(const RasterForward<float>& c, void* work, hipStream_t st);
