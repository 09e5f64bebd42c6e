// The three device buffers of the rasterizer, each carved in ONE place.  A layout is a plain struct of named pointers
// built by one function from the call's extents; its size comes from the same struct.  The size entries of the C ABI
// (sr_rasterize_scratch_bytes, sr_rasterize_grad_scratch_bytes, sr_rasterize_grad_state_ints), every launcher and the
// level tables RasterLevels / GradLevels take their pointers from here, and so do the *_levels kernels, which carve a
// level's buffers on the device (the builders are __host__ __device__ and fold to the one member a kernel reads).
//
//   gradient state `big` (int32, allocated by the caller of the forward pass, read by the gradient pass)
//       [count | b * nf ids of the large triangles | b * nf leader table | state word]
//   gradient scratch (R = float / double)
//       [quad plane 12 * b * nf | tail planes, 3 * b * nf each | ... up to 24 * b * nf values | valid words |
//        inverse incidence table 3 * b * nf ints]
//       With SR_RASTER_GRAD_SLOTS=0 the same 24 * b * nf values are b * nf per-triangle records of 24.
//   forward scratch: the larger of
//       global-key path   [keys 8 B / pixel | tmin 4 B / pixel (fp64 only)]
//       LDS-tiled path    [tile counters b * ntile | wide counters b | tile lists b * ntile * TILE_CAP | wide lists b * nf]
#pragma once
#include "common.h"

#define SR_LAYOUT_HD __host__ __device__ __forceinline__

constexpr int TILE = 32;            // screen tile edge (pixels) of the LDS-tiled forward
constexpr int TILE_CAP = 2048;      // list entries per (sample, tile); overflow spills to the sample's wide list

// ---- gradient state ---------------------------------------------------------------------------------------------------
struct GradState {
    int* count;                     // number of large triangles the forward listed
    int* ids;                       // their flat ids sample * nf + triangle, any order
    int* leaders;                   // [b * nf] smallest row-major pixel a triangle won (0x7FFFFFFF: none)
    int* state;                     // 1: leader table built by the tiled forward; 0: filled only (k_first_pix builds it)
    static SR_LAYOUT_HD long long ints(long long b, long long nf) { return 2 + 2 * b * nf; }
};
// (the member the *_levels kernels derive on the device from a level's `big`)
SR_LAYOUT_HD int* grad_leaders(int* big, long long b, long long nf) { return big + 1 + b * nf; }
SR_LAYOUT_HD GradState grad_state(int* big, long long b, long long nf) {
    GradState g;
    g.count = big;
    g.ids = big + 1;
    g.leaders = grad_leaders(big, b, nf);
    g.state = g.leaders + b * nf;
    return g;
}

// ---- gradient scratch -------------------------------------------------------------------------------------------------
// values per (sample, triangle) for the widest chunk (<= 4 channels) and either projection: 3 * (3 + 4) rounded up to 4
constexpr int GRAD_ROW_VALUES = 24;
constexpr int GRAD_QUAD_VALUES = 12;        // three corners x one 16-byte (fp32) quad
static_assert(GRAD_ROW_VALUES * sizeof(float) % 8 == 0 && GRAD_ROW_VALUES * sizeof(double) % 8 == 0,
              "the valid words behind b * nf records stay 8-byte aligned");
static_assert(GRAD_QUAD_VALUES + 3 * 3 <= GRAD_ROW_VALUES, "quad plane + three tail planes fit the records' space");

template <typename R>
struct GradScratch {
    R* quad;                        // quad plane: the first four values of every corner slot (also: the records)
    R* tail;                        // tail planes: value 4 + j of slot e at tail[j * plane + e]
    long long plane;                // slots per plane
    unsigned long long* valid;      // one bit per (sample, triangle): it won a pixel, its values are written
    int* inverse;                   // inverse incidence table, built per call when the caller hands none over
    static SR_LAYOUT_HD long long valid_words(long long rows) { return (rows + 63) / 64 + 1; }
    static long long bytes(long long b, long long nf) {
        const long long rows = (b > 0 ? b : 0) * (nf > 0 ? nf : 0);
        return rows * GRAD_ROW_VALUES * (long long)sizeof(R) + valid_words(rows) * 8 + rows * 12 + 16;
    }
};
// (the two members the *_levels kernels derive on the device from a level's `quad`)
template <typename R>
SR_LAYOUT_HD R* grad_tail(R* quad, long long b, long long nf) { return quad + b * nf * GRAD_QUAD_VALUES; }
SR_LAYOUT_HD long long grad_plane(long long b, long long nf) { return b * 3 * nf; }
template <typename R>
SR_LAYOUT_HD GradScratch<R> grad_scratch(void* work, long long b, long long nf) {
    GradScratch<R> s;
    s.quad = reinterpret_cast<R*>(work);
    s.tail = grad_tail(s.quad, b, nf);
    s.plane = grad_plane(b, nf);
    s.valid = reinterpret_cast<unsigned long long*>(s.quad + b * nf * GRAD_ROW_VALUES);
    s.inverse = reinterpret_cast<int*>(s.valid + GradScratch<R>::valid_words(b * nf));
    return s;
}

// ---- forward scratch --------------------------------------------------------------------------------------------------
struct KeyScratch {
    unsigned long long* keys;       // [b * h * w] packed depth keys (fp64: orderable depths)
    unsigned* tmin;                 // [b * h * w] fp64 only: lowest id among the depth maxima
    static long long bytes(long long npix, bool is_double) { return npix * (is_double ? 12 : 8); }
};
SR_LAYOUT_HD KeyScratch key_scratch(void* work, long long npix) {
    KeyScratch s;
    s.keys = reinterpret_cast<unsigned long long*>(work);
    s.tmin = reinterpret_cast<unsigned*>(s.keys + npix);
    return s;
}

struct TileScratch {
    int ntx;                        // tiles per row (= per column: square images)
    long long ntile;
    long long counters;             // tile_cnt and wide_cnt are adjacent: one zero fill of this many words
    unsigned* tile_cnt;             // [b * ntile]
    unsigned* wide_cnt;             // [b]
    unsigned* tile_list;            // [b * ntile * TILE_CAP]
    unsigned* wide_list;            // [b * nf]
    static long long words(long long b, long long nf, long long hres) {
        const long long ntx = sr_ceil_div(hres, TILE), ntile = ntx * ntx;
        return b * ntile + b + b * ntile * TILE_CAP + b * nf;
    }
};
inline TileScratch tile_scratch(void* work, long long b, long long nf, long long hres) {
    TileScratch s;
    s.ntx = (int)sr_ceil_div(hres, TILE);
    s.ntile = (long long)s.ntx * s.ntx;
    s.counters = b * s.ntile + b;
    s.tile_cnt = reinterpret_cast<unsigned*>(work);
    s.wide_cnt = s.tile_cnt + b * s.ntile;
    s.tile_list = s.wide_cnt + b;
    s.wide_list = s.tile_list + b * s.ntile * TILE_CAP;
    (void)nf;                       // the wide lists are the last part: their length only enters words()
    return s;
}

// what sr_rasterize_scratch_bytes answers: room for either forward path
inline long long forward_scratch_bytes(long long b, long long nf, long long h, long long w, bool is_double) {
    b = b > 0 ? b : 0;
    nf = nf > 0 ? nf : 0;
    const long long npix = b * (h > 0 ? h : 0) * (w > 0 ? w : 0);
    long long bytes = KeyScratch::bytes(npix, is_double) + 16;
    if (!is_double && h == w && h > 0) {
        const long long tiled = TileScratch::words(b, nf, h) * 4 + 16;
        if (tiled > bytes) bytes = tiled;
    }
    return bytes;
}
