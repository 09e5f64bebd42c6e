// The mip-mapped texture look-up of face reconstruction (C ABI: sr_mip_build_fwd / sr_mip_build_bwd / sr_mip_lod /
// sr_mip_sample_fwd / sr_mip_sample_bwd_uv / sr_mip_sample_bwd_pyr; definition: stylerenderer_amd/op/texture.py,
// mip_build_composite, mip_lod_composite, mip_sample_composite).  A (Th, Tw) texture has L levels: level 0 is the
// texture, level l + 1 has half of each side and exists while both sides of level l are even, so a level's sides are
// (Th >> l, Tw >> l) and its texel grid is nested exactly in the one below.  The pyramid is packed [Bt, C, P] with level l
// at offset_l = sum_{j < l} h_j w_j = (Th Tw - h_l w_l) 4 / 3 of a plane.
//
//   k_mip_build_fwd        a workgroup owns a 32 x 32 tile of a source level of one plane and reduces it through LDS by up
//                          to five levels, each written from the float32 values of the one below as
//                          ((a + b) + (c + d)) 0.25, partial tiles masked by the level's sides.  The host loops it with the
//                          last written level as the next source (512^2: two launches); the first launch also writes level
//                          0, a copy of tex.  Every element of pyr is written.
//   k_mip_build_bwd        a lane owns one level-0 texel for up to four channels per walk; it walks its L ancestors from the
//                          top down (t = g_l + 0.25 t) and writes grad_tex: a gather, one order, no scatter.
//   k_mip_lod              texture_sample.hip's staging: a lane owns four consecutive pixels of a row; it reads their
//                          neighbours in the row and in the rows above and below, takes per axis the smaller squared texel
//                          distance to a live neighbour, the larger of the two axes, one correctly rounded sqrtf and a
//                          comparison against the exact powers of two (no log2: not reproducible between host and device).
//   k_mip_sample_fwd       the same staging; the lane derives both levels' footprints once and walks the C planes; a pixel
//                          whose lod is whole loads four texels, not eight.
//   k_mip_sample_bwd_uv    the same staging; the channel sums run in channel order per level and are then blended.
//   k_mip_sample_bwd_pyr   a lane owns one element of the packed pyramid, at any level, for up to four channels per walk; it
//                          walks the element's list (op.texture.mip_tap_plan: entries ((b H + y) W + x) 8 + k, ascending)
//                          in order, recomputing level, fraction and weight from uv and lod; the loads of eight entries
//                          are issued together, the terms still added one by one.  Every element is written, taps or
//                          not.  Offsets and entries outside the list or the picture are skipped, never followed.
//
// The arithmetic is the definition's, one float32 operation per step in the same order (-ffp-contract=off, correctly
// rounded division and square root).  Vector stores and plain C++ only: no atomics, no scratch buffer, no memset, no host
// read, so all six run under graph capture on the caller's stream; reruns are bit-identical.
#include "common.h"

namespace {

constexpr int MIP_BLOCK = 256;
constexpr int MIP_CH = 4;                                                 // channels a lane carries per walk
constexpr int MIP_AHEAD = 8;                                              // list entries whose loads are issued together
constexpr int MIP_MAX_L = 21;                                             // sides up to 2^20
constexpr int MIP_TILE = 32;
constexpr int MIP_STEP = 5;                                               // levels one build launch goes down
constexpr float MIP_FLT_MAX = 3.4028234663852886e38f;

// the number of levels the rule gives a (Th, Tw) texture
int mip_levels(int64_t Th, int64_t Tw) {
    int n = 1;
    while (Th % 2 == 0 && Tw % 2 == 0 && n < MIP_MAX_L) Th /= 2, Tw /= 2, ++n;
    return n;
}

__host__ __device__ __forceinline__ int64_t mip_offset(int64_t Th, int64_t Tw, int l) {
    return (Th * Tw - (Th >> l) * (Tw >> l)) / 3 * 4;
}

int64_t mip_total(int64_t Th, int64_t Tw, int L) { return mip_offset(Th, Tw, L - 1) + (Th >> (L - 1)) * (Tw >> (L - 1)); }

// ---- the pyramid ------------------------------------------------------------------------------------------------------
struct BuildArgs {
    float* pyr;              // [N, P]
    const float* src;        // the planes of the source level: tex [N, Th Tw] (s == 0) or pyr + offset_s
    int64_t src_stride;      // Th Tw or P
    int64_t P;
    int64_t N;               // planes, Bt C
    int Th, Tw;              // level 0
    int s;                   // the source level
    int down;                // the levels written from it: s + 1 .. s + down (0 .. 5)
    int tiles_x, tiles_y;
};

__global__ __launch_bounds__(MIP_BLOCK) void k_mip_build_fwd(BuildArgs a) {
    __shared__ float lds_a[MIP_TILE * MIP_TILE];                            // the source tile, then every second level
    __shared__ float lds_b[MIP_TILE * MIP_TILE / 4];                        // the levels between
    const int64_t tiles = (int64_t)a.tiles_x * a.tiles_y;
    const int64_t plane = blockIdx.x / tiles;
    const int tile = (int)(blockIdx.x % tiles);
    if (plane >= a.N) return;
    const int ty = tile / a.tiles_x, tx = tile % a.tiles_x;
    const int hs = a.Th >> a.s, ws = a.Tw >> a.s;
    const float* src = a.src + plane * a.src_stride;
    float* dst = a.pyr + plane * a.P;
    float* cur = lds_a;
    // the source tile; outside the level: 0, never read by an element that is written
    for (int i = threadIdx.x; i < MIP_TILE * MIP_TILE; i += MIP_BLOCK) {
        const int ly = i / MIP_TILE, lx = i % MIP_TILE;
        const int gy = ty * MIP_TILE + ly, gx = tx * MIP_TILE + lx;
        float val = 0.f;
        if (gy < hs && gx < ws) {
            val = src[(int64_t)gy * ws + gx];
            if (a.s == 0) dst[(int64_t)gy * ws + gx] = val;                   // level 0: the copy
        }
        cur[i] = val;
    }
    __syncthreads();
    float* nxt = lds_b;
    int side = MIP_TILE;                                                    // the tile's side at the level held in cur
    for (int j = 1; j <= a.down; ++j) {
        const int half = side >> 1;
        const int l = a.s + j;
        const int hl = a.Th >> l, wl = a.Tw >> l;
        const int64_t off = mip_offset(a.Th, a.Tw, l);
        for (int i = threadIdx.x; i < half * half; i += MIP_BLOCK) {
            const int ly = i / half, lx = i % half;
            const float* p = cur + (2 * ly) * side + 2 * lx;
            const float val = ((p[0] + p[1]) + (p[side] + p[side + 1])) * 0.25f;
            nxt[i] = val;
            const int gy = ty * half + ly, gx = tx * half + lx;
            if (gy < hl && gx < wl) dst[off + (int64_t)gy * wl + gx] = val;
        }
        __syncthreads();
        float* t = cur;
        cur = nxt, nxt = t;
        side = half;
    }
}

struct BuildBwdArgs {
    float* gtex;             // [Bt, C, Th, Tw]
    const float* gpyr;       // [Bt, C, P]
    int64_t P;
    int64_t n;               // Bt Th Tw
    int C, Th, Tw, L;
};

__global__ __launch_bounds__(MIP_BLOCK) void k_mip_build_bwd(BuildBwdArgs a) {
    const int64_t item = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;    // bt Th Tw + texel
    if (item >= a.n) return;
    const int64_t tplane = (int64_t)a.Th * a.Tw;
    const int64_t bt = item / tplane, texel = item % tplane;
    const int y = (int)(texel / a.Tw), x = (int)(texel % a.Tw);
    for (int c0 = 0; c0 < a.C; c0 += MIP_CH) {
        const int nc = min(MIP_CH, a.C - c0);
        const float* g = a.gpyr + (bt * a.C + c0) * a.P;
        float t[MIP_CH];
#pragma unroll
        for (int cc = 0; cc < MIP_CH; ++cc) t[cc] = 0.f;
        for (int l = a.L - 1; l >= 0; --l) {
            const int wl = a.Tw >> l;
            const int64_t at = mip_offset(a.Th, a.Tw, l) + (int64_t)(y >> l) * wl + (x >> l);
#pragma unroll
            for (int cc = 0; cc < MIP_CH; ++cc)
                if (cc < nc) {
                    const float gl = g[cc * a.P + at];
                    t[cc] = l == a.L - 1 ? gl : gl + 0.25f * t[cc];
                }
        }
#pragma unroll
        for (int cc = 0; cc < MIP_CH; ++cc)
            if (cc < nc) a.gtex[(bt * a.C + c0 + cc) * tplane + texel] = t[cc];
    }
}

// ---- the look-up's per-pixel quantities -------------------------------------------------------------------------------
struct MipArgs {
    const float* pyr;        // [Bt, C, P]
    const float* uv;         // [B, H, W, 2]
    const uint8_t* cover;    // [B, H, W]
    const float* lod;        // [B, H, W]
    int64_t pyr_bstride;     // C P, or 0 for a shared pyramid
    int64_t P;
    int B, C, H, W, Th, Tw, L;
};

// texture_sample.hip's footprint, on one level: offsets into that level's block of a plane
struct Foot {
    int o00, o01, o10, o11;
    float fx, fy;
    bool inx, iny;
};

__device__ __forceinline__ bool is_live(float u, float v, bool cover) {
    return cover && fabsf(u) <= MIP_FLT_MAX && fabsf(v) <= MIP_FLT_MAX;     // (a NaN compares false)
}

__device__ __forceinline__ Foot footprint(float u, float v, int Th, int Tw) {
    Foot f;
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

// lod clamped to [0, L - 1] (a NaN counts as 0) -> (l0, f)
__device__ __forceinline__ void split_lod(float lod, int L, int& l0, float& f) {
    const float lc = lod >= 0.f ? fminf(lod, (float)(L - 1)) : 0.f;
    const float l0f = floorf(lc);
    f = lc - l0f;
    l0 = (int)l0f;
}

// what one pixel needs to blend its C planes: the two levels' footprints, the offsets made absolute in a plane
struct MipFoot {
    Foot a, b;               // level l0 and level l1 (b is valid only where two)
    float f;
    int l0;
    bool live, two;          // two: f != 0, level l1 takes part
};

__device__ __forceinline__ void shift(Foot& f, int off) { f.o00 += off, f.o01 += off, f.o10 += off, f.o11 += off; }

__device__ __forceinline__ MipFoot mip_footprint(float u, float v, bool cover, float lod, int Th, int Tw, int L) {
    MipFoot m;
    m.live = is_live(u, v, cover);
    m.two = false;
    m.f = 0.f;
    m.l0 = 0;
    m.a.o00 = m.a.o01 = m.a.o10 = m.a.o11 = 0;
    m.a.fx = m.a.fy = 0.f;
    m.a.inx = m.a.iny = false;
    m.b = m.a;
    if (!m.live) return m;
    split_lod(lod, L, m.l0, m.f);
    const int l0 = m.l0;
    m.a = footprint(u, v, Th >> l0, Tw >> l0);
    shift(m.a, (int)mip_offset(Th, Tw, l0));
    m.two = m.f != 0.f;                                                   // (then l0 < L - 1: lod <= L - 1 is not whole)
    if (m.two) {
        const int l1 = min(l0 + 1, L - 1);
        m.b = footprint(u, v, Th >> l1, Tw >> l1);
        shift(m.b, (int)mip_offset(Th, Tw, l1));
    }
    return m;
}

template <int V>
__device__ __forceinline__ void store4(float* p, const float* x, int count) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < count) p[j] = x[j];
    }
}

template <int V>
__device__ __forceinline__ void load4(float* x, const float* p, int count) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = j < count ? p[j] : 0.f;
    }
}

// the lane's four pixels: (b, y, x0 .. x0 + count - 1); false past the end
__device__ __forceinline__ bool lane_row(int B, int H, int W, int& b, int& y, int& x0, int& count) {
    const int groups = (W + 3) >> 2;                                      // lanes per row
    const int64_t item = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;
    if (item >= (int64_t)B * H * groups) return false;
    x0 = (int)(item % groups) * 4;
    const int64_t row = item / groups;
    y = (int)(row % H);
    b = (int)(row / H);
    count = min(4, W - x0);
    return true;
}

__device__ __forceinline__ bool lane_pixels(const MipArgs& a, int& b, int& y, int& x0, int& count, MipFoot* f) {
    if (!lane_row(a.B, a.H, a.W, b, y, x0, count)) return false;
    const int64_t p0 = ((int64_t)b * a.H + y) * a.W + x0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < count)
            f[j] = mip_footprint(a.uv[2 * (p0 + j)], a.uv[2 * (p0 + j) + 1], a.cover[p0 + j] != 0, a.lod[p0 + j], a.Th, a.Tw,
                                 a.L);
        else
            f[j] = mip_footprint(0.f, 0.f, false, 0.f, a.Th, a.Tw, a.L);
    }
    return true;
}

// ---- the level of detail ----------------------------------------------------------------------------------------------
struct LodArgs {
    float* lod;              // [B, H, W]
    const float* uv;         // [B, H, W, 2]
    const uint8_t* cover;    // [B, H, W]
    int B, H, W, Th, Tw, L;
    float bias;
};

struct Px {
    float u, v;
    bool live;
};

__device__ __forceinline__ Px pixel(const LodArgs& a, int b, int y, int x) {
    Px p;
    p.u = p.v = 0.f;
    p.live = false;
    if (y < 0 || y >= a.H || x < 0 || x >= a.W) return p;                 // outside the picture: not usable
    const int64_t at = ((int64_t)b * a.H + y) * a.W + x;
    p.u = a.uv[2 * at];
    p.v = a.uv[2 * at + 1];
    p.live = is_live(p.u, p.v, a.cover[at] != 0);
    return p;
}

// the smaller squared texel distance from c to its usable neighbours p and n; 0 with none.  A difference of two finite
// numbers is finite or an infinity and a square is not negative, so d is never NaN; an overflow gives inf: the top level
__device__ __forceinline__ float axis_q(const Px& c, const Px& p, const Px& n, float th, float tw) {
    float q = 0.f;
    bool any = false;
    if (n.live) {
        const float du = (n.u - c.u) * tw, dv = (n.v - c.v) * th;
        q = du * du + dv * dv;
        any = true;
    }
    if (p.live) {
        const float du = (p.u - c.u) * tw, dv = (p.v - c.v) * th;
        const float d = du * du + dv * dv;
        q = any ? fminf(q, d) : d;
    }
    return q;
}

template <int V>
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_lod(LodArgs a) {
    int b, y, x0, count;
    if (!lane_row(a.B, a.H, a.W, b, y, x0, count)) return;
    const float th = (float)a.Th, tw = (float)a.Tw;
    Px row[6];                                                            // x0 - 1 .. x0 + 4
#pragma unroll
    for (int j = 0; j < 6; ++j) row[j] = pixel(a, b, y, x0 - 1 + j);
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        out[j] = 0.f;
        const Px c = row[j + 1];
        if (j >= count || !c.live) continue;
        const float qx = axis_q(c, row[j], row[j + 2], th, tw);
        const float qy = axis_q(c, pixel(a, b, y - 1, x0 + j), pixel(a, b, y + 1, x0 + j), th, tw);
        const float rho = sqrtf(fmaxf(qx, qy));
        float lam = 0.f;
        if (rho >= 1.f) {
            int l = 0;
            float pw = 2.f, inv = 1.f;                                    // 2^(l + 1) and 2^-l, exact
            while (l < a.L - 1 && rho >= pw) ++l, pw = pw * 2.f, inv = inv * 0.5f;
            lam = l == a.L - 1 ? (float)(a.L - 1) : (float)l + (rho * inv - 1.f);
        }
        out[j] = fminf(fmaxf(lam + a.bias, 0.f), (float)(a.L - 1));
    }
    store4<V>(a.lod + ((int64_t)b * a.H + y) * a.W + x0, out, count);
}

// ---- the look-up ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float blend(const float* t, const Foot& f) {
    const float top = (1.f - f.fx) * t[f.o00] + f.fx * t[f.o01];
    const float bot = (1.f - f.fx) * t[f.o10] + f.fx * t[f.o11];
    return top * (1.f - f.fy) + bot * f.fy;
}

template <int V>
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_sample_fwd(MipArgs a, float* __restrict__ out, float background) {
    int b, y, x0, count;
    MipFoot f[4];
    if (!lane_pixels(a, b, y, x0, count, f)) return;
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t at = (int64_t)y * a.W + x0;
    for (int c = 0; c < a.C; ++c) {
        const float* t = a.pyr + (int64_t)b * a.pyr_bstride + c * a.P;
        float col[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            col[j] = background;
            if (f[j].live) {
                const float c0 = blend(t, f[j].a);
                col[j] = c0;
                if (f[j].two) col[j] = (1.f - f[j].f) * c0 + f[j].f * blend(t, f[j].b);
            }
        }
        store4<V>(out + ((int64_t)b * a.C + c) * plane + at, col, count);
    }
}

// one channel's term of the two partial derivatives on one level
__device__ __forceinline__ void slopes(const float* t, const Foot& f, float g, float& gx, float& gy) {
    const float t00 = t[f.o00], t01 = t[f.o01], t10 = t[f.o10], t11 = t[f.o11];
    const float top = (1.f - f.fx) * t00 + f.fx * t01;
    const float bot = (1.f - f.fx) * t10 + f.fx * t11;
    gx = gx + g * ((t01 - t00) * (1.f - f.fy) + (t11 - t10) * f.fy);
    gy = gy + g * (bot - top);
}

template <int V>
__global__ __launch_bounds__(MIP_BLOCK) void k_mip_sample_bwd_uv(MipArgs a, float* __restrict__ guv,
                                                               const float* __restrict__ gout) {
    int b, y, x0, count;
    MipFoot f[4];
    if (!lane_pixels(a, b, y, x0, count, f)) return;
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t at = (int64_t)y * a.W + x0;
    float gxa[4], gya[4], gxb[4], gyb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gxa[j] = gya[j] = gxb[j] = gyb[j] = 0.f;
    for (int c = 0; c < a.C; ++c) {
        const float* t = a.pyr + (int64_t)b * a.pyr_bstride + c * a.P;
        float g[4];
        load4<V>(g, gout + ((int64_t)b * a.C + c) * plane + at, count);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (f[j].live) {
                slopes(t, f[j].a, g[j], gxa[j], gya[j]);
                if (f[j].two) slopes(t, f[j].b, g[j], gxb[j], gyb[j]);
            }
        }
    }
    float o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[2 * j] = o[2 * j + 1] = 0.f;
        if (!f[j].live) continue;
        const int l0 = f[j].l0;
        const float fr = f[j].f;
        const float twa = (float)(a.Tw >> l0), tha = (float)(a.Th >> l0);
        const float ua = f[j].a.inx ? gxa[j] * twa : 0.f;
        const float va = f[j].a.iny ? -(gya[j] * tha) : 0.f;
        o[2 * j] = ua, o[2 * j + 1] = va;
        if (f[j].two) {
            const int l1 = min(l0 + 1, a.L - 1);
            const float twb = (float)(a.Tw >> l1), thb = (float)(a.Th >> l1);
            const float ub = f[j].b.inx ? gxb[j] * twb : 0.f;
            const float vb = f[j].b.iny ? -(gyb[j] * thb) : 0.f;
            o[2 * j] = (1.f - fr) * ua + fr * ub;
            o[2 * j + 1] = (1.f - fr) * va + fr * vb;
        }
    }
    float* p = guv + 2 * (((int64_t)b * a.H + y) * a.W + x0);
    store4<V>(p, o, 2 * count);
    store4<V>(p + 4, o + 4, 2 * count - 4);
}

struct TapArgs {
    float* gpyr;             // [Bt, C, P]
    const float* gout;       // [B, C, H, W]
    const float* uv;         // [B, H, W, 2]
    const uint8_t* cover;    // [B, H, W]
    const float* lod;        // [B, H, W]
    const int32_t* off;      // [keys + 2]: the CSR's offsets (the last bucket holds the entries without a tap)
    const int32_t* entries;  // [8 B H W]
    int64_t keys;            // Bt P
    int64_t n_entries;       // 8 B H W
    int64_t P;
    int C, H, W, Th, Tw, L;
};

__global__ __launch_bounds__(MIP_BLOCK) void k_mip_sample_bwd_pyr(TapArgs a) {
    const int64_t key = (int64_t)blockIdx.x * MIP_BLOCK + threadIdx.x;     // bt P + element
    if (key >= a.keys) return;
    const int64_t plane = (int64_t)a.H * a.W;
    const int64_t bt = key / a.P, elem = key % a.P;
    // a list that is not this call's (stale, or of another size) must not lead outside the tensors
    int64_t lo = a.off[key], hi = a.off[key + 1];
    lo = lo < 0 ? 0 : (lo > a.n_entries ? a.n_entries : lo);
    hi = hi < lo ? lo : (hi > a.n_entries ? a.n_entries : hi);
    for (int c0 = 0; c0 < a.C; c0 += MIP_CH) {
        const int nc = min(MIP_CH, a.C - c0);
        float acc[MIP_CH];
#pragma unroll
        for (int cc = 0; cc < MIP_CH; ++cc) acc[cc] = 0.f;
        // MIP_AHEAD entries at a time: their loads (the entry, then the pixel's uv, cover, lod and gradient) are issued
        // together, since a walk is a chain of dependent loads and the coarse levels' lists are long; the terms are
        // still added one by one in list order
        for (int64_t e = lo; e < hi; e += MIP_AHEAD) {
            int64_t ent[MIP_AHEAD];
#pragma unroll
            for (int j = 0; j < MIP_AHEAD; ++j) {
                ent[j] = e + j < hi ? (int64_t)a.entries[e + j] : -1;
                if (ent[j] >= a.n_entries) ent[j] = -1;
            }
            // (an entry that is skipped reads pixel 0 instead: every load below is unconditional and in bounds, so
            // nothing keeps the compiler from issuing them side by side)
            float pu[MIP_AHEAD], pv[MIP_AHEAD], pl[MIP_AHEAD], gv[MIP_AHEAD][MIP_CH];
            uint8_t pc[MIP_AHEAD];
#pragma unroll
            for (int j = 0; j < MIP_AHEAD; ++j) {
                const uint32_t pix = ent[j] < 0 ? 0u : (uint32_t)(ent[j] >> 3);        // below B H W < 2^28
                pu[j] = a.uv[2 * (int64_t)pix], pv[j] = a.uv[2 * (int64_t)pix + 1];
                pc[j] = a.cover[pix];
                pl[j] = a.lod[pix];
                const uint32_t b = pix / (uint32_t)plane, rem = pix - b * (uint32_t)plane;   // (a 32-bit division)
                const float* g = a.gout + ((int64_t)b * a.C + c0) * plane + rem;
#pragma unroll
                for (int cc = 0; cc < MIP_CH; ++cc) gv[j][cc] = g[(cc < nc ? cc : 0) * plane];
            }
            float w[MIP_AHEAD];
            bool use[MIP_AHEAD];
#pragma unroll
            for (int j = 0; j < MIP_AHEAD; ++j) {
                use[j] = false;
                w[j] = 0.f;
                if (ent[j] < 0) continue;
                const int k = (int)(ent[j] & 7);
                const float u = pu[j], v = pv[j];
                const bool live = is_live(u, v, pc[j] != 0);
                int l0;
                float fr;
                split_lod(pl[j], a.L, l0, fr);
                const bool upper = k >= 4;
                if (!live || (upper && fr == 0.f)) continue;
                const int l = upper ? min(l0 + 1, a.L - 1) : l0;
                const Foot f = footprint(u, v, a.Th >> l, a.Tw >> l);
                const float wx = (k & 1) ? f.fx : 1.f - f.fx;
                const float wy = (k & 2) ? f.fy : 1.f - f.fy;
                w[j] = (upper ? fr : 1.f - fr) * (wx * wy);
                use[j] = true;
            }
#pragma unroll
            for (int j = 0; j < MIP_AHEAD; ++j) {
                if (!use[j]) continue;
#pragma unroll
                for (int cc = 0; cc < MIP_CH; ++cc)
                    if (cc < nc) acc[cc] = acc[cc] + w[j] * gv[j][cc];
            }
        }
#pragma unroll
        for (int cc = 0; cc < MIP_CH; ++cc)
            if (cc < nc) a.gpyr[(bt * a.C + c0 + cc) * a.P + elem] = acc[cc];
    }
}

// ---- the checks the entries share ---------------------------------------------------------------------------------------
// the texture's sides and the number of levels: 0 to go on
int level_check(int64_t Th, int64_t Tw, int64_t L) {
    if (Th < 1 || Tw < 1 || L < 1) return SR_EINVAL;
    if (Th > (1 << 20) || Tw > (1 << 20) || Th * Tw >= (1LL << 31)) return SR_ERANGE;
    if (L > mip_levels(Th, Tw)) return SR_EINVAL;
    return SR_OK;
}

int sample_check(int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw, int64_t L, bool& empty) {
    empty = false;
    if (B < 0 || C < 1 || H < 0 || W < 0) return SR_EINVAL;
    const int rc = level_check(Th, Tw, L);
    if (rc != SR_OK) return rc;
    if (!(Bt == B || Bt == 1)) return SR_EINVAL;
    if (B == 0 || H == 0 || W == 0) {
        empty = true;
        return SR_OK;
    }
    if (B > 65535 || C > 65535 || H > (1 << 20) || W > (1 << 20) || Bt * mip_total(Th, Tw, (int)L) >= (1LL << 31) - 1 ||
        8 * B * H * W >= (1LL << 31))
        return SR_ERANGE;
    return SR_OK;
}

MipArgs mip_args(const float* pyr, const float* uv, const uint8_t* cover, const float* lod, int64_t B, int64_t Bt, int64_t C,
                 int64_t H, int64_t W, int64_t Th, int64_t Tw, int64_t L) {
    MipArgs a;
    a.pyr = pyr, a.uv = uv, a.cover = cover, a.lod = lod;
    a.P = mip_total(Th, Tw, (int)L);
    a.pyr_bstride = (Bt == 1 && B != 1) ? 0 : C * a.P;
    a.B = (int)B, a.C = (int)C, a.H = (int)H, a.W = (int)W, a.Th = (int)Th, a.Tw = (int)Tw, a.L = (int)L;
    return a;
}

}  // namespace

extern "C" int sr_mip_build_fwd(float* pyr, const float* tex, int64_t N, int64_t Th, int64_t Tw, int64_t L,
                                sr_stream_t stream) {
    if (N < 0) return SR_EINVAL;
    const int rc = level_check(Th, Tw, L);
    if (rc != SR_OK) return rc;
    if (N == 0) return SR_OK;
    if (!pyr || !tex || pyr == tex) return SR_EINVAL;
    const int64_t P = mip_total(Th, Tw, (int)L);
    if (N * P >= (1LL << 40)) return SR_ERANGE;
    for (int s = 0; s == 0 || s < L - 1; s += MIP_STEP) {
        BuildArgs a;
        a.pyr = pyr, a.P = P, a.N = N, a.Th = (int)Th, a.Tw = (int)Tw, a.s = s;
        a.src = s == 0 ? tex : pyr + mip_offset(Th, Tw, s);
        a.src_stride = s == 0 ? Th * Tw : P;
        a.down = (int)(L - 1 - s < MIP_STEP ? L - 1 - s : MIP_STEP);
        a.tiles_x = (int)sr_ceil_div(Tw >> s, MIP_TILE);
        a.tiles_y = (int)sr_ceil_div(Th >> s, MIP_TILE);
        const int64_t blocks = N * a.tiles_x * a.tiles_y;
        if (blocks >= (1LL << 31)) return SR_ERANGE;
        hipLaunchKernelGGL(k_mip_build_fwd, dim3((unsigned)blocks), dim3(MIP_BLOCK), 0, sr_stream(stream), a);
        const int st = sr_launch_status();
        if (st != SR_OK) return st;
    }
    return SR_OK;
}

extern "C" int sr_mip_build_bwd(float* gtex, const float* gpyr, int64_t Bt, int64_t C, int64_t Th, int64_t Tw, int64_t L,
                                sr_stream_t stream) {
    if (Bt < 0 || C < 1) return SR_EINVAL;
    const int rc = level_check(Th, Tw, L);
    if (rc != SR_OK) return rc;
    if (Bt == 0) return SR_OK;
    if (Bt > 65535 || C > 65535 || Bt * Th * Tw >= (1LL << 31) - 1) return SR_ERANGE;
    if (!gtex || !gpyr || gtex == gpyr) return SR_EINVAL;
    BuildBwdArgs a;
    a.gtex = gtex, a.gpyr = gpyr, a.P = mip_total(Th, Tw, (int)L), a.n = Bt * Th * Tw;
    a.C = (int)C, a.Th = (int)Th, a.Tw = (int)Tw, a.L = (int)L;
    hipLaunchKernelGGL(k_mip_build_bwd, dim3((unsigned)sr_ceil_div(a.n, MIP_BLOCK)), dim3(MIP_BLOCK), 0, sr_stream(stream), a);
    return sr_launch_status();
}

extern "C" int sr_mip_lod(float* lod, const float* uv, const uint8_t* cover, int64_t B, int64_t H, int64_t W, int64_t Th,
                          int64_t Tw, int64_t L, float bias, sr_stream_t stream) {
    if (B < 0 || H < 0 || W < 0) return SR_EINVAL;
    const int rc = level_check(Th, Tw, L);
    if (rc != SR_OK) return rc;
    if (B == 0 || H == 0 || W == 0) return SR_OK;
    if (B > 65535 || H > (1 << 20) || W > (1 << 20) || 8 * B * H * W >= (1LL << 31)) return SR_ERANGE;
    if (!lod || !uv || !cover || (const float*)lod == uv) return SR_EINVAL;
    LodArgs a;
    a.lod = lod, a.uv = uv, a.cover = cover, a.bias = bias;
    a.B = (int)B, a.H = (int)H, a.W = (int)W, a.Th = (int)Th, a.Tw = (int)Tw, a.L = (int)L;
    const dim3 grid((unsigned)sr_ceil_div(B * H * ((W + 3) / 4), MIP_BLOCK));
    if (W % 4 == 0 && sr_aligned16(lod))
        hipLaunchKernelGGL(k_mip_lod<4>, grid, dim3(MIP_BLOCK), 0, sr_stream(stream), a);
    else
        hipLaunchKernelGGL(k_mip_lod<1>, grid, dim3(MIP_BLOCK), 0, sr_stream(stream), a);
    return sr_launch_status();
}

extern "C" int sr_mip_sample_fwd(float* out, const float* pyr, const float* uv, const uint8_t* cover, const float* lod,
                                 int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw, int64_t L,
                                 float background, sr_stream_t stream) {
    bool empty;
    const int rc = sample_check(B, Bt, C, H, W, Th, Tw, L, empty);
    if (rc != SR_OK || empty) return rc;
    if (!out || !pyr || !uv || !cover || !lod || out == pyr) return SR_EINVAL;
    const MipArgs a = mip_args(pyr, uv, cover, lod, B, Bt, C, H, W, Th, Tw, L);
    const dim3 grid((unsigned)sr_ceil_div(B * H * ((W + 3) / 4), MIP_BLOCK));
    if (W % 4 == 0 && sr_aligned16(out))
        hipLaunchKernelGGL(k_mip_sample_fwd<4>, grid, dim3(MIP_BLOCK), 0, sr_stream(stream), a, out, background);
    else
        hipLaunchKernelGGL(k_mip_sample_fwd<1>, grid, dim3(MIP_BLOCK), 0, sr_stream(stream), a, out, background);
    return sr_launch_status();
}

extern "C" int sr_mip_sample_bwd_uv(float* guv, const float* gout, const float* pyr, const float* uv, const uint8_t* cover,
                                    const float* lod, int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th,
                                    int64_t Tw, int64_t L, sr_stream_t stream) {
    bool empty;
    const int rc = sample_check(B, Bt, C, H, W, Th, Tw, L, empty);
    if (rc != SR_OK || empty) return rc;
    if (!guv || !gout || !pyr || !uv || !cover || !lod || guv == uv || guv == gout) return SR_EINVAL;
    const MipArgs a = mip_args(pyr, uv, cover, lod, B, Bt, C, H, W, Th, Tw, L);
    const dim3 grid((unsigned)sr_ceil_div(B * H * ((W + 3) / 4), MIP_BLOCK));
    if (W % 4 == 0 && sr_aligned16(guv) && sr_aligned16(gout))
        hipLaunchKernelGGL(k_mip_sample_bwd_uv<4>, grid, dim3(MIP_BLOCK), 0, sr_stream(stream), a, guv, gout);
    else
        hipLaunchKernelGGL(k_mip_sample_bwd_uv<1>, grid, dim3(MIP_BLOCK), 0, sr_stream(stream), a, guv, gout);
    return sr_launch_status();
}

extern "C" int sr_mip_sample_bwd_pyr(float* gpyr, const float* gout, const float* uv, const uint8_t* cover, const float* lod,
                                     const int32_t* off, const int32_t* entries, int64_t B, int64_t Bt, int64_t C, int64_t H,
                                     int64_t W, int64_t Th, int64_t Tw, int64_t L, sr_stream_t stream) {
    bool empty;
    const int rc = sample_check(B, Bt, C, H, W, Th, Tw, L, empty);
    if (rc != SR_OK) return rc;
    if (!gpyr || !off) return SR_EINVAL;
    if (!empty && (!gout || !uv || !cover || !lod || !entries || gpyr == gout)) return SR_EINVAL;
    const int64_t P = mip_total(Th, Tw, (int)L);
    if (empty && (Bt > 65535 || C > 65535 || Bt * P >= (1LL << 31) - 1)) return SR_ERANGE;
    TapArgs a;
    a.gpyr = gpyr, a.gout = gout, a.uv = uv, a.cover = cover, a.lod = lod, a.off = off, a.entries = entries;
    a.P = P, a.keys = Bt * P, a.n_entries = 8 * B * H * W;                 // (no pixels: every list is empty, every element 0)
    a.C = (int)C, a.H = (int)H, a.W = (int)W, a.Th = (int)Th, a.Tw = (int)Tw, a.L = (int)L;
    hipLaunchKernelGGL(k_mip_sample_bwd_pyr, dim3((unsigned)sr_ceil_div(a.keys, MIP_BLOCK)), dim3(MIP_BLOCK), 0,
                       sr_stream(stream), a);
    return sr_launch_status();
}
