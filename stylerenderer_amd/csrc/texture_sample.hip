// The texture look-up node of face reconstruction (C ABI: sr_texture_sample_fwd / sr_texture_sample_bwd_uv /
// sr_texture_sample_bwd_tex; definition: stylerenderer_amd/op/texture.py, sample_composite).  A uv map [B, H, W, 2] with a
// cover mask [B, H, W] (op.texture.uv_map: the rasterizer's interpolation of a layout's coordinates over the posed mesh)
// names for every pixel a point of the texture [Bt, C, Th, Tw], Bt = B or 1 (one texture shared by all views).
//
//   k_texture_sample_fwd     a gather over pixels.  A lane owns four consecutive pixels of one row; it derives their four
//                            taps and the two fractions once and then walks the C planes: four loads, the bilinear blend in
//                            the bake's form, one 16-byte store per plane (V = 4: W % 4 == 0 and the planes 16-byte aligned)
//                            or scalar stores (V = 1: any width, the tail of a row included).  An uncovered pixel (cover 0
//                            or a non-finite coordinate) writes `background` and reads no texel.
//   k_texture_sample_bwd_uv  the same staging; a lane adds g_c times the blend's two partial derivatives over the channels
//                            in channel order and writes its pixels' (grad_u, grad_v): two 16-byte stores or eight scalar
//                            ones.  Beyond the clamp (sx outside [-1, Tw]) a coordinate's gradient is 0.
//   k_texture_sample_bwd_tex the gradient of the texture as a gather per texel: a lane owns one texel of one texture for all
//                            channels and walks that texel's tap list (a CSR built once per uv map by op.texture.tap_plan:
//                            entries ((b H + y) W + x) 4 + k, ascending) in order, recomputing the tap's weight from the uv
//                            map, so that no weights are stored.  Every texel is written, taps or not: one without taps
//                            gets exactly 0.  Up to four channels ride along per walk.
//
// A scatter with float atomics (what a library's grid sampler does) would add a texel's taps in the order the hardware
// happens to retire them; this sum has one order, the list's, and is the host definition's bit for bit.  The arithmetic is
// the definition's, one float32 operation per step in the same order (-ffp-contract=off).  Vector stores and plain C++
// only: no atomics, no scratch, no memset, no host read, so all three run under graph capture on the caller's stream.
#include "common.h"
#include "texture_footprint.h"

namespace {

constexpr int TS_BLOCK = 256;
constexpr int TS_CH = 4;                                                  // channels a texel's lane carries per walk

struct SampleArgs {
    const float* tex;        // [Bt, C, Th, Tw]
    const float* uv;         // [B, H, W, 2]
    const uint8_t* cover;    // [B, H, W]
    int64_t tex_bstride;     // C Th Tw, or 0 for a shared texture
    int B, C, H, W, Th, Tw;
};

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
__device__ __forceinline__ bool lane_pixels(const SampleArgs& a, int& b, int& y, int& x0, int& count, Foot* f) {
    const int groups = (a.W + 3) >> 2;                                    // lanes per row
    const int64_t item = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x;
    if (item >= (int64_t)a.B * a.H * groups) return false;
    x0 = (int)(item % groups) * 4;
    const int64_t row = item / groups;
    y = (int)(row % a.H);
    b = (int)(row / a.H);
    count = min(4, a.W - x0);
    const int64_t p0 = ((int64_t)b * a.H + y) * a.W + x0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < count)
            f[j] = footprint(a.uv[2 * (p0 + j)], a.uv[2 * (p0 + j) + 1], a.cover[p0 + j] != 0, a.Th, a.Tw);
        else
            f[j] = footprint(0.f, 0.f, false, a.Th, a.Tw);
    }
    return true;
}

template <int V>
__global__ __launch_bounds__(TS_BLOCK) void k_texture_sample_fwd(SampleArgs a, float* __restrict__ out, float background) {
    int b, y, x0, count;
    Foot f[4];
    if (!lane_pixels(a, b, y, x0, count, f)) return;
    const int64_t tplane = (int64_t)a.Th * a.Tw, plane = (int64_t)a.H * a.W;
    const int64_t at = (int64_t)y * a.W + x0;
    for (int c = 0; c < a.C; ++c) {
        const float* t = a.tex + (int64_t)b * a.tex_bstride + c * tplane;
        float col[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            col[j] = background;
            if (f[j].live) {
                const float fx = f[j].fx, fy = f[j].fy;
                const float top = (1.f - fx) * t[f[j].o00] + fx * t[f[j].o01];
                const float bot = (1.f - fx) * t[f[j].o10] + fx * t[f[j].o11];
                col[j] = top * (1.f - fy) + bot * fy;
            }
        }
        store4<V>(out + ((int64_t)b * a.C + c) * plane + at, col, count);
    }
}

template <int V>
__global__ __launch_bounds__(TS_BLOCK) void k_texture_sample_bwd_uv(SampleArgs a, float* __restrict__ guv,
                                                                   const float* __restrict__ gout) {
    int b, y, x0, count;
    Foot f[4];
    if (!lane_pixels(a, b, y, x0, count, f)) return;
    const int64_t tplane = (int64_t)a.Th * a.Tw, plane = (int64_t)a.H * a.W;
    const int64_t at = (int64_t)y * a.W + x0;
    float gx[4], gy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gx[j] = gy[j] = 0.f;
    for (int c = 0; c < a.C; ++c) {
        const float* t = a.tex + (int64_t)b * a.tex_bstride + c * tplane;
        float g[4];
        load4<V>(g, gout + ((int64_t)b * a.C + c) * plane + at, count);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (f[j].live) {
                const float fx = f[j].fx, fy = f[j].fy;
                const float t00 = t[f[j].o00], t01 = t[f[j].o01], t10 = t[f[j].o10], t11 = t[f[j].o11];
                const float top = (1.f - fx) * t00 + fx * t01;
                const float bot = (1.f - fx) * t10 + fx * t11;
                gx[j] = gx[j] + g[j] * ((t01 - t00) * (1.f - fy) + (t11 - t10) * fy);
                gy[j] = gy[j] + g[j] * (bot - top);
            }
        }
    }
    const float tw = (float)a.Tw, th = (float)a.Th;
    float o[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[2 * j] = (f[j].live && f[j].inx) ? gx[j] * tw : 0.f;
        o[2 * j + 1] = (f[j].live && f[j].iny) ? -(gy[j] * th) : 0.f;
    }
    float* p = guv + 2 * (((int64_t)b * a.H + y) * a.W + x0);
    store4<V>(p, o, 2 * count);
    store4<V>(p + 4, o + 4, 2 * count - 4);
}

struct TapArgs {
    float* gtex;             // [Bt, C, Th, Tw]
    const float* gout;       // [B, C, H, W]
    const float* uv;         // [B, H, W, 2]
    const uint8_t* cover;    // [B, H, W]
    const int32_t* off;      // [keys + 2]: the CSR's offsets (the last bucket holds the uncovered pixels' entries)
    const int32_t* entries;  // [4 B H W]
    int64_t keys;            // Bt Th Tw
    int64_t n_entries;       // 4 B H W
    int C, H, W, Th, Tw;
};

__global__ __launch_bounds__(TS_BLOCK) void k_texture_sample_bwd_tex(TapArgs a) {
    const int64_t key = (int64_t)blockIdx.x * TS_BLOCK + threadIdx.x;      // bt Th Tw + texel
    if (key >= a.keys) return;
    const int64_t tplane = (int64_t)a.Th * a.Tw, plane = (int64_t)a.H * a.W;
    const int64_t bt = key / tplane, texel = key % tplane;
    // a list that is not this call's (stale, or of another size) must not lead outside the tensors
    int64_t lo = a.off[key], hi = a.off[key + 1];
    lo = lo < 0 ? 0 : (lo > a.n_entries ? a.n_entries : lo);
    hi = hi < lo ? lo : (hi > a.n_entries ? a.n_entries : hi);
    for (int c0 = 0; c0 < a.C; c0 += TS_CH) {
        const int nc = min(TS_CH, a.C - c0);
        float acc[TS_CH];
#pragma unroll
        for (int cc = 0; cc < TS_CH; ++cc) acc[cc] = 0.f;
        for (int64_t e = lo; e < hi; ++e) {
            const int64_t ent = a.entries[e];
            if (ent < 0 || ent >= a.n_entries) continue;
            const int64_t pix = ent >> 2;
            const int k = (int)(ent & 3);
            const Foot f = footprint(a.uv[2 * pix], a.uv[2 * pix + 1], a.cover[pix] != 0, a.Th, a.Tw);
            if (!f.live) continue;
            const float wx = (k & 1) ? f.fx : 1.f - f.fx;
            const float wy = (k & 2) ? f.fy : 1.f - f.fy;
            const float w = wx * wy;
            const int64_t b = pix / plane, rem = pix % plane;
            const float* g = a.gout + (b * a.C + c0) * plane + rem;
#pragma unroll
            for (int cc = 0; cc < TS_CH; ++cc)
                if (cc < nc) acc[cc] = acc[cc] + w * g[cc * plane];
        }
#pragma unroll
        for (int cc = 0; cc < TS_CH; ++cc)
            if (cc < nc) a.gtex[(bt * a.C + c0 + cc) * tplane + texel] = acc[cc];
    }
}

// the checks the three entries share: 0 to go on, else the code to return (SR_OK included: nothing to do)
int sample_check(int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw, bool& empty) {
    empty = false;
    if (B < 0 || C < 1 || H < 0 || W < 0 || Th < 1 || Tw < 1) return SR_EINVAL;
    if (!(Bt == B || Bt == 1)) return SR_EINVAL;
    if (B == 0 || H == 0 || W == 0) {
        empty = true;
        return SR_OK;
    }
    if (B > 65535 || C > 65535 || H > (1 << 20) || W > (1 << 20) || Th > (1 << 20) || Tw > (1 << 20) ||
        Th * Tw >= (1LL << 31) || Bt * Th * Tw >= (1LL << 31) - 1 || 4 * B * H * W >= (1LL << 31))
        return SR_ERANGE;
    return SR_OK;
}

SampleArgs sample_args(const float* tex, const float* uv, const uint8_t* cover, int64_t B, int64_t Bt, int64_t C, int64_t H,
                       int64_t W, int64_t Th, int64_t Tw) {
    SampleArgs a;
    a.tex = tex, a.uv = uv, a.cover = cover;
    a.tex_bstride = (Bt == 1 && B != 1) ? 0 : C * Th * Tw;
    a.B = (int)B, a.C = (int)C, a.H = (int)H, a.W = (int)W, a.Th = (int)Th, a.Tw = (int)Tw;
    return a;
}

}  // namespace

extern "C" int sr_texture_sample_fwd(float* out, const float* tex, const float* uv, const uint8_t* cover, int64_t B,
                                     int64_t Bt, int64_t C, int64_t H, int64_t W, int64_t Th, int64_t Tw, float background,
                                     sr_stream_t stream) {
    bool empty;
    const int rc = sample_check(B, Bt, C, H, W, Th, Tw, empty);
    if (rc != SR_OK || empty) return rc;
    if (!out || !tex || !uv || !cover || out == tex) return SR_EINVAL;
    const SampleArgs a = sample_args(tex, uv, cover, B, Bt, C, H, W, Th, Tw);
    const dim3 grid((unsigned)sr_ceil_div(B * H * ((W + 3) / 4), TS_BLOCK));
    if (W % 4 == 0 && sr_aligned16(out))
        hipLaunchKernelGGL(k_texture_sample_fwd<4>, grid, dim3(TS_BLOCK), 0, sr_stream(stream), a, out, background);
    else
        hipLaunchKernelGGL(k_texture_sample_fwd<1>, grid, dim3(TS_BLOCK), 0, sr_stream(stream), a, out, background);
    return sr_launch_status();
}

extern "C" int sr_texture_sample_bwd_uv(float* guv, const float* gout, const float* tex, const float* uv,
                                        const uint8_t* cover, int64_t B, int64_t Bt, int64_t C, int64_t H, int64_t W,
                                        int64_t Th, int64_t Tw, sr_stream_t stream) {
    bool empty;
    const int rc = sample_check(B, Bt, C, H, W, Th, Tw, empty);
    if (rc != SR_OK || empty) return rc;
    if (!guv || !gout || !tex || !uv || !cover || guv == uv || guv == gout) return SR_EINVAL;
    const SampleArgs a = sample_args(tex, uv, cover, B, Bt, C, H, W, Th, Tw);
    const dim3 grid((unsigned)sr_ceil_div(B * H * ((W + 3) / 4), TS_BLOCK));
    if (W % 4 == 0 && sr_aligned16(guv) && sr_aligned16(gout))
        hipLaunchKernelGGL(k_texture_sample_bwd_uv<4>, grid, dim3(TS_BLOCK), 0, sr_stream(stream), a, guv, gout);
    else
        hipLaunchKernelGGL(k_texture_sample_bwd_uv<1>, grid, dim3(TS_BLOCK), 0, sr_stream(stream), a, guv, gout);
    return sr_launch_status();
}

extern "C" int sr_texture_sample_bwd_tex(float* gtex, const float* gout, const float* uv, const uint8_t* cover,
                                         const int32_t* off, const int32_t* entries, int64_t B, int64_t Bt, int64_t C,
                                         int64_t H, int64_t W, int64_t Th, int64_t Tw, sr_stream_t stream) {
    bool empty;
    const int rc = sample_check(B, Bt, C, H, W, Th, Tw, empty);
    if (rc != SR_OK) return rc;
    if (!gtex || !off) return SR_EINVAL;
    if (!empty && (!gout || !uv || !cover || !entries || gtex == gout)) return SR_EINVAL;
    if (empty && (Bt > 65535 || C > 65535 || Th > (1 << 20) || Tw > (1 << 20) || Bt * Th * Tw >= (1LL << 31) - 1))
        return SR_ERANGE;
    TapArgs a;
    a.gtex = gtex, a.gout = gout, a.uv = uv, a.cover = cover, a.off = off, a.entries = entries;
    a.keys = Bt * Th * Tw, a.n_entries = 4 * B * H * W;                    // (no pixels: every list is empty, every texel 0)
    a.C = (int)C, a.H = (int)H, a.W = (int)W, a.Th = (int)Th, a.Tw = (int)Tw;
    hipLaunchKernelGGL(k_texture_sample_bwd_tex, dim3((unsigned)sr_ceil_div(a.keys, TS_BLOCK)), dim3(TS_BLOCK), 0,
                       sr_stream(stream), a);
    return sr_launch_status();
}
