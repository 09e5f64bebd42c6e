// Region-weighted image loss of face reconstruction (definition: stylerenderer_amd/op/region.py; declarations:
// include/stylerenderer_amd.h).  Compiled with -ffp-contract=off: every product and sum of the blend is rounded on its
// own, in the order the host composite writes it, so the float32 results carry the host's bits.
//
//   k_region_fill   one lane per pixel, uint8 out.  A sample's triangles are gathered (index -> integer point) into LDS
//                   FILL_CHUNK at a time by the workgroup, so T is unbounded; a lane rejects a triangle by its bounding
//                   box first, then takes the three int64 edge functions, and stops testing once its pixel is set; the
//                   workgroup leaves the chunk loop when all of its pixels are set.  Integers only.
//   k_region_grow   one lane per pixel over the (2 |r| + 1)^2 window, clipped to the picture.  This runs once per
//                   picture, not per step: at 256^2 and |r| = 32 it is 2.8e8 byte reads, which the caches serve — a
//                   separable or van Herk form would save microseconds nobody waits for.
//   k_region_blend_fwd / k_region_blend_bwd   the per-step path.  A lane owns one pixel (V = 1) or four consecutive
//                   pixels (V = 4: float4 loads and stores; H W % 4 == 0 and every pointer 16-byte aligned) of one
//                   sample and walks its C channels; the mask and the normal map's three channels are read once per
//                   pixel.  The normal map is read through its four strides (the rasterizer's permuted view is not
//                   copied); NV says that its four pixels of a lane are one aligned float4 per channel.
//
// No atomics, no memset, no host read: all four run under graph capture on the caller's stream.
#include "common.h"

namespace {

constexpr int FILL_BLOCK = 256, FILL_CHUNK = 256;

__global__ __launch_bounds__(FILL_BLOCK) void k_region_fill(uint8_t* __restrict__ out, const int32_t* __restrict__ pts,
                                                            const int32_t* __restrict__ tris, int64_t tri_bstride, int P,
                                                            int T, int H, int W) {
    __shared__ int32_t tri_s[FILL_CHUNK][6];
    const int b = blockIdx.y;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * FILL_BLOCK + threadIdx.x;
    const bool live = pix < hw;
    const int x = live ? (int)(pix % W) : 0, y = live ? (int)(pix / W) : 0;
    const int32_t* p = pts + (int64_t)b * P * 2;
    const int32_t* t = tris + (int64_t)b * tri_bstride;
    bool set = false;
    for (int c0 = 0; c0 < T; c0 += FILL_CHUNK) {
        // (also the barrier between the previous chunk's readers and this chunk's writers)
        if (__syncthreads_and(set || !live)) break;
        const int count = min(FILL_CHUNK, T - c0);
        if ((int)threadIdx.x < count) {
            const int32_t* tt = t + (int64_t)(c0 + threadIdx.x) * 3;
            const int ia = tt[0], ib = tt[1], ic = tt[2];
            // an index outside the points (the caller validates them) makes a triangle whose bounding box no pixel is in,
            // never a read past the points
            const bool ok = (unsigned)ia < (unsigned)P && (unsigned)ib < (unsigned)P && (unsigned)ic < (unsigned)P;
            int32_t* s = tri_s[threadIdx.x];
            s[0] = ok ? p[2 * ia] : 0x7fffffff, s[1] = ok ? p[2 * ia + 1] : 0;
            s[2] = ok ? p[2 * ib] : 0x7fffffff, s[3] = ok ? p[2 * ib + 1] : 0;
            s[4] = ok ? p[2 * ic] : 0x7fffffff, s[5] = ok ? p[2 * ic + 1] : 0;
        }
        __syncthreads();
        if (live && !set) {
            for (int k = 0; k < count; ++k) {
                const int ax = tri_s[k][0], ay = tri_s[k][1], bx = tri_s[k][2], by = tri_s[k][3];
                const int cx = tri_s[k][4], cy = tri_s[k][5];
                if (x < min(ax, min(bx, cx)) || x > max(ax, max(bx, cx)) || y < min(ay, min(by, cy)) ||
                    y > max(ay, max(by, cy)))
                    continue;
                const int64_t e0 = (int64_t)(bx - ax) * (y - ay) - (int64_t)(by - ay) * (x - ax);
                const int64_t e1 = (int64_t)(cx - bx) * (y - by) - (int64_t)(cy - by) * (x - bx);
                const int64_t e2 = (int64_t)(ax - cx) * (y - cy) - (int64_t)(ay - cy) * (x - cx);
                if ((e0 >= 0 && e1 >= 0 && e2 >= 0) || (e0 <= 0 && e1 <= 0 && e2 <= 0)) {
                    set = true;
                    break;
                }
            }
        }
    }
    if (live) out[(int64_t)b * hw + pix] = set ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_region_grow(uint8_t* __restrict__ out, const uint8_t* __restrict__ in, int r,
                                                     int H, int W, int64_t total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t hw = (int64_t)H * W;
    const int64_t pix = i % hw;
    const uint8_t* img = in + (i - pix);
    const int x = (int)(pix % W), y = (int)(pix / W);
    const int a = r < 0 ? -r : r;
    const int x0 = max(x - a, 0), x1 = min(x + a, W - 1), y0 = max(y - a, 0), y1 = min(y + a, H - 1);
    // dilation looks for a set pixel, erosion for a clear one; pixels outside the picture count for neither
    const bool want = r > 0;
    bool found = false;
    for (int yy = y0; yy <= y1 && !found; ++yy) {
        const uint8_t* row = img + (int64_t)yy * W;
        for (int xx = x0; xx <= x1; ++xx)
            if ((row[xx] != 0) == want) {
                found = true;
                break;
            }
    }
    out[i] = (found == want) ? 1 : 0;
}

struct BlendArgs {
    float* y;            // [B, C, H, W]
    float* m_eff;        // [B, 1, H, W]
    const float* img;    // [B, C, H, W]
    const float* target; // [B, C, H, W]
    const float* mask;   // [B, 1, H, W]
    const float* n;      // logical [B, 3, H, W] through the strides below, or NULL
    int64_t nsb, nsc, nsh, nsw;
    float thresh;
    int64_t B, C, hw;
    int W;
};

// m_eff of V consecutive pixels starting at pixel p of sample b
template <int V, bool NV>
__device__ __forceinline__ void gate_v(const BlendArgs& a, int64_t b, int64_t p, float* m) {
    sr_load_v<V>(m, a.mask + b * a.hw + p);
    if (a.n == nullptr) return;
    float nn[3][V];
    if (NV) {
        // (NV only with V = 4: the four pixels are contiguous and aligned in every channel)
#pragma unroll
        for (int c = 0; c < 3; ++c) sr_load_v<V>(nn[c], a.n + b * a.nsb + c * a.nsc + p);
    } else {
#pragma unroll
        for (int q = 0; q < V; ++q) {
            const int64_t yy = (p + q) / a.W, xx = (p + q) % a.W;
            const float* base = a.n + b * a.nsb + yy * a.nsh + xx * a.nsw;
#pragma unroll
            for (int c = 0; c < 3; ++c) nn[c][q] = base[c * a.nsc];
        }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) {
        const float d = nn[0][q] * nn[0][q] + nn[1][q] * nn[1][q] + nn[2][q] * nn[2][q];
        m[q] = m[q] * (d > a.thresh ? 1.0f : 0.0f);
    }
}

template <int V>
__device__ __forceinline__ void store_v(float* p, const float* v) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else p[0] = v[0];
}

template <int V, bool NV>
__global__ __launch_bounds__(256) void k_region_blend_fwd(BlendArgs a) {
    const int64_t units = a.hw / V, total = a.B * units;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / units, p = (i % units) * V;
        float m[V];
        gate_v<V, NV>(a, b, p, m);
        store_v<V>(a.m_eff + b * a.hw + p, m);
        for (int64_t c = 0; c < a.C; ++c) {
            const int64_t o = (b * a.C + c) * a.hw + p;
            float x[V], t[V], y[V];
            sr_load_v<V>(x, a.img + o);
            sr_load_v<V>(t, a.target + o);
#pragma unroll
            for (int q = 0; q < V; ++q) y[q] = t[q] + m[q] * (x[q] - t[q]);
            store_v<V>(a.y + o, y);
        }
    }
}

template <int V>
__global__ __launch_bounds__(256) void k_region_blend_bwd(float* __restrict__ g_img, const float* __restrict__ g_y,
                                                          const float* __restrict__ m_eff, int64_t B, int64_t C,
                                                          int64_t hw) {
    const int64_t units = hw / V, total = B * units;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / units, p = (i % units) * V;
        float m[V];
        sr_load_v<V>(m, m_eff + b * hw + p);
        for (int64_t c = 0; c < C; ++c) {
            const int64_t o = (b * C + c) * hw + p;
            float g[V], r[V];
            sr_load_v<V>(g, g_y + o);
#pragma unroll
            for (int q = 0; q < V; ++q) r[q] = m[q] * g[q];
            store_v<V>(g_img + o, r);
        }
    }
}

}  // namespace

extern "C" int sr_region_fill(uint8_t* out, const int32_t* points, const int32_t* tris, int64_t tri_bstride, int64_t B,
                              int64_t P, int64_t T, int64_t H, int64_t W, sr_stream_t stream) {
    if (B < 0 || P < 1 || T < 0 || H < 1 || W < 1 || (tri_bstride != 0 && tri_bstride != 3 * T)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!out || !points || (T > 0 && !tris)) return SR_EINVAL;
    if (B > 65535 || H > (1 << 20) || W > (1 << 20) || P > (1 << 28) || T > (1 << 28)) return SR_ERANGE;
    const dim3 grid((unsigned)sr_ceil_div(H * W, FILL_BLOCK), (unsigned)B);
    hipLaunchKernelGGL(k_region_fill, grid, dim3(FILL_BLOCK), 0, sr_stream(stream), out, points, tris, tri_bstride, (int)P,
                       (int)T, (int)H, (int)W);
    return sr_launch_status();
}

extern "C" int sr_region_grow(uint8_t* out, const uint8_t* in, int64_t N, int64_t H, int64_t W, int r,
                              sr_stream_t stream) {
    if (N < 0 || H < 1 || W < 1 || r == 0 || r < -32 || r > 32) return SR_EINVAL;
    if (N == 0) return SR_OK;
    if (!out || !in || out == in) return SR_EINVAL;
    if (H > (1 << 20) || W > (1 << 20) || N * H * W > (int64_t)0x7fffffff * 256) return SR_ERANGE;
    const int64_t total = N * H * W;
    hipLaunchKernelGGL(k_region_grow, dim3((unsigned)sr_ceil_div(total, 256)), dim3(256), 0, sr_stream(stream), out, in, r,
                       (int)H, (int)W, total);
    return sr_launch_status();
}

extern "C" int sr_region_blend_fwd(float* y, float* m_eff, const float* img, const float* target, const float* mask,
                                   const float* normal_map, int64_t nsb, int64_t nsc, int64_t nsh, int64_t nsw,
                                   float thresh, int64_t B, int64_t C, int64_t H, int64_t W, sr_stream_t stream) {
    if (B < 0 || C < 1 || H < 1 || W < 1) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!y || !m_eff || !img || !target || !mask) return SR_EINVAL;
    if (H > (1 << 20) || W > (1 << 20)) return SR_ERANGE;
    BlendArgs a;
    a.y = y, a.m_eff = m_eff, a.img = img, a.target = target, a.mask = mask, a.n = normal_map;
    a.nsb = nsb, a.nsc = nsc, a.nsh = nsh, a.nsw = nsw;
    a.thresh = thresh, a.B = B, a.C = C, a.hw = H * W, a.W = (int)W;
    const bool vec = a.hw % 4 == 0 && sr_aligned16(y) && sr_aligned16(m_eff) && sr_aligned16(img) &&
                     sr_aligned16(target) && sr_aligned16(mask);
    // the map's four pixels of a lane as one float4 per channel: pixels contiguous, every plane 16-byte aligned
    const bool nvec = vec && normal_map && nsw == 1 && nsh == W && nsb % 4 == 0 && nsc % 4 == 0 && sr_aligned16(normal_map);
    const int grid = sr_stream_grid(B * (a.hw / (vec ? 4 : 1)), 256);
    hipStream_t s = sr_stream(stream);
    if (nvec) hipLaunchKernelGGL((k_region_blend_fwd<4, true>), dim3(grid), dim3(256), 0, s, a);
    else if (vec) hipLaunchKernelGGL((k_region_blend_fwd<4, false>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_region_blend_fwd<1, false>), dim3(grid), dim3(256), 0, s, a);
    return sr_launch_status();
}

extern "C" int sr_region_blend_bwd(float* g_img, const float* g_y, const float* m_eff, int64_t B, int64_t C, int64_t H,
                                   int64_t W, sr_stream_t stream) {
    if (B < 0 || C < 1 || H < 1 || W < 1) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!g_img || !g_y || !m_eff) return SR_EINVAL;
    if (H > (1 << 20) || W > (1 << 20)) return SR_ERANGE;
    const int64_t hw = H * W;
    const bool vec = hw % 4 == 0 && sr_aligned16(g_img) && sr_aligned16(g_y) && sr_aligned16(m_eff);
    const int grid = sr_stream_grid(B * (hw / (vec ? 4 : 1)), 256);
    hipStream_t s = sr_stream(stream);
    if (vec) hipLaunchKernelGGL((k_region_blend_bwd<4>), dim3(grid), dim3(256), 0, s, g_img, g_y, m_eff, B, C, hw);
    else hipLaunchKernelGGL((k_region_blend_bwd<1>), dim3(grid), dim3(256), 0, s, g_img, g_y, m_eff, B, C, hw);
    return sr_launch_status();
}
