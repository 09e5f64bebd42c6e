// Albedo and lighting of the textured head: Lambertian shading under second-order spherical harmonics (C ABI:
// sr_light_shade_fwd / sr_light_shade_bwd / sr_light_reduce / sr_light_moments / sr_light_texel_attr; definition:
// stylerenderer_amd/op/light.py).  Per pixel, with the normal n = (nx, ny, nz):
//     r = sqrt((nx nx + ny ny) + nz nz);  len = r > 1e-12 ? r : 1e-12;  (x, y, z) = n / len
//     Y = [1, x, y, z, x y, x z, y z, x x - y y, 3 (z z) - 1]
//     s_l = (((g0 + g1 Y1) + g2 Y2) + ...) + g8 Y8          gamma [B, Cl, 9]; channel c reads light c (Cl = C) or 0 (Cl = 1)
//     shade:    out_c = (a_c - black) (s > 0 ? s : 0) + black;      unshade:  out_c = (a_c - black) / (s > floor ? s : floor) + black
// on the live pixels (`on` and a finite normal); `background` (shade) or a_c itself (unshade) elsewhere.
//
// Every step is one float32 operation in the definition's order (compiled with -ffp-contract=off and correctly rounded
// division and square root), so out, ga and gn are the host definition's bit for bit.
//
//   k_light_shade<V, DIV>   streaming, grid.y = sample.  A lane owns four consecutive pixels of a row: it normalises the
//                           normals and forms Y once, then walks the C planes.  V = 4: W % 4 == 0 and every base 16-byte
//                           aligned (the mask 4-byte): one 16-byte access per plane.  V = 1: scalar accesses, any width and
//                           alignment, the row's tail included.
//   k_light_shade_bwd<V, CL>  the same staging over ITEMS items per lane (item (blockIdx.x ITEMS + i) BLOCK + lane): ga and,
//                           when wanted, gn.  When the light's gradient is wanted a lane keeps its CL x 9 sums over its
//                           pixels in index order; a wave tree of depth 6 (lane 0 of each wave holds its sum), then a tree of
//                           depth 2 over the four waves in LDS; lanes 0 .. 9 CL - 1 write the workgroup's partial row.
//   k_light_reduce<T>       one lane per output element adds the partial rows in ascending order.
//   k_light_moments<V, C>   the 45 + 9 C float64 sums of `moments`, staged and reduced as the backward's.
//   k_light_texel_attr<V>   a gather over texels as k_texture_bake: a lane owns four texels of a row, reads face, the tri
//                           row and coeff once and walks the B samples.
//
// Vector stores and plain C++ only: no atomics, no memset, no allocation, no host read (scratch is the caller's), so every
// entry runs under graph capture on the caller's stream; reruns are bit-identical.
#include "common.h"

namespace {

constexpr int LT_BLOCK = 256;                 // op/light.py: BLOCK
constexpr int LT_ITEMS = 4;                   // ITEMS
constexpr int LT_WAVES = LT_BLOCK / SR_WAVE;  // 4: the LDS tree's depth is 2
constexpr int LT_NB = 9;
constexpr int LT_NM = 45;
constexpr float LT_TINY = 1e-12f;
constexpr float LT_FLT_MAX = 3.402823466e38f;

template <int V>
__device__ __forceinline__ void lt_load(float* x, const float* p, int count) {
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = j < count ? p[j] : 0.f;
    }
}

template <int V>
__device__ __forceinline__ void lt_store(float* p, const float* x, int count) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < count) p[j] = x[j];
    }
}

template <int V>
__device__ __forceinline__ void lt_load_mask(bool* m, const uint8_t* p, int count) {
    if constexpr (V == 4) {
        const uchar4 q = *reinterpret_cast<const uchar4*>(p);
        m[0] = q.x != 0, m[1] = q.y != 0, m[2] = q.z != 0, m[3] = q.w != 0;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = j < count ? p[j] != 0 : false;
    }
}

__device__ __forceinline__ bool lt_finite(float x) { return fabsf(x) <= LT_FLT_MAX; }

// the normalised normal and Y[1..8] of one pixel; returns r
struct LtBasis {
    float x, y, z, len, r;
    float Y[LT_NB];
};

__device__ __forceinline__ void lt_basis(LtBasis& o, float nx, float ny, float nz) {
    o.r = sqrtf((nx * nx + ny * ny) + nz * nz);
    o.len = o.r > LT_TINY ? o.r : LT_TINY;
    o.x = nx / o.len;
    o.y = ny / o.len;
    o.z = nz / o.len;
    o.Y[0] = 1.f;
    o.Y[1] = o.x;
    o.Y[2] = o.y;
    o.Y[3] = o.z;
    o.Y[4] = o.x * o.y;
    o.Y[5] = o.x * o.z;
    o.Y[6] = o.y * o.z;
    o.Y[7] = o.x * o.x - o.y * o.y;
    o.Y[8] = 3.f * (o.z * o.z) - 1.f;
}

__device__ __forceinline__ float lt_shading(const float* __restrict__ g, const float* Y) {
    float s = g[0] + g[1] * Y[1];
#pragma unroll
    for (int k = 2; k < LT_NB; ++k) s = s + g[k] * Y[k];
    return s;
}

// the four pixels of item j of a sample's H x W planes: offset of the first, how many are inside the row
struct LtItem {
    int64_t pix;
    int count;
};

__device__ __forceinline__ LtItem lt_item(int64_t j, int W, int groups) {
    LtItem it;
    const int64_t row = j / groups;
    const int x0 = (int)(j % groups) * 4;
    it.pix = row * W + x0;
    it.count = min(4, W - x0);
    return it;
}

// normals and mask of an item: live[] and the bases of the live pixels (the others get the basis of +z, never used)
template <int V>
__device__ __forceinline__ void lt_stage(LtBasis* bs, bool* live, const float* __restrict__ n, const uint8_t* __restrict__ on,
                                         const float* __restrict__ weight, int64_t plane, const LtItem& it) {
    float nx[4], ny[4], nz[4];
    lt_load<V>(nx, n + it.pix, it.count);
    lt_load<V>(ny, n + plane + it.pix, it.count);
    lt_load<V>(nz, n + 2 * plane + it.pix, it.count);
    if (on) {
        lt_load_mask<V>(live, on + it.pix, it.count);
    } else {
        float w[4];
        lt_load<V>(w, weight + it.pix, it.count);
#pragma unroll
        for (int p = 0; p < 4; ++p) live[p] = p < it.count && w[p] > 0.f;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        live[p] = live[p] && lt_finite(nx[p]) && lt_finite(ny[p]) && lt_finite(nz[p]);
        if (live[p]) lt_basis(bs[p], nx[p], ny[p], nz[p]);
        else lt_basis(bs[p], 0.f, 0.f, 1.f);
    }
}

struct ShadeArgs {
    float* out;            // [B, C, H, W]
    const float* a;        // [B, C, H, W]
    const float* n;        // [B, 3, H, W]
    const uint8_t* on;     // [B, H, W]
    const float* gamma;    // [B, Cl, 9]
    int C, Cl, H, W;
    float black, floor, background;
};

template <int V, bool DIV>
__global__ __launch_bounds__(LT_BLOCK) void k_light_shade(ShadeArgs k) {
    const int groups = (k.W + 3) >> 2;
    const int64_t j = (int64_t)blockIdx.x * LT_BLOCK + threadIdx.x;
    if (j >= (int64_t)k.H * groups) return;
    const int64_t b = blockIdx.y, plane = (int64_t)k.H * k.W;
    const LtItem it = lt_item(j, k.W, groups);
    LtBasis bs[4];
    bool live[4];
    lt_stage<V>(bs, live, k.n + b * 3 * plane, k.on + b * plane, nullptr, plane, it);
    float m[4];
    for (int c = 0; c < k.C; ++c) {
        if (c == 0 || k.Cl > 1) {
            const float* g = k.gamma + (b * k.Cl + (k.Cl > 1 ? c : 0)) * LT_NB;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float s = lt_shading(g, bs[p].Y);
                m[p] = DIV ? (s > k.floor ? s : k.floor) : (s > 0.f ? s : 0.f);
            }
        }
        float av[4], o[4];
        lt_load<V>(av, k.a + (b * k.C + c) * plane + it.pix, it.count);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (DIV) o[p] = live[p] ? (av[p] - k.black) / m[p] + k.black : av[p];
            else o[p] = live[p] ? (av[p] - k.black) * m[p] + k.black : k.background;
        }
        lt_store<V>(k.out + (b * k.C + c) * plane + it.pix, o, it.count);
    }
}

// The sum of every lane's x[0..N) over the workgroup, written by lanes 0..N-1 to row[0..N): a wave tree of depth 6 by
// shuffles (lane 0 of a wave ends with ((l0 + l32) + (l16 + l48)) + ... in a fixed order), then (w0 + w1) + (w2 + w3).
template <typename T, int N>
__device__ __forceinline__ void lt_block_sum(T* x, T (*lds)[LT_WAVES], T* __restrict__ row) {
    const int lane = threadIdx.x & (SR_WAVE - 1), wave = threadIdx.x / SR_WAVE;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T v = x[i];
#pragma unroll
        for (int off = SR_WAVE / 2; off > 0; off >>= 1) v = v + __shfl_down(v, off, SR_WAVE);
        if (lane == 0) lds[i][wave] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        const T* w = lds[threadIdx.x];
        row[threadIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
    }
}

struct BwdArgs {
    float* ga;             // [B, C, H, W]
    float* gn;             // [B, 3, H, W] or NULL
    float* partial;        // [B, P, CL, 9] or NULL
    const float* g;        // [B, C, H, W]
    const float* a;
    const float* n;
    const uint8_t* on;
    const float* gamma;    // [B, CL, 9]
    int C, H, W;
    float black;
};

// CL lights: CL == 1 serves any C (every channel reads light 0), CL > 1 means C == CL
template <int V, int CL>
__global__ __launch_bounds__(LT_BLOCK) void k_light_shade_bwd(BwdArgs k) {
    __shared__ float lds[CL * LT_NB][LT_WAVES];
    const int groups = (k.W + 3) >> 2;
    const int64_t items = (int64_t)k.H * groups;
    const int64_t b = blockIdx.y, plane = (int64_t)k.H * k.W;
    float gam[CL][LT_NB];
#pragma unroll
    for (int l = 0; l < CL; ++l)
#pragma unroll
        for (int i = 0; i < LT_NB; ++i) gam[l][i] = k.gamma[(b * CL + l) * LT_NB + i];
    float acc[CL * LT_NB];
#pragma unroll
    for (int i = 0; i < CL * LT_NB; ++i) acc[i] = 0.f;

    for (int i = 0; i < LT_ITEMS; ++i) {
        const int64_t j = ((int64_t)blockIdx.x * LT_ITEMS + i) * LT_BLOCK + threadIdx.x;
        if (j >= items) continue;
        const LtItem it = lt_item(j, k.W, groups);
        LtBasis bs[4];
        bool live[4];
        lt_stage<V>(bs, live, k.n + b * 3 * plane, k.on + b * plane, nullptr, plane, it);
        float sp[CL][4], e[CL][4];
        bool pos[CL][4];
#pragma unroll
        for (int l = 0; l < CL; ++l)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float s = lt_shading(gam[l], bs[p].Y);
                pos[l][p] = s > 0.f;
                sp[l][p] = pos[l][p] ? s : 0.f;
                e[l][p] = 0.f;
            }
        if constexpr (CL == 1) {
            for (int c = 0; c < k.C; ++c) {
                float gv[4], av[4], o[4];
                lt_load<V>(gv, k.g + (b * k.C + c) * plane + it.pix, it.count);
                lt_load<V>(av, k.a + (b * k.C + c) * plane + it.pix, it.count);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    o[p] = live[p] ? gv[p] * sp[0][p] : 0.f;
                    e[0][p] = e[0][p] + gv[p] * (av[p] - k.black);
                }
                lt_store<V>(k.ga + (b * k.C + c) * plane + it.pix, o, it.count);
            }
        } else {
#pragma unroll
            for (int c = 0; c < CL; ++c) {
                float gv[4], av[4], o[4];
                lt_load<V>(gv, k.g + (b * CL + c) * plane + it.pix, it.count);
                lt_load<V>(av, k.a + (b * CL + c) * plane + it.pix, it.count);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    o[p] = live[p] ? gv[p] * sp[c][p] : 0.f;
                    e[c][p] = e[c][p] + gv[p] * (av[p] - k.black);
                }
                lt_store<V>(k.ga + (b * CL + c) * plane + it.pix, o, it.count);
            }
        }
#pragma unroll
        for (int l = 0; l < CL; ++l)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (!(pos[l][p] && live[p])) e[l][p] = 0.f;
        if (k.partial) {                                                   // (uniform: a kernel argument)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (!live[p]) continue;
#pragma unroll
                for (int l = 0; l < CL; ++l) {
                    acc[l * LT_NB] = acc[l * LT_NB] + e[l][p];
#pragma unroll
                    for (int q = 1; q < LT_NB; ++q) acc[l * LT_NB + q] = acc[l * LT_NB + q] + e[l][p] * bs[p].Y[q];
                }
            }
        }
        if (k.gn) {
            float ox[4], oy[4], oz[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float gY[LT_NB];
#pragma unroll
                for (int q = 1; q < LT_NB; ++q) {
                    float t = 0.f;
#pragma unroll
                    for (int l = 0; l < CL; ++l) t = t + e[l][p] * gam[l][q];
                    gY[q] = t;
                }
                const float x = bs[p].x, y = bs[p].y, z = bs[p].z;
                const float gx = ((gY[1] + gY[4] * y) + gY[5] * z) + (2.f * gY[7]) * x;
                const float gy = ((gY[2] + gY[4] * x) + gY[6] * z) - (2.f * gY[7]) * y;
                const float gz = ((gY[3] + gY[5] * x) + gY[6] * y) + (6.f * gY[8]) * z;
                const float d = (x * gx + y * gy) + z * gz;
                const bool keep = live[p] && !(bs[p].r < LT_TINY);
                ox[p] = keep ? (gx - x * d) / bs[p].len : 0.f;
                oy[p] = keep ? (gy - y * d) / bs[p].len : 0.f;
                oz[p] = keep ? (gz - z * d) / bs[p].len : 0.f;
            }
            float* gn = k.gn + b * 3 * plane + it.pix;
            lt_store<V>(gn, ox, it.count);
            lt_store<V>(gn + plane, oy, it.count);
            lt_store<V>(gn + 2 * plane, oz, it.count);
        }
    }
    if (!k.partial) return;                                                // (uniform)
    lt_block_sum<float, CL * LT_NB>(acc, lds, k.partial + (b * gridDim.x + blockIdx.x) * (CL * LT_NB));
}

template <typename T>
__global__ __launch_bounds__(LT_BLOCK) void k_light_reduce(T* __restrict__ out, const T* __restrict__ partial, int64_t B,
                                                           int64_t P, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * LT_BLOCK + threadIdx.x;
    if (idx >= B * n) return;
    const int64_t b = idx / n, i = idx % n;
    const T* row = partial + b * P * n + i;
    T acc = row[0];
    for (int64_t p = 1; p < P; ++p) acc = acc + row[p * n];
    out[idx] = acc;
}

struct MomentArgs {
    double* partial;       // [B, P, 45 + 9 C]
    const float* a;        // [B, C, H, W]
    const float* n;        // [B, 3, H, W]
    const float* weight;   // [B, 1, H, W]
    int H, W;
    float black;
};

template <int V, int C>
__global__ __launch_bounds__(LT_BLOCK) void k_light_moments(MomentArgs k) {
    constexpr int N = LT_NM + LT_NB * C;
    __shared__ double lds[N][LT_WAVES];
    const int groups = (k.W + 3) >> 2;
    const int64_t items = (int64_t)k.H * groups;
    const int64_t b = blockIdx.y, plane = (int64_t)k.H * k.W;
    double acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.0;
    for (int i = 0; i < LT_ITEMS; ++i) {
        const int64_t j = ((int64_t)blockIdx.x * LT_ITEMS + i) * LT_BLOCK + threadIdx.x;
        if (j >= items) continue;
        const LtItem it = lt_item(j, k.W, groups);
        LtBasis bs[4];
        bool live[4];
        lt_stage<V>(bs, live, k.n + b * 3 * plane, nullptr, k.weight + b * plane, plane, it);
        float w[4], av[C][4];
        lt_load<V>(w, k.weight + b * plane + it.pix, it.count);
#pragma unroll
        for (int c = 0; c < C; ++c) lt_load<V>(av[c], k.a + (b * C + c) * plane + it.pix, it.count);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (!live[p]) continue;
            double wy[LT_NB];
#pragma unroll
            for (int q = 0; q < LT_NB; ++q) wy[q] = (double)w[p] * (double)bs[p].Y[q];
            int at = 0;
#pragma unroll
            for (int q = 0; q < LT_NB; ++q)
#pragma unroll
                for (int r = q; r < LT_NB; ++r, ++at) acc[at] = acc[at] + wy[q] * (double)bs[p].Y[r];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const double d = (double)(av[c][p] - k.black);
#pragma unroll
                for (int q = 0; q < LT_NB; ++q) acc[LT_NM + LT_NB * c + q] = acc[LT_NM + LT_NB * c + q] + wy[q] * d;
            }
        }
    }
    lt_block_sum<double, N>(acc, lds, k.partial + (b * gridDim.x + blockIdx.x) * N);
}

struct AttrArgs {
    float* out;            // [B, A, Th, Tw]
    const float* attr;     // [B, nv, A]
    const int64_t* tri;    // [nf, 3]
    const int32_t* face;   // [Th, Tw]
    const float* coeff;    // [Th, Tw, 3]
    int64_t nv, nf;
    int B, A, Th, Tw;
};

template <int V>
__global__ __launch_bounds__(LT_BLOCK) void k_light_texel_attr(AttrArgs a) {
    const int groups = (a.Tw + 3) >> 2;
    const int64_t item = (int64_t)blockIdx.x * LT_BLOCK + threadIdx.x;
    if (item >= (int64_t)a.Th * groups) return;
    const LtItem it = lt_item(item, a.Tw, groups);
    const int64_t plane = (int64_t)a.Th * a.Tw;
    // the map: read once per texel, shared by the batch.  A face or a vertex outside the mesh counts as empty.
    int64_t i0[4], i1[4], i2[4];
    float c0[4], c1[4], c2[4];
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        live[j] = false;
        i0[j] = i1[j] = i2[j] = 0;
        c0[j] = c1[j] = c2[j] = 0.f;
        if (j < it.count) {
            const int f = a.face[it.pix + j];
            if (f >= 0 && f < a.nf) {
                const int64_t t0 = a.tri[3 * (int64_t)f], t1 = a.tri[3 * (int64_t)f + 1], t2 = a.tri[3 * (int64_t)f + 2];
                live[j] = t0 >= 0 && t0 < a.nv && t1 >= 0 && t1 < a.nv && t2 >= 0 && t2 < a.nv;
                if (live[j]) {
                    i0[j] = t0 * a.A, i1[j] = t1 * a.A, i2[j] = t2 * a.A;
                    c0[j] = a.coeff[3 * (it.pix + j)];
                    c1[j] = a.coeff[3 * (it.pix + j) + 1];
                    c2[j] = a.coeff[3 * (it.pix + j) + 2];
                }
            }
        }
    }
    for (int b = 0; b < a.B; ++b) {
        const float* ab = a.attr + (int64_t)b * a.nv * a.A;
        for (int q = 0; q < a.A; ++q) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = live[j] ? (c0[j] * ab[i0[j] + q] + c1[j] * ab[i1[j] + q]) + c2[j] * ab[i2[j] + q] : 0.f;
            lt_store<V>(a.out + ((int64_t)b * a.A + q) * plane + it.pix, o, it.count);
        }
    }
}

bool lt_shape_ok(int64_t B, int64_t C, int64_t H, int64_t W) { return B >= 0 && C >= 1 && H >= 0 && W >= 0; }

bool lt_range_ok(int64_t B, int64_t C, int64_t H, int64_t W) {
    return B <= 65535 && C <= 65535 && H <= (1 << 20) && W <= (1 << 20) && H * ((W + 3) / 4) < (1LL << 31) * LT_BLOCK;
}

int64_t lt_partial_rows(int64_t H, int64_t W) {
    const int64_t rows = sr_ceil_div(H * ((W + 3) / 4), (int64_t)LT_BLOCK * LT_ITEMS);
    return rows < 1 ? 1 : rows;
}

bool lt_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

template <int V>
void lt_launch_bwd(int cl, dim3 grid, hipStream_t s, const BwdArgs& k) {
    switch (cl) {
        case 1: hipLaunchKernelGGL((k_light_shade_bwd<V, 1>), grid, dim3(LT_BLOCK), 0, s, k); break;
        case 2: hipLaunchKernelGGL((k_light_shade_bwd<V, 2>), grid, dim3(LT_BLOCK), 0, s, k); break;
        case 3: hipLaunchKernelGGL((k_light_shade_bwd<V, 3>), grid, dim3(LT_BLOCK), 0, s, k); break;
        default: hipLaunchKernelGGL((k_light_shade_bwd<V, 4>), grid, dim3(LT_BLOCK), 0, s, k); break;
    }
}

template <int V>
void lt_launch_moments(int c, dim3 grid, hipStream_t s, const MomentArgs& k) {
    switch (c) {
        case 1: hipLaunchKernelGGL((k_light_moments<V, 1>), grid, dim3(LT_BLOCK), 0, s, k); break;
        case 2: hipLaunchKernelGGL((k_light_moments<V, 2>), grid, dim3(LT_BLOCK), 0, s, k); break;
        case 3: hipLaunchKernelGGL((k_light_moments<V, 3>), grid, dim3(LT_BLOCK), 0, s, k); break;
        default: hipLaunchKernelGGL((k_light_moments<V, 4>), grid, dim3(LT_BLOCK), 0, s, k); break;
    }
}

}  // namespace

extern "C" int sr_light_shade_fwd(float* out, const float* a, const float* normals, const uint8_t* on, const float* gamma,
                                  int64_t B, int64_t C, int64_t Cl, int64_t H, int64_t W, float black, float floor,
                                  float background, int divide, sr_stream_t stream) {
    if (!lt_shape_ok(B, C, H, W) || (Cl != 1 && Cl != C) || (divide && !(floor > 0.f))) return SR_EINVAL;
    if (B == 0 || H == 0 || W == 0) return SR_OK;
    if (!out || !a || !normals || !on || !gamma) return SR_EINVAL;
    if (!lt_range_ok(B, C, H, W)) return SR_ERANGE;
    ShadeArgs k;
    k.out = out, k.a = a, k.n = normals, k.on = on, k.gamma = gamma;
    k.C = (int)C, k.Cl = (int)Cl, k.H = (int)H, k.W = (int)W, k.black = black, k.floor = floor, k.background = background;
    const dim3 grid((unsigned)sr_ceil_div(H * ((W + 3) / 4), LT_BLOCK), (unsigned)B);
    const bool wide = W % 4 == 0 && sr_aligned16(out) && sr_aligned16(a) && sr_aligned16(normals) && lt_aligned4(on);
    hipStream_t s = sr_stream(stream);
    if (wide && divide) hipLaunchKernelGGL((k_light_shade<4, true>), grid, dim3(LT_BLOCK), 0, s, k);
    else if (wide) hipLaunchKernelGGL((k_light_shade<4, false>), grid, dim3(LT_BLOCK), 0, s, k);
    else if (divide) hipLaunchKernelGGL((k_light_shade<1, true>), grid, dim3(LT_BLOCK), 0, s, k);
    else hipLaunchKernelGGL((k_light_shade<1, false>), grid, dim3(LT_BLOCK), 0, s, k);
    return sr_launch_status();
}

extern "C" int sr_light_shade_bwd(float* ga, float* gn, float* partial, const float* g, const float* a,
                                  const float* normals, const uint8_t* on, const float* gamma, int64_t B, int64_t C,
                                  int64_t Cl, int64_t H, int64_t W, float black, sr_stream_t stream) {
    if (!lt_shape_ok(B, C, H, W) || (Cl != 1 && Cl != C) || Cl > 4) return SR_EINVAL;
    if (B == 0 || H == 0 || W == 0) return SR_OK;
    if (!ga || !g || !a || !normals || !on || !gamma) return SR_EINVAL;
    if (!lt_range_ok(B, C, H, W)) return SR_ERANGE;
    BwdArgs k;
    k.ga = ga, k.gn = gn, k.partial = partial, k.g = g, k.a = a, k.n = normals, k.on = on, k.gamma = gamma;
    k.C = (int)C, k.H = (int)H, k.W = (int)W, k.black = black;
    const dim3 grid((unsigned)lt_partial_rows(H, W), (unsigned)B);
    const bool wide = W % 4 == 0 && sr_aligned16(ga) && sr_aligned16(g) && sr_aligned16(a) && sr_aligned16(normals) &&
                      lt_aligned4(on) && (!gn || sr_aligned16(gn));
    if (wide) lt_launch_bwd<4>((int)Cl, grid, sr_stream(stream), k);
    else lt_launch_bwd<1>((int)Cl, grid, sr_stream(stream), k);
    return sr_launch_status();
}

extern "C" int sr_light_reduce(void* out, const void* partial, int64_t B, int64_t P, int64_t n, int f64,
                               sr_stream_t stream) {
    if (B < 0 || P < 1 || n < 1) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!out || !partial || out == partial) return SR_EINVAL;
    if (B * n > (int64_t)0x7fffffff * LT_BLOCK) return SR_ERANGE;
    const dim3 grid((unsigned)sr_ceil_div(B * n, LT_BLOCK));
    if (f64)
        hipLaunchKernelGGL(k_light_reduce<double>, grid, dim3(LT_BLOCK), 0, sr_stream(stream), static_cast<double*>(out),
                           static_cast<const double*>(partial), B, P, n);
    else
        hipLaunchKernelGGL(k_light_reduce<float>, grid, dim3(LT_BLOCK), 0, sr_stream(stream), static_cast<float*>(out),
                           static_cast<const float*>(partial), B, P, n);
    return sr_launch_status();
}

extern "C" int sr_light_moments(double* partial, const float* a, const float* normals, const float* weight, int64_t B,
                                int64_t C, int64_t H, int64_t W, float black, sr_stream_t stream) {
    if (!lt_shape_ok(B, C, H, W) || C > 4) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!partial || ((H > 0 && W > 0) && (!a || !normals || !weight))) return SR_EINVAL;
    if (!lt_range_ok(B, C, H, W)) return SR_ERANGE;
    MomentArgs k;
    k.partial = partial, k.a = a, k.n = normals, k.weight = weight, k.H = (int)H, k.W = (int)W, k.black = black;
    const dim3 grid((unsigned)lt_partial_rows(H, W), (unsigned)B);
    const bool wide = W % 4 == 0 && sr_aligned16(a) && sr_aligned16(normals) && sr_aligned16(weight);
    if (wide) lt_launch_moments<4>((int)C, grid, sr_stream(stream), k);
    else lt_launch_moments<1>((int)C, grid, sr_stream(stream), k);
    return sr_launch_status();
}

extern "C" int sr_light_texel_attr(float* out, const float* attr, const int64_t* tri, const int32_t* face,
                                   const float* coeff, int64_t B, int64_t A, int64_t nv, int64_t nf, int64_t Th, int64_t Tw,
                                   sr_stream_t stream) {
    if (B < 0 || A < 1 || A > 4 || nv < 1 || nf < 1 || Th < 0 || Tw < 0) return SR_EINVAL;
    if (B == 0 || Th == 0 || Tw == 0) return SR_OK;
    if (!out || !attr || !tri || !face || !coeff) return SR_EINVAL;
    if (B > 65535 || Th > (1 << 20) || Tw > (1 << 20) || nf >= (1LL << 31) || nv >= (1LL << 40)) return SR_ERANGE;
    AttrArgs k;
    k.out = out, k.attr = attr, k.tri = tri, k.face = face, k.coeff = coeff, k.nv = nv, k.nf = nf;
    k.B = (int)B, k.A = (int)A, k.Th = (int)Th, k.Tw = (int)Tw;
    const dim3 grid((unsigned)sr_ceil_div(Th * ((Tw + 3) / 4), LT_BLOCK));
    if (Tw % 4 == 0 && sr_aligned16(out))
        hipLaunchKernelGGL(k_light_texel_attr<4>, grid, dim3(LT_BLOCK), 0, sr_stream(stream), k);
    else
        hipLaunchKernelGGL(k_light_texel_attr<1>, grid, dim3(LT_BLOCK), 0, sr_stream(stream), k);
    return sr_launch_status();
}
