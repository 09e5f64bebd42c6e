// Global-key forward: the path for non-square images, fp64, and for few tiles or few samples (rasterize_tiled.h says
// when).  A different algorithm from the reference's CUDA kernel (op/rasterize.cu:40-83), which is racy: atomicMax on the
// depth followed by a non-atomic re-read and unordered stores of weights / ids (op/rasterize.h:143-154), launched as only
// `b` blocks on the legacy default stream.
//
//   pass 1  k_depth_keys   one lane per (sample, triangle), ~b*nf lanes (>> 256 CUs x 64): exact
//           triangle setup, bbox walk, and ONE 64-bit atomicMax per covered pixel on the packed key
//           (orderable(z) << 32) | (0xFFFFFFFE - t).  max key == "largest z, ties -> lowest
//           triangle id" == the outcome of the CPU's in-order `if (zB < z)` sweep.
//   pass 2  k_resolve      one lane per pixel: decode the winner, redo its setup with the same
//           device functions (IEEE ops, no contraction => same bits as pass 1 and as x86), write
//           ids (+ nv*batch), weights, depth and, optionally, interpolated attributes.  Every
//           pixel is written, so no pre-initialised outputs and no float atomics are needed.
//           h > w: several samples of the winner may land on the pixel; k_resolve_alias finds the one that won it.
//   fp64    a 64-bit depth cannot share a word with the id: pass 1a atomicMax(orderable(z)),
//           pass 1b atomicMin(t) among lanes whose depth equals the maximum, then pass 2.
//
//   large triangles: a lane whose bounding box exceeds BIG_BOX pixels parks its triangle in an LDS queue and
//           the whole workgroup walks such boxes together afterwards (same per-pixel arithmetic, so the same
//           bits) — one lane per triangle is right at ~1 px per triangle (a 50k-triangle face at 256^2) and
//           would serialise on a few screen-filling triangles.
#include "rasterize_keys.h"

#include "raster_layout.h"
#include "raster_math.h"

namespace {

// (also resets the gradient state of the call when there is one: the big-triangle counter, the leader table — left
// EMPTY by this path — and the state word that tells the gradient pass so: 0 = table filled but not built)
__global__ __launch_bounds__(256) void k_fill_u64(unsigned long long* p, unsigned long long v,
                                                  long long n, int* counter, int* first, long long n_first) {
    if (counter && blockIdx.x == 0 && threadIdx.x == 0) {
        *counter = 0;
        if (first) first[n_first] = 0;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
    if (first)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_first; i += stride)
            first[i] = 0x7FFFFFFF;
}
__global__ __launch_bounds__(256) void k_fill_u32(unsigned* p, unsigned v, long long n) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

// MODE 0: fp32 packed key.  MODE 1: fp64 depth max.  MODE 2: fp64 lowest id among depth-maxima.
template <typename R, int MODE>
__device__ __forceinline__ void depth_test(const Tri<R>& t, int x, int y, long long w, long long hw,
                                           bool perspective, R eps, unsigned long long* __restrict__ ks,
                                           unsigned* __restrict__ tm, unsigned ti) {
    const long long pix = x + (long long)y * w;
    if (pix >= hw) return;                  // the reference would write out of bounds (w > h)
    R c0, c1, c2, z;
    if (!shade<R>(t, x, y, perspective, eps, c0, c1, c2, z)) return;
    if (!(z == z)) return;                  // NaN never passes `zB < z`
    if (MODE == 0) {
        const unsigned long long key =
            ((unsigned long long)ord32((float)z) << 32) | (unsigned long long)(0xFFFFFFFEu - ti);
        if (key > ks[pix]) atomicMax(&ks[pix], key);
    } else if (MODE == 1) {
        const unsigned long long key = ord64((double)z);
        if (key > ks[pix]) atomicMax(&ks[pix], key);
    } else {
        const unsigned long long key = ord64((double)z);
        if (key == ks[pix] && key > key_init_f64()) atomicMin(&tm[pix], ti);
    }
}

template <typename R, int MODE>
__device__ __forceinline__ void depth_keys_body(long long b, long long nv, long long nf, long long h, long long w,
                                                bool repeat_v, bool repeat_f, bool perspective,
                                                const R* __restrict__ v, const long long* __restrict__ f,
                                                unsigned long long* __restrict__ keys, unsigned* __restrict__ tmin,
                                                int* __restrict__ big, R eps) {
    __shared__ int s_nbig;
    __shared__ int s_big[256];
    if (threadIdx.x == 0) s_nbig = 0;
    __syncthreads();
    const long long hw = h * w;
    const long long base = (long long)blockIdx.x * 256;
    {
        const long long g = base + threadIdx.x;
        if (g < b * nf) {
            const long long s = g / nf, ti = g - s * nf;
            const R* vs = repeat_v ? v : v + s * nv * 3;
            const long long* fs = repeat_f ? f : f + s * nf * 3;
            Tri<R> t;
            long long i0, i1, i2;
            if (load_tri<R>(t, vs, fs, ti, nv, i0, i1, i2) && tri_setup<R>(t, h, w, perspective, eps)) {
                const long long box = (long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1);
                if (box > BIG_BOX) {
                    s_big[atomicAdd(&s_nbig, 1)] = threadIdx.x;        // walked by the workgroup below
                    // ... and remembered for the gradient pass (list order is irrelevant: one row each)
                    if (MODE != 2 && big) big[1 + atomicAdd(big, 1)] = (int)g;
                } else {
                    for (int y = t.y0; y <= t.y1; ++y)
                        for (int x = t.x0; x <= t.x1; ++x)
                            depth_test<R, MODE>(t, x, y, w, hw, perspective, eps, keys + s * hw, tmin + s * hw,
                                                (unsigned)ti);
                }
            }
        }
    }
    __syncthreads();
    const int nbig = s_nbig;
    for (int q = 0; q < nbig; ++q) {
        const long long g = base + s_big[q];
        const long long s = g / nf, ti = g - s * nf;
        const R* vs = repeat_v ? v : v + s * nv * 3;
        const long long* fs = repeat_f ? f : f + s * nf * 3;
        Tri<R> t;
        long long i0, i1, i2;
        load_tri<R>(t, vs, fs, ti, nv, i0, i1, i2);
        tri_setup<R>(t, h, w, perspective, eps);
        const int bw = t.x1 - t.x0 + 1;
        const long long npx = (long long)bw * (t.y1 - t.y0 + 1);
        for (long long p = threadIdx.x; p < npx; p += 256) {
            const int yy = (int)(p / bw);
            depth_test<R, MODE>(t, t.x0 + (int)(p - (long long)yy * bw), t.y0 + yy, w, hw, perspective, eps,
                                keys + s * hw, tmin + s * hw, (unsigned)ti);
        }
    }
}

template <typename R, int MODE>
__global__ __launch_bounds__(256) void k_depth_keys(long long b, long long nv, long long nf,
                                                    long long h, long long w, bool repeat_v,
                                                    bool repeat_f, bool perspective,
                                                    const R* __restrict__ v,
                                                    const long long* __restrict__ f,
                                                    unsigned long long* __restrict__ keys,
                                                    unsigned* __restrict__ tmin, int* __restrict__ big,
                                                    R eps) {
    depth_keys_body<R, MODE>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v, f, keys, tmin, big, eps);
}

// ALIAS: an image with h > w, where several samples of the winning triangle may land on the pixel and the one that won
// it — the one whose depth is in the key — has to be found first (alias_winner, raster_math.h).  Uniform per launch.
template <typename R, bool ALIAS>
__device__ __forceinline__ void resolve_body(long long b, long long nv, long long nf, long long h, long long w,
                                             bool repeat_v, bool repeat_f, bool perspective, const R* __restrict__ v,
                                             const long long* __restrict__ f,
                                             const unsigned long long* __restrict__ keys,
                                             const unsigned* __restrict__ tmin, long long* __restrict__ index,
                                             R* __restrict__ coeff, R* __restrict__ zbuf, const R* __restrict__ tex,
                                             long long tex_c, R* __restrict__ attr, int* __restrict__ win, R eps,
                                             bool chw) {
    const long long hw = h * w;
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= b * hw) return;
    const long long s = g / hw, pix = g - s * hw;
    long long ti = -1;
    if (sizeof(R) == 4) {
        const unsigned long long key = keys[g];
        if (key != key_init_f32()) ti = (long long)(0xFFFFFFFEu - (unsigned)(key & 0xFFFFFFFFull));
    } else {
        const unsigned tm = tmin[g];
        if (tm != 0xFFFFFFFFu) ti = tm;
    }
    long long i0 = 0, i1 = 0, i2 = 0;
    R c0 = 0, c1 = 0, c2 = 0;
    R z = Lim<R>::lowest();
    if (ti >= 0) {
        const R* vs = repeat_v ? v : v + s * nv * 3;
        const long long* fs = repeat_f ? f : f + s * nf * 3;
        Tri<R> t;
        load_tri<R>(t, vs, fs, ti, nv, i0, i1, i2);
        tri_setup<R>(t, h, w, perspective, eps);
        const int y = (int)(pix / w), x = (int)(pix - (long long)y * w);
        if constexpr (ALIAS) {
            int sx, sy;
            alias_winner<R>(t, x, y, w, perspective, eps, sx, sy, c0, c1, c2, z);
        } else {
            shade<R>(t, x, y, perspective, eps, c0, c1, c2, z);
        }
        const long long shift = repeat_v ? 0 : nv * s;
        i0 += shift; i1 += shift; i2 += shift;
    }
    if (index) {
        index[3 * g] = i0;
        index[3 * g + 1] = i1;
        index[3 * g + 2] = i2;
    }
    if (coeff) {
        coeff[3 * g] = c0;
        coeff[3 * g + 1] = c1;
        coeff[3 * g + 2] = c2;
    }
    if (zbuf) zbuf[g] = z;
    if (win) win[g] = (int)ti;
    if (attr) {
        for (long long ch = 0; ch < tex_c; ++ch) {
            const R a0 = tex[i0 * tex_c + ch] * c0;
            const R a1 = tex[i1 * tex_c + ch] * c1;
            const R a2 = tex[i2 * tex_c + ch] * c2;
            const R s01 = a0 + a1;
            attr[chw ? (s * tex_c + ch) * hw + pix : g * tex_c + ch] = s01 + a2;     // [b,c,h,w] or [b,h,w,c]
        }
    }
}

template <typename R>
__global__ __launch_bounds__(256) void k_resolve(long long b, long long nv, long long nf, long long h,
                                                 long long w, bool repeat_v, bool repeat_f,
                                                 bool perspective, const R* __restrict__ v,
                                                 const long long* __restrict__ f,
                                                 const unsigned long long* __restrict__ keys,
                                                 const unsigned* __restrict__ tmin,
                                                 long long* __restrict__ index, R* __restrict__ coeff,
                                                 R* __restrict__ zbuf, const R* __restrict__ tex,
                                                 long long tex_c, R* __restrict__ attr,
                                                 int* __restrict__ win, R eps, bool chw) {
    resolve_body<R, false>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v, f, keys, tmin, index, coeff, zbuf, tex,
                           tex_c, attr, win, eps, chw);
}

// k_resolve for h > w (a kernel of its own: the launch knows, and k_resolve stays the code it was)
template <typename R>
__global__ __launch_bounds__(256) void k_resolve_alias(long long b, long long nv, long long nf, long long h,
                                                       long long w, bool repeat_v, bool repeat_f,
                                                       bool perspective, const R* __restrict__ v,
                                                       const long long* __restrict__ f,
                                                       const unsigned long long* __restrict__ keys,
                                                       const unsigned* __restrict__ tmin,
                                                       long long* __restrict__ index, R* __restrict__ coeff,
                                                       R* __restrict__ zbuf, const R* __restrict__ tex,
                                                       long long tex_c, R* __restrict__ attr,
                                                       int* __restrict__ win, R eps, bool chw) {
    resolve_body<R, true>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v, f, keys, tmin, index, coeff, zbuf, tex,
                          tex_c, attr, win, eps, chw);
}

__global__ __launch_bounds__(256) void k_fill_levels(const RasterLevels t, long long b, long long nf) {
    const int l = blockIdx.y;
    const long long n = b * t.res_h[l] * t.res_w[l];
    unsigned long long* p = t.keys[l];
    int* counter = t.big[l];
    int* first = (counter && t.win[l]) ? grad_state(counter, b, nf).leaders : nullptr;
    const long long n_first = b * nf;
    if (counter && blockIdx.x == 0 && threadIdx.x == 0) {
        *counter = 0;
        if (first) first[n_first] = 0;
    }
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned long long v = key_init_f32();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
    if (first)
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_first; i += stride) first[i] = 0x7FFFFFFF;
}

__global__ __launch_bounds__(256) void k_depth_keys_levels(const RasterLevels t, long long b, long long nv, long long nf,
                                                           bool repeat_v, bool repeat_f, bool perspective,
                                                           const float* __restrict__ v, const long long* __restrict__ f,
                                                           float eps) {
    const int l = blockIdx.y;
    depth_keys_body<float, 0>(b, nv, nf, t.res_h[l], t.res_w[l], repeat_v, repeat_f, perspective, v, f, t.keys[l], nullptr,
                              t.big[l], eps);
}

__global__ __launch_bounds__(256) void k_resolve_levels(const RasterLevels t, long long b, long long nv, long long nf,
                                                        bool repeat_v, bool repeat_f, bool perspective,
                                                        const float* __restrict__ v, const long long* __restrict__ f,
                                                        const float* __restrict__ tex, long long tex_c, float eps,
                                                        bool chw) {
    const int l = blockIdx.y;
    resolve_body<float, false>(b, nv, nf, t.res_h[l], t.res_w[l], repeat_v, repeat_f, perspective, v, f, t.keys[l], nullptr, nullptr,
                        nullptr, nullptr, tex, tex_c, t.attr[l], t.win[l], eps, chw);
}

}  // namespace

template <typename R>
int raster_keys_launch(const RasterForward<R>& c, void* work, hipStream_t st) {
    const long long npix = c.b * c.h * c.w;
    const KeyScratch s = key_scratch(work, npix);
    const bool is64 = sizeof(R) == 8;
    hipLaunchKernelGGL(k_fill_u64, dim3(sr_stream_grid(npix, 256)), dim3(256), 0, st, s.keys,
                       is64 ? key_init_f64() : key_init_f32(), npix, c.big,
                       (c.big && c.win) ? grad_state(c.big, c.b, c.nf).leaders : nullptr, c.b * c.nf);
    if (is64)
        hipLaunchKernelGGL(k_fill_u32, dim3(sr_stream_grid(npix, 256)), dim3(256), 0, st, s.tmin, 0xFFFFFFFFu, npix);
    const long long ntri = c.b * c.nf;
    if (ntri > 0) {
        const unsigned grid = (unsigned)sr_ceil_div(ntri, 256);
        if (!is64) {
            hipLaunchKernelGGL((k_depth_keys<R, 0>), dim3(grid), dim3(256), 0, st, c.b, c.nv, c.nf, c.h, c.w, c.repeat_v,
                               c.repeat_f, c.perspective, c.v, c.tri, s.keys, s.tmin, c.big, c.eps);
        } else {
            hipLaunchKernelGGL((k_depth_keys<R, 1>), dim3(grid), dim3(256), 0, st, c.b, c.nv, c.nf, c.h, c.w, c.repeat_v,
                               c.repeat_f, c.perspective, c.v, c.tri, s.keys, s.tmin, c.big, c.eps);
            hipLaunchKernelGGL((k_depth_keys<R, 2>), dim3(grid), dim3(256), 0, st, c.b, c.nv, c.nf, c.h, c.w, c.repeat_v,
                               c.repeat_f, c.perspective, c.v, c.tri, s.keys, s.tmin, c.big, c.eps);
        }
    }
    if (c.h > c.w)
        hipLaunchKernelGGL((k_resolve_alias<R>), dim3((unsigned)sr_ceil_div(npix, 256)), dim3(256), 0, st, c.b, c.nv, c.nf,
                           c.h, c.w, c.repeat_v, c.repeat_f, c.perspective, c.v, c.tri, s.keys, s.tmin, c.index, c.coeff,
                           c.zbuf, c.tex, c.tex_c, c.attr, c.win, c.eps, c.chw);
    else
        hipLaunchKernelGGL((k_resolve<R>), dim3((unsigned)sr_ceil_div(npix, 256)), dim3(256), 0, st, c.b, c.nv, c.nf, c.h,
                           c.w, c.repeat_v, c.repeat_f, c.perspective, c.v, c.tri, s.keys, s.tmin, c.index, c.coeff, c.zbuf,
                           c.tex, c.tex_c, c.attr, c.win, c.eps, c.chw);
    return sr_launch_status();
}
template int raster_keys_launch<float>(const RasterForward<float>&, void*, hipStream_t);
template int raster_keys_launch<double>(const RasterForward<double>&, void*, hipStream_t);

int raster_keys_levels_launch(const RasterLevels& t, const RasterForward<float>& c, long long max_pix, hipStream_t st) {
    const unsigned n = (unsigned)t.n;
    const long long fill_items = max_pix > c.b * c.nf ? max_pix : c.b * c.nf;
    hipLaunchKernelGGL(k_fill_levels, dim3(sr_stream_grid(fill_items, 256), n), dim3(256), 0, st, t, c.b, c.nf);
    if (c.b * c.nf > 0)
        hipLaunchKernelGGL(k_depth_keys_levels, dim3((unsigned)sr_ceil_div(c.b * c.nf, 256), n), dim3(256), 0, st, t, c.b,
                           c.nv, c.nf, c.repeat_v, c.repeat_f, c.perspective, c.v, c.tri, c.eps);
    // A level with h > w is resolved by k_resolve_alias, in a launch of its own (the choice stays uniform per launch and
    // k_resolve_levels the code it was): in the table k_resolve_levels gets, such a level has no rows, so its lanes
    // leave at the bounds test.  Fill and depth keys are the same for every shape.
    RasterLevels own = t;
    for (int l = 0; l < t.n; ++l)
        if (t.res_h[l] > t.res_w[l]) own.res_h[l] = 0;
    hipLaunchKernelGGL(k_resolve_levels, dim3((unsigned)sr_ceil_div(max_pix, 256), n), dim3(256), 0, st, own, c.b, c.nv, c.nf,
                       c.repeat_v, c.repeat_f, c.perspective, c.v, c.tri, c.tex, c.tex_c, c.eps, c.chw);
    for (int l = 0; l < t.n; ++l) {
        if (t.res_h[l] <= t.res_w[l]) continue;
        const long long h = t.res_h[l], w = t.res_w[l];
        hipLaunchKernelGGL((k_resolve_alias<float>), dim3((unsigned)sr_ceil_div(c.b * h * w, 256)), dim3(256), 0, st, c.b,
                           c.nv, c.nf, h, w, c.repeat_v, c.repeat_f, c.perspective, c.v, c.tri, t.keys[l], nullptr, nullptr,
                           nullptr, nullptr, c.tex, c.tex_c, t.attr[l], t.win[l], c.eps, c.chw);
    }
    return sr_launch_status();
}
