// Perceptual path length (reference ppl.py:93-178): the glue between the mapping network, the generator and the LPIPS
// trunk, as three kernels instead of the composite passes over full tensors.
//
//   k_ppl_endpoints   the latents of every pair at t and t + eps (ppl.py:14-19 `lerp`, w space; ppl.py:102-112 two-input
//                     `slerp`, z space), one wave per pair, written interleaved: row 2i at t[i], row 2i+1 at t[i] + eps
//   k_ppl_prep        generator image -> trunk input: optional crop window, optional bilinear resize
//                     (F.interpolate(mode='bilinear', align_corners=False), no antialias), the LPIPS ScalingLayer
//                     (x - shift_c) / scale_c — one lane per output pixel
//   k_lpips_pair      per pair (samples 2i, 2i+1) and layer k: sum over pixels of sum_c lin_c (f0/n0 - f1/n1)^2,
//                     n = sqrt(sum_c f^2) + 1e-10 (lpips/__init__.py:42-44 normalize_tensor + networks_basic.py:66-76),
//                     the five layers table-driven in one launch; k_lpips_pair_finish sums the partials in fixed order,
//                     divides by the pixel count, adds the layers in order and divides by eps^2 (no atomics: the same
//                     inputs give the same bits)
#include "common.h"

namespace {

// wave64 sum with the result in every lane (xor butterfly)
__device__ __forceinline__ float wave_allsum(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, SR_WAVE);
    return x;
}

constexpr int EP_WAVES = 4;

// mode 0 (w): out = (0 + a * (1 - t)) + b * t, each operation rounded to fp32 in torch's order (-ffp-contract=off)
// mode 1 (z): a^ = a / max(|a|, 1e-8), b^ likewise, w = acos(a^ . b^) (no clamp, as the reference),
//             c = sin(w (1 - t)) a^ + sin(w t) b^, out = c / max(|c|, 1e-8)
__global__ __launch_bounds__(EP_WAVES * SR_WAVE) void k_ppl_endpoints(float* __restrict__ out, const float* __restrict__ a,
                                                                      const float* __restrict__ b, int64_t in_stride,
                                                                      const float* __restrict__ t, int64_t npairs, int d,
                                                                      int mode, int n_ends, float eps) {
    const int lane = threadIdx.x & (SR_WAVE - 1);
    const int64_t pair = (int64_t)blockIdx.x * EP_WAVES + (threadIdx.x >> 6);
    if (pair >= npairs) return;
    const float* pa = a + pair * in_stride;
    const float* pb = b + pair * in_stride;
    const float t0 = t[pair];
    float ia = 1.0f, ib = 1.0f, ang = 0.0f;
    if (mode == 1) {
        float saa = 0.0f, sbb = 0.0f;
        for (int i = lane; i < d; i += SR_WAVE) {
            const float x = pa[i], y = pb[i];
            saa += x * x;
            sbb += y * y;
        }
        ia = fmaxf(sqrtf(wave_allsum(saa)), 1e-8f);
        ib = fmaxf(sqrtf(wave_allsum(sbb)), 1e-8f);
        float dot = 0.0f;
        for (int i = lane; i < d; i += SR_WAVE) dot += (pa[i] / ia) * (pb[i] / ib);
        ang = acosf(wave_allsum(dot));
    }
    for (int e = 0; e < n_ends; ++e) {
        const float te = e == 0 ? t0 : t0 + eps;
        float* o = out + (pair * n_ends + e) * (int64_t)d;
        if (mode == 0) {
            const float w0 = 1.0f - te;
            for (int i = lane; i < d; i += SR_WAVE) o[i] = (0.0f + pa[i] * w0) + pb[i] * te;
        } else {
            const float w0 = sinf(ang * (1.0f - te)), w1 = sinf(ang * te);
            float scc = 0.0f;
            for (int i = lane; i < d; i += SR_WAVE) {
                const float c = w0 * (pa[i] / ia) + w1 * (pb[i] / ib);
                scc += c * c;
            }
            const float ic = fmaxf(sqrtf(wave_allsum(scc)), 1e-8f);
            for (int i = lane; i < d; i += SR_WAVE) o[i] = (w0 * (pa[i] / ia) + w1 * (pb[i] / ib)) / ic;
        }
    }
}

// ATen's upsample_bilinear2d source index (align_corners=False, no explicit scale): src = (in/out) (dst + 0.5) - 0.5,
// clamped at 0; the second tap stays inside the map.
__device__ __forceinline__ void bilinear_src(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.0f) s = 0.0f;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = fminf(fmaxf(s - (float)i0, 0.0f), 1.0f);
    l0 = 1.0f - l1;
}

__global__ __launch_bounds__(256) void k_ppl_prep(float* __restrict__ out, const float* __restrict__ img,
                                                  const float* __restrict__ shift, const float* __restrict__ scale,
                                                  int64_t planes, int h, int w, int y0, int x0, int ch, int cw, int oh,
                                                  int ow, int resize, float sy, float sx) {
    const int64_t total = planes * oh * ow;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % ow);
        const int oy = (int)((i / ow) % oh);
        const int64_t pl = i / ((int64_t)ow * oh);
        const int c = (int)(pl % 3);
        const float* src = img + (pl * h + y0) * (int64_t)w + x0;
        float v;
        if (!resize) {
            v = src[(int64_t)oy * w + ox];
        } else {
            int r0, r1, c0, c1;
            float h0, h1, w0, w1;
            bilinear_src(oy, ch, sy, r0, r1, h0, h1);
            bilinear_src(ox, cw, sx, c0, c1, w0, w1);
            const float* p0 = src + (int64_t)r0 * w;
            const float* p1 = src + (int64_t)r1 * w;
            v = h0 * (w0 * p0[c0] + w1 * p0[c1]) + h1 * (w0 * p1[c0] + w1 * p1[c1]);
        }
        out[i] = (v - shift[c]) / scale[c];
    }
}

// A 256-thread workgroup = 64 consecutive pixels x 4 channel slices (one wave per slice: every load of a wave is 256
// contiguous bytes).  Slice sl owns channels sl, sl + 4, ...; the per-pixel sums over the slices go through LDS in a
// fixed order.  The table holds the five layers; blockIdx.x runs over the blocks of all of them, blockIdx.y over pairs.
constexpr int PB = 256, PPX = 64, PSL = 4, MAXL = 8;

struct PairLayer {
    const float* f;       // [2 npairs, c, hw]
    const float* lin;     // [c]
    int c;
    int hw;
    int blk0;             // first block of this layer
    int nblk;
};

struct PairTable {
    PairLayer l[MAXL];
    int nl;
    int total_blk;
};

__global__ __launch_bounds__(PB) void k_lpips_pair(float* __restrict__ partial, PairTable tab) {
    __shared__ float s_red[PSL][PPX];
    __shared__ float s_part[PSL];
    int k = 0;
    while (k + 1 < tab.nl && (int)blockIdx.x >= tab.l[k + 1].blk0) ++k;
    const PairLayer L = tab.l[k];
    const int px = threadIdx.x & (PPX - 1), sl = threadIdx.x / PPX;
    const int64_t pair = blockIdx.y;
    const int64_t p = (int64_t)(blockIdx.x - L.blk0) * PPX + px;
    const bool live = p < L.hw;
    const int64_t plane = (int64_t)L.c * L.hw;
    const float* f0 = L.f + 2 * pair * plane + (live ? p : 0);
    const float* f1 = f0 + plane;
    float s0 = 0.0f, s1 = 0.0f;
    for (int c = sl; c < L.c; c += PSL) {
        const float u = f0[(int64_t)c * L.hw], v = f1[(int64_t)c * L.hw];
        s0 += u * u;
        s1 += v * v;
    }
    s_red[sl][px] = s0;
    __syncthreads();
    s0 = ((s_red[0][px] + s_red[1][px]) + s_red[2][px]) + s_red[3][px];
    __syncthreads();
    s_red[sl][px] = s1;
    __syncthreads();
    s1 = ((s_red[0][px] + s_red[1][px]) + s_red[2][px]) + s_red[3][px];
    const float n0 = sqrtf(s0) + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
    float acc = 0.0f;
    for (int c = sl; c < L.c; c += PSL) {
        const float u = f0[(int64_t)c * L.hw] / n0 - f1[(int64_t)c * L.hw] / n1;
        acc += L.lin[c] * (u * u);
    }
    if (!live) acc = 0.0f;
    acc = sr_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[pair * tab.total_blk + blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

__global__ __launch_bounds__(256) void k_lpips_pair_finish(float* __restrict__ d, const float* __restrict__ partial,
                                                           PairTable tab, float div) {
    __shared__ float s_part[4];
    const int64_t pair = blockIdx.x;
    const float* part = partial + pair * tab.total_blk;
    float val = 0.0f;
    for (int k = 0; k < tab.nl; ++k) {
        float s = 0.0f;
        for (int i = threadIdx.x; i < tab.l[k].nblk; i += 256) s += part[tab.l[k].blk0 + i];   // fixed assignment
        s = sr_wave_sum(s);
        if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
        __syncthreads();
        const float layer = (((s_part[0] + s_part[1]) + s_part[2]) + s_part[3]) / (float)tab.l[k].hw;
        val = k == 0 ? layer : val + layer;
        __syncthreads();
    }
    if (threadIdx.x == 0) d[pair] = val / div;
}

bool make_table(PairTable& tab, const float* const* f, const float* const* lin, const int64_t* c, const int64_t* hw,
                int64_t nl) {
    tab.nl = (int)nl;
    int64_t blk = 0;
    for (int64_t k = 0; k < nl; ++k) {
        if (!f || !lin || !f[k] || !lin[k] || c[k] <= 0 || hw[k] <= 0) return false;
        tab.l[k].f = f[k];
        tab.l[k].lin = lin[k];
        tab.l[k].c = (int)c[k];
        tab.l[k].hw = (int)hw[k];
        tab.l[k].blk0 = (int)blk;
        tab.l[k].nblk = (int)sr_ceil_div(hw[k], PPX);
        blk += tab.l[k].nblk;
    }
    tab.total_blk = (int)blk;
    return true;
}

}  // namespace

extern "C" int sr_ppl_endpoints(float* out, const float* a, const float* b, int64_t in_stride, const float* t, int64_t npairs,
                                int64_t d, int mode, int n_ends, float eps, sr_stream_t stream) {
    if (npairs < 0 || d <= 0 || (mode != 0 && mode != 1) || (n_ends != 1 && n_ends != 2) || in_stride < d) return SR_EINVAL;
    if (npairs == 0) return SR_OK;
    if (!out || !a || !b || !t) return SR_EINVAL;
    if (d > (1 << 30) || npairs > (1LL << 36)) return SR_ERANGE;
    hipLaunchKernelGGL(k_ppl_endpoints, dim3((unsigned)sr_ceil_div(npairs, EP_WAVES)), dim3(EP_WAVES * SR_WAVE), 0,
                       sr_stream(stream), out, a, b, in_stride, t, npairs, (int)d, mode, n_ends, eps);
    return sr_launch_status();
}

extern "C" int sr_ppl_prep(float* out, const float* img, const float* shift, const float* scale, int64_t n, int64_t h,
                           int64_t w, int64_t y0, int64_t x0, int64_t ch, int64_t cw, int64_t oh, int64_t ow,
                           sr_stream_t stream) {
    if (n < 0 || h <= 0 || w <= 0 || ch <= 0 || cw <= 0 || oh <= 0 || ow <= 0 || y0 < 0 || x0 < 0 || y0 + ch > h ||
        x0 + cw > w)
        return SR_EINVAL;
    if (n == 0) return SR_OK;
    if (!out || !img || !shift || !scale) return SR_EINVAL;
    if (h > 0x7FFFFFFF || w > 0x7FFFFFFF || oh > 0x7FFFFFFF || ow > 0x7FFFFFFF) return SR_ERANGE;
    const int resize = (oh != ch || ow != cw) ? 1 : 0;
    const int64_t total = n * 3 * oh * ow;
    hipLaunchKernelGGL(k_ppl_prep, dim3(sr_stream_grid(total, 256)), dim3(256), 0, sr_stream(stream), out, img, shift, scale,
                       n * 3, (int)h, (int)w, (int)y0, (int)x0, (int)ch, (int)cw, (int)oh, (int)ow, resize,
                       (float)ch / (float)oh, (float)cw / (float)ow);
    return sr_launch_status();
}

extern "C" int64_t sr_lpips_pair_scratch_floats(int64_t npairs, int64_t n_layers, const int64_t* hw) {
    if (npairs <= 0 || n_layers <= 0 || !hw) return 1;
    int64_t blk = 0;
    for (int64_t k = 0; k < n_layers; ++k) blk += hw[k] > 0 ? sr_ceil_div(hw[k], PPX) : 0;
    return npairs * (blk > 0 ? blk : 1);
}

extern "C" int sr_lpips_pair(float* d, const float* const* f, const float* const* lin, const int64_t* c, const int64_t* hw,
                             int64_t n_layers, int64_t npairs, float div, float* scratch, sr_stream_t stream) {
    if (npairs < 0 || n_layers <= 0 || n_layers > MAXL || !c || !hw) return SR_EINVAL;
    if (npairs == 0) return SR_OK;
    if (!d || !scratch) return SR_EINVAL;
    for (int64_t k = 0; k < n_layers; ++k)
        if (c[k] > (1 << 20) || hw[k] > (1LL << 30) || 2 * npairs * c[k] * hw[k] > (1LL << 46)) return SR_ERANGE;
    if (npairs > 65535) return SR_ERANGE;
    PairTable tab;
    if (!make_table(tab, f, lin, c, hw, n_layers)) return SR_EINVAL;
    hipStream_t st = sr_stream(stream);
    hipLaunchKernelGGL(k_lpips_pair, dim3((unsigned)tab.total_blk, (unsigned)npairs), dim3(PB), 0, st, scratch, tab);
    hipLaunchKernelGGL(k_lpips_pair_finish, dim3((unsigned)npairs), dim3(256), 0, st, d, scratch, tab, div);
    return sr_launch_status();
}
