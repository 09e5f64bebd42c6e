// Host side of the rasterizer: argument validation, flag decode, path choice and the extern "C" entries of
// include/stylerenderer_amd.h, each calling one launch of rasterize_keys / rasterize_tiled / rasterize_grad; and the
// sequential host loops.  No kernel lives here.
//
// Host path: the same setup / shading functions are __host__ __device__; sr_rasterize_*_cpu_* run the
// reference's sequential loops (op/rasterize.cpp:21-95) for CPU tensors, which the reference's extension also
// accepts (op/rasterize.cpp:126-150).  Device tensors never take it.
// They share raster_math.h with the kernels, so this file keeps -ffp-contract=off.
#include <vector>

#include "raster_layout.h"
#include "raster_math.h"
#include "rasterize_grad.h"
#include "rasterize_keys.h"
#include "rasterize_tiled.h"

namespace {

// `perspective` carries the flags of a call: bit 0 = perspective projection, bit 1 (SR_RASTER_CHW) = attribute maps and
// their gradient channel-major [b, c, h, w] instead of the reference's [b, h, w, c], bit 2 (SR_RASTER_GRAD_ACC, gradient
// entries only) = add to what grad_v / grad_tex hold
struct RasterFlags {
    bool perspective, chw, accumulate;
};
inline RasterFlags raster_flags(int word) {
    return {(word & 1) != 0, (word & SR_RASTER_CHW) != 0, (word & SR_RASTER_GRAD_ACC) != 0};
}

template <typename R>
inline R abs_eps(R eps) { return eps < 0 ? -eps : eps; }

template <typename R>
int forward_impl(long long b, long long nv, long long nf, long long h, long long w, int repeat_v,
                 int repeat_f, int perspective, const R* v, const long long* tri, long long* index,
                 R* coeff, R* zbuf, R eps, const R* tex, long long tex_c, R* attr, int* win, int* big,
                 void* work, hipStream_t st) {
    if (b < 0 || nv < 0 || nf < 0 || h <= 0 || w <= 0) return SR_EINVAL;
    if (nf >= 0xFFFFFFFELL || (win && nf >= 0x7FFFFFFFLL) || (big && b * nf >= 0x7FFFFFFFLL)) return SR_ERANGE;
    if (b == 0) return SR_OK;
    if (!work || (nf > 0 && (!v || !tri))) return SR_EINVAL;
    if (attr && (!tex || tex_c <= 0)) return SR_EINVAL;
    const RasterFlags fl = raster_flags(perspective);
    const RasterForward<R> c = {b, nv, nf, h, w, repeat_v != 0, repeat_f != 0, fl.perspective, fl.chw, v, tri, index, coeff,
                                zbuf, abs_eps(eps), tex, tex_c, attr, win, big};
    if constexpr (sizeof(R) == 4) {
        if (raster_tiled_ok(b, nf, h, w)) return raster_tiled_launch(c, work, st);
    }
    return raster_keys_launch<R>(c, work, st);
}

template <typename R>
int backward_impl(long long b, long long n, long long h, long long w, int perspective, const R* v,
                  const long long* index, R* dcoeff, R eps, hipStream_t st) {
    if (b < 0 || n < 0 || h < 0 || w < 0) return SR_EINVAL;
    if (b * h * w == 0) return SR_OK;
    if (!v || !index || !dcoeff) return SR_EINVAL;
    return raster_dcoeff_launch<R>(b, n, h, w, perspective != 0, v, index, dcoeff, abs_eps(eps), st);
}

template <typename R>
int grad_impl(long long b, long long nv, long long nf, long long h, long long w, int repeat_f, int perspective,
              const R* v, const R* tex, long long tex_c, const long long* tri, const int* win, const int* big,
              const R* grad_out, const int* adj_off, const int* adj, long long off_bs, long long adj_bs,
              const int* adj_slot, R* grad_v, R* grad_tex, R eps, void* work, hipStream_t st) {
    if (b < 0 || nv < 0 || nf < 0 || h < 0 || w < 0 || tex_c <= 0) return SR_EINVAL;
    if (b == 0 || nv == 0 || (!grad_v && !grad_tex)) return SR_OK;
    if (b > 65535 || nf >= 0x7FFFFFFFLL / 3 || tex_c > 0x7FFFFFFF) return SR_ERANGE;
    if (!v || !tex || !grad_out || !adj_off || !work || (nf > 0 && (!tri || !adj || !win || !big))) return SR_EINVAL;
    if (h * w >= 0x7FFFFFFFLL || b * h * w >= 0x7FFFFFFFLL) return SR_ERANGE;
    const RasterFlags fl = raster_flags(perspective);
    const RasterGrad<R> c = {b, nv, nf, h, w, repeat_f != 0, fl.perspective, fl.chw, fl.accumulate, v, tex, tex_c, tri, win,
                             big, grad_out, adj_off, adj, off_bs, adj_bs, adj_slot, grad_v, grad_tex, abs_eps(eps)};
    return raster_grad_launch<R>(c, work, st);
}

// ---- host path: the reference's sequential loops (op/rasterize.cpp:21-67, 69-95) on the shared arithmetic ------
template <typename R>
int forward_cpu(long long b, long long nv, long long nf, long long h, long long w, int repeat_v, int repeat_f,
                int perspective, const R* v, const long long* tri, long long* index, R* coeff, R* zbuf, R eps) {
    if (b < 0 || nv < 0 || nf < 0 || h <= 0 || w <= 0) return SR_EINVAL;
    if (b == 0) return SR_OK;
    if (!index || !coeff || (nf > 0 && (!v || !tri))) return SR_EINVAL;
    eps = abs_eps(eps);
    const long long hw = h * w;
    std::vector<R> own;
    if (!zbuf) {
        own.resize((size_t)(b * hw));
        zbuf = own.data();
    }
    for (long long i = 0; i < b * hw; ++i) {
        zbuf[i] = Lim<R>::lowest();
        index[3 * i] = index[3 * i + 1] = index[3 * i + 2] = 0;
        coeff[3 * i] = coeff[3 * i + 1] = coeff[3 * i + 2] = 0;
    }
    for (long long s = 0; s < b; ++s) {
        const R* vs = repeat_v ? v : v + s * nv * 3;
        const long long* fs = repeat_f ? tri : tri + s * nf * 3;
        const long long shift = repeat_v ? 0 : nv * s;
        for (long long ti = 0; ti < nf; ++ti) {
            Tri<R> t;
            long long i0, i1, i2;
            if (!load_tri<R>(t, vs, fs, ti, nv, i0, i1, i2)) continue;
            if (!tri_setup<R>(t, h, w, perspective != 0, eps)) continue;
            for (int y = t.y0; y <= t.y1; ++y)
                for (int x = t.x0; x <= t.x1; ++x) {
                    const long long pix = x + (long long)y * w;
                    if (pix >= hw) continue;
                    R c0, c1, c2, z;
                    if (!shade<R>(t, x, y, perspective != 0, eps, c0, c1, c2, z)) continue;
                    const long long o = s * hw + pix;
                    if (zbuf[o] < z) {                     // in order: later triangles win only when nearer
                        zbuf[o] = z;
                        coeff[3 * o] = c0; coeff[3 * o + 1] = c1; coeff[3 * o + 2] = c2;
                        index[3 * o] = i0 + shift; index[3 * o + 1] = i1 + shift; index[3 * o + 2] = i2 + shift;
                    }
                }
        }
    }
    return SR_OK;
}

template <typename R>
int backward_cpu(long long b, long long n, long long h, long long w, int perspective, const R* v,
                 const long long* index, R* dcoeff, R eps) {
    if (b < 0 || n < 0 || h < 0 || w < 0) return SR_EINVAL;
    const long long hw = h * w, total = b * hw;
    if (total == 0) return SR_OK;
    if (!v || !index || !dcoeff) return SR_EINVAL;
    eps = abs_eps(eps);
    for (long long g = 0; g < total; ++g) {
        R jac[27];
        for (int l = 0; l < 27; ++l) jac[l] = 0;
        R p[9];
        long long ids[3];
        if (load_pixel_tri<R>(index, g, n * b, v, p, ids)) {
            const long long pix = g % hw;
            weight_jacobian<R>(p, (R)(pix % w), (R)(pix / w), (R)h, (R)w, jac, perspective != 0, eps);
        }
        for (int l = 0; l < 27; ++l) dcoeff[g * 27 + l] = jac[l];
    }
    return SR_OK;
}

}  // namespace

extern "C" int64_t sr_rasterize_scratch_bytes(int64_t b, int64_t nf, int64_t h, int64_t w, int is_double) {
    return forward_scratch_bytes(b, nf, h, w, is_double != 0);
}
extern "C" int64_t sr_rasterize_grad_scratch_bytes(int64_t b, int64_t nf, int64_t tex_c, int is_double) {
    (void)tex_c;                              // sized for the widest chunk: the same for every attribute width
    return is_double ? GradScratch<double>::bytes(b, nf) : GradScratch<float>::bytes(b, nf);
}
extern "C" int64_t sr_rasterize_grad_state_ints(int64_t b, int64_t nf) { return GradState::ints(b, nf); }

extern "C" int sr_rasterize_forward_f32(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w,
                                        int repeat_v, int repeat_f, int perspective, const float* v,
                                        const int64_t* tri, int64_t* index, float* coeff, float* zbuf,
                                        float eps, const float* tex, int64_t tex_c, float* attr,
                                        int32_t* win, int32_t* big, void* work, sr_stream_t stream) {
    return forward_impl<float>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v,
                               reinterpret_cast<const long long*>(tri),
                               reinterpret_cast<long long*>(index), coeff, zbuf, eps, tex, tex_c, attr,
                               win, big, work, sr_stream(stream));
}
// n levels of the same mesh in three launches (global-key path, fp32): see k_fill_levels.  A level that the per-call
// dispatcher would hand to the LDS-tiled path makes the call refuse (SR_EINVAL; sr_rasterize_levels_supported says so in
// advance) — the caller then rasterises level by level.
extern "C" int sr_rasterize_levels_supported(int n, int64_t b, int64_t nf, const int64_t* h, const int64_t* w) {
    if (n <= 0 || n > SR_RASTER_MAX_LEVELS || !h || !w || b <= 0 || b > 65535) return 0;
    for (int l = 0; l < n; ++l) {
        if (h[l] <= 0 || w[l] <= 0 || h[l] > 0x7FFFFFFF || w[l] > 0x7FFFFFFF || b * h[l] * w[l] >= 0x7FFFFFFFLL) return 0;
        if (raster_tiled_ok(b, nf, h[l], w[l])) return 0;
    }
    return 1;
}


extern "C" int sr_rasterize_forward_levels_f32(int n, int64_t b, int64_t nv, int64_t nf, const int64_t* h, const int64_t* w,
                                               int repeat_v, int repeat_f, int perspective, const float* v,
                                               const int64_t* tri, float eps, const float* tex, int64_t tex_c,
                                               float* const* attr, int32_t* const* win, int32_t* const* big,
                                               void* const* work, sr_stream_t stream) {
    if (n < 0 || b < 0 || nv < 0 || nf < 0 || tex_c <= 0) return SR_EINVAL;
    if (n == 0 || b == 0) return SR_OK;
    if (!h || !w || !attr || !work || !tex || (nf > 0 && (!v || !tri))) return SR_EINVAL;
    if (!sr_rasterize_levels_supported(n, b, nf, h, w)) return SR_EINVAL;
    RasterLevels t;
    t.n = n;
    long long max_pix = 0;
    for (int l = 0; l < n; ++l) {
        if (!attr[l] || !work[l]) return SR_EINVAL;
        const long long npix = b * h[l] * w[l];
        t.res_h[l] = (int)h[l];
        t.res_w[l] = (int)w[l];
        t.keys[l] = key_scratch(work[l], npix).keys;
        t.big[l] = (big && win && big[l] && win[l]) ? big[l] : nullptr;
        t.win[l] = (win && t.big[l]) ? win[l] : nullptr;
        t.attr[l] = attr[l];
        if (npix > max_pix) max_pix = npix;
    }
    const RasterFlags fl = raster_flags(perspective);
    const RasterForward<float> c = {b, nv, nf, 0, 0, repeat_v != 0, repeat_f != 0, fl.perspective, fl.chw, v,
                                    reinterpret_cast<const long long*>(tri), nullptr, nullptr, nullptr, abs_eps(eps), tex, tex_c,
                                    nullptr, nullptr, nullptr};
    return raster_keys_levels_launch(t, c, max_pix, sr_stream(stream));
}
// Gradient of n levels of one mesh (sr_rasterize_forward_levels_f32 / any forward that left win / big per level) in four
// launches; grad_v / grad_tex receive the SUM over the levels, added in table order.  fp32, tex_c <= 4, nf > 0, the cached
// inverse incidence table adj_slot; anything else: SR_EINVAL (the caller accumulates level by level, SR_RASTER_GRAD_ACC).
extern "C" int sr_rasterize_grad_levels_f32(int n, int64_t b, int64_t nv, int64_t nf, const int64_t* h, const int64_t* w,
                                            int repeat_f, int perspective, const float* v, const float* tex, int64_t tex_c,
                                            const int64_t* tri, const int32_t* const* win, int32_t* const* big,
                                            const float* const* grad_out, const int32_t* adj_off, const int32_t* adj,
                                            int64_t off_bstride, int64_t adj_bstride, const int32_t* adj_slot,
                                            float* grad_v, float* grad_tex, float eps, void* const* work,
                                            sr_stream_t stream) {
    if (n <= 0 || n > SR_RASTER_MAX_LEVELS || b <= 0 || nv <= 0 || nf <= 0 || tex_c <= 0 || tex_c > 4) return SR_EINVAL;
    if (!h || !w || !v || !tex || !tri || !win || !big || !grad_out || !adj_off || !adj || !adj_slot || !work ||
        (!grad_v && !grad_tex))
        return SR_EINVAL;
    if (b > 65535 || nf >= 0x7FFFFFFFLL / 3) return SR_ERANGE;
    GradLevels t;
    t.n = n;
    long long max_pix = 0;
    for (int l = 0; l < n; ++l) {
        if (h[l] <= 0 || w[l] <= 0 || !win[l] || !big[l] || !grad_out[l] || !work[l]) return SR_EINVAL;
        if (b * h[l] * w[l] >= 0x7FFFFFFFLL) return SR_ERANGE;
        const GradScratch<float> s = grad_scratch<float>(work[l], b, nf);
        t.res_h[l] = (int)h[l];
        t.res_w[l] = (int)w[l];
        t.win[l] = win[l];
        t.big[l] = big[l];
        t.grad_out[l] = grad_out[l];
        t.tg[l] = s.quad;
        t.valid[l] = s.valid;
        if (b * h[l] * w[l] > max_pix) max_pix = b * h[l] * w[l];
    }
    const RasterFlags fl = raster_flags(perspective);
    const RasterGrad<float> c = {b, nv, nf, 0, 0, repeat_f != 0, fl.perspective, fl.chw, false, v, tex, tex_c,
                                 reinterpret_cast<const long long*>(tri), nullptr, nullptr, nullptr, adj_off, adj, off_bstride,
                                 adj_bstride, adj_slot, grad_v, grad_tex, abs_eps(eps)};
    return raster_grad_levels_launch(t, c, max_pix, sr_stream(stream));
}

extern "C" int sr_rasterize_forward_f64(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w,
                                        int repeat_v, int repeat_f, int perspective, const double* v,
                                        const int64_t* tri, int64_t* index, double* coeff,
                                        double* zbuf, double eps, const double* tex, int64_t tex_c,
                                        double* attr, int32_t* win, int32_t* big, void* work,
                                        sr_stream_t stream) {
    return forward_impl<double>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v,
                                reinterpret_cast<const long long*>(tri),
                                reinterpret_cast<long long*>(index), coeff, zbuf, eps, tex, tex_c, attr,
                                win, big, work, sr_stream(stream));
}
extern "C" int sr_rasterize_backward_f32(int64_t b, int64_t n, int64_t h, int64_t w, int repeat_v,
                                         int perspective, const float* v, const int64_t* index,
                                         float* dcoeff, float eps, sr_stream_t stream) {
    (void)repeat_v;
    return backward_impl<float>(b, n, h, w, perspective, v, reinterpret_cast<const long long*>(index),
                                dcoeff, eps, sr_stream(stream));
}
extern "C" int sr_rasterize_backward_f64(int64_t b, int64_t n, int64_t h, int64_t w, int repeat_v,
                                         int perspective, const double* v, const int64_t* index,
                                         double* dcoeff, double eps, sr_stream_t stream) {
    (void)repeat_v;
    return backward_impl<double>(b, n, h, w, perspective, v, reinterpret_cast<const long long*>(index),
                                 dcoeff, eps, sr_stream(stream));
}
extern "C" int sr_rasterize_grad_f32(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_f,
                                     int perspective, const float* v, const float* tex, int64_t tex_c,
                                     const int64_t* tri, const int32_t* win, const int32_t* big,
                                     const float* grad_out,
                                     const int32_t* adj_off, const int32_t* adj, int64_t adj_off_bstride,
                                     int64_t adj_bstride, const int32_t* adj_slot, float* grad_v, float* grad_tex,
                                     float eps, void* work, sr_stream_t stream) {
    return grad_impl<float>(b, nv, nf, h, w, repeat_f, perspective, v, tex, tex_c,
                            reinterpret_cast<const long long*>(tri), win, big, grad_out, adj_off, adj,
                            adj_off_bstride, adj_bstride, adj_slot, grad_v, grad_tex, eps, work, sr_stream(stream));
}
extern "C" int sr_rasterize_grad_f64(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_f,
                                     int perspective, const double* v, const double* tex, int64_t tex_c,
                                     const int64_t* tri, const int32_t* win, const int32_t* big,
                                     const double* grad_out,
                                     const int32_t* adj_off, const int32_t* adj, int64_t adj_off_bstride,
                                     int64_t adj_bstride, const int32_t* adj_slot, double* grad_v, double* grad_tex,
                                     double eps, void* work, sr_stream_t stream) {
    return grad_impl<double>(b, nv, nf, h, w, repeat_f, perspective, v, tex, tex_c,
                             reinterpret_cast<const long long*>(tri), win, big, grad_out, adj_off, adj,
                             adj_off_bstride, adj_bstride, adj_slot, grad_v, grad_tex, eps, work, sr_stream(stream));
}
extern "C" int sr_rasterize_forward_cpu_f32(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_v,
                                            int repeat_f, int perspective, const float* v, const int64_t* tri,
                                            int64_t* index, float* coeff, float* zbuf, float eps) {
    return forward_cpu<float>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v,
                              reinterpret_cast<const long long*>(tri), reinterpret_cast<long long*>(index), coeff,
                              zbuf, eps);
}
extern "C" int sr_rasterize_forward_cpu_f64(int64_t b, int64_t nv, int64_t nf, int64_t h, int64_t w, int repeat_v,
                                            int repeat_f, int perspective, const double* v, const int64_t* tri,
                                            int64_t* index, double* coeff, double* zbuf, double eps) {
    return forward_cpu<double>(b, nv, nf, h, w, repeat_v, repeat_f, perspective, v,
                               reinterpret_cast<const long long*>(tri), reinterpret_cast<long long*>(index), coeff,
                               zbuf, eps);
}
extern "C" int sr_rasterize_backward_cpu_f32(int64_t b, int64_t n, int64_t h, int64_t w, int perspective,
                                             const float* v, const int64_t* index, float* dcoeff, float eps) {
    return backward_cpu<float>(b, n, h, w, perspective, v, reinterpret_cast<const long long*>(index), dcoeff, eps);
}
extern "C" int sr_rasterize_backward_cpu_f64(int64_t b, int64_t n, int64_t h, int64_t w, int perspective,
                                             const double* v, const int64_t* index, double* dcoeff, double eps) {
    return backward_cpu<double>(b, n, h, w, perspective, v, reinterpret_cast<const long long*>(index), dcoeff, eps);
}
