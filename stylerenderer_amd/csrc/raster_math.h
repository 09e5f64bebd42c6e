// The triangle arithmetic of the rasterizer, shared by every device pass and the sequential host loops: bit-exact
// against the reference's CPU loops (reference op/rasterize.cpp:21-67, arithmetic op/rasterize.h:10-228).  Everything
// here is __host__ __device__ and is evaluated with the same IEEE operations in the same order wherever it runs.
//
// Bit-exactness rules: compiled with -ffp-contract=off (x86-64 baseline has no
// FMA), correctly-rounded fp32 division (hipcc default, kept explicit in the build), f32
// subnormals preserved (hipcc default kernel mode), `x - .5` evaluated in fp32 (equal to the
// reference's double-literal form for every float input), (h, w) passed swapped into the setup
// exactly like the reference's call sites, float->int64 casts with x86 semantics.
//
// Every translation unit that includes this header is compiled with -ffp-contract=off (build.py: EXACT).
#pragma once
#include <float.h>

#include "common.h"

#define SR_HD __host__ __device__ __forceinline__

namespace {

constexpr int BIG_BOX = 64;     // bounding boxes with more pixels than this are walked by the whole workgroup

template <typename R> struct Lim;
template <> struct Lim<float> {
    static __host__ __device__ float lowest() { return -FLT_MAX; }
};
template <> struct Lim<double> {
    static __host__ __device__ double lowest() { return -DBL_MAX; }
};

// Triangle state held as named scalars (never arrays: runtime-indexed arrays would be demoted
// to scratch memory).  p*: vertices (x, y in screen space after setup, z untouched);
// e0..e2 edge constants, e3..e5 d/dx, e6..e8 d/dy; area = |signed area sum|.
template <typename R>
struct Tri {
    R p0, p1, p2, p3, p4, p5, p6, p7, p8;
    R e0, e1, e2, e3, e4, e5, e6, e7, e8;
    R area;
    int x0, x1, y0, y1;
};

// (int64_t) cast as x86-64 cvtts[sd]2si performs it: NaN / out of range -> INT64_MIN.
template <typename R>
SR_HD long long to_i64_x86(R f) {
    if (f >= (R)-9223372036854775808.0 && f < (R)9223372036854775808.0) return (long long)f;
    return (long long)0x8000000000000000ULL;
}

template <typename R> SR_HD R r_ceil(R x);
template <> SR_HD float r_ceil<float>(float x) { return ceilf(x); }
template <> SR_HD double r_ceil<double>(double x) { return ceil(x); }
template <typename R> SR_HD R r_floor(R x);
template <> SR_HD float r_floor<float>(float x) { return floorf(x); }
template <> SR_HD double r_floor<double>(double x) { return floor(x); }

// One vertex to screen space; false = rejected by the perspective near test.
template <typename R>
SR_HD bool to_screen(R& x, R& y, const R z, R sw, R sh, bool perspective, R eps) {
    if (perspective) {
        if (z >= -eps) return false;
        x = x / -z;
        y = y / -z;
    }
    const R sx = (1 + x) * sw / 2;
    const R sy = (1 - y) * sh / 2;
    x = sx - (R)0.5;
    y = sy - (R)0.5;
    return true;
}

template <typename R>
SR_HD void grow(R& lo, R& hi, R q) {
    // `if (lo > q) lo = q; else if (hi < q) hi = q;` as value selects (reference op/rasterize.h:27-34)
    const bool below = lo > q;
    const bool above = !below && (hi < q);
    lo = below ? q : lo;
    hi = above ? q : hi;
}

// Triangle setup.  sw / sh are what the reference's barycentric() receives as (w, h): the callers
// pass (h_arg, w_arg).  Returns false when the triangle is rejected.
template <typename R>
SR_HD bool tri_setup(Tri<R>& t, long long sw, long long sh, bool perspective,
                                          R eps) {
    const R fw = (R)sw, fh = (R)sh;
    if (!to_screen<R>(t.p0, t.p1, t.p2, fw, fh, perspective, eps)) return false;
    if (!to_screen<R>(t.p3, t.p4, t.p5, fw, fh, perspective, eps)) return false;
    if (!to_screen<R>(t.p6, t.p7, t.p8, fw, fh, perspective, eps)) return false;
    R lo_u = t.p0, hi_u = t.p0, lo_v = t.p1, hi_v = t.p1;
    grow<R>(lo_u, hi_u, t.p3);
    grow<R>(lo_v, hi_v, t.p4);
    grow<R>(lo_u, hi_u, t.p6);
    grow<R>(lo_v, hi_v, t.p7);
    long long x0 = to_i64_x86<R>(r_ceil<R>(lo_u)), x1 = to_i64_x86<R>(r_floor<R>(hi_u));
    long long y0 = to_i64_x86<R>(r_ceil<R>(lo_v)), y1 = to_i64_x86<R>(r_floor<R>(hi_v));
    if (x0 < 0) x0 = 0;
    if (x1 > sw - 1) x1 = sw - 1;
    if (y0 < 0) y0 = 0;
    if (y1 > sh - 1) y1 = sh - 1;
    if (x1 < x0 || y1 < y0) return false;
    t.x0 = (int)x0; t.x1 = (int)x1; t.y0 = (int)y0; t.y1 = (int)y1;

    R m0 = t.p3 * t.p7, m1 = t.p4 * t.p6;
    t.e0 = m0 - m1;
    m0 = t.p1 * t.p6; m1 = t.p0 * t.p7;
    t.e1 = m0 - m1;
    m0 = t.p0 * t.p4; m1 = t.p1 * t.p3;
    t.e2 = m0 - m1;
    R det = t.e0 + t.e1;
    det = det + t.e2;
    if (det > eps) return false;
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
    return true;
}

template <typename R>
SR_HD void edge_values(const Tri<R>& t, R px, R py, R& c0, R& c1, R& c2) {
    R gx = t.e3 * px, gy = t.e6 * py;
    R a = t.e0 + gx;
    c0 = a + gy;
    gx = t.e4 * px; gy = t.e7 * py;
    a = t.e1 + gx;
    c1 = a + gy;
    gx = t.e5 * px; gy = t.e8 * py;
    a = t.e2 + gx;
    c2 = a + gy;
}

#define SR_SEL3(a0, a1, a2, n) ((n) == 0 ? (a0) : ((n) == 1 ? (a1) : (a2)))

// Launders a value through an empty asm so that a later select between such values cannot be
// folded back into a runtime-indexed load of the triangle struct (which would force the whole
// struct into scratch memory).  Emits no instruction.
SR_HD float opaque(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}
SR_HD double opaque(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(x));
#endif
    return x;
}

// Barycentric weights from the edge values; false = pixel outside.
template <typename R>
SR_HD bool pixel_weights(const Tri<R>& t, R px, R py, R& c0, R& c1, R& c2, R eps) {
    if (c0 < -eps || c1 < -eps || c2 < -eps) return false;
    if (t.area > eps) {
        R s = c0 + c1;
        s = s + c2;
        c0 = c0 / s;
        c1 = c1 / s;
        c2 = c2 / s;
        return true;
    }
    // zero-area triangle: longest edge (segment) or a point (reference op/rasterize.h:87-121).
    const R E3 = opaque(t.e3), E4 = opaque(t.e4), E5 = opaque(t.e5);
    const R E6 = opaque(t.e6), E7 = opaque(t.e7), E8 = opaque(t.e8);
    const R P0 = opaque(t.p0), P1 = opaque(t.p1), P3 = opaque(t.p3);
    const R P4 = opaque(t.p4), P6 = opaque(t.p6), P7 = opaque(t.p7);
    R l0, l1, l2;
    {
        R a = E3 * E3, b = E6 * E6;
        l0 = a + b;
        a = E4 * E4; b = E7 * E7;
        l1 = a + b;
        a = E5 * E5; b = E8 * E8;
        l2 = a + b;
    }
    l0 = opaque(l0); l1 = opaque(l1); l2 = opaque(l2);
    int i = (l0 > l1) ? 0 : 1;
    const R li_len = (i == 0) ? l0 : l1;
    i = (li_len > l2) ? i : 2;
    const R lmax = (i == 2) ? l2 : li_len;
    const int j = (i == 2) ? 0 : i + 1, k = (j == 2) ? 0 : j + 1;
    const R e3i = SR_SEL3(E3, E4, E5, i), e6i = SR_SEL3(E6, E7, E8, i);
    R ci, cj, ck;
    bool inside;
    if (lmax > eps) {
        const R pkx = SR_SEL3(P0, P3, P6, k), pky = SR_SEL3(P1, P4, P7, k);
        const R pjx = SR_SEL3(P0, P3, P6, j), pjy = SR_SEL3(P1, P4, P7, j);
        R a = -(px - pkx) * e6i;
        R b = (py - pky) * e3i;
        const R lj = a + b;
        a = (px - pjx) * e6i;
        b = (py - pjy) * e3i;
        const R lk = a - b;
        const R li = lj + lk;
        ci = 0;
        cj = lj / li;
        ck = lk / li;
        inside = cj >= -eps && ck >= -eps;
    } else {
        const R pix_ = SR_SEL3(P0, P3, P6, i), piy_ = SR_SEL3(P1, P4, P7, i);
        ci = 1;
        cj = 0;
        ck = 0;
        const R dx = px - pix_, dy = py - piy_;
        const R a = dx * dx, b = dy * dy;
        inside = (a + b) < eps;
    }
    ci = opaque(ci); cj = opaque(cj); ck = opaque(ck);
    c0 = (i == 0) ? ci : ((j == 0) ? cj : ck);
    c1 = (i == 1) ? ci : ((j == 1) ? cj : ck);
    c2 = (i == 2) ? ci : ((j == 2) ? cj : ck);
    return inside;
}

template <typename R>
SR_HD bool pixel_depth(const Tri<R>& t, R& c0, R& c1, R& c2, bool perspective,
                                            R eps, R& z) {
    if (perspective) {
        c0 = c0 / t.p2;
        c1 = c1 / t.p5;
        c2 = c2 / t.p8;
        R s = c0 + c1;
        s = s + c2;
        if (s >= -eps) return false;
        c0 = c0 * s;
        c1 = c1 * s;
        c2 = c2 * s;
        z = s;
    } else {
        const R a = c0 * t.p2, b = c1 * t.p5, d = c2 * t.p8;
        const R s = a + b;
        z = s + d;
    }
    return true;
}

// Total order on floats as unsigned integers; -0 is folded onto +0 so that equal depths tie.
__device__ __forceinline__ unsigned ord32(float z) {
    unsigned u = __float_as_uint(z);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long ord64(double z) {
    unsigned long long u = (unsigned long long)__double_as_longlong(z);
    if (u == 0x8000000000000000ULL) u = 0ULL;
    return (u & 0x8000000000000000ULL) ? ~u : (u | 0x8000000000000000ULL);
}
__host__ __device__ inline unsigned long long key_init_f32() {
    // orderable(-FLT_MAX) = ~0xFF7FFFFF = 0x00800000
    return ((unsigned long long)0x00800000u << 32) | 0xFFFFFFFFull;
}
__host__ __device__ inline unsigned long long key_init_f64() { return 0x0010000000000000ULL; }

// Three consecutive values with ONE memory instruction (global_load_dwordx3 for fp32: element alignment is all a
// global load needs).  The gather kernels are bound by the number of divergent memory instructions a wave issues — the
// texture-address unit walks a fully divergent load one lane per cycle, whatever its width — not by bytes.
template <typename R>
SR_HD void load3(const R* __restrict__ p, R& a, R& b, R& c) {
    R q[3];
    __builtin_memcpy(q, p, 3 * sizeof(R));
    a = q[0]; b = q[1]; c = q[2];
}

template <typename R>
SR_HD bool load_tri(Tri<R>& t, const R* __restrict__ vs,
                                         const long long* __restrict__ fs, long long ti,
                                         long long nv, long long& i0, long long& i1, long long& i2) {
    i0 = fs[3 * ti];
    i1 = fs[3 * ti + 1];
    i2 = fs[3 * ti + 2];
    if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nv || i1 >= nv || i2 >= nv) return false;
    load3<R>(vs + 3 * i0, t.p0, t.p1, t.p2);
    load3<R>(vs + 3 * i1, t.p3, t.p4, t.p5);
    load3<R>(vs + 3 * i2, t.p6, t.p7, t.p8);
    return true;
}

// Weights + depth of triangle `t` at pixel (x, y); false = not covered.  The ONE per-pixel evaluation every
// pass uses (depth keys, resolve, gradient walk, host loops), so they all see the same bits.
template <typename R>
SR_HD bool shade(const Tri<R>& t, int x, int y, bool perspective, R eps, R& c0, R& c1, R& c2, R& z) {
    const R px = (R)x, py = (R)y;
    edge_values<R>(t, px, py, c0, c1, c2);
    if (!pixel_weights<R>(t, px, py, c0, c1, c2, eps)) return false;
    return pixel_depth<R>(t, c0, c1, c2, perspective, eps, z);
}

// An h x w image with h > w.  The call convention lets x span h columns and y span w rows, and sample
// (x, y) lands on buffer entry x + y w: the samples (px + k w, py - k), k = 0, 1, ..., of a triangle's box all land on
// pixel (px, py).  Among one triangle's samples on a pixel the sequential sweep keeps the largest depth and, of equal
// depths, the sample it meets first in box order — the smaller sample row, i.e. the larger k (`zB < z` is strict).
// This finds that sample of triangle `t` (set up) for pixel (px, py): where it is, and its weights and depth, from the
// same shade() every pass uses.  false (outputs untouched) = no sample of the box covers the pixel.  With w >= h no two
// samples share a pixel and nobody calls this.
template <typename R>
SR_HD bool alias_winner(const Tri<R>& t, int px, int py, long long w, bool perspective, R eps, int& sx, int& sy, R& c0,
                        R& c1, R& c2, R& z) {
    long long k = t.x1 >= px ? (t.x1 - px) / w : -1;          // the largest k with px + k w inside the box's columns
    if (k > (long long)py - t.y0) k = (long long)py - t.y0;   // ... and py - k inside its rows
    const long long k_end = py > t.y1 ? (long long)py - t.y1 : 0;
    bool found = false;
    for (; k >= k_end; --k) {                                 // descending k = box order
        const int qx = (int)(px + k * w), qy = (int)(py - k);
        if (qx < t.x0) continue;
        R a0, a1, a2, az;
        if (!shade<R>(t, qx, qy, perspective, eps, a0, a1, a2, az)) continue;
        if (!(az == az)) continue;                            // NaN never passes `zB < z`
        if (!found || az > z) {
            found = true;
            sx = qx; sy = qy;
            c0 = a0; c1 = a1; c2 = a2; z = az;
        }
    }
    return found;
}

// d(3 weights)/d(3 vertices x xyz) at one pixel (reference op/rasterize.h:169-228).  `g` = 27 values
// [weight][vertex][component]; returns false (g untouched) for a degenerate triangle.
template <typename R>
SR_HD bool weight_jacobian(const R p[9], R px, R py, R sw, R sh, R g[27],
                                                bool perspective, R eps) {
    const R u = (px * 2 - sw + 1) / sw;
    const R vv = (py * -2 + sh - 1) / sh;
    R e[9], det;
    R m0 = p[3] * p[7], m1 = p[4] * p[6];
    e[0] = m0 - m1;
    m0 = p[1] * p[6]; m1 = p[0] * p[7];
    e[1] = m0 - m1;
    m0 = p[0] * p[4]; m1 = p[1] * p[3];
    e[2] = m0 - m1;
    if (perspective) {
        if (p[2] >= -eps || p[5] >= -eps || p[8] >= -eps) return false;
        const R a = e[0] * p[2], b = e[1] * p[5], d = e[2] * p[8];
        det = a + b;
        det = det + d;
        if (det >= -eps && det <= eps) return false;
        e[0] = -e[0];
        e[1] = -e[1];
        e[2] = -e[2];
        m0 = p[4] * p[8]; m1 = p[5] * p[7]; e[3] = m0 - m1;
        m0 = p[2] * p[7]; m1 = p[1] * p[8]; e[4] = m0 - m1;
        m0 = p[1] * p[5]; m1 = p[2] * p[4]; e[5] = m0 - m1;
        m0 = p[5] * p[6]; m1 = p[3] * p[8]; e[6] = m0 - m1;
        m0 = p[0] * p[8]; m1 = p[2] * p[6]; e[7] = m0 - m1;
        m0 = p[2] * p[3]; m1 = p[0] * p[5]; e[8] = m0 - m1;
    } else {
        det = e[0] + e[1];
        det = det + e[2];
        e[3] = p[4] - p[7];
        e[4] = p[7] - p[1];
        e[5] = p[1] - p[4];
        e[6] = p[6] - p[3];
        e[7] = p[0] - p[6];
        e[8] = p[3] - p[0];
    }
    if (!(det < -eps || det > eps)) return false;
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = e[k] / det;
    R c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const R gx = e[3 + k] * u, gy = e[6 + k] * vv;
        const R a = e[k] + gx;
        c[k] = a + gy;
    }
#pragma unroll
    for (int l = 0; l < 27; ++l) {
        const int wi = l / 9, comp = (l + 1) % 3, vert = (l / 3) % 3;
        g[l] = -c[vert] * e[wi + comp * 3];
    }
    if (perspective) {
        R s = c[0] + c[1];
        s = s + c[2];
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            R tot = g[l] + g[l + 9];
            tot = tot + g[l + 18];
#pragma unroll
            for (int wi = 0; wi < 3; ++wi) {
                const R corr = c[wi] * tot / s;
                if (l % 3 == 2) g[l + wi * 9] = (-g[l + wi * 9] - corr) / s;
                else g[l + wi * 9] = (g[l + wi * 9] - corr) / s;
            }
        }
    } else {
#pragma unroll
        for (int l = 0; l < 9; ++l) g[2 + l * 3] = 0;
    }
    return true;
}

template <typename R>
SR_HD bool load_pixel_tri(const long long* __restrict__ index, long long g,
                                               long long rows, const R* __restrict__ v, R p[9],
                                               long long ids[3]) {
    ids[0] = index[3 * g];
    ids[1] = index[3 * g + 1];
    ids[2] = index[3 * g + 2];
    if (ids[0] == ids[1] || ids[0] == ids[2] || ids[1] == ids[2]) return false;
    if (ids[0] < 0 || ids[1] < 0 || ids[2] < 0 || ids[0] >= rows || ids[1] >= rows || ids[2] >= rows)
        return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = v[3 * ids[0] + k];
        p[3 + k] = v[3 * ids[1] + k];
        p[6 + k] = v[3 * ids[2] + k];
    }
    return true;
}

}  // namespace
