// Adaptive discriminator augmentation (reference utils_3d.py:155-188 random_apply_color, 189-349 random_apply_pose2D_img
// with pad=None, 350-359 augment; train.py:269-280 the p controller) as four device kernels that run under graph capture:
//
//   k_ada_params      one lane per sample: raw standard-normal draws -> the sample's record (SR_ADA_REC floats):
//                       [0..11]  6 doubles: source pixel = A (x, y, 1): ix = a0 x + a1 y + a2, iy = a3 x + a4 y + a5 — the flip,
//                                translation, rotation and zoom of the composite, zoom raised to the corner bound (fmax),
//                                its grid (linspace(0, W, W): step W / (W - 1), half = max(H, W) / 2) and
//                                grid_sample(align_corners=True)'s unnormalisation folded into one affine map
//                       [12..23] the 3x4 colour matrix: saturation . hue rotation . luma flip . contrast / brightness
//                       [24]     1 when the sample is augmented (select draw < p), else 0
//                     all of it evaluated in fp64; the map stays fp64 (a source coordinate near 255 in fp32 is off by up
//                     to 1.5e-5 px, which a sharp image turns into 1e-4 of output error), the rest is rounded once
//   k_ada_apply       one lane per 1 or 4 output pixels, all three channels (the colour matrix mixes them):
//                     out = C[:, :3] bilinear(img, A (x, y)) (+ C[:, 3]); zero padding; unselected samples are copied
//   k_ada_apply_grad  the adjoint in the image, as a GATHER: one lane per input pixel walks, row by row and in a fixed
//                     order, the output pixels whose bilinear footprint holds it (the preimage of the 2x2 square under A,
//                     tightened per row) — no atomics, the same bits on every run
//   k_ada_update      one lane: the ADA state machine of the eager trainer in fp64, same operation order
#include <math.h>

#include "common.h"

namespace {

constexpr int REC = SR_ADA_REC;
constexpr int NDRAW = SR_ADA_NDRAW;
constexpr int AB = 256;

struct AdaSigma {
    float pose[6];     // |sigma| of tx, ty, rotation, log-zoom; zoom mean; flip probability
    float color[5];    // |sigma| of brightness, log-contrast; luma-flip probability; |sigma| of hue, log-saturation
};

// the uniform slots carry standard normals too: u = Phi(n) is uniform on (0, 1) (one draw launch for everything)
__device__ __forceinline__ double uniform_of(float n) { return 0.5 * erfc(-(double)n * M_SQRT1_2); }

__global__ __launch_bounds__(64) void k_ada_params(float* __restrict__ rec, const float* __restrict__ draws, int64_t B,
                                                   AdaSigma sg, const double* __restrict__ p_dev, double p_host, int H,
                                                   int W) {
    const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const float* d = draws + b * NDRAW;
    float* r = rec + b * REC;
    double* ra = reinterpret_cast<double*>(r);
    // ---- pose (random_apply_pose2D_img, pad=None)
    const double tx = (double)d[0] * sg.pose[0], ty = (double)d[1] * sg.pose[1], rot = (double)d[2] * sg.pose[2];
    const double logz = (double)sg.pose[4] + (double)d[3] * sg.pose[3];
    const bool flip = uniform_of(d[4]) < (double)sg.pose[5];
    const double s = sin(rot), c = cos(rot);
    const double M = (double)(W > H ? W : H), half = M / 2.0;
    const double sx = W > 1 ? (double)W / (double)(W - 1) : 0.0, sy = H > 1 ? (double)H / (double)(H - 1) : 0.0;
    const double sgn = flip ? -1.0 : 1.0;
    // x1(x) = ax x + bx, y1(y) = ay y + by: the composite's grid after the flip and the translation
    const double ax = sgn * sx / half, bx = sgn * (-(double)W / 2.0) / half - tx;
    const double ay = -sy / half, by = ((double)H / 2.0) / half - ty;
    double f = exp(logz), fcov = 0.0;
    for (int k = 0; k < 4; ++k) {
        const double cx = ax * (double)((k & 1) ? W - 1 : 0) + bx, cy = ay * (double)((k & 2) ? H - 1 : 0) + by;
        const double rx = (c * cx + s * cy) * M / (double)W, ry = (-s * cx + c * cy) * M / (double)H;
        fcov = fmax(fcov, fmax(fabs(rx), fabs(ry)));
    }
    if (f < fcov) f = fcov;                                   // zoom-to-cover: no border shows
    const double kx = M / (double)W * (double)(W - 1) / 2.0, ky = M / (double)H * (double)(H - 1) / 2.0;
    ra[0] = kx * c * ax / f;
    ra[1] = kx * s * ay / f;
    ra[2] = kx * (c * bx + s * by) / f + (double)(W - 1) / 2.0;
    ra[3] = ky * s * ax / f;
    ra[4] = -ky * c * ay / f;
    ra[5] = -ky * (-s * bx + c * by) / f + (double)(H - 1) / 2.0;
    // ---- colour (random_apply_color): C = S . R . L . [con I | con bri 1]
    const double bri = (double)d[5] * sg.color[0], con = exp((double)d[6] * sg.color[1]);
    const double luma = uniform_of(d[7]) < (double)sg.color[2] ? 1.0 : 0.0;
    const double hue = (double)d[8] * sg.color[3], sat = exp((double)d[9] * sg.color[4]);
    double C[3][4];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) C[i][j] = j == 3 ? con * bri : (i == j ? con : 0.0);
    double T[3][3];
    // L = I - 2/3 luma J
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[i][j] = (i == j ? 1.0 : 0.0) - luma * 2.0 / 3.0;
    auto lmul = [&](const double A[3][3]) {
        double O[3][4];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) O[i][j] = A[i][0] * C[0][j] + A[i][1] * C[1][j] + A[i][2] * C[2][j];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) C[i][j] = O[i][j];
    };
    lmul(T);
    // hue: Rodrigues about (1, 1, 1) / sqrt(3) with the composite's clamp_min(1e-12) (hue = 0 gives the identity)
    const double a = hue / sqrt(3.0);
    const double theta = fmax(sqrt(3.0 * a * a), 1e-12), kk = a / theta;
    const double K[3][3] = {{0.0, -kk, kk}, {kk, 0.0, -kk}, {-kk, kk, 0.0}};
    const double st = sin(theta), ct = 1.0 - cos(theta);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double k2 = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
            T[i][j] = (i == j ? 1.0 : 0.0) + st * K[i][j] + ct * k2;
        }
    lmul(T);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[i][j] = (i == j ? sat : 0.0) + (1.0 - sat) / 3.0;
    lmul(T);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) r[12 + 4 * i + j] = (float)C[i][j];
    const double p = p_dev ? *p_dev : p_host;
    r[24] = uniform_of(d[10]) < p ? 1.0f : 0.0f;
    r[25] = r[26] = r[27] = 0.0f;
}

// source coordinates of output pixel (x, y) in fp64: the ONE expression both the forward and the adjoint evaluate
__device__ __forceinline__ void src_of(const double* A, int x, int y, double& ix, double& iy) {
    ix = fma(A[0], (double)x, fma(A[1], (double)y, A[2]));
    iy = fma(A[3], (double)x, fma(A[4], (double)y, A[5]));
}

// taps outside the map contribute 0; a coordinate off the map by a whole pixel (or not finite) samples nothing
__device__ __forceinline__ bool in_reach(double ix, double iy, int H, int W) {
    return ix > -1.0 && ix < (double)W && iy > -1.0 && iy < (double)H;
}

// the two 1-D weights of the taps floor(t) and floor(t) + 1, each rounded once from fp64
__device__ __forceinline__ void lin_weights(double t, double t0, float& w0, float& w1) {
    w0 = (float)((t0 + 1.0) - t);
    w1 = (float)(t - t0);
}

__device__ __forceinline__ void bilinear3(const float* __restrict__ src, int64_t plane, int H, int W, double ix, double iy,
                                          float v[3]) {
    v[0] = v[1] = v[2] = 0.0f;
    if (!in_reach(ix, iy, H, W)) return;
    const double x0d = floor(ix), y0d = floor(iy);
    const int x0 = (int)x0d, y0 = (int)y0d;
    float wx0, wx1, wy0, wy1;
    lin_weights(ix, x0d, wx0, wx1);
    lin_weights(iy, y0d, wy0, wy1);
    const float w[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int xi = x0 + (t & 1), yi = y0 + (t >> 1);
        if (xi < 0 || xi >= W || yi < 0 || yi >= H) continue;
        const float* p = src + (int64_t)yi * W + xi;
        v[0] = fmaf(w[t], p[0], v[0]);
        v[1] = fmaf(w[t], p[plane], v[1]);
        v[2] = fmaf(w[t], p[2 * plane], v[2]);
    }
}

// grid (ceil(plane / (AB * VEC)) capped, B): a workgroup's pixels belong to one sample, so the select branch is uniform
template <int VEC>
__global__ __launch_bounds__(AB) void k_ada_apply(float* __restrict__ out, const float* __restrict__ img,
                                                  const float* __restrict__ rec, int H, int W, int with_bias) {
    const int64_t plane = (int64_t)H * W;
    const int64_t b = blockIdx.y;
    const float* r = rec + b * REC;
    const float* src = img + b * 3 * plane;
    float* dst = out + b * 3 * plane;
    const bool sel = r[24] != 0.0f;
    double A[6];
    float C[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) A[i] = reinterpret_cast<const double*>(r)[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) C[i] = r[12 + i];
    if (!with_bias) C[3] = C[7] = C[11] = 0.0f;
    for (int64_t i0 = ((int64_t)blockIdx.x * AB + threadIdx.x) * VEC; i0 < plane; i0 += (int64_t)gridDim.x * AB * VEC) {
        if (!sel) {
            if constexpr (VEC == 4) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    *reinterpret_cast<float4*>(dst + ch * plane + i0) =
                        *reinterpret_cast<const float4*>(src + ch * plane + i0);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dst[ch * plane + i0] = src[ch * plane + i0];
            }
            continue;
        }
        float o[3][VEC];
        const int y = (int)(i0 / W), x0 = (int)(i0 - (int64_t)y * W);   // VEC = 4 only when W % 4 == 0: one row
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            double ix, iy;
            float s[3];
            src_of(A, x0 + v, y, ix, iy);
            bilinear3(src, plane, H, W, ix, iy, s);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                o[ch][v] = fmaf(C[4 * ch + 2], s[2], fmaf(C[4 * ch + 1], s[1], fmaf(C[4 * ch], s[0], C[4 * ch + 3])));
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (VEC == 4)
                *reinterpret_cast<float4*>(dst + ch * plane + i0) = make_float4(o[ch][0], o[ch][1], o[ch][2], o[ch][3]);
            else
                dst[ch * plane + i0] = o[ch][0];
        }
    }
}

// [lo, hi] of t (real) with a t + b0 in [lo_v, hi_v], widened by one pixel; |a| tiny: unconstrained
__device__ __forceinline__ void row_range(float a, float b0, float lo_v, float hi_v, float& lo, float& hi) {
    if (fabsf(a) < 1e-6f) return;
    float t0 = (lo_v - b0) / a, t1 = (hi_v - b0) / a;
    if (t0 > t1) {
        const float t = t0;
        t0 = t1;
        t1 = t;
    }
    lo = fmaxf(lo, t0 - 1.0f);
    hi = fminf(hi, t1 + 1.0f);
}

template <int VEC>
__global__ __launch_bounds__(AB) void k_ada_apply_grad(float* __restrict__ gin, const float* __restrict__ gout,
                                                       const float* __restrict__ rec, int H, int W) {
    const int64_t plane = (int64_t)H * W;
    const int64_t b = blockIdx.y;
    const float* r = rec + b * REC;
    const float* g = gout + b * 3 * plane;
    float* dst = gin + b * 3 * plane;
    const bool sel = r[24] != 0.0f;
    double Ad[6];
    float A[6], C[12];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        Ad[i] = reinterpret_cast<const double*>(r)[i];
        A[i] = (float)Ad[i];                                   // for the (widened) search box only
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) C[i] = r[12 + i];
    // inverse of the linear part (output pixel per source pixel), for the preimage box
    const float det = A[0] * A[4] - A[1] * A[3];
    const bool invertible = isfinite(det) && fabsf(det) > 1e-12f;
    const float i00 = invertible ? A[4] / det : 0.0f, i01 = invertible ? -A[1] / det : 0.0f;
    const float i10 = invertible ? -A[3] / det : 0.0f, i11 = invertible ? A[0] / det : 0.0f;
    for (int64_t i0 = ((int64_t)blockIdx.x * AB + threadIdx.x) * VEC; i0 < plane; i0 += (int64_t)gridDim.x * AB * VEC) {
        if (!sel) {
            if constexpr (VEC == 4) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    *reinterpret_cast<float4*>(dst + ch * plane + i0) = *reinterpret_cast<const float4*>(g + ch * plane + i0);
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) dst[ch * plane + i0] = g[ch * plane + i0];
            }
            continue;
        }
        float acc[3][VEC];
        const int qy = (int)(i0 / W), qx0 = (int)(i0 - (int64_t)qy * W);
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const int qx = qx0 + v;
            acc[0][v] = acc[1][v] = acc[2][v] = 0.0f;
            // output pixels with qx - 1 <= ix < qx + 1 and qy - 1 <= iy < qy + 1: the box of the square's preimage
            float xlo = 0.0f, xhi = (float)(W - 1), ylo = 0.0f, yhi = (float)(H - 1);
            if (invertible) {
                float bxl = INFINITY, bxh = -INFINITY, byl = INFINITY, byh = -INFINITY;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float u = (float)(qx + ((k & 1) ? 1 : -1)) - A[2], w = (float)(qy + ((k & 2) ? 1 : -1)) - A[5];
                    const float ox = i00 * u + i01 * w, oy = i10 * u + i11 * w;
                    bxl = fminf(bxl, ox);
                    bxh = fmaxf(bxh, ox);
                    byl = fminf(byl, oy);
                    byh = fmaxf(byh, oy);
                }
                xlo = fmaxf(xlo, bxl - 1.0f);
                xhi = fminf(xhi, bxh + 1.0f);
                ylo = fmaxf(ylo, byl - 1.0f);
                yhi = fminf(yhi, byh + 1.0f);
            }
            if (!(xlo <= xhi && ylo <= yhi)) continue;        // empty (or NaN) box: nothing maps here
            const int y_lo = (int)ceilf(ylo), y_hi = (int)floorf(yhi);
            for (int oy = y_lo; oy <= y_hi; ++oy) {
                // along the row, ix and iy are affine in ox: tighten the column range to where both can reach q
                float lo = xlo, hi = xhi;
                const float bxr = fmaf(A[1], (float)oy, A[2]), byr = fmaf(A[4], (float)oy, A[5]);
                row_range(A[0], bxr, (float)qx - 1.0f, (float)qx + 1.0f, lo, hi);
                row_range(A[3], byr, (float)qy - 1.0f, (float)qy + 1.0f, lo, hi);
                if (!(lo <= hi)) continue;
                const int x_lo = (int)ceilf(lo), x_hi = (int)floorf(hi);
                for (int ox = x_lo; ox <= x_hi; ++ox) {
                    double ix, iy;
                    src_of(Ad, ox, oy, ix, iy);
                    if (!in_reach(ix, iy, H, W)) continue;
                    const double x0d = floor(ix), y0d = floor(iy);
                    float wx0, wx1, wy0, wy1;
                    lin_weights(ix, x0d, wx0, wx1);
                    lin_weights(iy, y0d, wy0, wy1);
                    float wx, wy;
                    if (x0d == (double)qx) wx = wx0;
                    else if (x0d + 1.0 == (double)qx) wx = wx1;
                    else continue;
                    if (y0d == (double)qy) wy = wy0;
                    else if (y0d + 1.0 == (double)qy) wy = wy1;
                    else continue;
                    const float wt = wx * wy;                  // the forward's tap weight, same operands, same order
                    const int64_t o = (int64_t)oy * W + ox;
                    const float g0 = g[o], g1 = g[plane + o], g2 = g[2 * plane + o];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float h = fmaf(C[8 + k], g2, fmaf(C[4 + k], g1, C[k] * g0));
                        acc[k][v] = fmaf(wt, h, acc[k][v]);
                    }
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            if constexpr (VEC == 4)
                *reinterpret_cast<float4*>(dst + ch * plane + i0) =
                    make_float4(acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]);
            else
                dst[ch * plane + i0] = acc[ch][0];
        }
    }
}

// state = {sum sign D(real), count, p, r_t}; the eager trainer's update (train.py Trainer.step) in its operation order
__global__ void k_ada_update(double* st, const float* stat, double target, double length) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double s0 = st[0] + (double)stat[0], n = st[1] + (double)stat[1];
    if (n > 255.0) {
        const double rt = s0 / n;
        const double sign = rt > target ? 1.0 : -1.0;
        double v = st[2] + ((sign * target) / length) * n;
        v = v > 0.0 ? v : 0.0;                                 // max(0.0, v), then min(1.0, v), as Python picks them
        v = v < 1.0 ? v : 1.0;
        st[2] = v;
        st[3] = rt;
        st[0] = 0.0;
        st[1] = 0.0;
    } else {
        st[0] = s0;
        st[1] = n;
    }
}

int grid_x(int64_t plane, int vec) {
    int64_t g = sr_ceil_div(plane, (int64_t)AB * vec);
    return (int)(g > 1024 ? 1024 : g);
}

bool bad_image_size(int64_t B, int64_t H, int64_t W) { return B > 65535 || H > (1 << 24) || W > (1 << 24) || H * W > (1LL << 40); }

}  // namespace

extern "C" int sr_ada_params(float* rec, const float* draws, int64_t B, const float* pose_p, const float* color_p,
                             const double* p_dev, double p_host, int64_t H, int64_t W, sr_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!rec || !draws || !pose_p || !color_p) return SR_EINVAL;
    if (bad_image_size(B, H, W)) return SR_ERANGE;
    AdaSigma sg;
    for (int i = 0; i < 6; ++i) sg.pose[i] = fabsf(pose_p[i]);
    for (int i = 0; i < 5; ++i) sg.color[i] = fabsf(color_p[i]);
    if ((uintptr_t)rec % 8) return SR_EINVAL;                 // the record starts with six doubles
    hipLaunchKernelGGL(k_ada_params, dim3((unsigned)sr_ceil_div(B, 64)), dim3(64), 0, sr_stream(stream), rec, draws, B, sg,
                       p_dev, p_host, (int)H, (int)W);
    return sr_launch_status();
}

extern "C" int sr_ada_apply(float* out, const float* img, const float* rec, int64_t B, int64_t H, int64_t W, int with_bias,
                            sr_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0 || (with_bias != 0 && with_bias != 1)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!out || !img || !rec || out == img || (uintptr_t)rec % 8) return SR_EINVAL;
    if (bad_image_size(B, H, W)) return SR_ERANGE;
    const bool vec = W % 4 == 0 && ((uintptr_t)out | (uintptr_t)img) % 16 == 0;
    const dim3 grid((unsigned)grid_x(H * W, vec ? 4 : 1), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(k_ada_apply<4>, grid, dim3(AB), 0, sr_stream(stream), out, img, rec, (int)H, (int)W, with_bias);
    else
        hipLaunchKernelGGL(k_ada_apply<1>, grid, dim3(AB), 0, sr_stream(stream), out, img, rec, (int)H, (int)W, with_bias);
    return sr_launch_status();
}

extern "C" int sr_ada_apply_grad(float* gin, const float* gout, const float* rec, int64_t B, int64_t H, int64_t W,
                                 sr_stream_t stream) {
    if (B < 0 || H <= 0 || W <= 0) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!gin || !gout || !rec || gin == gout || (uintptr_t)rec % 8) return SR_EINVAL;
    if (bad_image_size(B, H, W)) return SR_ERANGE;
    const bool vec = W % 4 == 0 && ((uintptr_t)gin | (uintptr_t)gout) % 16 == 0;
    const dim3 grid((unsigned)grid_x(H * W, vec ? 4 : 1), (unsigned)B);
    if (vec)
        hipLaunchKernelGGL(k_ada_apply_grad<4>, grid, dim3(AB), 0, sr_stream(stream), gin, gout, rec, (int)H, (int)W);
    else
        hipLaunchKernelGGL(k_ada_apply_grad<1>, grid, dim3(AB), 0, sr_stream(stream), gin, gout, rec, (int)H, (int)W);
    return sr_launch_status();
}

extern "C" int sr_ada_update(double* state, const float* stat, double target, double length, sr_stream_t stream) {
    if (!state || !stat || !(length > 0.0)) return SR_EINVAL;
    hipLaunchKernelGGL(k_ada_update, dim3(1), dim3(64), 0, sr_stream(stream), state, stat, target, length);
    return sr_launch_status();
}
