// Axis-angle rotations of the skinning node (skin.hip): utils_3d.rodrigues and its first-order backward, row-major 3x3
// (reference utils_3d.py:81-154).
//   R = cos(r) I + cc a a^T + sc [a]_x,   r = |a|,   sc = sin(r) / r,   cc = (1 - cos(r)) / r^2
// and for r <= eps the series sc = 1 - r^2/6, cc = 1/2 - r^2/24 (backward: dsc = -1/3 + r^2/30, dcc = -1/12 + r^2/180).
// 1 - cos(r) is taken as 2 sin^2(r/2): the same number without the cancellation of the fp32 cosine near 1.
#pragma once
#include <hip/hip_runtime.h>

struct sr_rodrigues_coef {
    float c, sc, cc, r2;
    bool small;
};

static __device__ __forceinline__ sr_rodrigues_coef rodrigues_coef(const float* a, float eps) {
    sr_rodrigues_coef k;
    k.r2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
    const float r = sqrtf(k.r2);
    k.small = r <= eps;
    if (k.small) {
        k.c = cosf(r);
        k.sc = 1.f - k.r2 / 6.f;
        k.cc = .5f - k.r2 / 24.f;
    } else {
        const float h = sinf(.5f * r);
        k.c = cosf(r);
        k.sc = sinf(r) / r;
        k.cc = 2.f * h * h / k.r2;
    }
    return k;
}

static __device__ __forceinline__ void rodrigues_fwd(const float* a, float eps, float* R) {
    const sr_rodrigues_coef k = rodrigues_coef(a, eps);
    const float x = a[0], y = a[1], z = a[2];
    R[0] = k.c + k.cc * x * x;      R[1] = k.cc * x * y - k.sc * z; R[2] = k.cc * x * z + k.sc * y;
    R[3] = k.cc * y * x + k.sc * z; R[4] = k.c + k.cc * y * y;      R[5] = k.cc * y * z - k.sc * x;
    R[6] = k.cc * z * x - k.sc * y; R[7] = k.cc * z * y + k.sc * x; R[8] = k.c + k.cc * z * z;
}

// ga[j] = sum_mn g[m][n] dR[m][n] / da[j]
static __device__ __forceinline__ void rodrigues_bwd(const float* a, float eps, const float* g, float* ga) {
    const sr_rodrigues_coef k = rodrigues_coef(a, eps);
    const float x = a[0], y = a[1], z = a[2];
    const float dcc = k.small ? -1.f / 12.f + k.r2 / 180.f : (k.sc - 2.f * k.cc) / k.r2;
    const float dsc = k.small ? -1.f / 3.f + k.r2 / 30.f : (k.c - k.sc) / k.r2;
    // dr = <g, dcc a a^T + dsc [a]_x - sc I>: the part of dR that goes through r, per unit of a
    const float gaa = (g[0] * x * x + g[4] * y * y + g[8] * z * z) + ((g[1] + g[3]) * x * y + (g[2] + g[6]) * x * z)
                      + (g[5] + g[7]) * y * z;
    const float gx = (g[7] - g[5]) * x + (g[2] - g[6]) * y + (g[3] - g[1]) * z;          // <g, [a]_x>
    const float dr = dcc * gaa + dsc * gx - k.sc * ((g[0] + g[4]) + g[8]);
    // cc * d(a a^T)/da[j] = cc * (row j + column j of g) . a
    const float s0 = (2.f * g[0] * x + (g[1] + g[3]) * y) + (g[2] + g[6]) * z;
    const float s1 = ((g[1] + g[3]) * x + 2.f * g[4] * y) + (g[5] + g[7]) * z;
    const float s2 = ((g[2] + g[6]) * x + (g[5] + g[7]) * y) + 2.f * g[8] * z;
    ga[0] = dr * x + k.cc * s0 + k.sc * (g[7] - g[5]);
    ga[1] = dr * y + k.cc * s1 + k.sc * (g[2] - g[6]);
    ga[2] = dr * z + k.cc * s2 + k.sc * (g[3] - g[1]);
}
