// The rigid pose shared by the mesh kernels (mesh.hip), the morphable-mesh node (morph.hip) and the skinning node
// (skin.hip): pose = (yaw, pitch, roll, tx, ty, tz, log-scale) -> rot = Rz(roll) Rx(pitch) Ry(yaw) ("yxz" order of
// utils_3d.euler_mat: later axes multiply from the left) and lin = exp(log-scale) * rot, and the gradient of the four
// numbers behind them given the gradients of the two matrices.  Row-major 3x3 throughout.
#pragma once
#include <hip/hip_runtime.h>

static __device__ __forceinline__ void mat3_mul(const float* a, const float* b, float* o) {      // o = a @ b, row-major
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
static __device__ __forceinline__ void axis_mats(const float* pose, float* ry, float* rx, float* rz, float* dry, float* drx,
                                          float* drz) {
    const float c0 = cosf(pose[0]), s0 = sinf(pose[0]), c1 = cosf(pose[1]), s1 = sinf(pose[1]);
    const float c2 = cosf(pose[2]), s2 = sinf(pose[2]);
    const float y[9] = {c0, 0.f, s0, 0.f, 1.f, 0.f, -s0, 0.f, c0}, dy[9] = {-s0, 0.f, c0, 0.f, 0.f, 0.f, -c0, 0.f, -s0};
    const float x[9] = {1.f, 0.f, 0.f, 0.f, c1, -s1, 0.f, s1, c1}, dx[9] = {0.f, 0.f, 0.f, 0.f, -s1, -c1, 0.f, c1, -s1};
    const float z[9] = {c2, -s2, 0.f, s2, c2, 0.f, 0.f, 0.f, 1.f}, dz[9] = {-s2, -c2, 0.f, c2, -s2, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 9; ++i) { ry[i] = y[i]; rx[i] = x[i]; rz[i] = z[i]; dry[i] = dy[i]; drx[i] = dx[i]; drz[i] = dz[i]; }
}

// rot[9] and lin[9] of one pose[7].
static __device__ __forceinline__ void pose_fwd(const float* pose, float* lin, float* rot) {
    float ry[9], rx[9], rz[9], d0[9], d1[9], d2[9], t[9];
    axis_mats(pose, ry, rx, rz, d0, d1, d2);
    mat3_mul(rx, ry, t);
    mat3_mul(rz, t, rot);
    const float sc = expf(pose[6]);
#pragma unroll
    for (int i = 0; i < 9; ++i) lin[i] = sc * rot[i];
}

// gpose[0..2] and gpose[6] of one pose[7] from glin[9] and grot[9] (either may be NULL: zero): dL/dR = grot + exp(s) glin
// through the three derivative products, the log-scale through <glin, R>.  Entries 3..5 (the translation) are the
// caller's.
static __device__ __forceinline__ void pose_bwd(const float* pose, const float* glin, const float* grot, float* gpose) {
    float ry[9], rx[9], rz[9], dry[9], drx[9], drz[9], t[9], r[9], u[9], dm[9];
    axis_mats(pose, ry, rx, rz, dry, drx, drz);
    mat3_mul(rx, ry, t);
    mat3_mul(rz, t, r);
    const float sc = expf(pose[6]);
    float gm[9];
    float gs = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const float gl = glin ? glin[i] : 0.f;
        gm[i] = (grot ? grot[i] : 0.f) + sc * gl;
        gs += gl * r[i];
    }
    auto dot9 = [&](const float* m) {
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < 9; ++i) a += gm[i] * m[i];
        return a;
    };
    mat3_mul(rx, dry, u); mat3_mul(rz, u, dm); gpose[0] = dot9(dm);      // d/d yaw:   Rz Rx Ry'
    mat3_mul(drx, ry, u); mat3_mul(rz, u, dm); gpose[1] = dot9(dm);      // d/d pitch: Rz Rx' Ry
    mat3_mul(drz, t, dm);                      gpose[2] = dot9(dm);      // d/d roll:  Rz' Rx Ry
    gpose[6] = sc * gs;
}
