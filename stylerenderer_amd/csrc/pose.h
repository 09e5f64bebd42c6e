// Pose helpers shared by the mesh kernels (mesh.hip: sr_pose_fwd / _bwd) and the morphable-mesh node (morph.hip):
// the three axis rotations of utils_3d.euler_mat(angles, "yxz") with their derivatives, and a row-major 3x3 product.
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

