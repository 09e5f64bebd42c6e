// The perspective camera of face reconstruction (C ABI: sr_camera_fwd / sr_camera_bwd; definition:
// stylerenderer_amd/op/camera.py).  One node between the posed mesh and everything that consumes it: per vertex (x, y, z)
// of row b, with k = kappa[b],
//     q0 = 1 - k z;  clamped = q0 < 1/16;  q = clamped ? 1/16 : q0;  v' = (x / q, y / q, z / q)
// and, for the facing gates, the normal turned by the smallest rotation that takes the ray to the camera onto +z:
//     a = (k x', k y');  len = sqrt(1 + (a.x a.x + a.y a.y));  d = (-a.x / len, -a.y / len, 1 / len)
//     c = (N.x d.x + N.y d.y) + N.z d.z;  e = (c + N.z) / (1 + d.z)
//     n_view = (N.x - e d.x, N.y - e d.y, (N.z - e (d.z + 1)) + 2 c);   k == 0: n_view = N
// Backward (n_view is a constant of it):
//     u = (x' gx' + y' gy') + z' gz';  t = u / q;  g = g' / q;  g.z += k t unless clamped;  gkappa[b] = sum_i z_i t_i
//     (a clamped vertex adds 0).
//
// Every step is one float32 operation in that order (compiled with -ffp-contract=off and correctly rounded division and
// square root), so v', n_view and gv are the host definition's bit for bit.
//
//   k_camera_fwd<V>   streaming, one launch for the batch (grid.y = row).  A row is 12 B per vertex.  V = 4: a lane owns
//                     four consecutive vertices = 48 B = three 16-byte loads and stores.  Row b starts 12 nv b bytes into
//                     the tensor, so its first h = (-nv b) mod 4 vertices and the last (nv - h) mod 4 are not part of an
//                     aligned group: those (at most 6 per row) go one per lane through the scalar form, in the same
//                     launch.  V = 1: every vertex through the scalar form (a base pointer that is not 16-byte aligned).
//   k_camera_bwd<V>   the same items; every lane writes its gv.  With gkappa, one workgroup of 1024 lanes per row: a lane
//                     adds the terms z t of its items in index order (item j, j + 1024, ...; the four vertices of a group
//                     in order), then a fixed-order LDS tree of depth 10.  No atomics: reruns are bit-identical.  Without
//                     gkappa (a fixed camera) there is nothing to reduce and the rows are spread over the grid.
//
// Vector stores and plain C++ only: no atomics, no scratch, no memset, no allocation, no host read, so both run under graph
// capture on the caller's stream.
#include "common.h"

namespace {

constexpr float CAM_QMIN = 0.0625f;
constexpr int CAM_FWD_BLOCK = 256;
constexpr int CAM_BWD_BLOCK = 1024;

// The items of row b: `groups` aligned groups of four vertices from vertex `head` on, then the head's and the tail's
// vertices one by one.
struct CamRow {
    int64_t head, groups, items;
};

template <int V>
__host__ __device__ __forceinline__ CamRow cam_row(int64_t nv, int64_t b) {
    CamRow r;
    if constexpr (V == 4) {
        r.head = (4 - (nv * b) % 4) % 4;
        if (r.head > nv) r.head = nv;
        r.groups = (nv - r.head) / 4;
        r.items = nv - 3 * r.groups;
    } else {
        r.head = 0;
        r.groups = 0;
        r.items = nv;
    }
    return r;
}

// the vertex of scalar item j >= groups
__device__ __forceinline__ int64_t cam_single(const CamRow& r, int64_t j) {
    const int64_t s = j - r.groups;
    return s < r.head ? s : s + 4 * r.groups;
}

__device__ __forceinline__ float cam_q(float k, float z, bool& clamped) {
    const float q0 = 1.f - k * z;
    clamped = q0 < CAM_QMIN;
    return clamped ? CAM_QMIN : q0;
}

__device__ __forceinline__ void cam_project(float k, const float* p, float* o) {
    bool clamped;
    const float q = cam_q(k, p[2], clamped);
    o[0] = p[0] / q;
    o[1] = p[1] / q;
    o[2] = p[2] / q;
}

__device__ __forceinline__ void cam_normal(float k, const float* vp, const float* N, float* o) {
    if (k == 0.f) {
        o[0] = N[0]; o[1] = N[1]; o[2] = N[2];
        return;
    }
    const float ax = k * vp[0], ay = k * vp[1];
    const float len = sqrtf(1.f + (ax * ax + ay * ay));
    const float dx = -ax / len, dy = -ay / len, dz = 1.f / len;
    const float c = (N[0] * dx + N[1] * dy) + N[2] * dz;
    const float e = (c + N[2]) / (1.f + dz);
    o[0] = N[0] - e * dx;
    o[1] = N[1] - e * dy;
    o[2] = (N[2] - e * (dz + 1.f)) + 2.f * c;
}

// gv of one vertex; returns its term of gkappa
__device__ __forceinline__ float cam_grad(float k, const float* p, const float* vp_in, const float* g, float* o) {
    bool clamped;
    const float q = cam_q(k, p[2], clamped);
    float vp[3];
    if (vp_in) {
        vp[0] = vp_in[0]; vp[1] = vp_in[1]; vp[2] = vp_in[2];
    } else {
        vp[0] = p[0] / q; vp[1] = p[1] / q; vp[2] = p[2] / q;
    }
    const float u = (vp[0] * g[0] + vp[1] * g[1]) + vp[2] * g[2];
    const float t = u / q;
    o[0] = g[0] / q;
    o[1] = g[1] / q;
    const float gz = g[2] / q;
    o[2] = clamped ? gz : gz + k * t;
    return clamped ? 0.f : p[2] * t;
}

__device__ __forceinline__ void cam_load12(float* o, const float* p) {
    sr_load_v<4>(o, p);
    sr_load_v<4>(o + 4, p + 4);
    sr_load_v<4>(o + 8, p + 8);
}

__device__ __forceinline__ void cam_store12(float* p, const float* a) {
    float4* q = reinterpret_cast<float4*>(p);
    q[0] = make_float4(a[0], a[1], a[2], a[3]);
    q[1] = make_float4(a[4], a[5], a[6], a[7]);
    q[2] = make_float4(a[8], a[9], a[10], a[11]);
}

template <int V>
__global__ __launch_bounds__(CAM_FWD_BLOCK) void k_camera_fwd(float* __restrict__ vp, float* __restrict__ nview,
                                                              const float* __restrict__ v, const float* __restrict__ n,
                                                              const float* __restrict__ kappa, int64_t nv) {
    const int64_t b = blockIdx.y;
    const CamRow r = cam_row<V>(nv, b);
    const int64_t j = (int64_t)blockIdx.x * CAM_FWD_BLOCK + threadIdx.x;
    if (j >= r.items) return;
    const float k = kappa[b];
    if (V == 4 && j < r.groups) {
        const int64_t off = (b * nv + r.head + 4 * j) * 3;
        float a[12], o[12];
        cam_load12(a, v + off);
#pragma unroll
        for (int i = 0; i < 4; ++i) cam_project(k, a + 3 * i, o + 3 * i);
        cam_store12(vp + off, o);
        if (nview) {
            float nn[12], w[12];
            cam_load12(nn, n + off);
#pragma unroll
            for (int i = 0; i < 4; ++i) cam_normal(k, o + 3 * i, nn + 3 * i, w + 3 * i);
            cam_store12(nview + off, w);
        }
        return;
    }
    const int64_t off = (b * nv + cam_single(r, j)) * 3;
    const float a[3] = {v[off], v[off + 1], v[off + 2]};
    float o[3];
    cam_project(k, a, o);
    vp[off] = o[0]; vp[off + 1] = o[1]; vp[off + 2] = o[2];
    if (nview) {
        const float nn[3] = {n[off], n[off + 1], n[off + 2]};
        float w[3];
        cam_normal(k, o, nn, w);
        nview[off] = w[0]; nview[off + 1] = w[1]; nview[off + 2] = w[2];
    }
}

template <int V>
__global__ __launch_bounds__(CAM_BWD_BLOCK) void k_camera_bwd(float* __restrict__ gv, float* __restrict__ gkappa,
                                                              const float* __restrict__ v, const float* __restrict__ vp,
                                                              const float* __restrict__ g, const float* __restrict__ kappa,
                                                              int64_t nv) {
    __shared__ float s[CAM_BWD_BLOCK];
    const int64_t b = blockIdx.y;
    const CamRow r = cam_row<V>(nv, b);
    const float k = kappa[b];
    float acc = 0.f;
    // (with gkappa the grid is one workgroup wide: a lane's items are j, j + 1024, ... in this order)
    for (int64_t j = (int64_t)blockIdx.x * CAM_BWD_BLOCK + threadIdx.x; j < r.items;
         j += (int64_t)gridDim.x * CAM_BWD_BLOCK) {
        if (V == 4 && j < r.groups) {
            const int64_t off = (b * nv + r.head + 4 * j) * 3;
            float a[12], gg[12], pp[12], o[12];
            cam_load12(a, v + off);
            cam_load12(gg, g + off);
            if (vp) cam_load12(pp, vp + off);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = acc + cam_grad(k, a + 3 * i, vp ? pp + 3 * i : nullptr, gg + 3 * i, o + 3 * i);
            cam_store12(gv + off, o);
        } else {
            const int64_t off = (b * nv + cam_single(r, j)) * 3;
            const float a[3] = {v[off], v[off + 1], v[off + 2]};
            const float gg[3] = {g[off], g[off + 1], g[off + 2]};
            float pp[3] = {0.f, 0.f, 0.f}, o[3];
            if (vp) { pp[0] = vp[off]; pp[1] = vp[off + 1]; pp[2] = vp[off + 2]; }
            acc = acc + cam_grad(k, a, vp ? pp : nullptr, gg, o);
            gv[off] = o[0]; gv[off + 1] = o[1]; gv[off + 2] = o[2];
        }
    }
    if (!gkappa) return;                                           // (uniform: a kernel argument)
    s[threadIdx.x] = acc;
    __syncthreads();
    for (int off = CAM_BWD_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] = s[threadIdx.x] + s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) gkappa[b] = s[0];
}

// the widest row of the batch, in items
template <int V>
int64_t cam_max_items(int64_t nv) {
    return V == 4 ? nv / 4 + 6 : nv;
}

}  // namespace

extern "C" int sr_camera_fwd(float* vp, float* nview, const float* v, const float* n, const float* kappa, int64_t B,
                             int64_t nv, sr_stream_t stream) {
    if (B < 0 || nv < 0) return SR_EINVAL;
    if (B == 0 || nv == 0) return SR_OK;
    if (!vp || !v || !kappa || ((nview != nullptr) != (n != nullptr))) return SR_EINVAL;
    if (B > 65535 || nv >= (1LL << 40)) return SR_ERANGE;
    const bool wide = sr_aligned16(vp) && sr_aligned16(v) && (!nview || (sr_aligned16(nview) && sr_aligned16(n)));
    if (wide) {
        const int64_t blocks = sr_ceil_div(cam_max_items<4>(nv), CAM_FWD_BLOCK);
        if (blocks > 0x7fffffffLL) return SR_ERANGE;
        hipLaunchKernelGGL(k_camera_fwd<4>, dim3((unsigned)blocks, (unsigned)B), dim3(CAM_FWD_BLOCK), 0, sr_stream(stream),
                           vp, nview, v, n, kappa, nv);
    } else {
        const int64_t blocks = sr_ceil_div(cam_max_items<1>(nv), CAM_FWD_BLOCK);
        if (blocks > 0x7fffffffLL) return SR_ERANGE;
        hipLaunchKernelGGL(k_camera_fwd<1>, dim3((unsigned)blocks, (unsigned)B), dim3(CAM_FWD_BLOCK), 0, sr_stream(stream),
                           vp, nview, v, n, kappa, nv);
    }
    return sr_launch_status();
}

extern "C" int sr_camera_bwd(float* gv, float* gkappa, const float* v, const float* vp, const float* g,
                             const float* kappa, int64_t B, int64_t nv, sr_stream_t stream) {
    if (B < 0 || nv < 0) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!kappa || (nv > 0 && (!gv || !v || !g))) return SR_EINVAL;
    if (B > 65535 || nv >= (1LL << 40)) return SR_ERANGE;
    const bool wide = sr_aligned16(gv) && sr_aligned16(v) && sr_aligned16(g) && (!vp || sr_aligned16(vp));
    if (nv == 0 && !gkappa) return SR_OK;
    if (wide) {
        int64_t blocks = gkappa ? 1 : sr_ceil_div(cam_max_items<4>(nv), CAM_BWD_BLOCK);
        if (blocks > 0x7fffffffLL) return SR_ERANGE;
        hipLaunchKernelGGL(k_camera_bwd<4>, dim3((unsigned)blocks, (unsigned)B), dim3(CAM_BWD_BLOCK), 0, sr_stream(stream),
                           gv, gkappa, v, vp, g, kappa, nv);
    } else {
        int64_t blocks = gkappa ? 1 : sr_ceil_div(cam_max_items<1>(nv), CAM_BWD_BLOCK);
        if (blocks > 0x7fffffffLL) return SR_ERANGE;
        hipLaunchKernelGGL(k_camera_bwd<1>, dim3((unsigned)blocks, (unsigned)B), dim3(CAM_BWD_BLOCK), 0, sr_stream(stream),
                           gv, gkappa, v, vp, g, kappa, nv);
    }
    return sr_launch_status();
}
