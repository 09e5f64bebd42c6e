// Morphable-mesh node of the face-reconstruction loop (C ABI: sr_morph_*): 3DMM coefficients and a rigid pose to the posed
// vertices and normals the rasterizer takes, and the first-order backward of that chain (reference face_model.py:71-74
// LinearMorphableModel.forward / regulation, utils_3d.py euler_mat "yxz" and mesh_point_normal).
//
//   vs[b]  = (bias + W coeff[b]).view(nv, 3)            W = fc.weight [3 nv, d] as stored (row-major)
//   v[b]   = vs[b] @ lin[b] + t[b]                      lin = exp(s) R(yaw, pitch, roll), t = pose[3:6]
//   n[b]   = normalize(vn(vs[b])) @ R[b]                (= mesh_point_normal(v[b]) up to rounding: s > 0 is uniform)
//   reg    = lam * sum_{b,k} (coeff[b,k] / sigma[k])^2
//
// The hot part is one streaming pass over W each way (42.8 MB at nv = 24 770, d = 144): the forward reads each vertex's
// three contiguous rows once for all B samples (coefficients in LDS), the coefficient gradient reads slabs of rows once
// for all B and writes per-slab partials that a second pass sums in a fixed order.  The vertex-normal backward gathers
// the cross-product adjoints of each vertex's incident faces over the same CSR lists as k_vertex_normals (mesh.hip), in
// the same fixed order and with the same wave-wide path for high-valence vertices.  No atomics anywhere: reruns are
// bit-identical.  Vector stores only.
#include "common.h"
#include "pose.h"

#define SR_MORPH_MAXB 8          // samples per register block (larger B loops over blocks, re-reading W from cache)
#define SR_MORPH_MAX_BD 8192     // coefficients held in LDS by the forward (B * d)
#define SR_MORPH_MAX_SLAB 512    // rows per slab of the coefficient gradient

namespace {

// One wave per vertex: lanes stride over the 3 d contiguous weights of its three rows (V per load), every sample's dot
// products accumulate in registers, a fixed butterfly sums the lanes, lane 0 adds the mean, applies the pose and stores.
template <int V>
__global__ __launch_bounds__(256) void k_morph_fwd(float* __restrict__ v, float* __restrict__ vs, float* __restrict__ reg,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   const float* __restrict__ coeff, const float* __restrict__ lin,
                                                   const float* __restrict__ pose, const float* __restrict__ sigma,
                                                   float lam, int B, int nv, int d) {
    extern __shared__ float sc[];                                 // [B * d]: sized by the launch, not the maximum
    for (int e = threadIdx.x; e < B * d; e += 256) sc[e] = coeff[e];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    if (reg && blockIdx.x == 0 && threadIdx.x < 64) {            // the regulariser: wave 0 of block 0, fixed order
        float a = 0.f;
        for (int e = lane; e < B * d; e += 64) {
            const float x = sigma ? sc[e] / sigma[e % d] : sc[e];
            a += x * x;
        }
        a = sr_wave_sum(a);
        if (lane == 0) reg[0] = lam * a;
    }
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nv) return;
    const int nq = 3 * d / V;
    const float* wr = w + (int64_t)i * 3 * d;
    for (int b0 = 0; b0 < B; b0 += SR_MORPH_MAXB) {
        float acc[SR_MORPH_MAXB][3];
#pragma unroll
        for (int bb = 0; bb < SR_MORPH_MAXB; ++bb) acc[bb][0] = acc[bb][1] = acc[bb][2] = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const int e = q * V;
            const int r = e / d, k = e - r * d;                  // d % V == 0: a load never straddles two rows
            float wv[V];
            sr_load_v<V>(wv, wr + e);
#pragma unroll
            for (int bb = 0; bb < SR_MORPH_MAXB; ++bb) {
                if (b0 + bb < B) {
                    const float* c = sc + (b0 + bb) * d + k;
                    float t = 0.f;
#pragma unroll
                    for (int u = 0; u < V; ++u) t += wv[u] * c[u];
                    acc[bb][0] += r == 0 ? t : 0.f;
                    acc[bb][1] += r == 1 ? t : 0.f;
                    acc[bb][2] += r == 2 ? t : 0.f;
                }
            }
        }
#pragma unroll
        for (int bb = 0; bb < SR_MORPH_MAXB; ++bb) {
            if (b0 + bb < B) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                    for (int r = 0; r < 3; ++r) acc[bb][r] += __shfl_xor(acc[bb][r], o, 64);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int bb = 0; bb < SR_MORPH_MAXB; ++bb) {
                const int b = b0 + bb;
                if (b < B) {
                    const float x = bias[3 * i] + acc[bb][0], y = bias[3 * i + 1] + acc[bb][1];
                    const float z = bias[3 * i + 2] + acc[bb][2];
                    const float* m = lin + 9 * b;
                    const float* t = pose + 7 * b + 3;
                    float* o = vs + ((int64_t)b * nv + i) * 3;
                    o[0] = x; o[1] = y; o[2] = z;
                    o = v + ((int64_t)b * nv + i) * 3;
                    o[0] = ((x * m[0] + y * m[3]) + z * m[6]) + t[0];
                    o[1] = ((x * m[1] + y * m[4]) + z * m[7]) + t[1];
                    o[2] = ((x * m[2] + y * m[5]) + z * m[8]) + t[2];
                }
            }
        }
    }
}

// ---- backward of the vertex normals (and of the pose's action on the vertices) ---------------------------------------
// out[b, i] = gv[b, i] @ lin[b]^T + sum over the incident faces f of vertex i of d<g_a, vn>/d p_i, where
//   g_ns[j] = gn[b, j] @ rot[b]^T                                   (gradient of the unposed normal)
//   g_a[j]  = (g_ns - ns (ns . g_ns)) / |a|                  |a| >= eps
//           = (g_ns - ns (ns . g_ns) / |ns|) / eps           |a| <  eps  (ns = a / eps; g_ns / eps when a = 0)
// which is the exact gradient of the composite normalize() (its clamp is pass-through), and per face (i0, i1, i2) with
// e1 = p1 - p0, e2 = p2 - p0, gf = (g_a[i0] + g_a[i1]) + g_a[i2]:
//   d/dp1 = e2 x gf,   d/dp2 = gf x e1,   d/dp0 = -(e2 x gf + gf x e1).
// g_a of a neighbour is recomputed where it is needed (seven floats read) instead of being written by a launch of its own.
__global__ __launch_bounds__(256) void k_vertex_normals_bwd(
    float* __restrict__ out, const float* __restrict__ gv, const float* __restrict__ gn, const float* __restrict__ lin,
    const float* __restrict__ rot, const float* __restrict__ v, const float* __restrict__ ns,
    const float* __restrict__ normc, const int64_t* __restrict__ tri, const int* __restrict__ adj_off,
    const int* __restrict__ adj, int nv, int nf, float eps) {
    const int vert = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    const bool live = vert < nv;
    const int64_t bo = (int64_t)b * nv;
    const float* vb = v + bo * 3;
    float r[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (rot) {
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = rot[9 * b + k];
    }
    auto grad_a = [&](int64_t j, float& x, float& y, float& z) {
        const float* q = gn + (bo + j) * 3;
        const float g0 = q[0], g1 = q[1], g2 = q[2];
        const float hx = (g0 * r[0] + g1 * r[1]) + g2 * r[2];
        const float hy = (g0 * r[3] + g1 * r[4]) + g2 * r[5];
        const float hz = (g0 * r[6] + g1 * r[7]) + g2 * r[8];
        const float* m = ns + (bo + j) * 3;
        const float nx = m[0], ny = m[1], nz = m[2];
        const float c = normc[bo + j];
        float dot = (nx * hx + ny * hy) + nz * hz;
        float den = c;
        if (c <= eps) {
            const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
            dot = len > 0.f ? dot / len : 0.f;
            den = eps;
        }
        x = (hx - nx * dot) / den;
        y = (hy - ny * dot) / den;
        z = (hz - nz * dot) / den;
    };
    auto face_adj = [&](int f, int k, float& ox, float& oy, float& oz) {
        const int64_t i0 = tri[(int64_t)f * 3], i1 = tri[(int64_t)f * 3 + 1], i2 = tri[(int64_t)f * 3 + 2];
        const float p0x = vb[i0 * 3], p0y = vb[i0 * 3 + 1], p0z = vb[i0 * 3 + 2];
        const float e1x = vb[i1 * 3] - p0x, e1y = vb[i1 * 3 + 1] - p0y, e1z = vb[i1 * 3 + 2] - p0z;
        const float e2x = vb[i2 * 3] - p0x, e2y = vb[i2 * 3 + 1] - p0y, e2z = vb[i2 * 3 + 2] - p0z;
        float ax, ay, az, bx, by, bz, cx, cy, cz;
        grad_a(i0, ax, ay, az);
        grad_a(i1, bx, by, bz);
        grad_a(i2, cx, cy, cz);
        const float gx = (ax + bx) + cx, gy = (ay + by) + cy, gz = (az + bz) + cz;
        const float ux = e2y * gz - e2z * gy, uy = e2z * gx - e2x * gz, uz = e2x * gy - e2y * gx;    // e2 x gf
        const float wx = gy * e1z - gz * e1y, wy = gz * e1x - gx * e1z, wz = gx * e1y - gy * e1x;    // gf x e1
        if (k == 1) { ox = ux; oy = uy; oz = uz; }
        else if (k == 2) { ox = wx; oy = wy; oz = wz; }
        else { ox = -(ux + wx); oy = -(uy + wy); oz = -(uz + wz); }
    };
    float ax = 0.f, ay = 0.f, az = 0.f;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int cur_k = 0;
    const int e0 = live ? adj_off[vert] : 0, e1 = live ? adj_off[vert + 1] : 0;
    const bool wide = e1 - e0 > 24;                      // the forward's split (k_vertex_normals)
    if (!wide) {
        for (int e = e0; e < e1; ++e) {
            const int idx = adj[e];
            const int k = idx / nf, f = idx - k * nf;
            if (k != cur_k) {
                ax += sx; ay += sy; az += sz;
                sx = sy = sz = 0.f;
                cur_k = k;
            }
            float ox, oy, oz;
            face_adj(f, k, ox, oy, oz);
            sx += ox; sy += oy; sz += oz;
        }
    }
    unsigned long long wm = __ballot(wide);
    const int lane = threadIdx.x & 63;
    while (wm) {
        const int src = __ffsll((long long)wm) - 1;
        wm &= wm - 1ull;
        const int we0 = __shfl(e0, src, 64), we1 = __shfl(e1, src, 64);
        float p[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
        for (int e = we0 + lane; e < we1; e += 64) {
            const int idx = adj[e];
            const int k = idx / nf, f = idx - k * nf;
            float ox, oy, oz;
            face_adj(f, k, ox, oy, oz);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk)
                if (k == kk) { p[kk][0] += ox; p[kk][1] += oy; p[kk][2] += oz; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int kk = 0; kk < 3; ++kk)
#pragma unroll
                for (int j = 0; j < 3; ++j) p[kk][j] += __shfl_down(p[kk][j], o, 64);
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
#pragma unroll
            for (int j = 0; j < 3; ++j) p[kk][j] = __shfl(p[kk][j], 0, 64);
        if (lane == src) {
            ax = (0.f + p[0][0]) + p[1][0]; ay = (0.f + p[0][1]) + p[1][1]; az = (0.f + p[0][2]) + p[1][2];
            sx = p[2][0]; sy = p[2][1]; sz = p[2][2];
        }
    }
    if (!live) return;
    ax += sx; ay += sy; az += sz;
    if (gv) {
        const float* q = gv + (bo + vert) * 3;
        const float* m = lin + 9 * b;
        const float g0 = q[0], g1 = q[1], g2 = q[2];
        ax += (g0 * m[0] + g1 * m[1]) + g2 * m[2];
        ay += (g0 * m[3] + g1 * m[4]) + g2 * m[5];
        az += (g0 * m[6] + g1 * m[7]) + g2 * m[8];
    }
    float* o = out + (bo + vert) * 3;
    o[0] = ax; o[1] = ay; o[2] = az;
}

// ---- coefficient gradient: gcoeff[b, k] = sum_j W[j, k] gvs[b, j] (+ 2 lam g_reg coeff / sigma^2) ----------------------
// Pass 1: workgroup s reads rows [s R, s R + R) of W once.  A row is d / V float-V loads wide; G = 256 / (d / V) groups
// of threads take every G-th row of the slab (one load of V columns each), the gvs values of the slab for all samples
// sit in LDS, and the groups' sums meet in LDS in group order: part[s, b, k].
template <int V>
__global__ __launch_bounds__(256) void k_morph_gcoeff_partial(float* __restrict__ part, const float* __restrict__ w,
                                                              const float* __restrict__ gvs, int B, int64_t rows, int d,
                                                              int R) {
    __shared__ float sg[SR_MORPH_MAXB * SR_MORPH_MAX_SLAB];
    __shared__ float red[256 * 4 * SR_MORPH_MAXB];
    const int t = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * R;
    const int nr = (int)(rows - j0 < R ? rows - j0 : R);
    const int dq = d / V;
    const bool grouped = dq < 256;
    const int G = grouped ? 256 / dq : 1;
    const int grp = grouped ? t / dq : 0;
    const int kq0 = grouped ? t - grp * dq : t;
    const bool act = grp < G;
    for (int b0 = 0; b0 < B; b0 += SR_MORPH_MAXB) {
        const int nb = B - b0 < SR_MORPH_MAXB ? B - b0 : SR_MORPH_MAXB;
        __syncthreads();                                 // previous block of samples done with sg / red
        for (int e = t; e < nb * nr; e += 256) {
            const int bb = e / nr, jj = e - bb * nr;
            sg[bb * SR_MORPH_MAX_SLAB + jj] = gvs[(int64_t)(b0 + bb) * rows + j0 + jj];
        }
        __syncthreads();
        if (act) {
            for (int kq = kq0; kq < dq; kq += (grouped ? dq : 256)) {
                float acc[SR_MORPH_MAXB][V];
#pragma unroll
                for (int bb = 0; bb < SR_MORPH_MAXB; ++bb)
#pragma unroll
                    for (int u = 0; u < V; ++u) acc[bb][u] = 0.f;
#pragma unroll 4
                for (int jj = grp; jj < nr; jj += G) {
                    float wv[V];
                    sr_load_v<V>(wv, w + (j0 + jj) * d + kq * V);
#pragma unroll
                    for (int bb = 0; bb < SR_MORPH_MAXB; ++bb) {
                        if (bb < nb) {
                            const float g = sg[bb * SR_MORPH_MAX_SLAB + jj];
#pragma unroll
                            for (int u = 0; u < V; ++u) acc[bb][u] += wv[u] * g;
                        }
                    }
                }
#pragma unroll
                for (int bb = 0; bb < SR_MORPH_MAXB; ++bb) {
                    if (bb < nb) {
#pragma unroll
                        for (int u = 0; u < V; ++u) {
                            if (grouped) red[((grp * dq + kq) * V + u) * SR_MORPH_MAXB + bb] = acc[bb][u];
                            else part[((int64_t)blockIdx.x * B + b0 + bb) * d + kq * V + u] = acc[bb][u];
                        }
                    }
                }
            }
        }
        if (grouped) {
            __syncthreads();
            if (t < dq) {
                for (int bb = 0; bb < nb; ++bb)
#pragma unroll
                    for (int u = 0; u < V; ++u) {
                        float s = 0.f;
                        for (int g = 0; g < G; ++g) s += red[((g * dq + t) * V + u) * SR_MORPH_MAXB + bb];
                        part[((int64_t)blockIdx.x * B + b0 + bb) * d + t * V + u] = s;
                    }
            }
        }
    }
}

// Pass 2: one wave per output (b, k); lanes take slabs s = lane, lane + 64, ... in order, then a fixed shuffle tree.
__global__ __launch_bounds__(256) void k_morph_gcoeff_reduce(float* __restrict__ gcoeff, const float* __restrict__ part,
                                                             const float* __restrict__ coeff,
                                                             const float* __restrict__ sigma, float lam,
                                                             const float* __restrict__ greg, int S, int B, int d) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= B * d) return;
    float a = 0.f;
    for (int s = lane; s < S; s += 64) a += part[(int64_t)s * B * d + o];
    a = sr_wave_sum(a);
    if (lane == 0) {
        if (greg && lam != 0.f) {
            const float sg = sigma ? sigma[o % d] : 1.f;
            a += (2.f * lam * greg[0]) * (coeff[o] / sg) / sg;
        }
        gcoeff[o] = a;
    }
}

// Pose gradient of a batch (pose.h's pose_bwd; as k_pose_bwd in mesh.hip up to that file's rounding: it is compiled without
// floating-point contraction), with the translation's gradient gt (NULL: zero), one lane per sample.
__global__ void k_morph_pose_bwd(float* __restrict__ gpose, const float* __restrict__ glin,
                                 const float* __restrict__ grot, const float* __restrict__ gt,
                                 const float* __restrict__ pose, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float* o = gpose + 7 * b;
    pose_bwd(pose + 7 * b, glin ? glin + 9 * b : nullptr, grot ? grot + 9 * b : nullptr, o);
    o[3] = gt ? gt[3 * b] : 0.f;
    o[4] = gt ? gt[3 * b + 1] : 0.f;
    o[5] = gt ? gt[3 * b + 2] : 0.f;
}

int slab_rows(int64_t d) {
    // ~64 KB of W per workgroup (112 rows at d = 144: ~670 workgroups for the face-sized model), whole thread groups
    const int64_t dq = d % 4 == 0 ? d / 4 : d;
    const int64_t G = dq < 256 ? 256 / dq : 1;
    int64_t r = 16384 / (d > 0 ? d : 1);
    r = r < G ? G : (r / G) * G;
    if (r > SR_MORPH_MAX_SLAB) r = (SR_MORPH_MAX_SLAB / G) * G;
    return (int)(r < 1 ? 1 : r);
}

}  // namespace

extern "C" int sr_morph_fwd(float* v, float* vs, float* reg, const float* w, const float* bias, const float* coeff,
                            const float* lin, const float* pose, const float* sigma, float lam, int64_t B, int64_t nv,
                            int64_t d, sr_stream_t stream) {
    if (B < 0 || nv < 0 || d < 0) return SR_EINVAL;
    if (B == 0 || nv == 0) return SR_OK;
    if (!v || !vs || !bias || !lin || !pose || (d > 0 && (!w || !coeff))) return SR_EINVAL;
    if (B * d > SR_MORPH_MAX_BD || nv >= (1LL << 30) || d >= (1LL << 20)) return SR_ERANGE;
    const int64_t blocks = sr_ceil_div(nv, 4);
    if (blocks > 0x7fffffff) return SR_ERANGE;
    const bool vec = d % 4 == 0 && sr_aligned16(w);
    const size_t lds = (size_t)(B * d > 0 ? B * d : 1) * sizeof(float);
    if (vec)
        hipLaunchKernelGGL(k_morph_fwd<4>, dim3((unsigned)blocks), dim3(256), lds, sr_stream(stream), v, vs, reg, w,
                           bias, coeff, lin, pose, sigma, lam, (int)B, (int)nv, (int)d);
    else
        hipLaunchKernelGGL(k_morph_fwd<1>, dim3((unsigned)blocks), dim3(256), lds, sr_stream(stream), v, vs, reg, w,
                           bias, coeff, lin, pose, sigma, lam, (int)B, (int)nv, (int)d);
    return sr_launch_status();
}

extern "C" int sr_vertex_normals_bwd_f32(float* gvs, const float* gv, const float* gn, const float* lin,
                                         const float* rot, const float* v, const float* ns, const float* normc,
                                         const int64_t* tri, const int32_t* adj_off, const int32_t* adj, int64_t B,
                                         int64_t nv, int64_t nf, float eps, sr_stream_t stream) {
    if (B < 0 || nv < 0 || nf < 0) return SR_EINVAL;
    if (B == 0 || nv == 0) return SR_OK;
    if (!gvs || !gn || !v || !ns || !normc || !adj_off || (gv && !lin) || (nf > 0 && (!tri || !adj)))
        return SR_EINVAL;
    if (B > 65535 || nv >= (1LL << 30) || 3 * nf >= (1LL << 31)) return SR_ERANGE;
    hipLaunchKernelGGL(k_vertex_normals_bwd, dim3((unsigned)sr_ceil_div(nv, 256), (unsigned)B), dim3(256), 0,
                       sr_stream(stream), gvs, gv, gn, lin, rot, v, ns, normc, tri, adj_off, adj, (int)nv,
                       (int)(nf > 0 ? nf : 1), eps);
    return sr_launch_status();
}

extern "C" int64_t sr_morph_gcoeff_scratch_floats(int64_t rows, int64_t B, int64_t d) {
    if (rows <= 0 || B <= 0 || d <= 0) return 0;
    return sr_ceil_div(rows, slab_rows(d)) * B * d;
}

extern "C" int sr_morph_gcoeff(float* gcoeff, float* scratch, const float* w, const float* gvs, const float* coeff,
                               const float* sigma, float lam, const float* greg, int64_t B, int64_t rows, int64_t d,
                               sr_stream_t stream) {
    if (B < 0 || rows < 0 || d < 0) return SR_EINVAL;
    if (B == 0 || d == 0) return SR_OK;
    if (!gcoeff || !coeff) return SR_EINVAL;
    if (rows > 0 && (!scratch || !w || !gvs)) return SR_EINVAL;
    if (rows >= (1LL << 31) || d >= (1LL << 20) || B * d >= (1LL << 31)) return SR_ERANGE;
    const int R = slab_rows(d);
    const int64_t S = rows > 0 ? sr_ceil_div(rows, R) : 0;
    if (S > 0x7fffffff) return SR_ERANGE;
    if (S > 0) {
        const bool vec = d % 4 == 0 && sr_aligned16(w);
        if (vec)
            hipLaunchKernelGGL(k_morph_gcoeff_partial<4>, dim3((unsigned)S), dim3(256), 0, sr_stream(stream), scratch,
                               w, gvs, (int)B, rows, (int)d, R);
        else
            hipLaunchKernelGGL(k_morph_gcoeff_partial<1>, dim3((unsigned)S), dim3(256), 0, sr_stream(stream), scratch,
                               w, gvs, (int)B, rows, (int)d, R);
        const int rc = sr_launch_status();
        if (rc != SR_OK) return rc;
    }
    hipLaunchKernelGGL(k_morph_gcoeff_reduce, dim3((unsigned)sr_ceil_div(B * d, 4)), dim3(256), 0, sr_stream(stream),
                       gcoeff, scratch, coeff, sigma, lam, greg, (int)S, (int)B, (int)d);
    return sr_launch_status();
}

extern "C" int sr_morph_pose_bwd(float* gpose, const float* glin, const float* grot, const float* gt, const float* pose,
                                 int64_t B, sr_stream_t stream) {
    if (B < 0) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!gpose || !pose) return SR_EINVAL;
    if (B > (1 << 24)) return SR_ERANGE;
    hipLaunchKernelGGL(k_morph_pose_bwd, dim3((unsigned)sr_ceil_div(B, 64)), dim3(64), 0, sr_stream(stream), gpose, glin,
                       grot, gt, pose, (int)B);
    return sr_launch_status();
}
