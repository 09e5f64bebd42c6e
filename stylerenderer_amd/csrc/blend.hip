// Bilinear blendshape node of the face-reconstruction loop (C ABI: sr_blend_*): identity and expression coefficients of a
// FaceWarehouse-style model to the unposed / posed vertices and the Dirichlet / Beta prior, and the first-order backward
// (reference face_model.py:128-146 BlendShapeModel.forward / regulation).
//
//   l[b]   = cat(x[b, :ds], -sum x[b, :ds])         xs[b] = softmax(l[b])                         [ds + 1]
//   s[b]   = sigmoid(x[b, ds:])                      xe[b] = cat(1 - sum s[b], s[b])               [de + 1]
//   z[b]   = xs[b] (x) xe[b]                         K = (ds + 1)(de + 1) products, k = i (de + 1) + j
//   vs[b]  = z[b] W                                  W = weight [K, C] as stored, C = 3 nv contiguous
//   v[b]   = vs[b].view(nv, 3) @ lin[b] + t[b]
//   prior[b] = lam * regulation(x[b]),  reg = sum_b prior[b] in sample order
//
// The node is linear in z, so both hot kernels are one streaming pass over W (974 MB at ds = 149, de = 46, nv = 11 510:
// HBM-bound, W never fits a cache) for all samples of a register block:
//   k_blend_fwd      a workgroup owns 64 vertices (192 columns, 48 lanes of four columns); its 16 waves take every 16th
//                    row, the coefficients of a row are wave-uniform (scalar loads of z, stored [k][8] with zeros for the
//                    samples beyond B), the waves' sums meet in LDS in wave order, then the pose.
//   k_blend_gz       gz[b, k] = sum_c W[k, c] gvs[b, c]: a workgroup owns four rows, its threads stride over the columns
//                    (each loaded gvs value serves four rows), a fixed butterfly and the four waves in order.
// Rows of W start at multiples of C floats, so with C % 4 != 0 (FaceWarehouse: C = 34 530) they are not 16-byte aligned:
// the four-column loads are declared 4-byte aligned (one global_load_dwordx4 on gfx950, which needs dword alignment
// only) and the last C % 4 columns of a row are read one by one.  That is the only shape-selected path in this file:
//   * columns [0, 4 floor(C / 4)) four at a time, columns [4 floor(C / 4), C) singly (C % 4 in {0, 1, 2, 3})
//   * samples in register blocks of SR_BLEND_MAXB = 8: B > 8 loops over blocks (W is read once per block)
// No atomics, no scratch, vector stores only: reruns are bit-identical.
#include "common.h"

#define SR_BLEND_MAXB 8          // samples per register block
#define SR_BLEND_FWD_WAVES 16    // waves of a forward workgroup = its split of the rows
#define SR_BLEND_TILE_Q 48       // four-column items of a forward workgroup: 192 columns = 64 vertices
#define SR_BLEND_GZ_ROWS 4       // rows of W per workgroup of the backward contraction
#define SR_BLEND_MAX_DIMS 8192   // (ds + 1) + (de + 1) held in LDS by the head and tail kernels

namespace {

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };

// Columns [4 q, 4 q + 4) of a row of C floats: one 16-byte load, or the row's last C % 4 columns singly (zeros beyond).
__device__ __forceinline__ void load_cols(float* o, const float* row, int q, int C) {
    const int c = 4 * q;
    if (c + 4 <= C) {
        const f4u t = *reinterpret_cast<const f4u*>(row + c);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) o[u] = c + u < C ? row[c + u] : 0.f;
    }
}

// Sum over the 256 threads of a workgroup in a fixed order (butterfly per wave, then the waves in order); every thread
// gets the result.  `red` holds 4 floats.
__device__ __forceinline__ float block_sum(float x, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float block_max(float x, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// ---- head: one workgroup per sample -------------------------------------------------------------------------------------
// xs [B, ds + 1], xe [B, de + 1], prior [B] = lam * regulation(x[b]) (log-sum-exp and softplus: the reference's
// log(sum(exp)) and log(exp + 1) wherever those are finite), z [ceil(B / 8), K, 8] with zeros in the unused sample slots.
__global__ __launch_bounds__(256) void k_blend_head(float* __restrict__ xs, float* __restrict__ xe,
                                                    float* __restrict__ prior, float* __restrict__ z,
                                                    const float* __restrict__ x, const float* __restrict__ beta,
                                                    float lam, int B, int ds, int de) {
    extern __shared__ float sh[];                     // xs [ds + 1], xe [de + 1]
    __shared__ float red[4];
    float* sxs = sh;
    float* sxe = sh + ds + 1;
    const int b = blockIdx.x, t = threadIdx.x;
    const int ns = ds + 1, ne = de + 1, K = ns * ne;
    const float* xb = x + (int64_t)b * (ds + de);
    float a = 0.f;
    for (int i = t; i < ds; i += 256) a += xb[i];
    const float last = -block_sum(a, red);            // the logit of the last identity
    float m = last;
    for (int i = t; i < ds; i += 256) m = fmaxf(m, xb[i]);
    m = block_max(m, red);
    float se = 0.f, lb = 0.f, bs = 0.f;               // sum exp(l - m), sum l beta, sum beta
    for (int i = t; i < ns; i += 256) {
        const float l = i < ds ? xb[i] : last;
        const float e = expf(l - m);
        sxs[i] = e;
        se += e;
        lb += l * beta[i];
        bs += beta[i];
    }
    se = block_sum(se, red);
    lb = block_sum(lb, red);
    bs = block_sum(bs, red);
    float ss = 0.f, ea = 0.f, sp = 0.f;               // sum sigmoid, sum (x a - 1), sum softplus(x) (a + b - 2)
    for (int j = t; j < de; j += 256) {
        const float v = xb[ds + j];
        const float s = 1.f / (1.f + expf(-v));
        sxe[j + 1] = s;
        ss += s;
        const float pa = beta[ns + 2 * j], pb = beta[ns + 2 * j + 1];
        ea += v * pa - 1.f;
        sp += softplus(v) * ((pa + pb) - 2.f);
    }
    ss = block_sum(ss, red);
    ea = block_sum(ea, red);
    sp = block_sum(sp, red);
    if (t == 0) {
        sxe[0] = 1.f - ss;
        const float lse = m + logf(se);
        prior[b] = lam * -(((lb - lse * (bs - (float)ns)) + ea) - sp);
    }
    __syncthreads();
    for (int i = t; i < ns; i += 256) {
        const float v = sxs[i] / se;
        sxs[i] = v;
        xs[(int64_t)b * ns + i] = v;
    }
    for (int j = t; j < ne; j += 256) xe[(int64_t)b * ne + j] = sxe[j];
    __syncthreads();
    float* zb = z + (int64_t)(b / SR_BLEND_MAXB) * K * SR_BLEND_MAXB + (b % SR_BLEND_MAXB);
    for (int k = t; k < K; k += 256) {
        const int i = k / ne, j = k - i * ne;
        zb[(int64_t)k * SR_BLEND_MAXB] = sxs[i] * sxe[j];
    }
    // the unused sample slots of the last register block: written by the block's first sample
    const int nbk = B - (b / SR_BLEND_MAXB) * SR_BLEND_MAXB;
    if (b % SR_BLEND_MAXB == 0 && nbk < SR_BLEND_MAXB) {
        const int pad = SR_BLEND_MAXB - nbk;
        for (int e = t; e < K * pad; e += 256) {
            const int k = e / pad, u = e - k * pad;
            zb[(int64_t)k * SR_BLEND_MAXB + nbk + u] = 0.f;
        }
    }
}

// ---- forward contraction ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SR_BLEND_FWD_WAVES * 64) void k_blend_fwd(
    float* __restrict__ v, float* __restrict__ vs, float* __restrict__ reg, const float* __restrict__ w,
    const float* __restrict__ z, const float* __restrict__ prior, const float* __restrict__ lin,
    const float* __restrict__ pose, int B, int nv, int K) {
    __shared__ float red[SR_BLEND_FWD_WAVES][SR_BLEND_TILE_Q * 4];
    __shared__ float fin[SR_BLEND_MAXB][SR_BLEND_TILE_Q * 4];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int C = 3 * nv;
    if (reg && blockIdx.x == 0 && t == 0) {           // the prior's total, in sample order
        float a = 0.f;
        for (int b = 0; b < B; ++b) a += prior[b];
        reg[0] = a;
    }
    const int q = blockIdx.x * SR_BLEND_TILE_Q + lane;
    const bool live = lane < SR_BLEND_TILE_Q && 4 * q < C;
    for (int b0 = 0; b0 < B; b0 += SR_BLEND_MAXB) {
        const int nb = B - b0 < SR_BLEND_MAXB ? B - b0 : SR_BLEND_MAXB;
        const float* zb = z + (int64_t)(b0 / SR_BLEND_MAXB) * K * SR_BLEND_MAXB;
        float acc[SR_BLEND_MAXB][4];
#pragma unroll
        for (int bb = 0; bb < SR_BLEND_MAXB; ++bb) acc[bb][0] = acc[bb][1] = acc[bb][2] = acc[bb][3] = 0.f;
        if (live) {
#pragma unroll 4
            for (int k = wave; k < K; k += SR_BLEND_FWD_WAVES) {
                float wv[4];
                load_cols(wv, w + (int64_t)k * C, q, C);
                const float* zk = zb + (int64_t)k * SR_BLEND_MAXB;
#pragma unroll
                for (int bb = 0; bb < SR_BLEND_MAXB; ++bb) {
                    const float c = zk[bb];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[bb][u] += c * wv[u];
                }
            }
        }
        for (int bb = 0; bb < nb; ++bb) {
            __syncthreads();                          // the previous sample's sums are out of red
            if (lane < SR_BLEND_TILE_Q) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float a = 0.f;
#pragma unroll
                    for (int s = 0; s < SR_BLEND_MAXB; ++s) a = s == bb ? acc[s][u] : a;
                    red[wave][4 * lane + u] = a;
                }
            }
            __syncthreads();
            if (t < SR_BLEND_TILE_Q * 4) {
                float a = 0.f;
#pragma unroll
                for (int s = 0; s < SR_BLEND_FWD_WAVES; ++s) a += red[s][t];
                fin[bb][t] = a;
            }
        }
        __syncthreads();
        for (int e = t; e < nb * 64; e += SR_BLEND_FWD_WAVES * 64) {
            const int bb = e >> 6, b = b0 + bb;
            const int i = blockIdx.x * 64 + (e & 63);
            if (i < nv) {
                const float x = fin[bb][3 * (e & 63)], y = fin[bb][3 * (e & 63) + 1], zc = fin[bb][3 * (e & 63) + 2];
                float* o = vs + ((int64_t)b * nv + i) * 3;
                o[0] = x; o[1] = y; o[2] = zc;
                if (v) {
                    const float* m = lin + 9 * b;
                    const float* tr = pose + 7 * b + 3;
                    o = v + ((int64_t)b * nv + i) * 3;
                    o[0] = ((x * m[0] + y * m[3]) + zc * m[6]) + tr[0];
                    o[1] = ((x * m[1] + y * m[4]) + zc * m[7]) + tr[1];
                    o[2] = ((x * m[2] + y * m[5]) + zc * m[8]) + tr[2];
                }
            }
        }
        __syncthreads();                              // fin is free for the next register block
    }
}

// ---- backward contraction -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blend_gz(float* __restrict__ gz, const float* __restrict__ w,
                                                  const float* __restrict__ gvs, int B, int C, int K) {
    __shared__ float red[4][SR_BLEND_GZ_ROWS * SR_BLEND_MAXB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int k0 = blockIdx.x * SR_BLEND_GZ_ROWS;
    const int nr = K - k0 < SR_BLEND_GZ_ROWS ? K - k0 : SR_BLEND_GZ_ROWS;
    const int Q = (C + 3) / 4;
    for (int b0 = 0; b0 < B; b0 += SR_BLEND_MAXB) {
        const int nb = B - b0 < SR_BLEND_MAXB ? B - b0 : SR_BLEND_MAXB;
        float acc[SR_BLEND_GZ_ROWS][SR_BLEND_MAXB];
#pragma unroll
        for (int r = 0; r < SR_BLEND_GZ_ROWS; ++r)
#pragma unroll
            for (int bb = 0; bb < SR_BLEND_MAXB; ++bb) acc[r][bb] = 0.f;
#pragma unroll 2
        for (int q = t; q < Q; q += 256) {
            float wv[SR_BLEND_GZ_ROWS][4];
#pragma unroll
            for (int r = 0; r < SR_BLEND_GZ_ROWS; ++r) {
                if (r < nr) load_cols(wv[r], w + (int64_t)(k0 + r) * C, q, C);
                else wv[r][0] = wv[r][1] = wv[r][2] = wv[r][3] = 0.f;
            }
#pragma unroll
            for (int bb = 0; bb < SR_BLEND_MAXB; ++bb) {
                if (bb < nb) {
                    float g[4];
                    load_cols(g, gvs + (int64_t)(b0 + bb) * C, q, C);
#pragma unroll
                    for (int r = 0; r < SR_BLEND_GZ_ROWS; ++r)
                        acc[r][bb] += (wv[r][0] * g[0] + wv[r][1] * g[1]) + (wv[r][2] * g[2] + wv[r][3] * g[3]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < SR_BLEND_GZ_ROWS; ++r)
#pragma unroll
            for (int bb = 0; bb < SR_BLEND_MAXB; ++bb)
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc[r][bb] += __shfl_xor(acc[r][bb], o, 64);
        __syncthreads();                              // the previous register block's sums are out of red
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < SR_BLEND_GZ_ROWS; ++r)
#pragma unroll
                for (int bb = 0; bb < SR_BLEND_MAXB; ++bb) red[wave][r * SR_BLEND_MAXB + bb] = acc[r][bb];
        }
        __syncthreads();
        if (t < SR_BLEND_GZ_ROWS * SR_BLEND_MAXB) {
            const int r = t / SR_BLEND_MAXB, bb = t - r * SR_BLEND_MAXB;
            if (r < nr && bb < nb) gz[(int64_t)(b0 + bb) * K + k0 + r] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        }
    }
}

// ---- tail: one workgroup per sample -------------------------------------------------------------------------------------
// gxs[i] = sum_j gz[i, j] xe[j], gxe[j] = sum_i gz[i, j] xs[i], then the softmax / sigmoid Jacobians and the couplings of
// the last identity (-sum) and the neutral expression (1 - sum), plus greg * lam * d regulation / dx:
//   d/dl_i = (sum beta - ds - 1) xs_i - beta_i,     d/dx_e[j] = (a_j + b_j - 2) s_j - a_j.
__global__ __launch_bounds__(256) void k_blend_tail(float* __restrict__ gcoeff, const float* __restrict__ gz,
                                                    const float* __restrict__ xs, const float* __restrict__ xe,
                                                    const float* __restrict__ beta, float lam,
                                                    const float* __restrict__ greg, int ds, int de) {
    extern __shared__ float sh[];                     // xs, gl [ds + 1]; xe, gxe [de + 1]
    __shared__ float red[4];
    const int ns = ds + 1, ne = de + 1;
    float* sxs = sh;
    float* sgl = sh + ns;
    float* sxe = sh + 2 * ns;
    float* sge = sh + 2 * ns + ne;
    const int b = blockIdx.x, t = threadIdx.x;
    const float* g = gz ? gz + (int64_t)b * ns * ne : nullptr;
    const float pr = (greg && lam != 0.f) ? lam * greg[0] : 0.f;
    for (int i = t; i < ns; i += 256) sxs[i] = xs[(int64_t)b * ns + i];
    for (int j = t; j < ne; j += 256) sxe[j] = xe[(int64_t)b * ne + j];
    __syncthreads();
    float dot = 0.f, bs = 0.f;
    for (int i = t; i < ns; i += 256) {
        float a = 0.f;
        if (g)
            for (int j = 0; j < ne; ++j) a += g[i * ne + j] * sxe[j];
        sgl[i] = a;
        dot += sxs[i] * a;
        bs += beta[i];
    }
    for (int j = t; j < ne; j += 256) {
        float a = 0.f;
        if (g)
            for (int i = 0; i < ns; ++i) a += g[i * ne + j] * sxs[i];
        sge[j] = a;
    }
    dot = block_sum(dot, red);
    bs = block_sum(bs, red);
    for (int i = t; i < ns; i += 256) {
        float gl = sxs[i] * (sgl[i] - dot);
        if (pr != 0.f) gl += pr * ((bs - (float)ns) * sxs[i] - beta[i]);
        sgl[i] = gl;
    }
    __syncthreads();
    float* o = gcoeff + (int64_t)b * (ds + de);
    for (int i = t; i < ds; i += 256) o[i] = sgl[i] - sgl[ds];
    for (int j = t; j < de; j += 256) {
        const float s = sxe[j + 1];
        float ge = (sge[j + 1] - sge[0]) * (s * (1.f - s));
        if (pr != 0.f) {
            const float pa = beta[ns + 2 * j], pb = beta[ns + 2 * j + 1];
            ge += pr * (((pa + pb) - 2.f) * s - pa);
        }
        o[ds + j] = ge;
    }
}

bool dims_ok(int64_t B, int64_t nv, int64_t ds, int64_t de) {
    return B <= 65535 && nv < (1LL << 29) && ds + de + 2 <= SR_BLEND_MAX_DIMS && (ds + 1) * (de + 1) < (1LL << 24);
}

}  // namespace

extern "C" int64_t sr_blend_z_floats(int64_t B, int64_t ds, int64_t de) {
    if (B <= 0 || ds < 0 || de < 0) return 0;
    return sr_ceil_div(B, SR_BLEND_MAXB) * SR_BLEND_MAXB * (ds + 1) * (de + 1);
}

extern "C" int sr_blend_head(float* xs, float* xe, float* prior, float* z, const float* x, const float* beta, float lam,
                             int64_t B, int64_t ds, int64_t de, sr_stream_t stream) {
    if (B < 0 || ds < 0 || de < 0) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!xs || !xe || !prior || !z || !beta || (ds + de > 0 && !x)) return SR_EINVAL;
    if (!dims_ok(B, 0, ds, de)) return SR_ERANGE;
    hipLaunchKernelGGL(k_blend_head, dim3((unsigned)B), dim3(256), (size_t)(ds + de + 2) * sizeof(float),
                       sr_stream(stream), xs, xe, prior, z, x, beta, lam, (int)B, (int)ds, (int)de);
    return sr_launch_status();
}

extern "C" int sr_blend_fwd(float* v, float* vs, float* reg, const float* w, const float* z, const float* prior,
                            const float* lin, const float* pose, int64_t B, int64_t nv, int64_t ds, int64_t de,
                            sr_stream_t stream) {
    if (B < 0 || nv < 0 || ds < 0 || de < 0) return SR_EINVAL;
    if (B == 0 || nv == 0) return SR_OK;
    if (!vs || !w || !z || (reg && !prior) || (v && (!lin || !pose))) return SR_EINVAL;
    if (!dims_ok(B, nv, ds, de)) return SR_ERANGE;
    hipLaunchKernelGGL(k_blend_fwd, dim3((unsigned)sr_ceil_div(nv, 64)), dim3(SR_BLEND_FWD_WAVES * 64), 0,
                       sr_stream(stream), v, vs, reg, w, z, prior, lin, pose, (int)B, (int)nv,
                       (int)((ds + 1) * (de + 1)));
    return sr_launch_status();
}

extern "C" int sr_blend_gz(float* gz, const float* w, const float* gvs, int64_t B, int64_t nv, int64_t ds, int64_t de,
                           sr_stream_t stream) {
    if (B < 0 || nv < 0 || ds < 0 || de < 0) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!gz || (nv > 0 && (!w || !gvs))) return SR_EINVAL;
    if (!dims_ok(B, nv, ds, de)) return SR_ERANGE;
    const int64_t K = (ds + 1) * (de + 1);
    hipLaunchKernelGGL(k_blend_gz, dim3((unsigned)sr_ceil_div(K, SR_BLEND_GZ_ROWS)), dim3(256), 0, sr_stream(stream), gz,
                       w, gvs, (int)B, (int)(3 * nv), (int)K);
    return sr_launch_status();
}

extern "C" int sr_blend_tail(float* gcoeff, const float* gz, const float* xs, const float* xe, const float* beta,
                             float lam, const float* greg, int64_t B, int64_t ds, int64_t de, sr_stream_t stream) {
    if (B < 0 || ds < 0 || de < 0) return SR_EINVAL;
    if (B == 0 || ds + de == 0) return SR_OK;
    if (!gcoeff || !xs || !xe || !beta) return SR_EINVAL;
    if (!dims_ok(B, 0, ds, de)) return SR_ERANGE;
    hipLaunchKernelGGL(k_blend_tail, dim3((unsigned)B), dim3(256), (size_t)(2 * (ds + de + 2)) * sizeof(float),
                       sr_stream(stream), gcoeff, gz, xs, xe, beta, lam, greg, (int)ds, (int)de);
    return sr_launch_status();
}
