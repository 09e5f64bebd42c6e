// Finish of a K-sliced, transform-domain weight gradient that also yields the style gradient.
//
// For y = oscale * conv(iscale (.) x, W) let P_b[t][c][n] = corr(x[b,c], oscale[b,n] g[b,n])[t] be the weight gradient
// of sample b WITHOUT the style.  Both gradients are linear in it:
//   dW[t][c][n] = sum_b iscale[b][c] * P_b[t][c][n]            gis[b][c] = sum_{t,n} W[t][c][n] * P_b[t][c][n]
// k_wgrad_wino and k_wgrad_s2p write split-K slabs of 16 transform-domain positions; where no K slice straddles a
// sample (`sps` whole slices per sample) and the main kernel ran with the style scale left out, the slabs of sample b
// sum to the transform of P_b and this finish produces dW and gis from the bytes the plain finish reads for dW alone —
// no pass over x or the data gradient (the row-dot pass of csrc/fused_elem.hip) is needed.
//
// Both transforms pull 4 x 4 positions back to 3 x 3 taps with one 3 x 4 matrix L per dimension,
// tap[ty][tx] = sum_{i,j} L[ty][i] L[tx][j] m[i][j].  Thread (lane, g) of a 256-thread workgroup owns position row g
// of 64 consecutive v of one u (partial [slice][16][CU][CV], v contiguous): per sample it adds that sample's slices
// in slice order, pulls its row back to r[tx] = sum_j L[tx][j] m[g][j], adds iscale * r to its share of dW and
// forms r . (sum_ty L[ty][g] W[ty][tx]), its share of the sample's style gradient.  The pull-back is linear in the rows,
// so the four rows meet only once, after the last sample: one barrier per workgroup.  Every sum runs in a fixed order
// (no atomics): results repeat bit for bit.
#pragma once
#include "common.h"

struct SrStyleFinish {
    const float* partial;    // [B * sps][16][CU][CV]
    const float* iscale;     // [B][C]
    const float* wt;         // forward weight [9][C][ldw]
    float* dwt;              // [9][C][N]
    float* part;             // style-gradient partials, summed by k_wgrad_style_sum
    int B, sps, CU, CV, C, N, ldw;
};

// G^T . G of Winograd F(3x3, 2x2) (k_wgrad_wino_finish): rows (1, 1/2, 1/2, 0), (0, 1/2, -1/2, 0), (0, 1/2, 1/2, 1)
struct SrPullWino {
    static __host__ __device__ constexpr float l(int t, int i) {
        return t == 0 ? (i == 0 ? 1.f : i < 3 ? 0.5f : 0.f) : t == 1 ? (i == 1 ? 0.5f : i == 2 ? -0.5f : 0.f)
                                                                     : (i == 3 ? 1.f : i > 0 ? 0.5f : 0.f);
    }
};
// slots of the polyphase stride-2 products (k_wgrad_s2p_finish): S(0) = {0, 3}, S(1) = {1}, S(2) = {2, 3}
struct SrPullS2p {
    static __host__ __device__ constexpr float l(int t, int i) { return (i == t || (i == 3 && t != 1)) ? 1.f : 0.f; }
};

namespace sr_style_finish {
constexpr int GP = 65;                // lane pitch of one position row: 64 + 1, rows of a sample land in different banks
constexpr int PITCH = 4 * GP;         // floats per sample of the per-thread style shares
inline size_t lds_bytes(int B) { return (size_t)(B * PITCH + 4 * 3 * 64 + 4 * B) * sizeof(float); }
// acc + l * x with the constant folded where l is 0 or 1 (l is a compile-time value after unrolling)
__device__ __forceinline__ float lmad(float l, float x, float acc) {
    return l == 0.f ? acc : l == 1.f ? acc + x : fmaf(l, x, acc);
}
}  // namespace sr_style_finish

// STYLE_ON_V false: the style channel is u (regular convolution: (u, v) = (c, n)); the 64 lanes of a workgroup are 64
//   output channels of one input channel and part is [B][C][CV / 64].
// STYLE_ON_V true: the style channel is v (transposed convolution: (u, v) = (n, c)); part is [B][CU][CV].
// Grid: CU * CV / 64 workgroups of 256; dynamic LDS sr_style_finish::lds_bytes(B).
template <class PULL, bool STYLE_ON_V>
__global__ __launch_bounds__(256) void k_wgrad_style_finish(const SrStyleFinish p) {
    using namespace sr_style_finish;
    extern __shared__ float sm[];
    float* const smw = sm + p.B * PITCH;          // [4 rows][3 tx][64]
    float* const sm2 = smw + 4 * 3 * 64;          // [B][4]
    const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
    const int nvb = p.CV / 64;
    const int u = blockIdx.x / nvb, vb = blockIdx.x % nvb, v = vb * 64 + lane;
    const int c = STYLE_ON_V ? v : u, n = STYLE_ON_V ? u : v;
    const int64_t plane = (int64_t)p.CU * p.CV;

    float weff[3];
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
        float w = 0.f;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) w = fmaf(PULL::l(ty, g), p.wt[((int64_t)(ty * 3 + tx) * p.C + c) * p.ldw + n], w);
        weff[tx] = w;
    }

    const float* src = p.partial + (int64_t)(4 * g) * plane + (int64_t)u * p.CV + v;
    float dw[3] = {0.f, 0.f, 0.f};
#pragma unroll 2
    for (int b = 0; b < p.B; ++b) {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
        const float* q = src + (int64_t)b * p.sps * 16 * plane;
#pragma unroll 4
        for (int s = 0; s < p.sps; ++s) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += q[((int64_t)s * 16 + j) * plane];
        }
        float r[3];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            r[tx] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) r[tx] = lmad(PULL::l(tx, j), a[j], r[tx]);
        }
        const float sc = p.iscale[(int64_t)b * p.C + c];
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) dw[tx] = fmaf(sc, r[tx], dw[tx]);
        sm[b * PITCH + g * GP + lane] = fmaf(r[2], weff[2], fmaf(r[1], weff[1], r[0] * weff[0]));
    }
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) smw[(g * 3 + tx) * 64 + lane] = dw[tx];
    __syncthreads();

    // dW: wave ty < 3 combines the four rows, in row order
    if (g < 3) {
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
            float o = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) o = fmaf(PULL::l(g, i), smw[(i * 3 + tx) * 64 + lane], o);
            p.dwt[((int64_t)(g * 3 + tx) * p.C + c) * p.N + n] = o;
        }
    }
    // style gradient
    if (STYLE_ON_V) {
        for (int i = tid; i < p.B * 64; i += 256) {
            const int b = i >> 6, l = i & 63;
            const float* q = sm + b * PITCH + l;
            p.part[((int64_t)b * p.CU + u) * p.CV + vb * 64 + l] = ((q[0] + q[GP]) + q[2 * GP]) + q[3 * GP];
        }
    } else {
        for (int i = tid; i < p.B * 4; i += 256) {      // (b, row): the 64 lanes in lane order
            const float* q = sm + (i >> 2) * PITCH + (i & 3) * GP;
            float s = 0.f;
            for (int k = 0; k < 64; ++k) s += q[k];
            sm2[i] = s;
        }
        __syncthreads();
        if (tid < p.B)
            p.part[((int64_t)tid * p.C + c) * nvb + vb] = ((sm2[4 * tid] + sm2[4 * tid + 1]) + sm2[4 * tid + 2]) + sm2[4 * tid + 3];
    }
}

// gis[b][c] = sum_{k < cnt} part[b * sb + c * sc + k * sk] in a fixed order: wave g of a workgroup adds the g-th quarter
// of the k range for 64 consecutive c of one sample, then the four quarters are added in order.  Grid: B * ceil(C / 64).
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_wgrad_style_sum(float* __restrict__ gis, const float* __restrict__ part, int C,
                                                                int cnt, int64_t sb, int64_t sc, int64_t sk) {
    __shared__ float sm[WAVES][64];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int cb = (C + 63) / 64;
    const int b = blockIdx.x / cb, c = (blockIdx.x % cb) * 64 + lane;
    const int per = (cnt + WAVES - 1) / WAVES;
    const int k0 = g * per, k1 = min(cnt, k0 + per);
    float s = 0.f;
    if (c < C) {
        const float* q = part + b * sb + c * sc;
#pragma unroll 8
        for (int k = k0; k < k1; ++k) s += q[k * sk];
    }
    sm[g][lane] = s;
    __syncthreads();
    if (g == 0 && c < C) {
        float t = sm[0][lane];
#pragma unroll
        for (int i = 1; i < WAVES; ++i) t += sm[i][lane];
        gis[(int64_t)b * C + c] = t;
    }
}

// launches both kernels; style_on_v as above.  B <= SR_STYLE_FINISH_MAX_B, CV % 64 == 0.
constexpr int SR_STYLE_FINISH_MAX_B = 32;
template <class PULL, bool STYLE_ON_V>
int sr_wgrad_style_finish_launch(const SrStyleFinish& p, float* gis, hipStream_t st) {
    if (p.B <= 0 || p.B > SR_STYLE_FINISH_MAX_B || p.CV % 64 != 0 || p.sps <= 0) return SR_EINVAL;
    hipLaunchKernelGGL((k_wgrad_style_finish<PULL, STYLE_ON_V>), dim3((unsigned)(p.CU * (p.CV / 64))), dim3(256),
                       sr_style_finish::lds_bytes(p.B), st, p);
    const unsigned blocks = (unsigned)(p.B * ((p.C + 63) / 64));
    if (STYLE_ON_V)
        hipLaunchKernelGGL(k_wgrad_style_sum<4>, dim3(blocks), dim3(256), 0, st, gis, p.part, p.C, p.CU,
                           (int64_t)p.CU * p.CV, (int64_t)1, (int64_t)p.CV);
    else
        hipLaunchKernelGGL(k_wgrad_style_sum<4>, dim3(blocks), dim3(256), 0, st, gis, p.part, p.C, p.CV / 64,
                           (int64_t)p.C * (p.CV / 64), (int64_t)(p.CV / 64), (int64_t)1);
    return sr_launch_status();
}
// floats of `part`
inline int64_t sr_wgrad_style_part_floats(int64_t B, int64_t CU, int64_t CV, bool style_on_v) {
    return style_on_v ? B * CU * CV : B * CU * (CV / 64);
}
