// Landmark reprojection term of face reconstruction (C ABI: sr_landmark_loss_fwd / sr_landmark_loss_bwd; definition:
// stylerenderer_amd/op/landmark.py).  A landmark is a barycentric combination of up to three vertices of the posed mesh;
// it is projected to the rasterizer's pixel index coordinates (orthographic, reference op/rasterize.h:21-22) and compared
// with a target point under smooth-L1 (torch's function; beta = one pixel in reference train.py:329):
//     P_l = sum_k bary[l, k] v[b, idx[l, k], :]       p_l = ((1 + P_l.x) W / 2 - 1/2, (1 - P_l.y) H / 2 - 1/2)
//     rows[b] = scale * sum_l c[b, l] (rho(p_l.x - q.x) + rho(p_l.y - q.y)) / max(sum_l c[b, l], tiny)
// Both kernels are latency-bound (L is 68, the gradient touches L of ~25 000 vertices): the point is two launches per
// step, no memset node, no scatter and no atomics.  Forward: one workgroup per sample, every lane sums its landmarks in
// index order, then a fixed-order LDS tree, so the sum does not depend on the grid and reruns are bit-identical.
// Backward: one lane per (sample, vertex) walks that vertex's entries of a CSR list built once per embedding on the host
// (ascending 3 l + k) and writes the dense gradient, zeros included.  Compiled with -ffp-contract=off.
#include "common.h"

namespace {

constexpr int LM_BLOCK = 256;
constexpr float LM_TINY = 1e-12f;

__device__ __forceinline__ float smooth_l1(float e, float beta) {
    const float a = fabsf(e);
    return a < beta ? (0.5f * e) * e / beta : a - 0.5f * beta;
}

// d rho / d e: e / beta inside (-beta, beta), the sign outside (0 at e = 0 when beta = 0: torch's l1 there)
__device__ __forceinline__ float smooth_l1_grad(float e, float beta) {
    return fabsf(e) < beta ? e / beta : (float)(e > 0.f) - (float)(e < 0.f);
}

__global__ __launch_bounds__(LM_BLOCK) void k_landmark_fwd(float* __restrict__ rows, float* __restrict__ p,
                                                           float* __restrict__ g, const float* __restrict__ v,
                                                           const int* __restrict__ idx, const float* __restrict__ bary,
                                                           const float* __restrict__ q, const float* __restrict__ c,
                                                           int L, int64_t nv, float half_w, float half_h, float beta,
                                                           float scale) {
    __shared__ float s_num[LM_BLOCK], s_den[LM_BLOCK];
    const int b = blockIdx.x;
    const float* vb = v + (int64_t)b * nv * 3;
    const float* qb = q + (int64_t)b * L * 2;
    const float* cb = c + (int64_t)b * L;
    float* pb = p + (int64_t)b * L * 2;
    float num = 0.f, den = 0.f;
    for (int l = threadIdx.x; l < L; l += LM_BLOCK) {
        float px = 0.f, py = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float w = bary[3 * l + k];
            const float* pv = vb + (int64_t)idx[3 * l + k] * 3;
            px += w * pv[0];
            py += w * pv[1];
        }
        px = (1.f + px) * half_w - 0.5f;
        py = (1.f - py) * half_h - 0.5f;
        pb[2 * l] = px;
        pb[2 * l + 1] = py;
        const float cl = cb[l];
        num += cl * (smooth_l1(px - qb[2 * l], beta) + smooth_l1(py - qb[2 * l + 1], beta));
        den += cl;
    }
    s_num[threadIdx.x] = num;
    s_den[threadIdx.x] = den;
    __syncthreads();
    for (int off = LM_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            s_num[threadIdx.x] += s_num[threadIdx.x + off];
            s_den[threadIdx.x] += s_den[threadIdx.x + off];
        }
        __syncthreads();
    }
    const float norm = scale / fmaxf(s_den[0], LM_TINY);
    if (threadIdx.x == 0) rows[b] = norm * s_num[0];
    // g = d rows[b] / d p_l (a lane reads back the p it wrote itself)
    float* gb = g + (int64_t)b * L * 2;
    for (int l = threadIdx.x; l < L; l += LM_BLOCK) {
        const float k = norm * cb[l];
        gb[2 * l] = k * smooth_l1_grad(pb[2 * l] - qb[2 * l], beta);
        gb[2 * l + 1] = k * smooth_l1_grad(pb[2 * l + 1] - qb[2 * l + 1], beta);
    }
}

// gv[b, i, :] (+)= g_rows[b] * (W/2 * sum_e w_e g[b, l_e, 0], -H/2 * sum_e w_e g[b, l_e, 1], 0), e over vertex i's entries
template <bool ACC>
__global__ __launch_bounds__(LM_BLOCK) void k_landmark_bwd(float* __restrict__ gv, const float* __restrict__ g,
                                                           const float* __restrict__ g_rows, int64_t g_rows_stride,
                                                           const int* __restrict__ csr_off, const int* __restrict__ csr_l,
                                                           const float* __restrict__ csr_w, int L, int64_t nv,
                                                           float half_w, float half_h) {
    const int64_t i = (int64_t)blockIdx.x * LM_BLOCK + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= nv) return;
    const float* gb = g + (int64_t)b * L * 2;
    float sx = 0.f, sy = 0.f;
    const int e1 = csr_off[i + 1];
    for (int e = csr_off[i]; e < e1; ++e) {
        const int l = csr_l[e];
        const float w = csr_w[e];
        sx += w * gb[2 * l];
        sy += w * gb[2 * l + 1];
    }
    const float gr = g_rows[b * g_rows_stride];
    const float rx = gr * (half_w * sx), ry = gr * (-half_h * sy);
    float* o = gv + ((int64_t)b * nv + i) * 3;
    if (ACC) {
        o[0] += rx;
        o[1] += ry;
        o[2] += 0.f;
    } else {
        o[0] = rx;
        o[1] = ry;
        o[2] = 0.f;
    }
}

}  // namespace

extern "C" int sr_landmark_loss_fwd(float* rows, float* p, float* g, const float* v, const int32_t* idx,
                                    const float* bary, const float* target, const float* conf, int64_t B, int64_t L,
                                    int64_t nv, int64_t H, int64_t W, float beta, float weight, sr_stream_t stream) {
    if (B < 0 || L < 0 || nv < 0 || H <= 0 || W <= 0 || !(beta >= 0.f)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!rows || (L > 0 && (!p || !g || !v || !idx || !bary || !target || !conf || nv == 0))) return SR_EINVAL;
    if (B >= (1LL << 31) || L >= (1LL << 28) || nv >= (1LL << 31)) return SR_ERANGE;
    const float scale = weight * (2.f / (float)(W > H ? W : H));
    hipLaunchKernelGGL(k_landmark_fwd, dim3((unsigned)B), dim3(LM_BLOCK), 0, sr_stream(stream), rows, p, g, v, idx, bary,
                       target, conf, (int)L, nv, 0.5f * (float)W, 0.5f * (float)H, beta, scale);
    return sr_launch_status();
}

extern "C" int sr_landmark_loss_bwd(float* gv, const float* g, const float* g_rows, int64_t g_rows_stride,
                                    const int32_t* csr_off, const int32_t* csr_l, const float* csr_w, int64_t B, int64_t L,
                                    int64_t nv, int64_t H, int64_t W, int accumulate, sr_stream_t stream) {
    if (B < 0 || L < 0 || nv < 0 || H <= 0 || W <= 0) return SR_EINVAL;
    if (B == 0 || nv == 0) return SR_OK;
    if (!gv || !g_rows || !csr_off || (L > 0 && !g)) return SR_EINVAL;
    if (B > 65535 || L >= (1LL << 28) || nv >= (1LL << 31)) return SR_ERANGE;
    const dim3 grid((unsigned)sr_ceil_div(nv, LM_BLOCK), (unsigned)B);
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    if (accumulate)
        hipLaunchKernelGGL(k_landmark_bwd<true>, grid, dim3(LM_BLOCK), 0, sr_stream(stream), gv, g, g_rows, g_rows_stride,
                           csr_off, csr_l, csr_w, (int)L, nv, hw, hh);
    else
        hipLaunchKernelGGL(k_landmark_bwd<false>, grid, dim3(LM_BLOCK), 0, sr_stream(stream), gv, g, g_rows,
                           g_rows_stride, csr_off, csr_l, csr_w, (int)L, nv, hw, hh);
    return sr_launch_status();
}
