// Landmark reprojection term of face reconstruction (C ABI: sr_landmark_loss_fwd / sr_landmark_loss_bwd, and their
// pose-aware forms sr_landmark_dyn_fwd / sr_landmark_dyn_bwd further down; definition:
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
constexpr int64_t LM_MAX_LINES = 8192;            // contour lines of one embedding: their selections sit in LDS

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

// ---- pose-aware landmarks: sliding contour lines and a visibility gate (sr_landmark_dyn_fwd / sr_landmark_dyn_bwd) -------
// Contour line c replaces landmark line_lmk[c] by the candidate vertex that lies furthest out across the face:
//     a = (v[i_up] - v[i_down]).xy    u = (a.y, -a.x) / |a| (|a| < 1e-6: (1, 0))    score_j = side[c] dot(v[cand_j].xy, u)
//     sel[b, c] = cand[first arg max_j score_j]
// and every other landmark's confidence is multiplied by gate = smoothstep((m - lo) / (hi - lo)), m = N.z / |N| of its
// interpolated normal.  sel and gate are constants of the backward pass.
constexpr int LM_WAVE = 64;
constexpr int LM_NO_POS = 0x7fffffff;

__global__ __launch_bounds__(LM_BLOCK) void k_landmark_dyn_fwd(
    float* __restrict__ rows, float* __restrict__ p, float* __restrict__ g, int* __restrict__ sel,
    float* __restrict__ gate, const float* __restrict__ v, const float* __restrict__ normals,
    const int* __restrict__ idx, const float* __restrict__ bary, const float* __restrict__ q,
    const float* __restrict__ c, const int* __restrict__ lmk_line, const int* __restrict__ side,
    const int* __restrict__ cand_off, const int* __restrict__ cand, int L, int C, int64_t nv, int i_up, int i_down,
    int use_vis, float vis_lo, float vis_hi, float half_w, float half_h, float beta, float scale) {
    __shared__ float s_num[LM_BLOCK], s_den[LM_BLOCK];
    extern __shared__ int s_sel[];                                        // [C]
    const int b = blockIdx.x;
    const float* vb = v + (int64_t)b * nv * 3;
    const float* qb = q + (int64_t)b * L * 2;
    const float* cb = c + (int64_t)b * L;
    float* pb = p + (int64_t)b * L * 2;
    float* gateb = gate + (int64_t)b * L;
    if (C > 0) {
        // phase 1: the image direction across the face; every lane runs the same operations on the same two vertices, so
        // every wave holds the same bits
        const float ax = vb[(int64_t)i_up * 3] - vb[(int64_t)i_down * 3];
        const float ay = vb[(int64_t)i_up * 3 + 1] - vb[(int64_t)i_down * 3 + 1];
        const float an = sqrtf(ax * ax + ay * ay);
        const float ux = an >= 1e-6f ? ay / an : 1.f;
        const float uy = an >= 1e-6f ? -ax / an : 0.f;
        // phase 2: a wave per line, lanes over its candidates; higher score wins, then the lower position
        const int lane = threadIdx.x & (LM_WAVE - 1);
        for (int line = threadIdx.x / LM_WAVE; line < C; line += LM_BLOCK / LM_WAVE) {
            const int e0 = cand_off[line], n = cand_off[line + 1] - e0;
            const float sd = (float)side[line];
            float best = -INFINITY;
            int pos = LM_NO_POS;
            for (int j = lane; j < n; j += LM_WAVE) {                     // ascending positions: strict > keeps the first
                const float* pv = vb + (int64_t)cand[e0 + j] * 3;
                const float s = sd * (pv[0] * ux + pv[1] * uy);
                if (s > best) {
                    best = s;
                    pos = j;
                }
            }
#pragma unroll
            for (int o = LM_WAVE / 2; o > 0; o >>= 1) {
                const float ob = __shfl_xor(best, o, LM_WAVE);
                const int op = __shfl_xor(pos, o, LM_WAVE);
                if (ob > best || (ob == best && op < pos)) {
                    best = ob;
                    pos = op;
                }
            }
            if (pos >= n) pos = 0;                                        // no finite score at all: the static vertex
            if (lane == 0) {
                const int vi = cand[e0 + pos];
                s_sel[line] = vi;
                sel[(int64_t)b * C + line] = vi;
            }
        }
    }
    __syncthreads();
    // phase 3: the static term's sums with P_l read through sel and the confidences gated
    float num = 0.f, den = 0.f;
    for (int l = threadIdx.x; l < L; l += LM_BLOCK) {
        float px = 0.f, py = 0.f, gt = 1.f;
        const int line = lmk_line[l];
        if (line >= 0) {
            const float* pv = vb + (int64_t)s_sel[line] * 3;
            px = pv[0];
            py = pv[1];
        } else {
            float nx = 0.f, ny = 0.f, nz = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float w = bary[3 * l + k];
                const int64_t vi = idx[3 * l + k];
                const float* pv = vb + vi * 3;
                px += w * pv[0];
                py += w * pv[1];
                if (use_vis) {
                    const float* pn = normals + ((int64_t)b * nv + vi) * 3;
                    nx += w * pn[0];
                    ny += w * pn[1];
                    nz += w * pn[2];
                }
            }
            if (use_vis) {
                const float m = nz / fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), LM_TINY);
                if (vis_hi > vis_lo) {
                    const float t = fminf(fmaxf((m - vis_lo) / (vis_hi - vis_lo), 0.f), 1.f);
                    gt = t * t * (3.f - 2.f * t);
                } else {
                    gt = m > vis_lo ? 1.f : 0.f;
                }
            }
        }
        px = (1.f + px) * half_w - 0.5f;
        py = (1.f - py) * half_h - 0.5f;
        pb[2 * l] = px;
        pb[2 * l + 1] = py;
        gateb[l] = gt;
        const float cl = cb[l] * gt;
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
    // g = d rows[b] / d p_l (a lane reads back the p and the gate it wrote itself)
    float* gb = g + (int64_t)b * L * 2;
    for (int l = threadIdx.x; l < L; l += LM_BLOCK) {
        const float k = norm * (cb[l] * gateb[l]);
        gb[2 * l] = k * smooth_l1_grad(pb[2 * l] - qb[2 * l], beta);
        gb[2 * l + 1] = k * smooth_l1_grad(pb[2 * l + 1] - qb[2 * l + 1], beta);
    }
}

// k_landmark_bwd with a second list: vertex i's (line, landmark) entries, one for every line in which it is a candidate
// (ascending line); the entry counts iff the line selected this vertex.  Static entries first, then the line entries.
template <bool ACC>
__global__ __launch_bounds__(LM_BLOCK) void k_landmark_dyn_bwd(
    float* __restrict__ gv, const float* __restrict__ g, const float* __restrict__ g_rows, int64_t g_rows_stride,
    const int* __restrict__ sel, const int* __restrict__ csr_off, const int* __restrict__ csr_l,
    const float* __restrict__ csr_w, const int* __restrict__ line_off, const int* __restrict__ line_c,
    const int* __restrict__ line_l, int L, int C, int64_t nv, float half_w, float half_h) {
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
    if (C > 0) {
        const int* selb = sel + (int64_t)b * C;
        const int f1 = line_off[i + 1];
        for (int e = line_off[i]; e < f1; ++e) {
            if (selb[line_c[e]] == (int)i) {
                const int l = line_l[e];
                sx += gb[2 * l];
                sy += gb[2 * l + 1];
            }
        }
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

extern "C" int sr_landmark_dyn_fwd(float* rows, float* p, float* g, int32_t* sel, float* gate, const float* v,
                                   const float* normals, const int32_t* idx, const float* bary, const float* target,
                                   const float* conf, const int32_t* lmk_line, const int32_t* side,
                                   const int32_t* cand_off, const int32_t* cand, int64_t B, int64_t L, int64_t C,
                                   int64_t nv, int64_t i_up, int64_t i_down, int use_vis, float vis_lo, float vis_hi,
                                   int64_t H, int64_t W, float beta, float weight, sr_stream_t stream) {
    if (B < 0 || L < 0 || C < 0 || nv < 0 || H <= 0 || W <= 0 || !(beta >= 0.f)) return SR_EINVAL;
    if (use_vis && !(vis_lo <= vis_hi)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!rows || (L > 0 && (!p || !g || !gate || !v || !idx || !bary || !target || !conf || !lmk_line || nv == 0)))
        return SR_EINVAL;
    if (L > 0 && use_vis && !normals) return SR_EINVAL;
    if (C > 0 && (L == 0 || !sel || !side || !cand_off || !cand || i_up < 0 || i_up >= nv || i_down < 0 || i_down >= nv))
        return SR_EINVAL;
    if (B >= (1LL << 31) || L >= (1LL << 28) || nv >= (1LL << 31) || C > LM_MAX_LINES) return SR_ERANGE;
    const float scale = weight * (2.f / (float)(W > H ? W : H));
    hipLaunchKernelGGL(k_landmark_dyn_fwd, dim3((unsigned)B), dim3(LM_BLOCK), (size_t)C * sizeof(int), sr_stream(stream),
                       rows, p, g, sel, gate, v, normals, idx, bary, target, conf, lmk_line, side, cand_off, cand, (int)L,
                       (int)C, nv, (int)i_up, (int)i_down, use_vis ? 1 : 0, vis_lo, vis_hi, 0.5f * (float)W,
                       0.5f * (float)H, beta, scale);
    return sr_launch_status();
}

extern "C" int sr_landmark_dyn_bwd(float* gv, const float* g, const float* g_rows, int64_t g_rows_stride,
                                   const int32_t* sel, const int32_t* csr_off, const int32_t* csr_l, const float* csr_w,
                                   const int32_t* line_off, const int32_t* line_c, const int32_t* line_l, int64_t B,
                                   int64_t L, int64_t C, int64_t nv, int64_t H, int64_t W, int accumulate,
                                   sr_stream_t stream) {
    if (B < 0 || L < 0 || C < 0 || nv < 0 || H <= 0 || W <= 0) return SR_EINVAL;
    if (B == 0 || nv == 0) return SR_OK;
    if (!gv || !g_rows || !csr_off || (L > 0 && !g)) return SR_EINVAL;
    if (C > 0 && (!sel || !line_off || !line_c || !line_l || L == 0)) return SR_EINVAL;
    if (B > 65535 || L >= (1LL << 28) || nv >= (1LL << 31) || C > LM_MAX_LINES) return SR_ERANGE;
    const dim3 grid((unsigned)sr_ceil_div(nv, LM_BLOCK), (unsigned)B);
    const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
    if (accumulate)
        hipLaunchKernelGGL(k_landmark_dyn_bwd<true>, grid, dim3(LM_BLOCK), 0, sr_stream(stream), gv, g, g_rows,
                           g_rows_stride, sel, csr_off, csr_l, csr_w, line_off, line_c, line_l, (int)L, (int)C, nv, hw, hh);
    else
        hipLaunchKernelGGL(k_landmark_dyn_bwd<false>, grid, dim3(LM_BLOCK), 0, sr_stream(stream), gv, g, g_rows,
                           g_rows_stride, sel, csr_off, csr_l, csr_w, line_off, line_c, line_l, (int)L, (int)C, nv, hw, hh);
    return sr_launch_status();
}
