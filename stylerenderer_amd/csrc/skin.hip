// Skinning node of face reconstruction (C ABI: sr_skin_*): shape coefficients, one axis-angle per non-root joint and a
// rigid pose to the posed vertices of a linear-blend-skinning model (FLAME), and the first-order backward (reference
// face_model.py:313-341 LinearBlendSkinningModel.forward / regulation, utils_3d.py rodrigues and euler_mat "yxz").
// Row-vector convention, np = nj - nroot moving joints, D = ds + 9 np rows of the stacked basis S:
//
//   cx[b]     = [beta, vec(R_i - I)]                          R_i = rodrigues(theta_i)
//   J[b]      = J0 + JS beta                                  J0 = Jreg v_template [nj, 3], JS = Jreg S[:ds] [3 nj, ds]
//   chain     root: A = I, t = J;  child c of p: A_c = R_c^T A_p,  t_c = (J_c - J_p) A_p + t_p
//   G[b, i]   = [A_i lin ; (t_i - J_i A_i) lin + t_pose]      lin = exp(s) R(yaw, pitch, roll): the global pose, fused
//   vp[b]     = (v_template + S^T cx[b]).view(nv, 3)          one streaming pass over S^T [3 nv, D] for all B
//   v[b, k]   = vp[b, k] (sum_i W[k, i] G_i[:3]) + sum_i W[k, i] G_i[3]
//   reg       = lam * sum_b (sum_k (beta_k / sigma_k)^2 + sum_i |theta_i Pinv_i|^2)
//
// Forward: k_skin_joints (one workgroup: everything that is per sample and per joint), k_skin_fwd (the basis pass with
// the blend as its epilogue).  Backward: k_skin_bwd (per vertex g vp = g M_k^T, and per workgroup the twelve sums of
// every joint's gG_i, stage one of a fixed-order two-level reduction), the split-K coefficient gradient of morph.hip over
// S^T, and k_skin_joints_bwd (stage two of the reduction, the adjoints of the fused pose, the chain and the joint
// regressor, the Rodrigues backward, the prior's gradient and the pose gradient; one workgroup per sample).  No
// atomics: reruns are bit-identical.  Vector stores only.
#include "common.h"
#include "pose.h"
#include "rodrigues.h"

// Tuned for FLAME-sized trees (nj ~ 5): the blend epilogue of k_skin_fwd runs on lane 0 of a wave (12 nj FMAs per sample)
// and k_skin_bwd does 12 nj wave reductions per wave.  The ABI takes up to 32 joints, but an SMPL-sized tree would want
// the epilogue spread over lanes and the per-joint sums kept per lane before one reduction.
#define SR_SKIN_MAXJ 32          // joints (LDS of the per-sample kernels)
#define SR_SKIN_MAXB 8           // samples per register block of the basis pass
#define SR_SKIN_MAX_LDS 12288    // floats of coefficients and transforms held by one launch of k_skin_fwd (samples (D + 12 nj))
#define SR_SKIN_EPS 1e-8f

namespace {

__device__ __forceinline__ void pose_lin(const float* pose, float* lin, float* t) {
    if (!pose) {
#pragma unroll
        for (int i = 0; i < 9; ++i) lin[i] = (i % 4 == 0) ? 1.f : 0.f;
        t[0] = t[1] = t[2] = 0.f;
        return;
    }
    float rot[9];
    pose_fwd(pose, lin, rot);
    t[0] = pose[3]; t[1] = pose[4]; t[2] = pose[5];
}

// row vector times matrix, and times its transpose
__device__ __forceinline__ void vec_mat(const float* x, const float* m, float* o) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = (x[0] * m[j] + x[1] * m[3 + j]) + x[2] * m[6 + j];
}
__device__ __forceinline__ void vec_matT(const float* x, const float* m, float* o) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = (x[0] * m[3 * j] + x[1] * m[3 * j + 1]) + x[2] * m[3 * j + 2];
}

// One workgroup of four waves; wave w takes samples w, w + 4, ...: lanes regress the joints (one wave-wide dot product per
// coordinate) and rotate, lane 0 walks the chain.  chain[b, i] = (A_i [9], t_i [3], J_i [3]) is kept for the backward.
__global__ __launch_bounds__(256) void k_skin_joints(float* __restrict__ cx, float* __restrict__ G,
                                                     float* __restrict__ chain, float* __restrict__ reg,
                                                     const float* __restrict__ coeff, const float* __restrict__ pose,
                                                     const float* __restrict__ j0, const float* __restrict__ js,
                                                     const int* __restrict__ parent, const float* __restrict__ sigma,
                                                     const float* __restrict__ pinv, float lam, int B, int nj, int nroot,
                                                     int ds) {
    __shared__ float sJ[4][SR_SKIN_MAXJ * 3];
    __shared__ float sR[4][SR_SKIN_MAXJ * 9];
    __shared__ float sreg[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int np = nj - nroot, dc = ds + 3 * np, D = ds + 9 * np;
    float racc = 0.f;                                             // lane 0: this wave's samples, in order
    for (int b0 = 0; b0 < B; b0 += 4) {                           // uniform trip count: the barriers below
        const int b = b0 + wave;
        const bool act = b < B;
        const float* c = coeff + (int64_t)(act ? b : 0) * dc;
        float* J = sJ[wave];
        float* R = sR[wave];
        for (int o = 0; act && o < 3 * nj; ++o) {
            float a = 0.f;
            for (int k = lane; k < ds; k += 64) a += js[(int64_t)o * ds + k] * c[k];
            a = sr_wave_sum(a);
            if (lane == 0) J[o] = j0[o] + a;
        }
        float pr = 0.f;
        for (int k = lane; act && k < ds; k += 64) {
            const float x = sigma ? c[k] / sigma[k] : c[k];
            cx[(int64_t)b * D + k] = c[k];
            pr += x * x;
        }
        for (int i = lane; act && i < np; i += 64) {
            const float* th = c + ds + 3 * i;
            float r[9];
            rodrigues_fwd(th, SR_SKIN_EPS, r);
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                R[9 * i + e] = r[e];
                cx[(int64_t)b * D + ds + 9 * i + e] = r[e] - (e % 4 == 0 ? 1.f : 0.f);
            }
            float y[3];
            if (pinv) vec_mat(th, pinv + 9 * i, y);
            else { y[0] = th[0]; y[1] = th[1]; y[2] = th[2]; }
            pr += (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
        }
        pr = sr_wave_sum(pr);
        __syncthreads();                                          // R of this wave's sample is in LDS
        if (act && lane == 0) {
            racc += pr;
            float lin[9], tg[3];
            pose_lin(pose ? pose + 7 * b : nullptr, lin, tg);
            float* ch = chain + (int64_t)b * nj * 15;
            for (int i = 0; i < nj; ++i) {
                float A[9], t[3];
                if (i < nroot) {
#pragma unroll
                    for (int e = 0; e < 9; ++e) A[e] = (e % 4 == 0) ? 1.f : 0.f;
                    t[0] = J[3 * i]; t[1] = J[3 * i + 1]; t[2] = J[3 * i + 2];
                } else {
                    const int p = parent[i - nroot];
                    const float* Ap = ch + 15 * p;
                    const float* r = R + 9 * (i - nroot);
                    float rt[9], ap[9];
#pragma unroll
                    for (int e = 0; e < 9; ++e) { rt[e] = r[3 * (e % 3) + e / 3]; ap[e] = Ap[e]; }
                    mat3_mul(rt, ap, A);
                    const float dj[3] = {J[3 * i] - J[3 * p], J[3 * i + 1] - J[3 * p + 1], J[3 * i + 2] - J[3 * p + 2]};
                    vec_mat(dj, ap, t);
                    t[0] += Ap[9]; t[1] += Ap[10]; t[2] += Ap[11];
                }
                float* o = ch + 15 * i;
#pragma unroll
                for (int e = 0; e < 9; ++e) o[e] = A[e];
                o[9] = t[0]; o[10] = t[1]; o[11] = t[2];
                o[12] = J[3 * i]; o[13] = J[3 * i + 1]; o[14] = J[3 * i + 2];
                float ja[3], tp[3], g3[3], gl[9];
                vec_mat(J + 3 * i, A, ja);
                tp[0] = t[0] - ja[0]; tp[1] = t[1] - ja[1]; tp[2] = t[2] - ja[2];
                mat3_mul(A, lin, gl);
                vec_mat(tp, lin, g3);
                float* g = G + ((int64_t)b * nj + i) * 12;
#pragma unroll
                for (int e = 0; e < 9; ++e) g[e] = gl[e];
                g[9] = g3[0] + tg[0]; g[10] = g3[1] + tg[1]; g[11] = g3[2] + tg[2];
            }
        }
        __syncthreads();                                          // J / R are free for the next sample
    }
    if (lane == 0) sreg[wave] = racc;
    __syncthreads();
    if (reg && threadIdx.x == 0) reg[0] = lam * (((sreg[0] + sreg[1]) + sreg[2]) + sreg[3]);
}

// The basis pass: k_morph_fwd's wave per vertex over the 3 D contiguous weights of its three rows of S^T, every sample's
// dot products in registers, a fixed butterfly; lane 0 adds the template, blends the joints' transforms and stores.
template <int V>
__global__ __launch_bounds__(256) void k_skin_fwd(float* __restrict__ v, float* __restrict__ vp,
                                                  const float* __restrict__ st, const float* __restrict__ vt,
                                                  const float* __restrict__ cx, const float* __restrict__ wts,
                                                  const float* __restrict__ G, int B, int nv, int D, int nj) {
    extern __shared__ float sc[];                                 // cx [B D], then G [B nj 12]
    float* sG = sc + B * D;
    for (int e = threadIdx.x; e < B * D; e += 256) sc[e] = cx[e];
    for (int e = threadIdx.x; e < B * nj * 12; e += 256) sG[e] = G[e];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nv) return;
    const int nq = 3 * D / V;
    const float* wr = st + (int64_t)i * 3 * D;
    for (int b0 = 0; b0 < B; b0 += SR_SKIN_MAXB) {
        float acc[SR_SKIN_MAXB][3];
#pragma unroll
        for (int bb = 0; bb < SR_SKIN_MAXB; ++bb) acc[bb][0] = acc[bb][1] = acc[bb][2] = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const int e = q * V;
            const int r = e / D, k = e - r * D;                  // D % V == 0: a load never straddles two rows
            float wv[V];
            sr_load_v<V>(wv, wr + e);
#pragma unroll
            for (int bb = 0; bb < SR_SKIN_MAXB; ++bb) {
                if (b0 + bb < B) {
                    const float* c = sc + (b0 + bb) * D + k;
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
        for (int bb = 0; bb < SR_SKIN_MAXB; ++bb) {
            if (b0 + bb < B) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                    for (int r = 0; r < 3; ++r) acc[bb][r] += __shfl_xor(acc[bb][r], o, 64);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int bb = 0; bb < SR_SKIN_MAXB; ++bb) {
                const int b = b0 + bb;
                if (b < B) {
                    const float x = vt[3 * i] + acc[bb][0], y = vt[3 * i + 1] + acc[bb][1];
                    const float z = vt[3 * i + 2] + acc[bb][2];
                    float m[12];
#pragma unroll
                    for (int e = 0; e < 12; ++e) m[e] = 0.f;
                    for (int j = 0; j < nj; ++j) {
                        const float w = wts[(int64_t)i * nj + j];
                        const float* g = sG + (b * nj + j) * 12;
#pragma unroll
                        for (int e = 0; e < 12; ++e) m[e] += w * g[e];
                    }
                    float* o = vp + ((int64_t)b * nv + i) * 3;
                    o[0] = x; o[1] = y; o[2] = z;
                    o = v + ((int64_t)b * nv + i) * 3;
                    o[0] = ((x * m[0] + y * m[3]) + z * m[6]) + m[9];
                    o[1] = ((x * m[1] + y * m[4]) + z * m[7]) + m[10];
                    o[2] = ((x * m[2] + y * m[5]) + z * m[8]) + m[11];
                }
            }
        }
    }
}

// Backward of the blend.  One thread per vertex, blockIdx.y = sample: g = gv + gvn, gvp = g M_k^T, and for every joint
// the twelve sums over the workgroup's vertices of W[k, i] [vp_k^T g ; g] (a wave tree, then the four waves in order):
// part[b, blk, i, 12].
__global__ __launch_bounds__(256) void k_skin_bwd(float* __restrict__ gvp, float* __restrict__ part,
                                                  const float* __restrict__ gv, const float* __restrict__ gvn,
                                                  const float* __restrict__ vp, const float* __restrict__ wts,
                                                  const float* __restrict__ G, int nv, int nj) {
    __shared__ float sG[SR_SKIN_MAXJ * 12];
    __shared__ float red[4][SR_SKIN_MAXJ * 12];
    const int b = blockIdx.y;
    for (int e = threadIdx.x; e < nj * 12; e += 256) sG[e] = G[(int64_t)b * nj * 12 + e];
    __syncthreads();
    const int k = blockIdx.x * 256 + threadIdx.x;
    const bool live = k < nv;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t o = ((int64_t)b * nv + (live ? k : 0)) * 3;
    float g[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            g[c] = gv[o + c] + (gvn ? gvn[o + c] : 0.f);
            p[c] = vp[o + c];
        }
    }
    float m[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) m[e] = 0.f;
    for (int j = 0; j < nj; ++j) {
        const float w = live ? wts[(int64_t)k * nj + j] : 0.f;
#pragma unroll
        for (int e = 0; e < 9; ++e) m[e] += w * sG[12 * j + e];
        float s[12];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[3 * r + c] = w * (p[r] * g[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[9 + c] = w * g[c];
#pragma unroll
        for (int e = 0; e < 12; ++e) {
            const float a = sr_wave_sum(s[e]);
            if (lane == 0) red[wave][12 * j + e] = a;
        }
    }
    if (live) {
        float q[3];
        vec_matT(g, m, q);
        gvp[o] = q[0]; gvp[o + 1] = q[1]; gvp[o + 2] = q[2];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nj * 12; e += 256)
        part[((int64_t)b * gridDim.x + blockIdx.x) * nj * 12 + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

// One workgroup (one wave) per sample.  Lanes sum the partials of gG in workgroup order; lane 0 takes the fused pose
// apart (g lin, g t_pose, g A_i, g t_i, g J_i) and walks the chain backwards (g R_i, g J); lanes add JS^T gJ and the
// prior to the basis pass' g beta, and run the Rodrigues backward on gR_i + g vec(R_i - I) of the basis pass.
__global__ __launch_bounds__(64) void k_skin_joints_bwd(float* __restrict__ gcoeff, float* __restrict__ gpose,
                                                        const float* __restrict__ gcx, const float* __restrict__ part,
                                                        const float* __restrict__ coeff, const float* __restrict__ pose,
                                                        const float* __restrict__ chain, const float* __restrict__ js,
                                                        const int* __restrict__ parent, const float* __restrict__ sigma,
                                                        const float* __restrict__ pinv, float lam,
                                                        const float* __restrict__ greg, int nblk, int nj, int nroot,
                                                        int ds) {
    __shared__ float sg[SR_SKIN_MAXJ * 12];      // gG, then (gA [9], gt [3]) per joint
    __shared__ float sgJ[SR_SKIN_MAXJ * 3];
    __shared__ float sgR[SR_SKIN_MAXJ * 9];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int np = nj - nroot, dc = ds + 3 * np, D = ds + 9 * np;
    for (int e = lane; e < nj * 12; e += 64) {
        float a = 0.f;
        for (int s = 0; s < nblk; ++s) a += part[((int64_t)b * nblk + s) * nj * 12 + e];
        sg[e] = a;
    }
    __syncthreads();
    const float* c = coeff + (int64_t)b * dc;
    const float* ch = chain + (int64_t)b * nj * 15;
    if (lane == 0) {
        float lin[9], tg[3];
        pose_lin(pose ? pose + 7 * b : nullptr, lin, tg);
        float glin[9], gtg[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 9; ++e) glin[e] = 0.f;
        for (int i = 0; i < nj; ++i) {
            const float* A = ch + 15 * i;
            const float* J = A + 12;
            float* P = sg + 12 * i;
            const float q[3] = {P[9], P[10], P[11]};
            float ja[3], tp[3];
            vec_mat(J, A, ja);
            tp[0] = A[9] - ja[0]; tp[1] = A[10] - ja[1]; tp[2] = A[11] - ja[2];
            // glin += A^T P + tp^T q ; g t_pose += q
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc)
                    glin[3 * r + cc] += ((A[r] * P[cc] + A[3 + r] * P[3 + cc]) + A[6 + r] * P[6 + cc]) + tp[r] * q[cc];
            gtg[0] += q[0]; gtg[1] += q[1]; gtg[2] += q[2];
            float qp[3], gA[9], gj[3];
            vec_matT(q, lin, qp);                                // g t'_i = g t_i
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float row[3];
                vec_matT(P + 3 * r, lin, row);                   // (P lin^T) row r
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) gA[3 * r + cc] = row[cc] - J[r] * qp[cc];
            }
            vec_matT(qp, A, gj);
            sgJ[3 * i] = -gj[0]; sgJ[3 * i + 1] = -gj[1]; sgJ[3 * i + 2] = -gj[2];
#pragma unroll
            for (int e = 0; e < 9; ++e) P[e] = gA[e];
            P[9] = qp[0]; P[10] = qp[1]; P[11] = qp[2];
        }
        for (int i = nj - 1; i >= nroot; --i) {
            const int p = parent[i - nroot];
            const float* Ap = ch + 15 * p;
            const float* gA = sg + 12 * i;
            const float* gt = gA + 9;
            float r[9];
            rodrigues_fwd(c + ds + 3 * (i - nroot), SR_SKIN_EPS, r);
            // A_c = R^T A_p: gR = A_p gA_c^T, gA_p += R gA_c
            float* gR = sgR + 9 * (i - nroot);
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int n = 0; n < 3; ++n)
                    gR[3 * m + n] = (Ap[3 * m] * gA[3 * n] + Ap[3 * m + 1] * gA[3 * n + 1]) + Ap[3 * m + 2] * gA[3 * n + 2];
            float add[9];
            mat3_mul(r, gA, add);
            const float dj[3] = {ch[15 * i + 12] - Ap[12], ch[15 * i + 13] - Ap[13], ch[15 * i + 14] - Ap[14]};
            float* gAp = sg + 12 * p;
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int n = 0; n < 3; ++n) gAp[3 * m + n] += add[3 * m + n] + dj[m] * gt[n];
            float gd[3];
            vec_matT(gt, Ap, gd);
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                sgJ[3 * i + n] += gd[n];
                sgJ[3 * p + n] -= gd[n];
                gAp[9 + n] += gt[n];
            }
        }
        for (int i = 0; i < nroot; ++i)
#pragma unroll
            for (int n = 0; n < 3; ++n) sgJ[3 * i + n] += sg[12 * i + 9 + n];
        if (gpose) {
            // dL/dR = exp(s) glin: pose_bwd forms it as 0 + exp(s) glin, so a -0 there is now +0 (no value changes)
            float* o = gpose + 7 * b;
            pose_bwd(pose + 7 * b, glin, nullptr, o);
            o[3] = gtg[0]; o[4] = gtg[1]; o[5] = gtg[2];
        }
    }
    __syncthreads();
    const float pw = (greg && lam != 0.f) ? 2.f * lam * greg[0] : 0.f;
    for (int k = lane; k < ds; k += 64) {
        float a = gcx[(int64_t)b * D + k];
        for (int o = 0; o < 3 * nj; ++o) a += js[(int64_t)o * ds + k] * sgJ[o];
        if (pw != 0.f) {
            const float s = sigma ? sigma[k] : 1.f;
            a += pw * (c[k] / s) / s;
        }
        gcoeff[(int64_t)b * dc + k] = a;
    }
    for (int i = lane; i < np; i += 64) {
        const float* th = c + ds + 3 * i;
        float g[9], ga[3];
#pragma unroll
        for (int e = 0; e < 9; ++e) g[e] = sgR[9 * i + e] + gcx[(int64_t)b * D + ds + 9 * i + e];
        rodrigues_bwd(th, SR_SKIN_EPS, g, ga);
        if (pw != 0.f) {
            float y[3], z[3];
            if (pinv) { vec_mat(th, pinv + 9 * i, y); vec_matT(y, pinv + 9 * i, z); }
            else { z[0] = th[0]; z[1] = th[1]; z[2] = th[2]; }
            ga[0] += pw * z[0]; ga[1] += pw * z[1]; ga[2] += pw * z[2];
        }
        float* o = gcoeff + (int64_t)b * dc + ds + 3 * i;
        o[0] = ga[0]; o[1] = ga[1]; o[2] = ga[2];
    }
}

bool joints_ok(int64_t nj, int64_t nroot) { return nj >= 1 && nj <= SR_SKIN_MAXJ && nroot >= 1 && nroot <= nj; }

}  // namespace

extern "C" int sr_skin_joints_fwd(float* cx, float* G, float* chain, float* reg, const float* coeff, const float* pose,
                                  const float* j0, const float* js, const int32_t* parent, const float* sigma,
                                  const float* pose_inv, float lam, int64_t B, int64_t nj, int64_t nroot, int64_t ds,
                                  sr_stream_t stream) {
    if (B < 0 || ds < 0) return SR_EINVAL;
    if (!joints_ok(nj, nroot)) return SR_ERANGE;
    if (B == 0) return SR_OK;
    if (!cx || !G || !chain || !coeff || !j0 || (ds > 0 && !js) || (nj > nroot && !parent)) return SR_EINVAL;
    if (B > (1 << 20) || ds >= (1LL << 20)) return SR_ERANGE;
    hipLaunchKernelGGL(k_skin_joints, dim3(1), dim3(256), 0, sr_stream(stream), cx, G, chain, reg, coeff, pose, j0, js,
                       parent, sigma, pose_inv, lam, (int)B, (int)nj, (int)nroot, (int)ds);
    return sr_launch_status();
}

extern "C" int sr_skin_fwd(float* v, float* vp, const float* st, const float* vt, const float* cx, const float* wts,
                           const float* G, int64_t B, int64_t nv, int64_t D, int64_t nj, sr_stream_t stream) {
    if (B < 0 || nv < 0 || D < 0) return SR_EINVAL;
    if (nj < 1 || nj > SR_SKIN_MAXJ) return SR_ERANGE;
    if (B == 0 || nv == 0) return SR_OK;
    if (!v || !vp || !vt || !wts || !G || (D > 0 && (!st || !cx))) return SR_EINVAL;
    if (D + 12 * nj > SR_SKIN_MAX_LDS || nv >= (1LL << 30) || D >= (1LL << 20)) return SR_ERANGE;
    const int64_t blocks = sr_ceil_div(nv, 4);
    const bool vec = D % 4 == 0 && sr_aligned16(st);
    // the coefficients and transforms of a launch's samples sit in LDS: larger batches go in slices of `chunk` samples
    // (every array is sample-major, so a slice is a pointer offset), each slice one more pass over st
    const int64_t chunk = SR_SKIN_MAX_LDS / (D + 12 * nj);
    for (int64_t b0 = 0; b0 < B; b0 += chunk) {
        const int64_t nb = B - b0 < chunk ? B - b0 : chunk;
        const size_t lds = (size_t)(nb * (D + 12 * nj)) * sizeof(float);
        float* vo = v + b0 * nv * 3;
        float* vpo = vp + b0 * nv * 3;
        const float* cxo = cx + b0 * D;
        const float* Go = G + b0 * nj * 12;
        if (vec)
            hipLaunchKernelGGL(k_skin_fwd<4>, dim3((unsigned)blocks), dim3(256), lds, sr_stream(stream), vo, vpo, st, vt,
                               cxo, wts, Go, (int)nb, (int)nv, (int)D, (int)nj);
        else
            hipLaunchKernelGGL(k_skin_fwd<1>, dim3((unsigned)blocks), dim3(256), lds, sr_stream(stream), vo, vpo, st, vt,
                               cxo, wts, Go, (int)nb, (int)nv, (int)D, (int)nj);
        const int rc = sr_launch_status();
        if (rc != SR_OK) return rc;
    }
    return SR_OK;
}

extern "C" int64_t sr_skin_bwd_scratch_floats(int64_t nv, int64_t B, int64_t nj) {
    if (nv <= 0 || B <= 0 || nj <= 0) return 0;
    return B * sr_ceil_div(nv, 256) * nj * 12;
}

extern "C" int sr_skin_bwd(float* gvp, float* part, const float* gv, const float* gvn, const float* vp, const float* wts,
                           const float* G, int64_t B, int64_t nv, int64_t nj, sr_stream_t stream) {
    if (B < 0 || nv < 0) return SR_EINVAL;
    if (nj < 1 || nj > SR_SKIN_MAXJ) return SR_ERANGE;
    if (B == 0 || nv == 0) return SR_OK;
    if (!gvp || !part || !gv || !vp || !wts || !G) return SR_EINVAL;
    if (B > 65535 || nv >= (1LL << 30)) return SR_ERANGE;
    hipLaunchKernelGGL(k_skin_bwd, dim3((unsigned)sr_ceil_div(nv, 256), (unsigned)B), dim3(256), 0, sr_stream(stream),
                       gvp, part, gv, gvn, vp, wts, G, (int)nv, (int)nj);
    return sr_launch_status();
}

extern "C" int sr_skin_joints_bwd(float* gcoeff, float* gpose, const float* gcx, const float* part, const float* coeff,
                                  const float* pose, const float* chain, const float* js, const int32_t* parent,
                                  const float* sigma, const float* pose_inv, float lam, const float* greg, int64_t B,
                                  int64_t nblk, int64_t nj, int64_t nroot, int64_t ds, sr_stream_t stream) {
    if (B < 0 || ds < 0 || nblk < 0) return SR_EINVAL;
    if (!joints_ok(nj, nroot)) return SR_ERANGE;
    if (B == 0) return SR_OK;
    if (!gcoeff || !gcx || !coeff || !chain || (nblk > 0 && !part) || (ds > 0 && !js) || (nj > nroot && !parent) ||
        (gpose && !pose))
        return SR_EINVAL;
    if (B > 0x7fffffff || ds >= (1LL << 20) || nblk > 0x7fffffff) return SR_ERANGE;
    hipLaunchKernelGGL(k_skin_joints_bwd, dim3((unsigned)B), dim3(64), 0, sr_stream(stream), gcoeff, gpose, gcx, part,
                       coeff, pose, chain, js, parent, sigma, pose_inv, lam, greg, (int)nblk, (int)nj, (int)nroot,
                       (int)ds);
    return sr_launch_status();
}
