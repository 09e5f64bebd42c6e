// Backward of the rasterizer.
// k_dcoeff (API parity with rasterize_gpu_backward, coalesced through LDS), and the fused gradient
// of the autograd Function as a deterministic two-phase GATHER — no float atomics, run-to-run identical:
//   k_first_pix  one lane per pixel: integer atomicMin of the row-major pixel index into a per-(sample, triangle)
//                table — the first pixel a triangle won in box order, its LEADER (order-independent, deterministic);
//   k_grad_pix   one lane per PIXEL (coalesced winner-map reads); the leaders of a workgroup's 256 pixels are
//                compacted through LDS, then each sums, in box order, d/d(3 vertices) and d/d(3 attribute rows) over
//                the triangle's pixels (winner map written by k_resolve) into the triangle's three corner records;
//   k_grad_big   the large triangles k_depth_keys listed: one workgroup each, fixed-order tree over the lanes;
//   k_grad_pix_alias / k_grad_big_alias  the same two on an image with h > w, where samples alias onto pixels;
//   k_grad_vert  one lane per (sample, vertex): sums the corner blocks of its incident triangles in the fixed
//                order of a per-topology incidence list (corner-major, ascending triangle id).
// (The reference builds a COO matrix per call and runs sparse.mm, op/rasterize.py:46-77; round 1 of this repo
// scattered with float atomics.)
#include "rasterize_grad.h"

#include <algorithm>
#include <type_traits>

#include "raster_layout.h"
#include "raster_math.h"
#include "rasterize_tiled.h"

namespace {

// dcoeff [b*h*w, 27]: 256 pixels per workgroup, staged through LDS so the 27-float records leave
// as fully coalesced rows.
template <typename R>
__global__ __launch_bounds__(256) void k_dcoeff(long long b, long long n, long long h, long long w,
                                                bool perspective, const R* __restrict__ v,
                                                const long long* __restrict__ index,
                                                R* __restrict__ dcoeff, R eps) {
    __shared__ R s_g[256 * 27];
    const long long hw = h * w, total = b * hw;
    const long long base = (long long)blockIdx.x * 256;
    const long long g = base + threadIdx.x;
    R jac[27];
#pragma unroll
    for (int l = 0; l < 27; ++l) jac[l] = 0;
    if (g < total) {
        R p[9];
        long long ids[3];
        if (load_pixel_tri<R>(index, g, n * b, v, p, ids)) {
            const long long pix = g % hw;
            weight_jacobian<R>(p, (R)(pix % w), (R)(pix / w), (R)h, (R)w, jac, perspective, eps);
        }
    }
#pragma unroll
    for (int l = 0; l < 27; ++l) s_g[threadIdx.x * 27 + l] = jac[l];
    __syncthreads();
    const long long remain = total - base;
    const int cnt = (int)((remain < 256 ? remain : 256) * 27);
    for (int i = threadIdx.x; i < cnt; i += 256) dcoeff[base * 27 + i] = s_g[i];
}

// ---- fused gradient, phase 1: per-triangle sums over the pixels the triangle won ----------------------------
// Scratch layout: one 16-byte aligned row of RS floats per (sample, triangle), written whole with float4 stores
// (scattered 4-byte stores cost one L2 transaction each: measured 130 of 217 us):
//   corner k at [k * (NVC + CT)]:  NVC vertex-gradient values (x, y[, z]), then CT attribute-gradient values;
// NVC = 2 orthographic (d/dz is identically zero there), 3 perspective.  A byte per row marks the written ones.
//
// Per-triangle constants of d(weights)/d(vertices) (reference barycentric_grad, op/rasterize.h:169-228).
// Orthographic: dcoeff[wi][vert][comp] = -c[vert] * E[wi + 3*((comp+1)%3)] with the z column zeroed, so the
// 27-entry Jacobian collapses to   g_vert.x = -c[vert] * sum_wi d_wi E[3+wi],  g_vert.y = -c[vert] * sum_wi d_wi E[6+wi]
// (the same products re-associated): 9 triangle constants, ~20 flops per pixel, no 27-register array.
template <typename R, bool PERSP>
struct JacTri;

template <typename R>
struct JacTri<R, false> {
    static constexpr int NV = 6;           // accumulated vertex-gradient values: (vertex, x|y)
    R E0, E1, E2, E3, E4, E5, E6, E7, E8;
    bool ok;
    __device__ __forceinline__ void init(const R p[9], R eps) {
        R m0 = p[3] * p[7], m1 = p[4] * p[6];
        const R e0 = m0 - m1;
        m0 = p[1] * p[6]; m1 = p[0] * p[7];
        const R e1 = m0 - m1;
        m0 = p[0] * p[4]; m1 = p[1] * p[3];
        const R e2 = m0 - m1;
        R det = e0 + e1;
        det = det + e2;
        ok = det < -eps || det > eps;
        E0 = e0 / det; E1 = e1 / det; E2 = e2 / det;
        E3 = (p[4] - p[7]) / det; E4 = (p[7] - p[1]) / det; E5 = (p[1] - p[4]) / det;
        E6 = (p[6] - p[3]) / det; E7 = (p[0] - p[6]) / det; E8 = (p[3] - p[0]) / det;
    }
    __device__ __forceinline__ void add(R (&gv)[NV], R d0, R d1, R d2, R px, R py, R sw, R sh, R eps) const {
        const R u = (px * 2 - sw + 1) / sw;
        const R vv = (py * -2 + sh - 1) / sh;
        const R c0 = (E0 + E3 * u) + E6 * vv;
        const R c1 = (E1 + E4 * u) + E7 * vv;
        const R c2 = (E2 + E5 * u) + E8 * vv;
        const R qx = (d0 * E3 + d1 * E4) + d2 * E5;
        const R qy = (d0 * E6 + d1 * E7) + d2 * E8;
        gv[0] -= c0 * qx; gv[1] -= c0 * qy;
        gv[2] -= c1 * qx; gv[3] -= c1 * qy;
        gv[4] -= c2 * qx; gv[5] -= c2 * qy;
    }
    // value j of vertex k (0: x, 1: y, 2: z)
    static __device__ __forceinline__ R get(const R (&gv)[NV], int k, int j) { return j == 2 ? (R)0 : gv[2 * k + j]; }
};

template <typename R>
struct JacTri<R, true> {
    static constexpr int NV = 9;
    R p[9];
    bool ok;
    __device__ __forceinline__ void init(const R q[9], R) {
#pragma unroll
        for (int i = 0; i < 9; ++i) p[i] = q[i];
        ok = true;
    }
    __device__ __forceinline__ void add(R (&gv)[NV], R d0, R d1, R d2, R px, R py, R sw, R sh, R eps) const {
        R jac[27];
        if (!weight_jacobian<R>(p, px, py, sw, sh, jac, true, eps)) return;
#pragma unroll
        for (int j = 0; j < 9; ++j) gv[j] += d0 * jac[j] + d1 * jac[9 + j] + d2 * jac[18 + j];
    }
    static __device__ __forceinline__ R get(const R (&gv)[NV], int k, int j) { return gv[3 * k + j]; }
};

template <typename R, int CT, bool PERSP>
struct TriAcc {
    R gv[JacTri<R, PERSP>::NV];
    R gt[3 * CT];
    int n;
    __device__ __forceinline__ void clear() {
        n = 0;
#pragma unroll
        for (int j = 0; j < JacTri<R, PERSP>::NV; ++j) gv[j] = 0;
#pragma unroll
        for (int j = 0; j < 3 * CT; ++j) gt[j] = 0;
    }
};

// One pixel of triangle `ti` (skipped unless the triangle won it).
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void grad_pixel(TriAcc<R, CT, PERSP>& acc, const Tri<R>& t, const JacTri<R, PERSP>& jt,
                                           bool want_v, int x, int y, long long w, long long hw, long long h_arg,
                                           R eps, const int* __restrict__ wins, int ti,
                                           const R* __restrict__ gos, const R* __restrict__ tex0,
                                           const R* __restrict__ tex1, const R* __restrict__ tex2,
                                           int tex_c, int ch0, long long gcs) {
    const long long pix = x + (long long)y * w;
    if (pix >= hw || wins[pix] != ti) return;
    R c0, c1, c2, z;
    shade<R>(t, x, y, PERSP, eps, c0, c1, c2, z);        // same bits as k_resolve used for the interpolation
    // gcs: channel stride of grad_out — 1 for [b,h,w,c] (pixel stride tex_c), h*w for [b,c,h,w] (pixel stride 1)
    const R* go = gos + pix * (gcs == 1 ? tex_c : 1);
    acc.n += 1;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        if (ch0 + j < tex_c) {
            const R gch = go[(ch0 + j) * gcs];
            acc.gt[j] += gch * c0;
            acc.gt[CT + j] += gch * c1;
            acc.gt[2 * CT + j] += gch * c2;
        }
    }
    if (want_v) {
        R d0 = 0, d1 = 0, d2 = 0;
        for (int ch = 0; ch < tex_c; ++ch) {
            const R gch = go[ch * gcs];
            d0 += gch * tex0[ch];
            d1 += gch * tex1[ch];
            d2 += gch * tex2[ch];
        }
        jt.add(acc.gv, d0, d1, d2, (R)x, (R)y, (R)h_arg, (R)w, eps);
    }
}

// The same pixel with the triangle's three attribute rows already in registers (tex_c <= 4: the normal maps of
// the generator): k_grad_pix fetches them together with the vertex positions, one round trip earlier, and once per
// triangle instead of once per pixel.  Same operations in the same order as grad_pixel.
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void grad_pixel_regs(TriAcc<R, CT, PERSP>& acc, const Tri<R>& t, const JacTri<R, PERSP>& jt,
                                                bool want_v, int x, int y, long long w, long long hw, long long h_arg,
                                                R eps, const int* __restrict__ wins, int ti,
                                                const R* __restrict__ gos, const R (&tx)[3][4], int tex_c, int ch0,
                                                long long gcs) {
    // (the caller walks the pixels of its winner mask: this pixel IS inside the image and won by `ti`)
    const long long pix = x + (long long)y * w;
    R c0, c1, c2, z;
    shade<R>(t, x, y, PERSP, eps, c0, c1, c2, z);
    const R* go = gos + pix * (gcs == 1 ? tex_c : 1);
    R gch[4];
    if (tex_c == 3 && gcs == 1) {
        load3<R>(go, gch[0], gch[1], gch[2]);
        gch[3] = (R)0;
    } else {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) gch[ch] = ch < tex_c ? go[ch * gcs] : (R)0;
    }
    acc.n += 1;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        if (j < tex_c) {                                 // (tex_c <= 4: one channel chunk, ch0 == 0)
            acc.gt[j] += gch[j] * c0;
            acc.gt[CT + j] += gch[j] * c1;
            acc.gt[2 * CT + j] += gch[j] * c2;
        }
    }
    if (want_v) {
        R d0 = 0, d1 = 0, d2 = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch < tex_c) {
                d0 += gch[ch] * tx[0][ch];
                d1 += gch[ch] * tx[1][ch];
                d2 += gch[ch] * tx[2][ch];
            }
        }
        jt.add(acc.gv, d0, d1, d2, (R)x, (R)y, (R)h_arg, (R)w, eps);
    }
}

__device__ __forceinline__ float sr_shfl_down(float x, int off) { return __shfl_down(x, off, SR_WAVE); }
__device__ __forceinline__ double sr_shfl_down(double x, int off) { return __shfl_down(x, off, SR_WAVE); }

// Fixed-order sum over the 256 lanes of the workgroup (wave tree, then waves 0..3 in order); same value on all lanes.
template <typename R>
__device__ __forceinline__ R block_sum_256(R x, R* s_part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += sr_shfl_down(x, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = x;
    __syncthreads();
    R tot = s_part[0];
    tot += s_part[1];
    tot += s_part[2];
    tot += s_part[3];
    return tot;
}

// One record per triangle: for each corner k the first four of its CORNER values (d/d(vertex) then d/d(attribute row))
// as an aligned quad at 4 k, the remaining CORNER - 4 behind the three quads.  k_grad_vert, which is bound by the number
// of scattered load instructions it issues (every lane of a wave hits a different line), fetches a corner with one
// 16-byte load + one scalar instead of five scalars.
template <int CT, bool PERSP>
struct RowShape {
    static constexpr int NVC = PERSP ? 3 : 2;
    static constexpr int CORNER = NVC + CT;
    static constexpr int TAIL = CORNER > 4 ? CORNER - 4 : 0;     // values of a corner behind its quad
    static constexpr int RS = (12 + 3 * TAIL + 3) / 4 * 4;       // values per record, multiple of 4
    static __host__ __device__ constexpr int at(int k, int j) { return j < 4 ? 4 * k + j : 12 + k * TAIL + (j - 4); }
};
// a record, and the quad + tail planes of a triangle's three corner slots, fit the space the scratch gives a triangle
template <int CT>
constexpr bool row_fits() {
    return RowShape<CT, false>::RS <= GRAD_ROW_VALUES && RowShape<CT, true>::RS <= GRAD_ROW_VALUES &&
           GRAD_QUAD_VALUES + 3 * RowShape<CT, true>::TAIL <= GRAD_ROW_VALUES;
}
static_assert(row_fits<1>() && row_fits<2>() && row_fits<3>() && row_fits<4>(), "GRAD_ROW_VALUES (raster_layout.h)");

template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void store_row(const TriAcc<R, CT, PERSP>& acc, R* __restrict__ tg,
                                          long long rowid) {
    using S = RowShape<CT, PERSP>;
    R vals[S::RS];
#pragma unroll
    for (int i = 0; i < S::RS; ++i) vals[i] = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int j = 0; j < S::NVC; ++j) vals[S::at(k, j)] = JacTri<R, PERSP>::get(acc.gv, k, j);
#pragma unroll
        for (int j = 0; j < CT; ++j) vals[S::at(k, S::NVC + j)] = acc.gt[k * CT + j];
    }
    R* row = tg + rowid * S::RS;
    if (sizeof(R) == 4) {
        float4* dst = reinterpret_cast<float4*>(row);
#pragma unroll
        for (int i = 0; i < S::RS / 4; ++i)
            dst[i] = make_float4((float)vals[4 * i], (float)vals[4 * i + 1], (float)vals[4 * i + 2], (float)vals[4 * i + 3]);
    } else {
        double2* dst = reinterpret_cast<double2*>(row);
#pragma unroll
        for (int i = 0; i < S::RS / 2; ++i) dst[i] = make_double2((double)vals[2 * i], (double)vals[2 * i + 1]);
    }
}

// VERTEX-MAJOR corner slots (round 6).  The incidence list of a topology is sorted by vertex, so position e of the list
// (0 <= e < 3 nf) is a slot that belongs to ONE vertex, and the slots of a vertex — and of consecutive vertices — are
// contiguous.  Phase 1 writes the CORNER values of corner k of triangle f straight into slot e = slot_of[k * nf + f]
// (the inverse permutation of the list) instead of a 64-byte record per triangle; phase 2 then reads one contiguous span
// per vertex, consecutive lanes consecutive spans, instead of chasing six scattered records: same values, same summation
// order, a coalesced stream in place of a divergent gather.  Layout: quad plane Q[b * 3 nf] (the first four values of a
// corner, one 16-byte store / load) and TAIL scalar planes T[j][b * 3 nf] for the values behind it.
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void store_slots(const TriAcc<R, CT, PERSP>& acc, R* __restrict__ quad, R* __restrict__ tail,
                                            long long plane, long long slot_base, const int* __restrict__ slot_of,
                                            long long nf, long long ti) {
    using S = RowShape<CT, PERSP>;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        R vals[S::CORNER < 4 ? 4 : S::CORNER];
#pragma unroll
        for (int j = 0; j < 4; ++j) vals[j] = 0;
#pragma unroll
        for (int j = 0; j < S::NVC; ++j) vals[j] = JacTri<R, PERSP>::get(acc.gv, k, j);
#pragma unroll
        for (int j = 0; j < CT; ++j) vals[S::NVC + j] = acc.gt[k * CT + j];
        const long long e = slot_base + slot_of[k * nf + ti];
        if (sizeof(R) == 4) {
            reinterpret_cast<float4*>(quad)[e] = make_float4((float)vals[0], (float)vals[1], (float)vals[2], (float)vals[3]);
        } else {
            double2* dst = reinterpret_cast<double2*>(quad) + 2 * e;
            dst[0] = make_double2((double)vals[0], (double)vals[1]);
            dst[1] = make_double2((double)vals[2], (double)vals[3]);
        }
#pragma unroll
        for (int j = 0; j < S::TAIL; ++j) tail[j * plane + e] = vals[4 + j];
    }
}

// slot_of[adj[e]] = e: the inverse of a topology's incidence list (one int per corner; built per call when the caller
// does not hand a cached table over)
__global__ __launch_bounds__(256) void k_slot_inverse(long long n3, const int* __restrict__ adj, int* __restrict__ slot_of,
                                                      long long adj_bstride) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n3) return;
    const long long s = blockIdx.y;
    slot_of[s * n3 + adj[s * adj_bstride + e]] = (int)e;
}

// Large triangles (the list k_depth_keys recorded): one workgroup per triangle walks the box together; each lane
// sums its pixels in order, then a fixed-order tree over the 256 lanes.
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void grad_big_body(long long nv, long long nf, long long h, long long w, bool repeat_f,
                                              const R* __restrict__ v, const R* __restrict__ tex, int tex_c, int ch0,
                                              const long long* __restrict__ f, const int* __restrict__ win,
                                              const int* __restrict__ big, const R* __restrict__ grad_out, bool want_v,
                                              R* __restrict__ tg, R eps, bool chw, const int* __restrict__ slot_of,
                                              long long slot_bs, R* __restrict__ tail, long long plane) {
    __shared__ R s_part[4];
    const long long hw = h * w;
    const int count = big[0];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const long long g = big[1 + q];
        const long long s = g / nf, ti = g - s * nf;
        const R* vs = v + s * nv * 3;
        const long long* fs = repeat_f ? f : f + s * nf * 3;
        Tri<R> t;
        long long i0, i1, i2;
        load_tri<R>(t, vs, fs, ti, nv, i0, i1, i2);
        const R praw[9] = {t.p0, t.p1, t.p2, t.p3, t.p4, t.p5, t.p6, t.p7, t.p8};
        JacTri<R, PERSP> jt;
        jt.init(praw, eps);
        tri_setup<R>(t, h, w, PERSP, eps);
        TriAcc<R, CT, PERSP> acc;
        acc.clear();
        const bool distinct = want_v && jt.ok && i0 != i1 && i0 != i2 && i1 != i2;
        const R* tb = tex + s * nv * tex_c;
        const int bw = t.x1 - t.x0 + 1;
        const long long npx = (long long)bw * (t.y1 - t.y0 + 1);
        for (long long p = threadIdx.x; p < npx; p += 256) {
            const int yy = (int)(p / bw);
            grad_pixel<R, CT, PERSP>(acc, t, jt, distinct, t.x0 + (int)(p - (long long)yy * bw), t.y0 + yy, w, hw, h,
                                     eps, win + s * hw, (int)ti, grad_out + s * hw * tex_c, tb + i0 * tex_c,
                                     tb + i1 * tex_c, tb + i2 * tex_c, tex_c, ch0, chw ? hw : 1);
        }
        const R cnt = block_sum_256<R>((R)acc.n, s_part);
#pragma unroll
        for (int j = 0; j < JacTri<R, PERSP>::NV; ++j) acc.gv[j] = block_sum_256<R>(acc.gv[j], s_part);
#pragma unroll
        for (int j = 0; j < 3 * CT; ++j) acc.gt[j] = block_sum_256<R>(acc.gt[j], s_part);
        if (threadIdx.x == 0 && cnt > 0) {
            if (slot_of) store_slots<R, CT, PERSP>(acc, tg, tail, plane, s * 3 * nf, slot_of + s * slot_bs, nf, ti);
            else store_row<R, CT, PERSP>(acc, tg, g);
        }
    }
}

template <typename R, int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_big(long long nv, long long nf, long long h, long long w,
                                                  bool repeat_f, const R* __restrict__ v,
                                                  const R* __restrict__ tex, int tex_c, int ch0,
                                                  const long long* __restrict__ f, const int* __restrict__ win,
                                                  const int* __restrict__ big, const R* __restrict__ grad_out,
                                                  bool want_v, R* __restrict__ tg,
                                                  R eps, bool chw, const int* __restrict__ slot_of, long long slot_bs,
                                                  R* __restrict__ tail, long long plane) {
    grad_big_body<R, CT, PERSP>(nv, nf, h, w, repeat_f, v, tex, tex_c, ch0, f, win, big, grad_out, want_v, tg, eps, chw,
                                slot_of, slot_bs, tail, plane);
}

// first[s * nf + t] = the smallest row-major pixel index triangle t of sample s won (INT_MAX: none).  Row-major order
// over the image restricted to a triangle's box IS box order, so that pixel is the triangle's leader.
// A pixel whose left or upper neighbour was won by the same triangle cannot be the minimum and skips the atomic
// (most of a triangle's pixels: the table sees little more than one update per visible triangle).
// `built` (the state word the forward pass left behind the table): non-zero = the tiled forward has already built
// the table, every workgroup leaves at once.  The decision is the FORWARD's record, not a predicate re-evaluated at
// backward time (environment flips, a different heuristic input: the table would be read uninitialised).
__device__ __forceinline__ void first_pix_body(long long total, long long hw, long long w, long long nf,
                                               const int* __restrict__ win, int* __restrict__ first,
                                               const int* __restrict__ built) {
    if (*built) return;
    // grid-stride: the launch is capped at a few thousand workgroups, so that the common case (table already built by
    // the tiled forward: every workgroup leaves at the line above) costs ~1 us instead of retiring b*h*w/256 of them
    const long long stride = (long long)gridDim.x * 256;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += stride) {
        const int ti = win[g];
        if (ti < 0) continue;
        const long long s = g / hw, pix = g - s * hw;
        const long long x = pix % w;
        if (x > 0 && win[g - 1] == ti) continue;
        if (pix >= w && win[g - w] == ti) continue;
        atomicMin(&first[s * nf + ti], (int)pix);                // integer minimum: order independent
    }
}

__global__ __launch_bounds__(256) void k_first_pix(long long total, long long hw, long long w, long long nf,
                                                   const int* __restrict__ win, int* __restrict__ first,
                                                   const int* __restrict__ built) {
    first_pix_body(total, hw, w, nf, win, first, built);
}

// Small triangles: one lane per (sample, TRIANGLE).  The leader table says in ONE coalesced load whether the triangle
// won a pixel at all (culled, hidden and sub-pixel triangles leave at once) and where its first pixel is; the lane
// then sums the triangle's pixels in box order and writes the records.  Consecutive lanes own consecutive triangles:
// the index loads and the row stores are coalesced, and because visibility is spatially coherent on a mesh the waves are
// mostly dense or empty.  (History at config[3]: one lane per pixel with a 16-probe leader test, 202 us; leaders
// compacted per workgroup through LDS, 122-129 us; a dense leader list, 86 us + 600 us for its single append
// counter; this form needs neither list nor counter.)
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void grad_pix_body(long long b, long long nv, long long nf, long long h, long long w,
                                              bool repeat_f, const R* __restrict__ v, const R* __restrict__ tex, int tex_c,
                                              int ch0, const long long* __restrict__ f, const int* __restrict__ win,
                                              const int* __restrict__ first, unsigned long long* __restrict__ valid,
                                              const R* __restrict__ grad_out, bool want_v, R* __restrict__ tg, R eps,
                                              bool chw, const int* __restrict__ slot_of, long long slot_bs,
                                              R* __restrict__ tail, long long plane) {
    __shared__ int s_row[256], s_pix[256];
    __shared__ int s_cnt[4];
    const long long hw = h * w;
    const long long row0 = (long long)blockIdx.x * 256;
    int lead_pix;
    long long row;
    {
        const long long rq = row0 + threadIdx.x;
        const int pq = rq < b * nf ? first[rq] : 0x7FFFFFFF;
        // one bit per record, "this triangle won a pixel: its record is written" (by this kernel or by k_grad_big) —
        // what k_grad_vert tests before it reads a record: a wave's 64 consecutive rows are one word
        const unsigned long long won = __ballot(pq != 0x7FFFFFFF);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        if (lane == 0 && rq < b * nf) valid[rq >> 6] = won;                    // (waves beyond the last row own no word)
        // the winning triangles of the workgroup's 256 rows, compacted: the long part below runs in dense waves
        if (lane == 0) s_cnt[wv] = __popcll(won);
        __syncthreads();
        int base = 0;
        for (int i = 0; i < wv; ++i) base += s_cnt[i];
        const int n_won = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (pq != 0x7FFFFFFF) {
            const int slot = base + __popcll(won & ((1ull << lane) - 1ull));
            s_row[slot] = threadIdx.x;
            s_pix[slot] = pq;
        }
        __syncthreads();
        if ((int)threadIdx.x >= n_won) return;
        row = row0 + s_row[threadIdx.x];
        lead_pix = s_pix[threadIdx.x];
    }
    const long long s = row / nf;
    const int ti = (int)(row - s * nf);
    const long long pix = lead_pix;
    const int py = (int)(pix / w), px = (int)(pix - (long long)py * w);
    const R* vs = v + s * nv * 3;
    const long long* fs = repeat_f ? f : f + s * nf * 3;
    Tri<R> t;
    long long i0, i1, i2;
    load_tri<R>(t, vs, fs, ti, nv, i0, i1, i2);
    // attribute rows of the three corners: in flight together with the vertex positions (up to four channels)
    const R* tb = tex + s * nv * tex_c;
    const bool tex_regs = tex_c <= 4;
    R tx[3][4];
    if (tex_c == 3) {                               // the normal maps of the generator: one instruction per corner
        load3<R>(tb + i0 * 3, tx[0][0], tx[0][1], tx[0][2]);
        load3<R>(tb + i1 * 3, tx[1][0], tx[1][1], tx[1][2]);
        load3<R>(tb + i2 * 3, tx[2][0], tx[2][1], tx[2][2]);
        tx[0][3] = tx[1][3] = tx[2][3] = (R)0;
    } else {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const bool have = tex_regs && ch < tex_c;
            tx[0][ch] = have ? tb[i0 * tex_c + ch] : (R)0;
            tx[1][ch] = have ? tb[i1 * tex_c + ch] : (R)0;
            tx[2][ch] = have ? tb[i2 * tex_c + ch] : (R)0;
        }
    }
    const R praw[9] = {t.p0, t.p1, t.p2, t.p3, t.p4, t.p5, t.p6, t.p7, t.p8};
    if constexpr (sizeof(R) == 4) {
        // a triangle that won a pixel was accepted by the forward pass: on a square image the short setup (no
        // rejection tests, no 64-bit conversion emulation) gives the same box and the same edge constants
        if (h == w && h < 0x40000000LL) tri_setup_accepted<PERSP>(t, (int)h, eps, true);
        else tri_setup<R>(t, h, w, PERSP, eps);
    } else {
        tri_setup<R>(t, h, w, PERSP, eps);
    }
    if ((long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > BIG_BOX) return;      // k_grad_big owns it
    const int* wins = win + s * hw;
    // which pixels of the box did this triangle win?  All winner-map loads are issued together (a loop that
    // leaves at the first hit would serialise one memory round trip per pixel).  Bit index = box order.
    const int bw = t.x1 - t.x0 + 1, bh = t.y1 - t.y0 + 1;
    unsigned long long mask = 0;
    if (bw <= 4 && bh <= 4) {
        int got[16];
        if (t.x0 + 3 < w && t.x0 + 3 + (long long)(t.y0 + 3) * w < hw) {
            // a row of the box = four consecutive ints inside the image row: one 16-byte load per row (4-byte aligned)
            typedef int i4u __attribute__((ext_vector_type(4), aligned(4)));
#pragma unroll
            for (int yy = 0; yy < 4; ++yy) {
                const i4u r = *reinterpret_cast<const i4u*>(wins + t.x0 + (long long)(t.y0 + yy) * w);
                got[4 * yy + 0] = (0 < bw && yy < bh) ? r.x : -1;
                got[4 * yy + 1] = (1 < bw && yy < bh) ? r.y : -1;
                got[4 * yy + 2] = (2 < bw && yy < bh) ? r.z : -1;
                got[4 * yy + 3] = (3 < bw && yy < bh) ? r.w : -1;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int xx = i & 3, yy = i >> 2;
                const long long q = (t.x0 + xx) + (long long)(t.y0 + yy) * w;
                got[i] = (xx < bw && yy < bh && q < hw) ? wins[q] : -1;
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (got[i] == ti) mask |= 1ull << ((i >> 2) * bw + (i & 3));
    } else {
        int p = 0;
        for (int y = t.y0; y <= t.y1; ++y)
            for (int x = t.x0; x <= t.x1; ++x, ++p) {
                const long long q = x + (long long)y * w;
                if (q < hw && wins[q] == ti) mask |= 1ull << p;
            }
    }
    const int self = (py - t.y0) * bw + (px - t.x0);
    if (mask & ((1ull << self) - 1ull)) return;          // an earlier pixel of the box leads this triangle
    JacTri<R, PERSP> jt;
    jt.init(praw, eps);
    TriAcc<R, CT, PERSP> acc;
    acc.clear();
    const bool distinct = want_v && jt.ok && i0 != i1 && i0 != i2 && i1 != i2;
    while (mask) {                                        // ascending bit = box order
        const int p = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        const int yy = p / bw;
        if (tex_regs)
            grad_pixel_regs<R, CT, PERSP>(acc, t, jt, distinct, t.x0 + (p - yy * bw), t.y0 + yy, w, hw, h, eps, wins, ti,
                                          grad_out + s * hw * tex_c, tx, tex_c, ch0, chw ? hw : 1);
        else
            grad_pixel<R, CT, PERSP>(acc, t, jt, distinct, t.x0 + (p - yy * bw), t.y0 + yy, w, hw, h, eps, wins, ti,
                                     grad_out + s * hw * tex_c, tb + i0 * tex_c, tb + i1 * tex_c, tb + i2 * tex_c, tex_c,
                                     ch0, chw ? hw : 1);
    }
    if (slot_of) store_slots<R, CT, PERSP>(acc, tg, tail, plane, s * 3 * nf, slot_of + s * slot_bs, nf, ti);
    else store_row<R, CT, PERSP>(acc, tg, row);
}

template <typename R, int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_pix(long long b, long long nv, long long nf, long long h,
                                                  long long w, bool repeat_f, const R* __restrict__ v,
                                                  const R* __restrict__ tex, int tex_c, int ch0,
                                                  const long long* __restrict__ f, const int* __restrict__ win,
                                                  const int* __restrict__ first,
                                                  unsigned long long* __restrict__ valid,
                                                  const R* __restrict__ grad_out, bool want_v,
                                                  R* __restrict__ tg, R eps, bool chw, const int* __restrict__ slot_of,
                                                  long long slot_bs, R* __restrict__ tail, long long plane) {
    grad_pix_body<R, CT, PERSP>(b, nv, nf, h, w, repeat_f, v, tex, tex_c, ch0, f, win, first, valid, grad_out, want_v, tg,
                                eps, chw, slot_of, slot_bs, tail, plane);
}

// ---- phase 1 on an image with h > w -------------------------------------------------------------------------
// There several samples of a triangle's box may land on one pixel (alias_winner, raster_math.h), so a box walk meets
// a pixel the triangle won more than once, and the pixel's position is not the sample's.  The pixel counts ONCE, at
// the sample that won it: weights from that sample (what the resolve pass interpolated with), the Jacobian at the
// pixel's own position (pix % w, pix / w) like k_dcoeff.  Kernels of their own, chosen by the launch: the ones above
// stay the code they were.  Same records, same validity bits, summation in box order of the winning samples.
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void grad_sample_alias(TriAcc<R, CT, PERSP>& acc, const Tri<R>& t, const JacTri<R, PERSP>& jt,
                                                  bool want_v, int x, int y, long long w, long long hw, long long h_arg,
                                                  R eps, const int* __restrict__ wins, int ti,
                                                  const R* __restrict__ gos, const R* __restrict__ tex0,
                                                  const R* __restrict__ tex1, const R* __restrict__ tex2,
                                                  int tex_c, int ch0, long long gcs) {
    const long long pix = x + (long long)y * w;
    if (pix >= hw || wins[pix] != ti) return;
    const int py = (int)(pix / w), px = (int)(pix - (long long)py * w);
    int sx, sy;
    R c0, c1, c2, z;
    if (!alias_winner<R>(t, px, py, w, PERSP, eps, sx, sy, c0, c1, c2, z)) return;
    if (sx != x || sy != y) return;                       // another sample of the box won this pixel: counted there
    const R* go = gos + pix * (gcs == 1 ? tex_c : 1);
    acc.n += 1;
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        if (ch0 + j < tex_c) {
            const R gch = go[(ch0 + j) * gcs];
            acc.gt[j] += gch * c0;
            acc.gt[CT + j] += gch * c1;
            acc.gt[2 * CT + j] += gch * c2;
        }
    }
    if (want_v) {
        R d0 = 0, d1 = 0, d2 = 0;
        for (int ch = 0; ch < tex_c; ++ch) {
            const R gch = go[ch * gcs];
            d0 += gch * tex0[ch];
            d1 += gch * tex1[ch];
            d2 += gch * tex2[ch];
        }
        jt.add(acc.gv, d0, d1, d2, (R)px, (R)py, (R)h_arg, (R)w, eps);
    }
}

// k_grad_big for h > w: the same workgroup walk and fixed-order tree
template <typename R, int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_big_alias(long long nv, long long nf, long long h, long long w,
                                                        bool repeat_f, const R* __restrict__ v,
                                                        const R* __restrict__ tex, int tex_c, int ch0,
                                                        const long long* __restrict__ f, const int* __restrict__ win,
                                                        const int* __restrict__ big, const R* __restrict__ grad_out,
                                                        bool want_v, R* __restrict__ tg, R eps, bool chw,
                                                        const int* __restrict__ slot_of, long long slot_bs,
                                                        R* __restrict__ tail, long long plane) {
    __shared__ R s_part[4];
    const long long hw = h * w;
    const int count = big[0];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const long long g = big[1 + q];
        const long long s = g / nf, ti = g - s * nf;
        const long long* fs = repeat_f ? f : f + s * nf * 3;
        Tri<R> t;
        long long i0, i1, i2;
        load_tri<R>(t, v + s * nv * 3, fs, ti, nv, i0, i1, i2);
        const R praw[9] = {t.p0, t.p1, t.p2, t.p3, t.p4, t.p5, t.p6, t.p7, t.p8};
        JacTri<R, PERSP> jt;
        jt.init(praw, eps);
        tri_setup<R>(t, h, w, PERSP, eps);
        TriAcc<R, CT, PERSP> acc;
        acc.clear();
        const bool distinct = want_v && jt.ok && i0 != i1 && i0 != i2 && i1 != i2;
        const R* tb = tex + s * nv * tex_c;
        const int bw = t.x1 - t.x0 + 1;
        const long long npx = (long long)bw * (t.y1 - t.y0 + 1);
        for (long long p = threadIdx.x; p < npx; p += 256) {
            const int yy = (int)(p / bw);
            grad_sample_alias<R, CT, PERSP>(acc, t, jt, distinct, t.x0 + (int)(p - (long long)yy * bw), t.y0 + yy, w, hw, h,
                                            eps, win + s * hw, (int)ti, grad_out + s * hw * tex_c, tb + i0 * tex_c,
                                            tb + i1 * tex_c, tb + i2 * tex_c, tex_c, ch0, chw ? hw : 1);
        }
        const R cnt = block_sum_256<R>((R)acc.n, s_part);
#pragma unroll
        for (int j = 0; j < JacTri<R, PERSP>::NV; ++j) acc.gv[j] = block_sum_256<R>(acc.gv[j], s_part);
#pragma unroll
        for (int j = 0; j < 3 * CT; ++j) acc.gt[j] = block_sum_256<R>(acc.gt[j], s_part);
        if (threadIdx.x == 0 && cnt > 0) {
            if (slot_of) store_slots<R, CT, PERSP>(acc, tg, tail, plane, s * 3 * nf, slot_of + s * slot_bs, nf, ti);
            else store_row<R, CT, PERSP>(acc, tg, g);
        }
    }
}

// k_grad_pix for h > w: one lane per (sample, triangle), no compaction.  The leader table only says whether the
// triangle won a pixel; every row whose validity bit is set gets its record, here or from k_grad_big_alias.
template <typename R, int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_pix_alias(long long b, long long nv, long long nf, long long h,
                                                        long long w, bool repeat_f, const R* __restrict__ v,
                                                        const R* __restrict__ tex, int tex_c, int ch0,
                                                        const long long* __restrict__ f, const int* __restrict__ win,
                                                        const int* __restrict__ first,
                                                        unsigned long long* __restrict__ valid,
                                                        const R* __restrict__ grad_out, bool want_v,
                                                        R* __restrict__ tg, R eps, bool chw,
                                                        const int* __restrict__ slot_of, long long slot_bs,
                                                        R* __restrict__ tail, long long plane) {
    const long long hw = h * w;
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool has = row < b * nf && first[row] != 0x7FFFFFFF;
    const unsigned long long won = __ballot(has);
    if ((threadIdx.x & 63) == 0 && row < b * nf) valid[row >> 6] = won;
    if (!has) return;
    const long long s = row / nf;
    const int ti = (int)(row - s * nf);
    const long long* fs = repeat_f ? f : f + s * nf * 3;
    Tri<R> t;
    long long i0, i1, i2;
    load_tri<R>(t, v + s * nv * 3, fs, ti, nv, i0, i1, i2);
    const R praw[9] = {t.p0, t.p1, t.p2, t.p3, t.p4, t.p5, t.p6, t.p7, t.p8};
    tri_setup<R>(t, h, w, PERSP, eps);
    if ((long long)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) > BIG_BOX) return;      // k_grad_big_alias owns it
    JacTri<R, PERSP> jt;
    jt.init(praw, eps);
    TriAcc<R, CT, PERSP> acc;
    acc.clear();
    const bool distinct = want_v && jt.ok && i0 != i1 && i0 != i2 && i1 != i2;
    const R* tb = tex + s * nv * tex_c;
    for (int y = t.y0; y <= t.y1; ++y)
        for (int x = t.x0; x <= t.x1; ++x)
            grad_sample_alias<R, CT, PERSP>(acc, t, jt, distinct, x, y, w, hw, h, eps, win + s * hw, ti,
                                            grad_out + s * hw * tex_c, tb + i0 * tex_c, tb + i1 * tex_c, tb + i2 * tex_c,
                                            tex_c, ch0, chw ? hw : 1);
    if (slot_of) store_slots<R, CT, PERSP>(acc, tg, tail, plane, s * 3 * nf, slot_of + s * slot_bs, nf, ti);
    else store_row<R, CT, PERSP>(acc, tg, row);
}

// ---- fused gradient, phase 2: per-vertex sum over its incident corners, in incidence-list order ---------------
// One step of the gather: U list entries (already in registers; -1 = none) -> validity words -> records, every level's
// loads in flight together (unconditional loads from clamped addresses, masked afterwards); the sums keep list order.
template <typename R, int CT, bool PERSP, int U>
__device__ __forceinline__ void vert_gather(const int (&idx)[U], long long s, long long nf, const R* __restrict__ tg,
                                            const unsigned long long* __restrict__ valid, R (&av)[3], R (&at)[CT]) {
    using S = RowShape<CT, PERSP>;
    constexpr int NC = S::CORNER < 4 ? 4 : S::CORNER;
    int kk[U];
    long long row[U];
    unsigned long long word[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = idx[u] < 0 ? 0 : idx[u];
        kk[u] = i >= 2 * (int)nf ? 2 : (i >= (int)nf ? 1 : 0);
        row[u] = s * nf + (i - kk[u] * (int)nf);
        word[u] = valid[row[u] >> 6];
    }
    R c[U][NC];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        ok[u] = idx[u] >= 0 && ((word[u] >> (row[u] & 63)) & 1ull);      // won a pixel: the record exists
        const R* rec = tg + (ok[u] ? row[u] : s * nf) * S::RS;
        if (sizeof(R) == 4) {
            const float4 q = *reinterpret_cast<const float4*>(rec + 4 * kk[u]);
            c[u][0] = (R)q.x; c[u][1] = (R)q.y; c[u][2] = (R)q.z; c[u][3] = (R)q.w;
        } else {
            const double2 q0 = *reinterpret_cast<const double2*>(rec + 4 * kk[u]);
            const double2 q1 = *reinterpret_cast<const double2*>(rec + 4 * kk[u] + 2);
            c[u][0] = (R)q0.x; c[u][1] = (R)q0.y; c[u][2] = (R)q1.x; c[u][3] = (R)q1.y;
        }
#pragma unroll
        for (int j = 4; j < S::CORNER; ++j) c[u][j] = rec[12 + kk[u] * S::TAIL + (j - 4)];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
#pragma unroll
        for (int j = 0; j < S::NVC; ++j) av[j] += c[u][j];
#pragma unroll
        for (int j = 0; j < CT; ++j) at[j] += c[u][S::NVC + j];
    }
}

// The same step over vertex-major slots: entry u of the step is list position e0 + u, i.e. slot e0 + u — the records of a
// lane are one contiguous span and the spans of a wave's lanes follow each other.
// EAGER: the slot loads do not wait for the validity words (their address is the list position, known as soon as the
// offsets are): three dependent memory levels instead of four, at the price of fetching the unwritten slots of hidden
// triangles too — taken for small batches, where the pass is bound by that chain and not by bytes (inversion: batch 1).
template <typename R, int CT, bool PERSP, int U, bool EAGER>
__device__ __forceinline__ void vert_gather_slots(const int (&idx)[U], long long e0, long long s, long long nf,
                                                  const R* __restrict__ quad, const R* __restrict__ tail, long long plane,
                                                  const unsigned long long* __restrict__ valid, R (&av)[3], R (&at)[CT]) {
    using S = RowShape<CT, PERSP>;
    constexpr int NC = S::CORNER < 4 ? 4 : S::CORNER;
    long long row[U];
    unsigned long long word[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int i = idx[u] < 0 ? 0 : idx[u];
        const int kk = i >= 2 * (int)nf ? 2 : (i >= (int)nf ? 1 : 0);
        row[u] = s * nf + (i - kk * (int)nf);
        word[u] = valid[row[u] >> 6];
    }
    R c[U][NC];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        ok[u] = idx[u] >= 0 && ((word[u] >> (row[u] & 63)) & 1ull);      // won a pixel: the slot was written
        const long long e = s * 3 * nf + (EAGER ? (idx[u] >= 0 ? e0 + u : e0) : (ok[u] ? e0 + u : 0));
        if (sizeof(R) == 4) {
            const float4 q = reinterpret_cast<const float4*>(quad)[e];
            c[u][0] = (R)q.x; c[u][1] = (R)q.y; c[u][2] = (R)q.z; c[u][3] = (R)q.w;
        } else {
            const double2 q0 = reinterpret_cast<const double2*>(quad)[2 * e];
            const double2 q1 = reinterpret_cast<const double2*>(quad)[2 * e + 1];
            c[u][0] = (R)q0.x; c[u][1] = (R)q0.y; c[u][2] = (R)q1.x; c[u][3] = (R)q1.y;
        }
#pragma unroll
        for (int j = 4; j < S::CORNER; ++j) c[u][j] = tail[(j - 4) * plane + e];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!ok[u]) continue;
#pragma unroll
        for (int j = 0; j < S::NVC; ++j) av[j] += c[u][j];
#pragma unroll
        for (int j = 0; j < CT; ++j) at[j] += c[u][S::NVC + j];
    }
}

// 85 us at config[3] with one corner per step, 70 with six in flight.  (Round 4 tried the incidence list as fixed-width
// rows — one aligned 32-byte load per vertex instead of offsets -> entries, a dependent level less: no change, 69-74 us;
// the kernel is bound by the number of divergent L1 accesses, ~14 per lane at 48 % TCP utilisation, not by the chain.)
// The sums of one (sample, vertex) over its corner list [e0, e1) from ONE gradient state (tg / valid / tail): what
// k_grad_vert stores, and what k_grad_vert_levels adds up over the resolutions of a pyramid.
template <typename R, int CT, bool PERSP>
__device__ __forceinline__ void vert_sum(long long s, long long nf, const int* __restrict__ ad, int e0, int e1,
                                         const R* __restrict__ tg, const unsigned long long* __restrict__ valid, int slots,
                                         const R* __restrict__ tail, long long plane, R (&av)[3], R (&at)[CT]) {
    av[0] = av[1] = av[2] = 0;
#pragma unroll
    for (int j = 0; j < CT; ++j) at[j] = 0;
    constexpr int U = 6;                        // (the valence of an interior vertex of a triangulated grid)
    // A vertex of high valence (the two poles of the formula mesh: 192 corners; a fan anywhere) would be ONE lane walking
    // 32 dependent steps while its wave waits — at batch 1 those two lanes were the whole duration of the kernel (38 us for
    // 24 770 vertices).  Such a vertex is summed by its wave instead: lane l takes list positions e0 + l, e0 + l + 64, ...
    // in order, then a fixed-order tree over the lanes (deterministic; the order differs from the serial one by rounding).
    constexpr int WIDE = 4 * U;
    const bool wide = e1 - e0 > WIDE;
    if (!wide) {
        for (int base = e0; base < e1; base += U) {
            int idx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) idx[u] = base + u < e1 ? ad[base + u] : -1;
            if (slots == 2) vert_gather_slots<R, CT, PERSP, U, true>(idx, base, s, nf, tg, tail, plane, valid, av, at);
            else if (slots) vert_gather_slots<R, CT, PERSP, U, false>(idx, base, s, nf, tg, tail, plane, valid, av, at);
            else vert_gather<R, CT, PERSP, U>(idx, s, nf, tg, valid, av, at);
        }
    }
    unsigned long long wm = __ballot(wide);
    const int lane = threadIdx.x & 63;
    while (wm) {
        const int src = __ffsll((long long)wm) - 1;
        wm &= wm - 1ull;
        const int we0 = __shfl(e0, src, SR_WAVE), we1 = __shfl(e1, src, SR_WAVE);
        R pv[3] = {0, 0, 0};
        R pt[CT];
#pragma unroll
        for (int j = 0; j < CT; ++j) pt[j] = 0;
        for (int e = we0 + lane; e < we1; e += 64) {
            const int idx[1] = {ad[e]};
            if (slots) vert_gather_slots<R, CT, PERSP, 1, false>(idx, e, s, nf, tg, tail, plane, valid, pv, pt);
            else vert_gather<R, CT, PERSP, 1>(idx, s, nf, tg, valid, pv, pt);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) pv[j] += sr_shfl_down(pv[j], o);
#pragma unroll
            for (int j = 0; j < CT; ++j) pt[j] += sr_shfl_down(pt[j], o);
        }
        // the sums sit in lane 0; hand them to the lane that owns the vertex
#pragma unroll
        for (int j = 0; j < 3; ++j) pv[j] = __shfl(pv[j], 0, SR_WAVE);
#pragma unroll
        for (int j = 0; j < CT; ++j) pt[j] = __shfl(pt[j], 0, SR_WAVE);
        if (lane == src) {
#pragma unroll
            for (int j = 0; j < 3; ++j) av[j] = pv[j];
#pragma unroll
            for (int j = 0; j < CT; ++j) at[j] = pt[j];
        }
    }
}

template <typename R, int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_vert(long long nv, long long nf, const int* __restrict__ adj_off,
                                                   const int* __restrict__ adj, long long off_bstride,
                                                   long long adj_bstride, const R* __restrict__ tg,
                                                   const unsigned long long* __restrict__ valid, int tex_c, int ch0,
                                                   R* __restrict__ grad_v, R* __restrict__ grad_tex, int slots,
                                                   const R* __restrict__ tail, long long plane, bool accumulate) {
    const long long vert = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long s = blockIdx.y;
    const bool live = vert < nv;
    R av[3];
    R at[CT];
    const int* off = adj_off + s * off_bstride;
    const int* ad = adj + s * adj_bstride;
    const int e0 = live ? off[vert] : 0, e1 = live ? off[vert + 1] : 0;
    vert_sum<R, CT, PERSP>(s, nf, ad, e0, e1, tg, valid, slots, tail, plane, av, at);
    if (!live) return;
    if (grad_v && ch0 == 0) {
        // accumulate (SR_RASTER_GRAD_ACC): the buffers hold the gradient of earlier calls — the same mesh rasterised at
        // several resolutions sums its gradients here, in call order, instead of in one tensor addition per call
        R* o = grad_v + (s * nv + vert) * 3;
        o[0] = accumulate ? o[0] + av[0] : av[0];
        o[1] = accumulate ? o[1] + av[1] : av[1];
        o[2] = accumulate ? o[2] + av[2] : av[2];
    }
    if (grad_tex) {
        R* o = grad_tex + (s * nv + vert) * tex_c + ch0;
#pragma unroll
        for (int j = 0; j < CT; ++j)
            if (ch0 + j < tex_c) o[j] = accumulate ? o[j] + at[j] : at[j];
    }
}

__global__ __launch_bounds__(256) void k_first_pix_levels(const GradLevels t, long long b, long long nf) {
    const int l = blockIdx.y;
    const long long hw = (long long)t.res_h[l] * t.res_w[l];
    const GradState g = grad_state(t.big[l], b, nf);
    first_pix_body(b * hw, hw, t.res_w[l], nf, t.win[l], g.leaders, g.state);
}

template <int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_big_levels(const GradLevels t, long long b, long long nv, long long nf,
                                                         bool repeat_f, const float* __restrict__ v,
                                                         const float* __restrict__ tex, int tex_c,
                                                         const long long* __restrict__ f, bool want_v, float eps, bool chw,
                                                         const int* __restrict__ slot_of, long long slot_bs) {
    const int l = blockIdx.y;
    grad_big_body<float, CT, PERSP>(nv, nf, t.res_h[l], t.res_w[l], repeat_f, v, tex, tex_c, 0, f, t.win[l], t.big[l],
                                    t.grad_out[l], want_v, t.tg[l], eps, chw, slot_of, slot_bs,
                                    grad_tail(t.tg[l], b, nf), grad_plane(b, nf));
}

template <int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_pix_levels(const GradLevels t, long long b, long long nv, long long nf,
                                                         bool repeat_f, const float* __restrict__ v,
                                                         const float* __restrict__ tex, int tex_c,
                                                         const long long* __restrict__ f, bool want_v, float eps, bool chw,
                                                         const int* __restrict__ slot_of, long long slot_bs) {
    const int l = blockIdx.y;
    grad_pix_body<float, CT, PERSP>(b, nv, nf, t.res_h[l], t.res_w[l], repeat_f, v, tex, tex_c, 0, f, t.win[l],
                                    grad_leaders(t.big[l], b, nf), t.valid[l], t.grad_out[l], want_v, t.tg[l], eps, chw,
                                    slot_of, slot_bs, t.tg[l] + b * nf * GRAD_QUAD_VALUES, grad_plane(b, nf));
    // (grad_tail() written out: through the helper the instantiations with two or three tail planes compile differently)
}

template <int CT, bool PERSP>
__global__ __launch_bounds__(256) void k_grad_vert_levels(const GradLevels t, long long b, long long nv, long long nf,
                                                          const int* __restrict__ adj_off, const int* __restrict__ adj,
                                                          long long off_bstride, long long adj_bstride, int tex_c,
                                                          float* __restrict__ grad_v, float* __restrict__ grad_tex,
                                                          int slots) {
    const long long vert = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long s = blockIdx.y;
    const bool live = vert < nv;
    const int* off = adj_off + s * off_bstride;
    const int* ad = adj + s * adj_bstride;
    const int e0 = live ? off[vert] : 0, e1 = live ? off[vert + 1] : 0;
    float tv[3] = {0.0f, 0.0f, 0.0f}, tt[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) tt[j] = 0.0f;
    for (int l = 0; l < t.n; ++l) {
        float av[3], at[CT];
        vert_sum<float, CT, PERSP>(s, nf, ad, e0, e1, t.tg[l], t.valid[l], slots, grad_tail(t.tg[l], b, nf),
                                   grad_plane(b, nf), av, at);
        if (l == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) tv[j] = av[j];
#pragma unroll
            for (int j = 0; j < CT; ++j) tt[j] = at[j];
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j) tv[j] = tv[j] + av[j];
#pragma unroll
            for (int j = 0; j < CT; ++j) tt[j] = tt[j] + at[j];
        }
    }
    if (!live) return;
    if (grad_v) {
        float* o = grad_v + (s * nv + vert) * 3;
        o[0] = tv[0];
        o[1] = tv[1];
        o[2] = tv[2];
    }
    if (grad_tex) {
        float* o = grad_tex + (s * nv + vert) * tex_c;
#pragma unroll
        for (int j = 0; j < CT; ++j)
            if (j < tex_c) o[j] = tt[j];
    }
}

// SR_RASTER_GRAD_SLOTS=0: the per-triangle records of rounds 2-5 instead of vertex-major slots (A/B, tests)
bool grad_slots_enabled() { return !sr_env_off("SR_RASTER_GRAD_SLOTS"); }
// few lanes: the vertex gather is a latency chain, read the slots eagerly (SR_RASTER_GRAD_EAGER=0 / 1 forces)
bool grad_eager(long long b, long long nv) {
    const int c = sr_env_char("SR_RASTER_GRAD_EAGER");
    return c < 0 ? b * nv < 8 * 32768 : c == '1';
}

// f(integral_constant<int, CT>, bool_constant<PERSP>) for the accumulator width of a chunk of `ct` (1 .. 4) channels
template <typename F>
void for_ct_persp(long long ct, bool perspective, F&& f) {
    auto with = [&](auto CT) {
        if (perspective) f(CT, std::true_type{});
        else f(CT, std::false_type{});
    };
    if (ct == 1) with(std::integral_constant<int, 1>{});
    else if (ct == 2) with(std::integral_constant<int, 2>{});
    else if (ct == 3) with(std::integral_constant<int, 3>{});
    else with(std::integral_constant<int, 4>{});
}

// one chunk of <= 4 attribute channels from channel ch0: large triangles, small triangles, vertex sums
template <typename R, int CT, bool PERSP>
void grad_chunk_launch(const RasterGrad<R>& c, int ch0, const GradScratch<R>& s, const int* first, const int* slot_of,
                       long long slot_bs, hipStream_t st) {
    const bool want_v = c.grad_v != nullptr && ch0 == 0;
    const bool eager = grad_eager(c.b, c.nv);
    if (c.h > c.w) {                                      // samples alias onto pixels: the kernels that count a pixel once
        hipLaunchKernelGGL((k_grad_big_alias<R, CT, PERSP>), dim3(SR_NUM_CU * 2), dim3(256), 0, st, c.nv, c.nf, c.h, c.w,
                           c.repeat_f, c.v, c.tex, (int)c.tex_c, ch0, c.tri, c.win, c.big, c.grad_out, want_v, s.quad,
                           c.eps, c.chw, slot_of, slot_bs, s.tail, s.plane);
        if (c.b * c.nf > 0)
            hipLaunchKernelGGL((k_grad_pix_alias<R, CT, PERSP>), dim3((unsigned)sr_ceil_div(c.b * c.nf, 256)), dim3(256), 0,
                               st, c.b, c.nv, c.nf, c.h, c.w, c.repeat_f, c.v, c.tex, (int)c.tex_c, ch0, c.tri, c.win, first,
                               s.valid, c.grad_out, want_v, s.quad, c.eps, c.chw, slot_of, slot_bs, s.tail, s.plane);
    } else {
        hipLaunchKernelGGL((k_grad_big<R, CT, PERSP>), dim3(SR_NUM_CU * 2), dim3(256), 0, st, c.nv, c.nf, c.h, c.w,
                           c.repeat_f, c.v, c.tex, (int)c.tex_c, ch0, c.tri, c.win, c.big, c.grad_out, want_v, s.quad,
                           c.eps, c.chw, slot_of, slot_bs, s.tail, s.plane);
        if (c.b * c.nf > 0)
            hipLaunchKernelGGL((k_grad_pix<R, CT, PERSP>), dim3((unsigned)sr_ceil_div(c.b * c.nf, 256)), dim3(256), 0, st,
                               c.b, c.nv, c.nf, c.h, c.w, c.repeat_f, c.v, c.tex, (int)c.tex_c, ch0, c.tri, c.win, first,
                               s.valid, c.grad_out, want_v, s.quad, c.eps, c.chw, slot_of, slot_bs, s.tail, s.plane);
    }
    hipLaunchKernelGGL((k_grad_vert<R, CT, PERSP>), dim3((unsigned)sr_ceil_div(c.nv, 256), (unsigned)c.b), dim3(256), 0, st,
                       c.nv, c.nf, c.adj_off, c.adj, c.off_bs, c.adj_bs, s.quad, s.valid, (int)c.tex_c, ch0, c.grad_v,
                       c.grad_tex, slot_of == nullptr ? 0 : (eager ? 2 : 1), s.tail, s.plane, c.accumulate);
}

template <int CT, bool PERSP>
void grad_levels_launch(const GradLevels& t, const RasterGrad<float>& c, long long max_pix, hipStream_t st) {
    const bool want_v = c.grad_v != nullptr;
    const bool eager = grad_eager(c.b, c.nv);
    const unsigned n = (unsigned)t.n;
    hipLaunchKernelGGL(k_first_pix_levels, dim3((unsigned)std::min<long long>(sr_ceil_div(max_pix, 256), 1024), n), dim3(256),
                       0, st, t, c.b, c.nf);
    // Phase 1 of a level with h > w is k_grad_big_alias + k_grad_pix_alias, a pair of launches per such level (the choice
    // stays uniform per launch, the *_levels kernels the code they were); the other levels go, in their order, through
    // the *_levels pair as a table of their own.  Leaders before and vertex sums after run over all levels of `t`.
    GradLevels own = t;
    own.n = 0;
    for (int l = 0; l < t.n; ++l) {
        if (t.res_h[l] > t.res_w[l]) continue;
        const int k = own.n++;
        own.res_h[k] = t.res_h[l]; own.res_w[k] = t.res_w[l];
        own.win[k] = t.win[l]; own.big[k] = t.big[l]; own.grad_out[k] = t.grad_out[l];
        own.tg[k] = t.tg[l]; own.valid[k] = t.valid[l];
    }
    if (own.n > 0) {
        const unsigned m = (unsigned)own.n;
        hipLaunchKernelGGL((k_grad_big_levels<CT, PERSP>), dim3(SR_NUM_CU * 2, m), dim3(256), 0, st, own, c.b, c.nv, c.nf,
                           c.repeat_f, c.v, c.tex, (int)c.tex_c, c.tri, want_v, c.eps, c.chw, c.adj_slot, c.adj_bs);
        hipLaunchKernelGGL((k_grad_pix_levels<CT, PERSP>), dim3((unsigned)sr_ceil_div(c.b * c.nf, 256), m), dim3(256), 0, st,
                           own, c.b, c.nv, c.nf, c.repeat_f, c.v, c.tex, (int)c.tex_c, c.tri, want_v, c.eps, c.chw, c.adj_slot,
                           c.adj_bs);
    }
    for (int l = 0; l < t.n; ++l) {
        if (t.res_h[l] <= t.res_w[l]) continue;
        const long long h = t.res_h[l], w = t.res_w[l];
        hipLaunchKernelGGL((k_grad_big_alias<float, CT, PERSP>), dim3(SR_NUM_CU * 2), dim3(256), 0, st, c.nv, c.nf, h, w,
                           c.repeat_f, c.v, c.tex, (int)c.tex_c, 0, c.tri, t.win[l], t.big[l], t.grad_out[l], want_v, t.tg[l],
                           c.eps, c.chw, c.adj_slot, c.adj_bs, grad_tail(t.tg[l], c.b, c.nf), grad_plane(c.b, c.nf));
        hipLaunchKernelGGL((k_grad_pix_alias<float, CT, PERSP>), dim3((unsigned)sr_ceil_div(c.b * c.nf, 256)), dim3(256), 0,
                           st, c.b, c.nv, c.nf, h, w, c.repeat_f, c.v, c.tex, (int)c.tex_c, 0, c.tri, t.win[l],
                           grad_leaders(t.big[l], c.b, c.nf), t.valid[l], t.grad_out[l], want_v, t.tg[l], c.eps, c.chw,
                           c.adj_slot, c.adj_bs, grad_tail(t.tg[l], c.b, c.nf), grad_plane(c.b, c.nf));
    }
    hipLaunchKernelGGL((k_grad_vert_levels<CT, PERSP>), dim3((unsigned)sr_ceil_div(c.nv, 256), (unsigned)c.b), dim3(256), 0,
                       st, t, c.b, c.nv, c.nf, c.adj_off, c.adj, c.off_bs, c.adj_bs, (int)c.tex_c, c.grad_v, c.grad_tex,
                       eager ? 2 : 1);
}

}  // namespace

template <typename R>
int raster_dcoeff_launch(long long b, long long n, long long h, long long w, bool perspective, const R* v,
                         const long long* index, R* dcoeff, R eps, hipStream_t st) {
    hipLaunchKernelGGL((k_dcoeff<R>), dim3((unsigned)sr_ceil_div(b * h * w, 256)), dim3(256), 0, st, b, n, h, w, perspective,
                       v, index, dcoeff, eps);
    return sr_launch_status();
}
template int raster_dcoeff_launch<float>(long long, long long, long long, long long, bool, const float*, const long long*,
                                         float*, float, hipStream_t);
template int raster_dcoeff_launch<double>(long long, long long, long long, long long, bool, const double*, const long long*,
                                          double*, double, hipStream_t);

template <typename R>
int raster_grad_launch(const RasterGrad<R>& c, void* work, hipStream_t st) {
    const GradScratch<R> s = grad_scratch<R>(work, c.b, c.nf);
    // vertex-major slots by default; the inverse incidence table is the caller's cached one, or built here per call
    const bool use_slots = c.nf > 0 && grad_slots_enabled();
    const int* slot_of = nullptr;
    long long slot_bs = 0;
    if (use_slots && c.adj_slot) {
        slot_of = c.adj_slot;
        slot_bs = c.adj_bs;
    } else if (use_slots) {
        const long long topo = c.adj_bs ? c.b : 1;             // per-sample topologies carry a batch stride
        slot_bs = c.adj_bs ? 3 * c.nf : 0;
        hipLaunchKernelGGL(k_slot_inverse, dim3((unsigned)sr_ceil_div(3 * c.nf, 256), (unsigned)topo), dim3(256), 0, st,
                           3 * c.nf, c.adj, s.inverse, c.adj_bs);
        slot_of = s.inverse;
    }
    // leaders of all triangles, once per call (the attribute-channel chunks below share them): the table behind the
    // big-triangle list of the forward call's gradient state.  The tiled forward has built it (state word 1); the
    // global-key forward has only filled it (state word 0) and k_first_pix completes it here, in place (idempotent: a
    // second backward over the same state repeats the same integer minima).  Which of the two happened is read from
    // the state the FORWARD wrote, on the device — never re-derived from tiled_ok() at backward time.
    const GradState g = grad_state(const_cast<int*>(c.big), c.b, c.nf);
    if (c.b * c.nf > 0)
        hipLaunchKernelGGL(k_first_pix, dim3((unsigned)std::min<long long>(sr_ceil_div(c.b * c.h * c.w, 256), 1024)),
                           dim3(256), 0, st, c.b * c.h * c.w, c.h * c.w, c.w, c.nf, c.win, g.leaders, g.state);
    // attribute channels in chunks of <= 4 register accumulators; the vertex gradient rides with chunk 0
    for (long long ch0 = 0; ch0 < (c.grad_tex ? c.tex_c : 1); ch0 += 4) {
        const long long ct = c.tex_c - ch0 < 4 ? c.tex_c - ch0 : 4;
        for_ct_persp(ct, c.perspective, [&](auto CT, auto P) {
            grad_chunk_launch<R, decltype(CT)::value, decltype(P)::value>(c, (int)ch0, s, g.leaders, slot_of, slot_bs, st);
        });
    }
    return sr_launch_status();
}
template int raster_grad_launch<float>(const RasterGrad<float>&, void*, hipStream_t);
template int raster_grad_launch<double>(const RasterGrad<double>&, void*, hipStream_t);

int raster_grad_levels_launch(const GradLevels& t, const RasterGrad<float>& c, long long max_pix, hipStream_t st) {
    for_ct_persp(c.tex_c, c.perspective, [&](auto CT, auto P) {
        grad_levels_launch<decltype(CT)::value, decltype(P)::value>(t, c, max_pix, st);
    });
    return sr_launch_status();
}
