// Analytic antialiasing at occlusion boundaries (C ABI: sr_edge_aa_fwd / sr_edge_aa_bwd_image / sr_edge_aa_bwd_corner;
// definition: stylerenderer_amd/op/edge.py and DESIGN 7p).  Where two neighbouring pixels show different faces, the
// silhouette edge of the nearer face that crosses the segment between the two pixel centres blends the two pixels by how
// far it reaches past the midpoint.
//
// A pair is a pixel p and its right (horizontal pair) or lower (vertical pair) neighbour q; it is active iff
// face[p] != face[q].  The foreground a is q when face[p] < 0, p when face[q] < 0, else q iff z[q] > z[p]; o is the other
// pixel, F = face[a].  With X = (1 + x) (W / 2) - 0.5, Y = (1 - y) (H / 2) - 0.5 per corner of F, u the coordinate along
// the pair's axis and s the other one minus a's, for the edges k = 0, 1, 2 (corners i = k, j = (k + 1) mod 3):
//     crossing    (s_i < 0) != (s_j < 0);  den = s_i - s_j;  t = s_i / den;  du = u_j - u_i;  c = u_i + du t
//                 d = c - a_u when o lies on the positive side, a_u - c otherwise;  taken iff 0 <= d <= 1
//     silhouette  opp[F, k] == -1, or opp >= 0 and the cross products of the edge with F's third corner and with opp's
//                 vertex do not have strictly opposite signs
// The first such k is the pair's edge.  d >= 0.5: o receives (d - 0.5) (image[a] - image[o]); otherwise a receives
// (0.5 - d) (image[o] - image[a]).  Every step is one float32 operation in that order (-ffp-contract=off, correctly
// rounded division), so the host composite gives the same bits.
//
//   k_edge_fwd        a lane per pixel, channels inside.  It reads the faces of its cross, leaves after those five loads
//                     when they agree (interior and empty pixels), else analyses its up to four pairs (each pair is
//                     analysed by both of its pixels: that is what removes the scatter) and adds what it receives in the
//                     order left, right, upper, lower.
//   k_edge_bwd_image  the same walk as a gather: gimage[p] = g[p], then per pair in the same order - w g[p] where p
//                     receives and + w g[n] where the neighbour n does.
//   k_edge_bwd_corner a lane per (sample, face): the pixels of the face's bounding box grown by one, clipped to the
//                     picture, in row-major order, right pair before lower pair; a pair whose foreground face is this
//                     face adds its terms to the two corners of its edge.  A face whose box holds more than EDGE_BIG
//                     pixels is left to its wave: the 64 lanes take the pixels n = lane, lane + 64, ... of the box in
//                     that order, then a shuffle tree of depth 6 (lane l adds lane l + 32, 16, ..., 1).  The lane writes
//                     all nine values of its face (z = 0), zeros included.
//
// Vector stores and plain C++ only: no atomics, no LDS, no scratch, nothing that must start at zero, no allocation, no
// host read: all three run under graph capture on the caller's stream, and reruns are bit-identical.  Face and vertex
// numbers outside the mesh switch a pair off and are never followed.
#include "common.h"

namespace {

constexpr int EDGE_BLOCK = 256;
constexpr int EDGE_WAVE = 64;
constexpr int EDGE_BIG = 256;                  // bounding-box pixels above which a face is summed by its wave

struct EdgeMesh {
    const float* v;                            // [B, nv, 3]
    const int64_t* tri;                        // [nf, 3]
    const int32_t* opp;                        // [nf, 3]
    const int32_t* face;                       // [B, H, W]
    const float* zbuf;                         // [B, H, W]
    int64_t nv, nf, H, W;
    float hw, hh;                              // W / 2, H / 2
};

struct EdgePair {
    bool hit, a_is_p, recv_is_q;
    int k;
    int32_t F;
    float w, t, den, du, si, sj;
};

__device__ __forceinline__ bool edge_corners(const EdgeMesh& m, const float* vb, int64_t F, float* X, float* Y) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t id = m.tri[3 * F + k];
        if (id < 0 || id >= m.nv) return false;
        X[k] = (1.f + vb[3 * id]) * m.hw - 0.5f;
        Y[k] = (1.f - vb[3 * id + 1]) * m.hh - 0.5f;
    }
    return true;
}

// the pair (p, q) of sample b, p = (px, py), q its right (horiz) or lower neighbour; fp != fq is the caller's test
__device__ __forceinline__ EdgePair edge_pair(const EdgeMesh& m, int64_t b, int32_t fp, int32_t fq, int64_t px, int64_t py,
                                              bool horiz) {
    EdgePair r;
    r.hit = false;
    bool a_is_p;
    if (fp < 0) {
        a_is_p = false;
    } else if (fq < 0) {
        a_is_p = true;
    } else {
        const int64_t po = (b * m.H + py) * m.W + px;
        const float zp = m.zbuf[po], zq = m.zbuf[po + (horiz ? 1 : m.W)];
        a_is_p = !(zq > zp);
    }
    const int32_t F = a_is_p ? fp : fq;
    r.a_is_p = a_is_p;
    r.F = F;
    if (F < 0 || F >= m.nf) return r;
    const float* vb = m.v + b * m.nv * 3;
    float X[3], Y[3];
    if (!edge_corners(m, vb, F, X, Y)) return r;
    const float ax = (float)(px + ((horiz && !a_is_p) ? 1 : 0));
    const float ay = (float)(py + ((!horiz && !a_is_p) ? 1 : 0));
    const float ac_u = horiz ? ax : ay, ac_s = horiz ? ay : ax;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = k, j = (k + 1) % 3, own = (k + 2) % 3;
        const float ui = horiz ? X[i] : Y[i], uj = horiz ? X[j] : Y[j];
        const float si = (horiz ? Y[i] : X[i]) - ac_s, sj = (horiz ? Y[j] : X[j]) - ac_s;
        if ((si < 0.f) == (sj < 0.f)) continue;
        const float den = si - sj;
        const float t = si / den;
        const float du = uj - ui;
        const float c = ui + du * t;
        const float d = a_is_p ? c - ac_u : ac_u - c;
        if (!(d >= 0.f && d <= 1.f)) continue;
        const int32_t o = m.opp[3 * F + k];
        if (o != -1) {
            if (o < 0 || o >= m.nv) continue;
            const float xo = (1.f + vb[3 * (int64_t)o]) * m.hw - 0.5f;
            const float yo = (1.f - vb[3 * (int64_t)o + 1]) * m.hh - 0.5f;
            const float ex = X[j] - X[i], ey = Y[j] - Y[i];
            const float c_own = ex * (Y[own] - Y[i]) - ey * (X[own] - X[i]);
            const float c_opp = ex * (yo - Y[i]) - ey * (xo - X[i]);
            if ((c_own > 0.f && c_opp < 0.f) || (c_own < 0.f && c_opp > 0.f)) continue;
        }
        const bool past = d >= 0.5f;
        r.hit = true;
        r.k = k;
        r.recv_is_q = past == a_is_p;
        r.w = past ? d - 0.5f : 0.5f - d;
        r.t = t; r.den = den; r.du = du; r.si = si; r.sj = sj;
        return r;
    }
    return r;
}

// The four pairs of pixel (x, y) in the order left, right, upper, lower: mode 0 nothing, 1 this pixel receives, 2 the
// neighbour receives; w the weight, nb the neighbour's offset in the plane.  Returns false when no pair is active.
__device__ __forceinline__ bool edge_cross(const EdgeMesh& m, int64_t b, int64_t x, int64_t y, int* mode, float* w,
                                           int64_t* nb) {
    const int64_t plane = b * m.H * m.W, me = y * m.W + x;
    const int32_t fc = m.face[plane + me];
    const bool in[4] = {x > 0, x + 1 < m.W, y > 0, y + 1 < m.H};
    const int64_t step[4] = {-1, 1, -m.W, m.W};
    int32_t fn[4];
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        nb[k] = me + step[k];
        fn[k] = in[k] ? m.face[plane + nb[k]] : fc;
        any = any || fn[k] != fc;
        mode[k] = 0;
        w[k] = 0.f;
    }
    if (!any) return false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (fn[k] == fc) continue;
        const bool horiz = k < 2, me_is_q = (k & 1) == 0;          // left and upper: the neighbour is p
        const int64_t px = x - ((k == 0) ? 1 : 0), py = y - ((k == 2) ? 1 : 0);
        const EdgePair r = me_is_q ? edge_pair(m, b, fn[k], fc, px, py, horiz) : edge_pair(m, b, fc, fn[k], px, py, horiz);
        if (!r.hit) continue;
        mode[k] = (r.recv_is_q == me_is_q) ? 1 : 2;
        w[k] = r.w;
    }
    return true;
}

__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_fwd(float* __restrict__ out, const float* __restrict__ image,
                                                         EdgeMesh m, int64_t B, int64_t C) {
    const int64_t HW = m.H * m.W;
    const int64_t idx = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x;
    if (idx >= B * HW) return;
    const int64_t b = idx / HW, me = idx - b * HW;
    const int64_t y = me / m.W, x = me - y * m.W;
    int mode[4];
    float w[4];
    int64_t nb[4];
    const bool any = edge_cross(m, b, x, y, mode, w, nb);
    for (int64_t c = 0; c < C; ++c) {
        const int64_t base = (b * C + c) * HW;
        const float a0 = image[base + me];
        float acc = a0;
        if (any) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (mode[k] == 1) acc = acc + w[k] * (image[base + nb[k]] - a0);
        }
        out[base + me] = acc;
    }
}

__global__ __launch_bounds__(EDGE_BLOCK) void k_edge_bwd_image(float* __restrict__ gimage, const float* __restrict__ g,
                                                               EdgeMesh m, int64_t B, int64_t C) {
    const int64_t HW = m.H * m.W;
    const int64_t idx = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x;
    if (idx >= B * HW) return;
    const int64_t b = idx / HW, me = idx - b * HW;
    const int64_t y = me / m.W, x = me - y * m.W;
    int mode[4];
    float w[4];
    int64_t nb[4];
    const bool any = edge_cross(m, b, x, y, mode, w, nb);
    for (int64_t c = 0; c < C; ++c) {
        const int64_t base = (b * C + c) * HW;
        const float g0 = g[base + me];
        float acc = g0;
        if (any) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (mode[k] == 1) acc = acc - w[k] * g0;
                else if (mode[k] == 2) acc = acc + w[k] * g[base + nb[k]];
            }
        }
        gimage[base + me] = acc;
    }
}

// the terms of one pair of face F at pixel p = (px, py): added to acc[2 corner + (0: x, 1: y)]
__device__ __forceinline__ void edge_terms(const EdgeMesh& m, const float* __restrict__ g, const float* __restrict__ image,
                                           int64_t b, int64_t C, int32_t F, int32_t fp, int32_t fq, int64_t px, int64_t py,
                                           bool horiz, float* acc) {
    const EdgePair r = edge_pair(m, b, fp, fq, px, py, horiz);
    if (!r.hit || r.F != F) return;
    const int64_t HW = m.H * m.W;
    const int64_t po = py * m.W + px, qo = po + (horiz ? 1 : m.W);
    const int64_t ro = r.recv_is_q ? qo : po, ao = r.a_is_p ? po : qo, oo = r.a_is_p ? qo : po;
    float gd = 0.f;
    for (int64_t c = 0; c < C; ++c) {
        const int64_t base = (b * C + c) * HW;
        gd = gd + g[base + ro] * (image[base + ao] - image[base + oo]);
    }
    const float gsd = r.a_is_p ? gd : -gd;
    const float gui = gsd * (1.f - r.t), guj = gsd * r.t;
    const float q = (gsd * r.du) / (r.den * r.den);
    const float gsi = -(q * r.sj), gsj = q * r.si;
    const float nhh = -m.hh;
    const float gxi = (horiz ? gui : gsi) * m.hw, gyi = (horiz ? gsi : gui) * nhh;
    const float gxj = (horiz ? guj : gsj) * m.hw, gyj = (horiz ? gsj : guj) * nhh;
    const int i = r.k, j = (r.k + 1) % 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c == i) { acc[2 * c] = acc[2 * c] + gxi; acc[2 * c + 1] = acc[2 * c + 1] + gyi; }
        if (c == j) { acc[2 * c] = acc[2 * c] + gxj; acc[2 * c + 1] = acc[2 * c + 1] + gyj; }
    }
}

// pixel n of the box (x0, y0, bw): its right pair, then its lower pair
__device__ __forceinline__ void edge_box_pixel(const EdgeMesh& m, const float* __restrict__ g, const float* __restrict__ image,
                                               int64_t b, int64_t C, int32_t F, int x0, int y0, int bw, int n, float* acc) {
    const int64_t py = y0 + n / bw, px = x0 + n % bw;
    const int64_t po = (b * m.H + py) * m.W + px;
    const int32_t fp = m.face[po];
    if (px + 1 < m.W) {
        const int32_t fq = m.face[po + 1];
        if (fp != fq && (fp == F || fq == F)) edge_terms(m, g, image, b, C, F, fp, fq, px, py, true, acc);
    }
    if (py + 1 < m.H) {
        const int32_t fq = m.face[po + m.W];
        if (fp != fq && (fp == F || fq == F)) edge_terms(m, g, image, b, C, F, fp, fq, px, py, false, acc);
    }
}

__global__ __launch_bounds__(EDGE_WAVE) void k_edge_bwd_corner(float* __restrict__ gc, const float* __restrict__ g,
                                                               const float* __restrict__ image, EdgeMesh m, int64_t B,
                                                               int64_t C, int64_t chunks) {
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x / chunks;
    const int64_t F = (blockIdx.x % chunks) * EDGE_WAVE + lane;
    const bool live = F < m.nf;
    int x0 = 0, y0 = 0, bw = 0, count = 0;
    if (live) {
        float X[3], Y[3];
        const float* vb = m.v + b * m.nv * 3;
        if (edge_corners(m, vb, F, X, Y)) {
            const float xl = fminf(fminf(X[0], X[1]), X[2]), xh = fmaxf(fmaxf(X[0], X[1]), X[2]);
            const float yl = fminf(fminf(Y[0], Y[1]), Y[2]), yh = fmaxf(fmaxf(Y[0], Y[1]), Y[2]);
            const bool finite = (X[0] - X[0] == 0.f) && (X[1] - X[1] == 0.f) && (X[2] - X[2] == 0.f) &&
                                (Y[0] - Y[0] == 0.f) && (Y[1] - Y[1] == 0.f) && (Y[2] - Y[2] == 0.f);
            if (finite) {
                const float fw = (float)m.W, fh = (float)m.H;
                // (clamped in float first: the conversions below then see values in [-1, W] and [-1, H])
                x0 = (int)fmaxf(fminf(floorf(xl) - 1.f, fw), 0.f);
                y0 = (int)fmaxf(fminf(floorf(yl) - 1.f, fh), 0.f);
                const int x1 = (int)fminf(fmaxf(ceilf(xh) + 1.f, -1.f), fw - 1.f);
                const int y1 = (int)fminf(fmaxf(ceilf(yh) + 1.f, -1.f), fh - 1.f);
                bw = x1 - x0 + 1;
                const int bh = y1 - y0 + 1;
                count = (bw > 0 && bh > 0) ? bw * bh : 0;
            }
        }
    }
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool big = count > EDGE_BIG;
    if (!big)
        for (int n = 0; n < count; ++n) edge_box_pixel(m, g, image, b, C, (int32_t)F, x0, y0, bw, n, acc);
    if (live && !big) {
        float* o = gc + (b * m.nf + F) * 9;
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[3 * c] = acc[2 * c]; o[3 * c + 1] = acc[2 * c + 1]; o[3 * c + 2] = 0.f; }
    }
    // the large faces of this wave, one after the other, every lane taking part
    unsigned long long todo = __ballot(big);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int sx0 = __shfl(x0, src, EDGE_WAVE), sy0 = __shfl(y0, src, EDGE_WAVE);
        const int sbw = __shfl(bw, src, EDGE_WAVE), scount = __shfl(count, src, EDGE_WAVE);
        const int64_t sF = (blockIdx.x % chunks) * EDGE_WAVE + src;
        float part[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int n = lane; n < scount; n += EDGE_WAVE) edge_box_pixel(m, g, image, b, C, (int32_t)sF, sx0, sy0, sbw, n, part);
#pragma unroll
        for (int off = EDGE_WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int c = 0; c < 6; ++c) part[c] = part[c] + __shfl_down(part[c], off, EDGE_WAVE);
        }
        if (lane == 0) {
            float* o = gc + (b * m.nf + sF) * 9;
#pragma unroll
            for (int c = 0; c < 3; ++c) { o[3 * c] = part[2 * c]; o[3 * c + 1] = part[2 * c + 1]; o[3 * c + 2] = 0.f; }
        }
    }
}

int edge_check(const void* a, const void* b, const float* v, const int64_t* tri, const int32_t* opp, const int32_t* face,
               const float* zbuf, int64_t B, int64_t C, int64_t H, int64_t W, int64_t nv, int64_t nf) {
    if (B < 0 || C < 0 || H < 0 || W < 0 || nv < 0 || nf < 0) return SR_EINVAL;
    if (B == 0 || C == 0 || H == 0 || W == 0) return SR_OK;
    if (!a || !b || !face || !zbuf || (nf > 0 && (!tri || !opp || !v))) return SR_EINVAL;
    if (H > 16384 || W > 16384 || nf >= (1LL << 31) || nv >= (1LL << 31) || B * H * W >= (1LL << 38) ||
        B * C * H * W >= (1LL << 40))
        return SR_ERANGE;
    return 1;                                  // go on
}

EdgeMesh edge_mesh(const float* v, const int64_t* tri, const int32_t* opp, const int32_t* face, const float* zbuf,
                   int64_t H, int64_t W, int64_t nv, int64_t nf) {
    EdgeMesh m;
    m.v = v; m.tri = tri; m.opp = opp; m.face = face; m.zbuf = zbuf;
    m.nv = nv; m.nf = nf; m.H = H; m.W = W;
    m.hw = (float)W / 2.f;
    m.hh = (float)H / 2.f;
    return m;
}

}  // namespace

extern "C" int sr_edge_big_pixels(void) { return EDGE_BIG; }

extern "C" int sr_edge_aa_fwd(float* out, const float* image, const float* v, const int64_t* tri, const int32_t* opp,
                              const int32_t* face, const float* zbuf, int64_t B, int64_t C, int64_t H, int64_t W,
                              int64_t nv, int64_t nf, sr_stream_t stream) {
    const int rc = edge_check(out, image, v, tri, opp, face, zbuf, B, C, H, W, nv, nf);
    if (rc <= 0) return rc;
    const int64_t blocks = sr_ceil_div(B * H * W, EDGE_BLOCK);
    if (blocks > 0x7fffffffLL) return SR_ERANGE;
    hipLaunchKernelGGL(k_edge_fwd, dim3((unsigned)blocks), dim3(EDGE_BLOCK), 0, sr_stream(stream), out, image,
                       edge_mesh(v, tri, opp, face, zbuf, H, W, nv, nf), B, C);
    return sr_launch_status();
}

extern "C" int sr_edge_aa_bwd_image(float* gimage, const float* g, const float* v, const int64_t* tri, const int32_t* opp,
                                    const int32_t* face, const float* zbuf, int64_t B, int64_t C, int64_t H, int64_t W,
                                    int64_t nv, int64_t nf, sr_stream_t stream) {
    const int rc = edge_check(gimage, g, v, tri, opp, face, zbuf, B, C, H, W, nv, nf);
    if (rc <= 0) return rc;
    const int64_t blocks = sr_ceil_div(B * H * W, EDGE_BLOCK);
    if (blocks > 0x7fffffffLL) return SR_ERANGE;
    hipLaunchKernelGGL(k_edge_bwd_image, dim3((unsigned)blocks), dim3(EDGE_BLOCK), 0, sr_stream(stream), gimage, g,
                       edge_mesh(v, tri, opp, face, zbuf, H, W, nv, nf), B, C);
    return sr_launch_status();
}

extern "C" int sr_edge_aa_bwd_corner(float* gc, const float* g, const float* image, const float* v, const int64_t* tri,
                                     const int32_t* opp, const int32_t* face, const float* zbuf, int64_t B, int64_t C,
                                     int64_t H, int64_t W, int64_t nv, int64_t nf, sr_stream_t stream) {
    const int rc = edge_check(gc, g, v, tri, opp, face, zbuf, B, C, H, W, nv, nf);
    if (rc <= 0) return rc;
    if (!image) return SR_EINVAL;
    if (nf == 0) return SR_OK;
    const int64_t chunks = sr_ceil_div(nf, EDGE_WAVE);
    if (B * chunks > 0x7fffffffLL) return SR_ERANGE;
    hipLaunchKernelGGL(k_edge_bwd_corner, dim3((unsigned)(B * chunks)), dim3(EDGE_WAVE), 0, sr_stream(stream), gc, g, image,
                       edge_mesh(v, tri, opp, face, zbuf, H, W, nv, nf), B, C, chunks);
    return sr_launch_status();
}
