// The FID Inception-v3 trunk (reference inception.py fid_inception_v3 / InceptionV3([3])) and the feature statistics
// of the Fréchet Inception distance (reference fid.py / calc_inception.py), forward only, float32 NCHW.
//
//   k_incep_conv      BasicConv2d with its BatchNorm folded into weight and bias (conv -> + bias -> ReLU) as an
//                     implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): M = output channels,
//                     N = B * OH * OW output pixels, K = C * KH * KW taps, flattened (c, ky, kx) so that the 27 taps of
//                     the C = 3 stem convolution fill two 16-deep K steps instead of a per-channel padded tile.
//                     Any KH x KW in {1, 3, 5, 7}^2 (the network uses 1x1, 3x3, 5x5, 1x7, 7x1, 1x3, 3x1), stride
//                     1 or 2, padding per axis.  The M rows are split in up to three segments, each written to its own
//                     tensor at its own channel offset of its own channel count: a branch writes straight into its
//                     slice of the block's concatenated output, and the 1x1 convolutions of a block that read the same
//                     input run as one GEMM with their N concatenated (A: 64 + 48 + 64, C: 192 + c7 + c7,
//                     D: 192 + 192, E: 320 + 384 + 448).
//   k_incep_pool      the pools of the network: max 3x3 / 2 (stem, InceptionB / D), average 3x3 / 1 pad 1 excluding the
//                     padding (FIDInceptionA / C / E_1), max 3x3 / 1 pad 1 (FIDInceptionE_2); into a channel slice
//   k_incep_gap       global average of each [H, W] plane, sequential sum in row-major order
//   k_fs_*            FID feature statistics in fp64: per-batch shift by the first batch's mean, running sum and the
//                     upper tiles of the Gram matrix accumulated element by element in batch-row order (no atomics:
//                     the same features give the same bits), then mean and covariance (np.mean / np.cov)
//
// The bilinear resize to 299^2 is k_ppl_prep (csrc/ppl.hip) with shift 0 and scale 1.
#include "mfma_tile.h"

namespace {

constexpr int MAXSEG = 3;
constexpr int BK = 16;   // K depth of one LDS stage

struct Seg {
    float* out;
    int m0;      // first GEMM row of the segment
    int coff;    // channel offset of row m0 in `out`
    int ctot;    // channel count of `out`
};

struct ConvArgs {
    const float* in;     // [B, C, H, W]
    const float* wt;     // [K, M], K = (c, ky, kx)
    const float* bias;   // [M]
    int C, H, W, M, K, OH, OW, stride, ph, pw, npix;
    int nseg;
    Seg seg[MAXSEG];
};

// Workgroup = 4 waves laid out WM x WN; each wave owns TM x TN tiles of 32 x 32.  Tile BM x BN = 32 WM TM x 32 WN TN.
// The next K step is fetched into registers while the current one is multiplied out of LDS.
template <int KH, int KW, int WM, int WN, int TM, int TN>
__global__ __launch_bounds__(256) void k_incep_conv(const ConvArgs a) {
    constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN;
    constexpr int SA = BM % 64 == 0 ? BM + 32 : BM;   // row pitch: the two lane halves read banks 32 apart
    constexpr int SB = BN % 64 == 0 ? BN + 32 : BN;
    constexpr int KHW = KH * KW;
    constexpr int A_STEP = 256 / BM, A_CNT = BK / A_STEP;
    constexpr int B_STEP = 256 / BN, B_CNT = BK / B_STEP;
    __shared__ float As[BK * SA];
    __shared__ float Bs[BK * SB];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m_blk = blockIdx.y * BM, n_blk = blockIdx.x * BN;
    const int ohw = a.OH * a.OW;

    // this thread's fixed A column and B pixel
    const int am = t % BM, ak = t / BM;
    const bool am_ok = m_blk + am < a.M;
    const int bn = t % BN, bk = t / BN;
    const int p = n_blk + bn;
    const bool p_ok = p < a.npix;
    int iy0 = 0, ix0 = 0;
    const float* src = a.in;
    if (p_ok) {
        const int b = p / ohw, r = p - b * ohw;
        const int oy = r / a.OW, ox = r - oy * a.OW;
        iy0 = oy * a.stride - a.ph;
        ix0 = ox * a.stride - a.pw;
        src = a.in + (int64_t)b * a.C * a.H * a.W;
    }

    float ra[A_CNT], rb[B_CNT];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < A_CNT; ++j) {
            const int k = k0 + ak + j * A_STEP;
            ra[j] = (am_ok && k < a.K) ? a.wt[(int64_t)k * a.M + m_blk + am] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < B_CNT; ++j) {
            const int k = k0 + bk + j * B_STEP;
            float v = 0.0f;
            if (p_ok && k < a.K) {
                const int c = k / KHW, rr = k - c * KHW;
                const int ky = rr / KW, kx = rr - ky * KW;
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = src[((int64_t)c * a.H + iy) * a.W + ix];
            }
            rb[j] = v;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += BK) {
#pragma unroll
        for (int j = 0; j < A_CNT; ++j) As[(ak + j * A_STEP) * SA + am] = ra[j];
#pragma unroll
        for (int j = 0; j < B_CNT; ++j) Bs[(bk + j * B_STEP) * SB + bn] = rb[j];
        __syncthreads();
        if (k0 + BK < a.K) fetch(k0 + BK);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const int kr = kk + (lane >> 5);
            float fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = As[kr * SA + (wm * TM + i) * 32 + (lane & 31)];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = Bs[kr * SB + (wn * TN + j) * 32 + (lane & 31)];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: row m = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the tile, column (pixel) lane & 31
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int q = n_blk + (wn * TN + j) * 32 + (lane & 31);
        if (q >= a.npix) continue;
        const int b = q / ohw, rem = q - b * ohw;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // (sr_mfma32_row written out: through the helper all 32 instantiations compile differently)
                const int m = m_blk + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (m >= a.M) continue;
                // segment by selects (a dynamic index into the kernel-argument struct would go through scratch)
                const bool s1 = a.nseg > 1 && m >= a.seg[1].m0, s2 = a.nseg > 2 && m >= a.seg[2].m0;
                float* o = s2 ? a.seg[2].out : s1 ? a.seg[1].out : a.seg[0].out;
                const int m0 = s2 ? a.seg[2].m0 : s1 ? a.seg[1].m0 : a.seg[0].m0;
                const int coff = s2 ? a.seg[2].coff : s1 ? a.seg[1].coff : a.seg[0].coff;
                const int ctot = s2 ? a.seg[2].ctot : s1 ? a.seg[1].ctot : a.seg[0].ctot;
                const float v = fmaxf(acc[i][j][r] + a.bias[m], 0.0f);
                o[((int64_t)b * ctot + coff + (m - m0)) * ohw + rem] = v;
            }
        }
    }
}

typedef void (*conv_fn)(const ConvArgs);

struct Cfg {
    int bm, bn;
    conv_fn fn;
};

template <int KH, int KW>
void configs(Cfg* c) {
    c[0] = {128, 128, k_incep_conv<KH, KW, 2, 2, 2, 2>};
    c[1] = {64, 64, k_incep_conv<KH, KW, 2, 2, 1, 1>};
    c[2] = {32, 256, k_incep_conv<KH, KW, 1, 4, 1, 2>};
    c[3] = {32, 128, k_incep_conv<KH, KW, 1, 4, 1, 1>};
    c[4] = {64, 128, k_incep_conv<KH, KW, 1, 4, 2, 1>};
}

constexpr int NCFG = 5;

// every KH x KW in {1, 3, 5, 7}^2
bool kernel_configs(int kh, int kw, Cfg* c) {
#define SR_KHW(h, w) \
    if (kh == h && kw == w) return configs<h, w>(c), true;
#define SR_KH(h) SR_KHW(h, 1) SR_KHW(h, 3) SR_KHW(h, 5) SR_KHW(h, 7)
    SR_KH(1) SR_KH(3) SR_KH(5) SR_KH(7)
#undef SR_KH
#undef SR_KHW
    return false;
}

// Tile choice: the useful fraction of the padded M x N work times how well the grid fills 2 workgroups per CU;
// the larger tile wins ties (fewer redundant loads per MFMA).
int pick_config(const Cfg* c, int64_t M, int64_t npix) {
    double best = -1.0;
    int bi = 0;
    for (int i = 0; i < NCFG; ++i) {
        const int64_t gm = sr_ceil_div(M, c[i].bm), gn = sr_ceil_div(npix, c[i].bn);
        const double useful = (double)(M * npix) / (double)(gm * c[i].bm * gn * c[i].bn);
        const double blocks = (double)(gm * gn);
        const double fill = blocks >= 2.0 * SR_NUM_CU ? 1.0 : blocks / (2.0 * SR_NUM_CU);
        const double score = useful * fill * (1.0 + 1e-3 * (c[i].bm * c[i].bn) / 16384.0);
        if (score > best) best = score, bi = i;
    }
    return bi;
}

enum { POOL_MAX3S2 = 0, POOL_AVG3S1 = 1, POOL_MAX3S1 = 2 };

__global__ __launch_bounds__(256) void k_incep_pool(float* __restrict__ out, const float* __restrict__ in, int64_t planes,
                                                    int C, int H, int W, int OH, int OW, int mode, int coff, int ctot) {
    const int64_t total = planes * OH * OW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int ox = (int)(i % OW);
        const int oy = (int)((i / OW) % OH);
        const int64_t pl = i / ((int64_t)OW * OH);
        const int64_t b = pl / C;
        const int c = (int)(pl - b * C);
        const float* s = in + pl * H * W;
        float v;
        if (mode == POOL_MAX3S2) {
            const float* q = s + (int64_t)(2 * oy) * W + 2 * ox;
            v = q[0];
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, q[dy * W + dx]);
        } else {
            const int y0 = max(oy - 1, 0), y1 = min(oy + 2, H), x0 = max(ox - 1, 0), x1 = min(ox + 2, W);
            if (mode == POOL_AVG3S1) {
                float acc = 0.0f;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) acc += s[(int64_t)y * W + x];
                v = acc / (float)((y1 - y0) * (x1 - x0));
            } else {
                v = s[(int64_t)y0 * W + x0];
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) v = fmaxf(v, s[(int64_t)y * W + x]);
            }
        }
        out[((b * ctot + coff + c) * OH + oy) * (int64_t)OW + ox] = v;
    }
}

__global__ __launch_bounds__(256) void k_incep_gap(float* __restrict__ out, const float* __restrict__ in, int64_t planes,
                                                   int hw) {
    const int64_t pl = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pl >= planes) return;
    const float* s = in + pl * hw;
    float acc = 0.0f;
    for (int i = 0; i < hw; ++i) acc += s[i];
    out[pl] = acc / (float)hw;
}

// ---- feature statistics ------------------------------------------------------------------------------------------
// shift[j] = (sum_r f[r, j]) / n over the first batch, fp64, rows in order
__global__ __launch_bounds__(256) void k_fs_shift(double* __restrict__ shift, const float* __restrict__ f, int n, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += (double)f[(int64_t)r * d + j];
    shift[j] = s / (double)n;
}

// sum[j] += sum_r (f[r, j] - shift[j]), rows in order
__global__ __launch_bounds__(256) void k_fs_sum(double* __restrict__ sum, const float* __restrict__ f,
                                                const double* __restrict__ shift, int n, int d) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const double sh = shift[j];
    double s = sum[j];
    for (int r = 0; r < n; ++r) s += (double)f[(int64_t)r * d + j] - sh;
    sum[j] = s;
}

// gram[i, j] += sum_r x[r, i] x[r, j], x = f - shift, for the 64 x 64 tiles (ti <= tj) of the upper triangle.  Each
// thread owns a 4 x 4 block and adds the rows in order with fp64 fma: no atomics, fixed order.
constexpr int GT = 64, GR = 16;

__global__ __launch_bounds__(256) void k_fs_gram(double* __restrict__ gram, const float* __restrict__ f,
                                                 const double* __restrict__ shift, int n, int d, int nt) {
    __shared__ double xi[GR][GT], xj[GR][GT];
    int ti = 0, rest = blockIdx.x;
    while (rest >= nt - ti) rest -= nt - ti, ++ti;
    const int tj = ti + rest;
    const int t = threadIdx.x, ty = t / 16, tx = t % 16;
    const int i0 = ti * GT, j0 = tj * GT;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            acc[u][v] = (i < d && j < d) ? gram[(int64_t)i * d + j] : 0.0;
        }
    for (int r0 = 0; r0 < n; r0 += GR) {
        for (int e = t; e < GR * GT; e += 256) {
            const int rr = e / GT, cc = e % GT, r = r0 + rr;
            const int i = i0 + cc, j = j0 + cc;
            xi[rr][cc] = (r < n && i < d) ? (double)f[(int64_t)r * d + i] - shift[i] : 0.0;
            xj[rr][cc] = (r < n && j < d) ? (double)f[(int64_t)r * d + j] - shift[j] : 0.0;
        }
        __syncthreads();
        const int rn = min(GR, n - r0);
        for (int rr = 0; rr < rn; ++rr) {
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = xi[rr][ty * 4 + u];
#pragma unroll
            for (int v = 0; v < 4; ++v) b[v] = xj[rr][tx * 4 + v];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
            if (i < d && j < d) gram[(int64_t)i * d + j] = acc[u][v];
        }
}

// mean = shift + sum / count; cov[i, j] = (G[min, max] - sum_i sum_j / count) / (count - 1)
__global__ __launch_bounds__(256) void k_fs_finalize(double* __restrict__ mean, double* __restrict__ cov,
                                                     const double* __restrict__ sum, const double* __restrict__ gram,
                                                     const double* __restrict__ shift, int64_t count, int d) {
    const int64_t total = (int64_t)d * d;
    const double cn = (double)count;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / d), j = (int)(e % d);
        const double g = i <= j ? gram[e] : gram[(int64_t)j * d + i];
        cov[e] = (g - sum[i] * sum[j] / cn) / (cn - 1.0);
        if (i == 0) mean[j] = shift[j] + sum[j] / cn;
    }
}

}  // namespace

extern "C" int sr_incep_conv(const float* in, const float* wt, const float* bias, int64_t B, int64_t C, int64_t H,
                             int64_t W, int64_t M, int kh, int kw, int stride, int ph, int pw, int nseg,
                             float* const* seg_out, const int64_t* seg_m0, const int64_t* seg_coff,
                             const int64_t* seg_ctot, sr_stream_t stream) {
    if (B < 0 || C <= 0 || H <= 0 || W <= 0 || M <= 0 || (stride != 1 && stride != 2) || ph < 0 || pw < 0 ||
        nseg < 1 || nseg > MAXSEG || !seg_out || !seg_m0 || !seg_coff || !seg_ctot)
        return SR_EINVAL;
    const int64_t OH = (H + 2 * ph - kh) / stride + 1, OW = (W + 2 * pw - kw) / stride + 1;
    if (H + 2 * ph < kh || W + 2 * pw < kw || OH <= 0 || OW <= 0) return SR_EINVAL;
    Cfg cfg[NCFG];
    if (!kernel_configs(kh, kw, cfg)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!in || !wt || !bias) return SR_EINVAL;
    const int64_t K = C * kh * kw, npix = B * OH * OW;
    if (C * H * W > 0x7FFFFFFF || npix > 0x7FFFFFFF || K * M > 0x7FFFFFFF || H > 65535 || W > 65535) return SR_ERANGE;
    ConvArgs a;
    a.in = in;
    a.wt = wt;
    a.bias = bias;
    a.C = (int)C, a.H = (int)H, a.W = (int)W, a.M = (int)M, a.K = (int)K, a.OH = (int)OH, a.OW = (int)OW;
    a.stride = stride, a.ph = ph, a.pw = pw, a.npix = (int)npix;
    a.nseg = nseg;
    for (int s = 0; s < MAXSEG; ++s) a.seg[s] = {nullptr, (int)M, 0, 0};
    for (int s = 0; s < nseg; ++s) {
        const int64_t m1 = s + 1 < nseg ? seg_m0[s + 1] : M;
        if (!seg_out[s] || seg_m0[s] < 0 || m1 <= seg_m0[s] || m1 > M || (s == 0 && seg_m0[0] != 0) || seg_coff[s] < 0 ||
            seg_coff[s] + (m1 - seg_m0[s]) > seg_ctot[s])
            return SR_EINVAL;
        if (B * seg_ctot[s] * OH * OW > (1LL << 40)) return SR_ERANGE;
        a.seg[s] = {seg_out[s], (int)seg_m0[s], (int)seg_coff[s], (int)seg_ctot[s]};
    }
    const Cfg& c = cfg[pick_config(cfg, M, npix)];
    dim3 grid((unsigned)sr_ceil_div(npix, c.bn), (unsigned)sr_ceil_div(M, c.bm));
    if (grid.y > 65535) return SR_ERANGE;
    hipLaunchKernelGGL(c.fn, grid, dim3(256), 0, sr_stream(stream), a);
    return sr_launch_status();
}

extern "C" int sr_incep_pool(float* out, const float* in, int64_t B, int64_t C, int64_t H, int64_t W, int mode,
                             int64_t coff, int64_t ctot, sr_stream_t stream) {
    if (B < 0 || C <= 0 || H <= 0 || W <= 0 || coff < 0 || coff + C > ctot || mode < 0 || mode > 2) return SR_EINVAL;
    int64_t OH = H, OW = W;
    if (mode == POOL_MAX3S2) {
        if (H < 3 || W < 3) return SR_EINVAL;
        OH = (H - 3) / 2 + 1, OW = (W - 3) / 2 + 1;
    }
    if (B == 0) return SR_OK;
    if (!out || !in) return SR_EINVAL;
    if (H > 65535 || W > 65535 || B * ctot * OH * OW > (1LL << 40)) return SR_ERANGE;
    hipLaunchKernelGGL(k_incep_pool, dim3(sr_stream_grid(B * C * OH * OW, 256)), dim3(256), 0, sr_stream(stream), out, in,
                       B * C, (int)C, (int)H, (int)W, (int)OH, (int)OW, mode, (int)coff, (int)ctot);
    return sr_launch_status();
}

extern "C" int sr_incep_gap(float* out, const float* in, int64_t planes, int64_t hw, sr_stream_t stream) {
    if (planes < 0 || hw <= 0) return SR_EINVAL;
    if (planes == 0) return SR_OK;
    if (!out || !in) return SR_EINVAL;
    if (hw > 0x7FFFFFFF || planes > (1LL << 31) * 255) return SR_ERANGE;
    hipLaunchKernelGGL(k_incep_gap, dim3((unsigned)sr_ceil_div(planes, 256)), dim3(256), 0, sr_stream(stream), out, in,
                       planes, (int)hw);
    return sr_launch_status();
}

extern "C" int sr_fstats_update(double* sum, double* gram, double* shift, const float* f, int64_t n, int64_t d,
                                int first, sr_stream_t stream) {
    if (n < 0 || d <= 0) return SR_EINVAL;
    if (n == 0) return SR_OK;
    if (!sum || !gram || !shift || !f) return SR_EINVAL;
    if (d > 65536 || n > 0x7FFFFFFF || n * d > 0x7FFFFFFF) return SR_ERANGE;
    hipStream_t st = sr_stream(stream);
    const unsigned gb = (unsigned)sr_ceil_div(d, 256);
    if (first) hipLaunchKernelGGL(k_fs_shift, dim3(gb), dim3(256), 0, st, shift, f, (int)n, (int)d);
    hipLaunchKernelGGL(k_fs_sum, dim3(gb), dim3(256), 0, st, sum, f, shift, (int)n, (int)d);
    const int nt = (int)sr_ceil_div(d, GT);
    hipLaunchKernelGGL(k_fs_gram, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, gram, f, shift, (int)n, (int)d, nt);
    return sr_launch_status();
}

extern "C" int sr_fstats_finalize(double* mean, double* cov, const double* sum, const double* gram, const double* shift,
                                  int64_t count, int64_t d, sr_stream_t stream) {
    if (count < 2 || d <= 0 || !mean || !cov || !sum || !gram || !shift) return SR_EINVAL;
    if (d > 65536) return SR_ERANGE;
    hipLaunchKernelGGL(k_fs_finalize, dim3(sr_stream_grid(d * d, 256)), dim3(256), 0, sr_stream(stream), mean, cov, sum,
                       gram, shift, count, (int)d);
    return sr_launch_status();
}
