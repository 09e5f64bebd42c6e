// Stride-2 3x3 convolution (no padding) in a polyphase minimal-filtering form on the gfx950 matrix cores
// (fp32, v_mfma_f32_32x32x2_f32): 25 instead of 36 matrix products per 2x2 output tile.
//
//     y[j, i] = sum_{c, ky, kx} g_c[2j + ky, 2i + kx] * W_c[ky][kx]
//
// Per dimension a 2-output tile reads five samples s0..s4.  The even phase (s0, s2, s4) sees the taps w0, w2, the
// odd phase (s1, s3) the tap w1:
//
//     y0 = (s0 - s2) w0 + s1 w1 + s2 (w0 + w2)          y1 = (s4 - s2) w2 + s3 w1 + s2 (w0 + w2)
//
// i.e. five products  v = (s0 - s2, s1, s4 - s2, s3, s2)  x  u = (w0, w1, w2, w1, w0 + w2)  that land in three slots
// (0, 0, 1, 1, 2) with y0 = slot0 + slot2, y1 = slot1 + slot2.  The tensor product of both dimensions gives 25
// products into 3 x 3 = 9 accumulators per (tile, output channel); all constants are 0 or +-1.  The 25 positions
// are independent GEMMs  M[pos][n][tile] = sum_c U[pos][c][n] * V[pos][c][tile]  whose results are added into the
// accumulator of their slot by the matrix core itself.
//
// One 256-thread workgroup = 64 tiles (16 x 4 -> 32 x 8 output pixels) x 64 output channels, the geometry of
// k_conv_wino (csrc/conv_wino.hip), whose GEMM core this is:
//   * wave (i, j) owns tile block i (32 tiles) and channel block j (32 channels) for all 25 positions: nine
//     accumulator tiles of 32 x 32 = 144 registers, so the output transform is register-local.
//   * K loop over chunks of 4 input channels.  Per chunk the halo patch (17 rows x 65 columns per channel) and the
//     pre-transformed weights U (a contiguous 25.6 KB block, see k_s2_wino_weights) arrive by LDS-DMA; the input
//     transform (one (tile, channel) item per thread, the input scale multiplied in) runs on the VALU between the
//     MFMAs of the previous chunk and writes V in the operand layout; one ds_read_b64 fetches both k-steps of an
//     operand.
//   * Rows of the (2^k+1)-wide maps are not 16-byte aligned.  Row r of chunk channel c starts (c + r) mod 4 floats
//     behind a 16-byte boundary (IH, IW == 1 mod 4, whole tiles), so the DMA fetches the 17 aligned lines that
//     cover the row and the transform reads it behind that rotating lead.  Lines never cross the end of the
//     tensor: its size is a multiple of four floats.
//   * pipeline (one barrier per chunk):  iteration k:  DMA d[k+2], U[k+1]  |  transform d[k+1] -> V[k+1]  |  MFMA
//     over V[k], U[k].  The MFMA stream runs half a chunk behind the operand fetch, as in k_conv_wino.
//   * epilogue: output transform in registers, output scale / bias, float2 stores.
// Deterministic: no atomics, one fixed channel order.
// LDS: 2 x (U 25.6 KB + V 25.6 KB + halo 19.5 KB) + 3 KB landing zone + the scale row = 144.4 KB + 4 C bytes.
#include <type_traits>
#include "conv_s2_wino.h"

#include "mfma_tile.h"

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int TW = 16, TH = 4;            // tiles per workgroup: 32 x 8 output pixels
constexpr int NB = 64;                    // output channels per workgroup
constexpr int KC = 4;                     // input channels per chunk
constexpr int PR = 4 * TH + 1;            // 17 halo rows
constexpr int LPR = 17;                   // 16-byte lines per halo row: 65 columns + a lead of up to 3
constexpr int RP = 4 * LPR;               // row pitch, 68 floats
constexpr int PLANE = PR * RP;            // 1156 floats per channel
constexpr int D_LINES = KC * PR * LPR;    // 1156 lines per chunk
constexpr int D_INSTR = (D_LINES + 63) / 64;          // 19 DMA wave-instructions
constexpr int D_BUF = D_INSTR * 256;
constexpr int D_PER_WAVE = (D_INSTR + 3) / 4;         // 5
constexpr int NPOS = 25;
constexpr int UV = NPOS * 256;            // floats per U (or V) chunk: [pos][half 2][64][k-step 2], channel = 2 e + half
constexpr int U_INSTR = UV / 256;         // 25
constexpr int U_PER_WAVE = (U_INSTR + 3) / 4;         // 7
constexpr int PAD = 4 * UV + 2 * D_BUF;   // landing zone of the surplus DMA instructions (3 x 1 KB)
constexpr int STY = PAD + 3 * 256;        // scale row offset
constexpr int NA = 13;                    // positions of the first half of the MFMA stream (the second has 12)

// order in which the positions are fetched and multiplied: neighbours never share an accumulator
__host__ __device__ constexpr int ord_pos(int i) {
    const int bo[5] = {0, 2, 4, 1, 3};
    return (i / 5) * 5 + bo[i % 5];
}
__host__ __device__ constexpr int slot1(int a) { return a < 2 ? 0 : (a < 4 ? 1 : 2); }
__host__ __device__ constexpr int pos_slot(int pos) { return slot1(pos / 5) * 3 + slot1(pos % 5); }

struct S2WinoParams {
    const float* in;
    const float* u;
    const float* iscale;
    const float* oscale;
    const float* obias;
    float* out;
    int B, C, N, IH, IW, OH, OW;
    int tiles_x, tiles_y, tiles_n;
};

__global__ __launch_bounds__(256) void k_conv_s2_wino(const S2WinoParams p) {
#if __HIP_DEVICE_COMPILE__   // the buffer-resource builtins exist in the device pass only
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const ubuf = smem;
    float* const vbuf = smem + 2 * UV;
    float* const dbuf = smem + 4 * UV;
    float* const sty = smem + STY;

    // ---- tile decode (XCD-chunked: consecutive ids = the output-channel tiles of one input patch on one L2)
    const SrTile wg = sr_tile_decode(sr_xcd_chunk(blockIdx.x, gridDim.x), p.tiles_n, p.tiles_x, p.tiles_y);
    const int n_t = wg.n_t, b = wg.rest;
    const int oy0 = wg.ty * (2 * TH), ox0 = wg.tx * (2 * TW), n0 = n_t * NB;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int wn = wave & 1, wt = wave >> 1;
    const int nchunks = p.C / KC;

    // ---- DMA descriptors of the halo patch: byte offset of this lane's 16-byte line inside the sample (chunk 0).
    // Line L = (c * 17 + r) * 17 + l of the chunk is line l of row 2 oy0 + r of channel c, fetched from the 16-byte
    // boundary at or before the row's first column 2 ox0.  Surplus lanes get an offset beyond the buffer's range: a
    // buffer load returns zeros for them.
    int d_off[D_PER_WAVE];
#pragma unroll
    for (int i = 0; i < D_PER_WAVE; ++i) {
        const int j = wave + 4 * i;
        const int L = j * 64 + lane;
        int off = SR_BUF_OOB;
        if (j < D_INSTR && L < D_LINES) {
            const int c = L / (PR * LPR), q = L % (PR * LPR);
            const int r = q / LPR, l = q % LPR;
            const int first = (c * p.IH + 2 * oy0 + r) * p.IW + 2 * ox0;      // == (c + r) mod 4
            off = ((first & ~3) + 4 * l) * 4;
        }
        d_off[i] = off;
    }
    const int chunk_in_bytes = KC * p.IH * p.IW * 4;
    // (not uniform_rsrc: its readfirstlanes change this kernel's device code; every input here is uniform already)
    const __amdgpu_buffer_rsrc_t r_in = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.in + (int64_t)b * p.C * p.IH * p.IW), 0, nchunks * chunk_in_bytes, SR_BUF_RSRC_WORD3);
    const __amdgpu_buffer_rsrc_t r_u = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(p.u + (int64_t)n_t * nchunks * UV), 0, nchunks * UV * 4, SR_BUF_RSRC_WORD3);

    // one DMA instruction each (all waves issue the same number; surplus ones land in the pad zone)
    auto dma_d1 = [&](int k, int buf, int i) {
        const int j = wave + 4 * i;
        float* dst = j < D_INSTR ? dbuf + buf * D_BUF + j * 256 : smem + PAD + (wave - 1) * 256;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_in, (lptr_t)dst, 16, d_off[i], k * chunk_in_bytes, 0, 0);
    };
    auto dma_u1 = [&](int k, int buf, int i) {
        const int j = wave + 4 * i;
        const bool real = j < U_INSTR;
        float* dst = real ? ubuf + buf * UV + j * 256 : smem + PAD + (wave - 1) * 256;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_u, (lptr_t)dst, 16, real ? lane * 16 : SR_BUF_OOB,
                                                 real ? (k * UV + j * 256) * 4 : 0, 0, 0);
    };
    auto dma_d = [&](int k, int buf) {
#pragma unroll
        for (int i = 0; i < D_PER_WAVE; ++i) dma_d1(k, buf, i);
    };
    auto dma_u = [&](int k, int buf) {
#pragma unroll
        for (int i = 0; i < U_PER_WAVE; ++i) dma_u1(k, buf, i);
    };

    // ---- input transform item of this thread: tile = lane, chunk channel = wave (k-step t_e, half t_h)
    const int t_e = wave >> 1, t_h = wave & 1;
    const int t_rd = wave * PLANE + (4 * (lane >> 4)) * RP + 4 * (lane & 15);
    const int t_wr = t_h * 128 + lane * 2 + t_e;
    struct XF {
        float x[5][5];                // halo patch
        float t[5][5];                // after the row stage
        float v[5][5];                // result
    };
    auto xf_read = [&](XF& x, const float* d0, int a) {
        const float* row = d0 + a * RP + ((wave + a) & 3);       // rotating lead of row 4 ty + a of channel `wave`
#pragma unroll
        for (int j = 0; j < 5; ++j) x.x[a][j] = row[j];
    };
    // row stage with the scale folded in: s*x0 - s*x2, s*x1, s*x4 - s*x2, s*x3, s*x2 (columns j0 .. j1 - 1)
    auto xf_rows = [&](XF& x, float s, int j0, int j1) {
#pragma unroll
        for (int j = j0; j < j1; ++j) {
            const float m = s * x.x[2][j];
            x.t[4][j] = m;
            x.t[0][j] = __builtin_fmaf(s, x.x[0][j], -m);
            x.t[2][j] = __builtin_fmaf(s, x.x[4][j], -m);
            x.t[1][j] = s * x.x[1][j];
            x.t[3][j] = s * x.x[3][j];
        }
    };
    auto xf_cols = [&](XF& x, int a0, int a1) {
#pragma unroll
        for (int a = a0; a < a1; ++a) {
            x.v[a][0] = x.t[a][0] - x.t[a][2];
            x.v[a][1] = x.t[a][1];
            x.v[a][2] = x.t[a][4] - x.t[a][2];
            x.v[a][3] = x.t[a][3];
            x.v[a][4] = x.t[a][2];
        }
    };
    auto xf_step = [&](XF& x, int step, float s) {
        if (step == 0) xf_rows(x, s, 0, 3);
        else if (step == 1) xf_rows(x, s, 3, 5);
        else if (step == 2) xf_cols(x, 0, 3);
        else xf_cols(x, 3, 5);
    };
    auto xf_write = [&](const XF& x, float* vout, int w) { vout[w * 256] = x.v[w / 5][w % 5]; };

    f32x16 acc[9];
#pragma unroll
    for (int s = 0; s < 9; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.0f;

    const int a_off = (half * 64 + wn * 32 + l31) * 2;
    const int b_off = (half * 64 + wt * 32 + l31) * 2;

    // ---- prologue: d[0], U[0], d[1] in flight; V[0] from d[0]
    dma_d(0, 0);
    dma_u(0, 0);
    if (nchunks > 1) dma_d(1, 1);
    for (int c = tid; c < p.C; c += 256) sty[c] = p.iscale ? p.iscale[(int64_t)b * p.C + c] : 1.0f;
    __builtin_amdgcn_s_waitcnt(0x0070);      // vmcnt(0), lgkmcnt(0): this wave's DMAs have landed
    __syncthreads();
    {
        XF x;
        const float s = sty[wave];
#pragma unroll
        for (int a = 0; a < 5; ++a) xf_read(x, dbuf + t_rd, a);
#pragma unroll
        for (int st = 0; st < 4; ++st) xf_step(x, st, s);
#pragma unroll
        for (int w = 0; w < NPOS; ++w) xf_write(x, vbuf + t_wr, w);
    }

    // Operand registers, indexed by fetch order.  Body k issues the MFMAs of the last 12 positions of chunk k-1
    // (registers loaded in body k-1) in slots 0-11 while it fetches the first 13 positions of chunk k, then those 13
    // in slots 12-24 while it fetches the last 12: no MFMA waits on an LDS read issued just before it.
    f2 au[NPOS], bv[NPOS];
    auto mfma1 = [&](int idx, int e) {
        const int s = pos_slot(ord_pos(idx));
        if (e) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(au[idx].y, bv[idx].y, acc[s], 0, 0, 0);
        else acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(au[idx].x, bv[idx].x, acc[s], 0, 0, 0);
    };
    auto mfma_a = [&](int m) { mfma1(m % NA, m / NA); };                          // m = 0 .. 25
    auto mfma_b = [&](int m) { mfma1(NA + m % (NPOS - NA), m / (NPOS - NA)); };   // m = 0 .. 23
    auto body = [&](int k, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        // V[k] complete, d[k+1] / U[k] landed (every wave drained its own DMAs and LDS reads), body k-1's buffers free
        __builtin_amdgcn_s_waitcnt(0x0070);
        __syncthreads();
        // chunks fetched during this body (clamped at the end: a redundant fetch into a free buffer keeps the body
        // branch-free): d[k+2] -> dbuf[k & 1], U[k+1] -> ubuf[(k+1) & 1]
        const int kd = min(k + 2, nchunks - 1), ku = min(k + 1, nchunks - 1);
        const float* ub = ubuf + (k & 1) * UV + a_off;
        const float* vb_ = vbuf + (k & 1) * UV + b_off;
        // transform of chunk k+1 (stale data in, unused out in the last body: no branch in this block)
        const int kn = (k + 1 < nchunks) ? k + 1 : k;
        const float* d0 = dbuf + ((k + 1) & 1) * D_BUF + t_rd;
        float* vout = vbuf + ((k + 1) & 1) * UV + t_wr;
        const float s = sty[kn * KC + wave];
        XF x;
        auto load_op = [&](int idx) {
            const int pos = ord_pos(idx);
            au[idx] = *reinterpret_cast<const f2*>(ub + pos * 256);
            bv[idx] = *reinterpret_cast<const f2*>(vb_ + pos * 256);
        };
        // 25 slots of 2 MFMAs; the LDS / VALU / DMA work is pinned between them (sched_barrier: nothing crosses a
        // slot edge):  slots 0-4 halo rows of the transform item and the halo DMAs, 5-11 the weight DMAs, 5-8 the
        // transform arithmetic, 12-24 the operand stores; operand fetches of position i in slot i (12 also in 11).
#pragma unroll
        for (int sl = 0; sl < NPOS; ++sl) {
            if (sl < NPOS - NA) {
                if (!FIRST) { mfma_b(2 * sl); mfma_b(2 * sl + 1); }
            } else {
                mfma_a(2 * (sl - (NPOS - NA)));
                mfma_a(2 * (sl - (NPOS - NA)) + 1);
            }
            if (sl < NPOS - NA) {
                load_op(sl);
                if (sl == NPOS - NA - 1) load_op(NA - 1);
            } else if (sl < NPOS - 1) {
                load_op(sl + 1);
            }
            if (sl < D_PER_WAVE) dma_d1(kd, k & 1, sl);
            else if (sl < D_PER_WAVE + U_PER_WAVE) dma_u1(ku, (k + 1) & 1, sl - D_PER_WAVE);
            if (sl < 5) xf_read(x, d0, sl);
            else if (sl < 9) xf_step(x, sl - 5, s);
            if (sl >= 12) {
                xf_write(x, vout, 2 * (sl - 12));
                if (sl < 24) xf_write(x, vout, 2 * (sl - 12) + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    body(0, std::true_type{});
    for (int k = 1; k < nchunks; ++k) body(k, std::false_type{});
    // last 12 positions of the last chunk
#pragma unroll
    for (int m = 0; m < 2 * (NPOS - NA); ++m) mfma_b(m);

    // the clamped fetches of the last iteration are still landing in this workgroup's LDS: drain them before the
    // wave can retire
    __builtin_amdgcn_s_waitcnt(0x0070);

    // ---- epilogue: y[r][s] = (A[r][s] + A[2][s]) + (A[r][2] + A[2][2]) per (tile, channel); C/D layout: column
    // (tile) = lane & 31, row (channel) = sr_mfma32_row
    const int tile = wt * 32 + l31;
    const int oy = oy0 + 2 * (tile >> 4), ox = ox0 + 2 * (tile & 15);
    const int64_t plane = (int64_t)p.OH * p.OW;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = sr_mfma32_row(r, half, n0 + wn * 32);
        const float os = p.oscale ? p.oscale[(int64_t)b * p.N + n] : 1.0f;
        const float ob = p.obias ? p.obias[n] : 0.0f;
        float* o = p.out + ((int64_t)b * p.N + n) * plane + (int64_t)oy * p.OW + ox;
        const float c2 = acc[8][r];
        float y[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                y[a][s] = ((acc[a * 3 + s][r] + acc[6 + s][r]) + (acc[a * 3 + 2][r] + c2)) * os + ob;
        *reinterpret_cast<float2*>(o) = make_float2(y[0][0], y[0][1]);
        *reinterpret_cast<float2*>(o + p.OW) = make_float2(y[1][0], y[1][1]);
    }
#endif
}

// U[pos = 5 a + b][c][n] = u_a(ky) u_b(kx) with u = (w0, w1, w2, w1, w0 + w2) per dimension, written in the chunk order
// the kernel DMAs:  [n / 64][c / 4][pos][h][n % 64][e],  chunk-local channel = 2 e + h.  One thread = one output
// channel and the two channels (e = 0, 1) of a pair.
__global__ __launch_bounds__(64) void k_s2_wino_weights(float* __restrict__ u, const float* __restrict__ wt, int C,
                                                        int N, int ldw) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    const int chunk = blockIdx.y >> 1, h = blockIdx.y & 1;
    float q[2][5][5];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int c = chunk * KC + 2 * e + h;
        float g[3][3];
#pragma unroll
        for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = wt[((int64_t)t * C + c) * ldw + n];
        float hh[5][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            hh[0][j] = g[0][j];
            hh[1][j] = g[1][j];
            hh[2][j] = g[2][j];
            hh[3][j] = g[1][j];
            hh[4][j] = g[0][j] + g[2][j];
        }
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            q[e][a][0] = hh[a][0];
            q[e][a][1] = hh[a][1];
            q[e][a][2] = hh[a][2];
            q[e][a][3] = hh[a][1];
            q[e][a][4] = hh[a][0] + hh[a][2];
        }
    }
    float* dst = u + ((int64_t)blockIdx.x * (C / KC) + chunk) * UV + h * 128 + threadIdx.x * 2;
#pragma unroll
    for (int pos = 0; pos < NPOS; ++pos)
        *reinterpret_cast<float2*>(dst + pos * 256) = make_float2(q[0][pos / 5][pos % 5], q[1][pos / 5][pos % 5]);
}

}  // namespace

bool sr_conv_s2_wino_eligible(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                              const void* in, const void* out) {
    if (B <= 0 || C <= 0 || C % KC != 0 || N <= 0 || N % NB != 0 || OH <= 0 || OW <= 0) return false;
    if (OW % (2 * TW) != 0 || OH % (2 * TH) != 0 || IH != 2 * OH + 1 || IW != 2 * OW + 1) return false;
    // LDS: the buffers + the scale row (C floats) must fit the 160 KB of a CU
    if (C > 1024 || sr_conv_s2_wino_blocks(B, N, OH, OW) > 0x7FFFFFFFLL) return false;
    // buffer addressing: byte offsets inside one sample / one output-channel tile of U stay below 2^31 - 16
    if (C * IH * IW >= (1LL << 29) - 4 || (int64_t)NPOS * C * NB >= (1LL << 29)) return false;
    return ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
}

int64_t sr_conv_s2_wino_blocks(int64_t B, int64_t N, int64_t OH, int64_t OW) {
    return B * (OW / (2 * TW)) * (OH / (2 * TH)) * (N / NB);
}

int64_t sr_conv_s2_wino_scratch_floats(int64_t C, int64_t N) { return (int64_t)NPOS * C * N; }

int sr_conv_s2_wino_launch(float* out, const float* in, const float* wt, int64_t ldw, const float* iscale,
                           const float* oscale, const float* obias, int64_t B, int64_t C, int64_t N, int64_t IH,
                           int64_t IW, int64_t OH, int64_t OW, float* scratch, hipStream_t st) {
    S2WinoParams p;
    p.in = in; p.u = scratch; p.iscale = iscale; p.oscale = oscale; p.obias = obias; p.out = out;
    p.B = (int)B; p.C = (int)C; p.N = (int)N; p.IH = (int)IH; p.IW = (int)IW; p.OH = (int)OH; p.OW = (int)OW;
    p.tiles_x = (int)(OW / (2 * TW)); p.tiles_y = (int)(OH / (2 * TH)); p.tiles_n = (int)(N / NB);
    const int lds = (STY + (int)C) * 4;
    if (!sr_allow_dynamic_lds<k_conv_s2_wino>(160 * 1024)) return SR_EINVAL;
    hipLaunchKernelGGL(k_s2_wino_weights, dim3((unsigned)(N / NB), (unsigned)(C / 2)), dim3(64), 0, st, scratch, wt,
                       (int)C, (int)N, (int)ldw);
    const int64_t blocks = sr_conv_s2_wino_blocks(B, N, OH, OW);
    hipLaunchKernelGGL(k_conv_s2_wino, dim3((unsigned)blocks), dim3(256), lds, st, p);
    return sr_launch_status();
}
