// Stride-2 transposed 3x3 convolution (interior of the map) in 25 instead of 36 matrix products per 2x2 input tile,
// exact fp32 (v_mfma_f32_32x32x2_f32).  DESIGN.md 4.1z.
//
// Per dimension (the indexing of k_convt_fused): out[2j] = in[j] w0 + in[j-1] w2, out[2j+1] = in[j] w1.  Output-centred
// tiles: out[4t .. 4t+3] come from a = in[2t-1], b = in[2t], c = in[2t+1] (in[-1] = 0) as
//     m1 = (a-b) w2,  m2 = b (w0+w2),  m3 = (c-b) w0:   out[4t] = m1 + m2,  out[4t+2] = m3 + m2,
//     out[4t+1] = b w1,  out[4t+3] = c w1
// five products instead of six; in two dimensions 25 instead of 36 per 4x4 output tile, all constants 0 / +-1.
//
// The five row products fall into two groups that never meet in an output: {m1, m2, m3} feed the even output rows only,
// {b w1, c w1} the odd ones.  So the launch has two kinds of workgroup (template PAR): the even-row kind keeps 3 x 5 = 15
// accumulator tiles of 32 x 32 per wave (240 registers), the odd-row kind 2 x 5 = 10.  Nothing is combined across
// workgroups, the two kinds write disjoint output rows and read disjoint weight taps (ky = 0, 2 / ky = 1); only the small
// input patch is staged by both.  The even-row workgroups come first in the grid (they run 1.5x as long).
//
// Workgroup = 32 x 8 input positions (4 x 16 tiles -> 64 x 16 output pixels, every second row) x 64 output channels; four
// waves, one per SIMD, as 2 (tile halves) x 2 (channel halves): a wave owns 32 tiles x 32 channels for all of its
// products.  K chunks of 8 input channels: the raw halo patch [8][9][36] and the raw taps [9 or 3][8][64] are staged by
// 16-byte buffer-addressed LDS-DMA, double buffered, one barrier per chunk, by the code k_convt_fused uses (convt_stage.h).  Both transforms
// run in the MFMA wave on the fetched operands (as k_convt_fused scales its inputs): per k-step 18 / 9 operand fetches and
// 21 / 11 VALU instructions, pinned between the 15 / 10 MFMAs of the step before.  The style row is folded into the first
// stage of the input transform.  No scratch, no atomics, a fixed K order: the result is bit-repeatable.
#include "convt_wino.h"

#include "convt_stage.h"

namespace {

constexpr int KC = CONVT_KC;                              // input channels per chunk = 4 k-steps
constexpr int NB = 64;                                    // output channels per workgroup
constexpr int PW = CONVT_PW, PH = 8;                      // input positions per workgroup
constexpr int LEAD = CONVT_LEAD, EWP = CONVT_EWP;         // halo columns i0 - 4 .. i0 + 31: i0 - 1 is column 3 of 36
constexpr int EH = PH + 1;                                // rows j0 - 1 .. j0 + 7
constexpr int PLANE = EH * EWP;                           // 324
constexpr int I_INSTR = (KC * PLANE / 4 + 63) / 64;       // 11 wave instructions of 1 KiB
constexpr int I_FLOATS = I_INSTR * 256;                   // 2816
constexpr int I_PER_WAVE = (I_INSTR + 3) / 4;             // 3 slots (12: one surplus -> pad zone)
constexpr int BUF = I_FLOATS + 9 * KC * NB;               // halo patch, then the taps: 7424 floats = 29 KB
constexpr int PAD = 2 * BUF;
constexpr int STY = PAD + 4 * 256;

struct ConvtWinoParams {
    const float* in;
    const float* wt;
    const float* iscale;
    const float* oscale;
    const float* obias;
    float* out;
    int B, C, N, ldw, IH, IW, OH, OW;
    int tiles_x, tiles_y, tiles_n;
    int half_blocks;          // workgroups of one row parity
};

// PAR = 0: even output rows (row products m1, m2, m3; taps ky = 0, 2), PAR = 1: odd output rows (b w1, c w1; taps ky = 1)
template <int PAR>
__device__ __forceinline__ void convt_wino_body(const ConvtWinoParams& p, float* smem, int bid) {
#if __HIP_DEVICE_COMPILE__   // buffer-resource builtins: device pass only
    constexpr int NR = PAR ? 2 : 3;                       // row products = accumulator rows = input row variants
    constexpr int NWR = PAR ? 1 : 3;                      // weight row variants
    constexpr int NTAP = PAR ? 3 : 9, TAP0 = PAR ? 3 : 0; // staged taps
    constexpr int NM = NR * 5;                            // MFMAs per k-step
    constexpr int W_INSTR = NTAP * KC * NB / 256;         // 18 / 6
    constexpr int W_PER_WAVE = (W_INSTR + 3) / 4;         // 5 / 2
    constexpr int N_DMA = I_PER_WAVE + W_PER_WAVE;        // 8 / 5 per wave and chunk
    static_assert(N_DMA > 4 && N_DMA <= 8, "DMA slots: four behind the barrier, the rest in the first k-step");
    float* const sty = smem + STY;

    const SrTile tile = sr_tile_decode(sr_xcd_chunk(bid, p.half_blocks), p.tiles_n, p.tiles_x, p.tiles_y);
    const int b = tile.rest;
    const int n0 = tile.n_t * NB, j0 = tile.ty * PH, i0 = tile.tx * PW;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int wn = wave & 1, wt = wave >> 1;
    const int ty_l = wt * 2 + (l31 >> 4), tx_l = l31 & 15;    // this lane's tile inside the patch

    // ---- DMA descriptors: byte offsets for chunk 0 (csrc/convt_stage.h)
    int i_off[I_PER_WAVE], w_off[W_PER_WAVE];
#pragma unroll
    for (int i = 0; i < I_PER_WAVE; ++i) i_off[i] = convt_patch_offset<PLANE, I_INSTR>(p, wave + 4 * i, lane, j0, i0);
#pragma unroll
    for (int i = 0; i < W_PER_WAVE; ++i) {
        const int j = wave + 4 * i;
        const int row = 4 * j + (lane >> 4);                 // [tap slot * KC + c], 64 channels = 16 lanes per row
        const int t = TAP0 + row / KC, c = row % KC;
        w_off[i] = j < W_INSTR ? ((t * p.C + c) * p.ldw + n0 + (lane & 15) * 4) * 4 : SR_BUF_OOB;
    }
    const int plane_in = p.IH * p.IW;
    const __amdgpu_buffer_rsrc_t r_w = uniform_rsrc(p.wt, 9 * p.C * p.ldw * 4);
    const __amdgpu_buffer_rsrc_t r_in = uniform_rsrc(p.in + (int64_t)b * p.C * plane_in, p.C * plane_in * 4);
    const int nchunks = p.C / KC;

    // DMA instruction i (0 .. N_DMA - 1) of chunk k (clamped to the last chunk: a surplus fetch lands in a free buffer)
    auto dma1 = [&](int k, int i) {
        const int kc = min(k, nchunks - 1), c0 = kc * KC;
        float* dst = smem + (k & 1) * BUF;
        if (i < I_PER_WAVE) {                                // the halo patch first: it may come from HBM
            const int j = wave + 4 * i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r_in, (lptr_t)(j < I_INSTR ? dst + j * 256 : smem + PAD + wave * 256),
                                                     16, i_off[i], c0 * plane_in * 4, 0, 0);
        } else {                                             // then the (L2-resident) taps
            const int ii = i - I_PER_WAVE, j = wave + 4 * ii;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                r_w, (lptr_t)(j < W_INSTR ? dst + I_FLOATS + j * 256 : smem + PAD + wave * 256), 16, w_off[ii],
                c0 * p.ldw * 4, 0, 0);
        }
    };

    f32x16 acc[NR][5];                                       // [row product][column product]
#pragma unroll
    for (int i = 0; i < NR; ++i)
#pragma unroll
        for (int j = 0; j < 5; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // raw sample (ry, cx) of the tile = input (2 ty - 1 + ry, 2 tx - 1 + cx) = LDS row 2 ty + ry, column LEAD + 2 tx + cx
    const int x_off = half * PLANE + (2 * ty_l + (PAR ? 1 : 0)) * EWP + LEAD + 2 * tx_l;
    const int a_off = I_FLOATS + half * NB + wn * 32 + l31;

    // ---- prologue: chunk 0 complete, the first four instructions of chunk 1 under way
#pragma unroll
    for (int i = 0; i < N_DMA; ++i) dma1(0, i);
#pragma unroll
    for (int i = 0; i < 4; ++i) dma1(1, i);
    for (int c = tid; c < p.C; c += 256) sty[c] = p.iscale ? p.iscale[(int64_t)b * p.C + c] : 1.0f;
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();

    // operands.  Column products q = 0 .. 4 pair input column variant {a-b, b, c-b, b, c}[q] = X[.][CV[q]] with weight
    // column variant {w2, w0+w2, w0, w1, w1}[q] = A[.][CW[q]]; the row products of this parity likewise:
    // even rows: X rows {a-b, b, c-b}, A rows {w2, w0+w2, w0};  odd rows: X rows {b, c}, A row {w1}.
    float RX[NR][3], RA[NWR][3], T0[NR];                     // raw fetches of the next k-step, first-stage left column
    float X[2][NR][4], A[2][NWR][4];
    float sc_next;
    auto load_raw = [&](const float* sb, int c0, int cp) {
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int cx = 0; cx < 3; ++cx) RX[r][cx] = sb[(2 * cp) * PLANE + x_off + r * EWP + cx];
#pragma unroll
        for (int r = 0; r < NWR; ++r)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) RA[r][kx] = sb[((r * 3 + kx) * KC + 2 * cp) * NB + a_off];
        sc_next = sty[c0 + 2 * cp + half];
    };
    // the transform work pinned behind MFMA m of a k-step (at most three VALU instructions per gap), into set s
    auto xform = [&](int m, int s) {
        if (m >= 1 && m <= 3) {                              // first stage, raw column cx: style, row differences
            const int cx = m - 1;
            float v[NR];
            if constexpr (PAR == 0) {
                v[1] = RX[1][cx] * sc_next;
                v[0] = __builtin_fmaf(RX[0][cx], sc_next, -v[1]);
                v[2] = __builtin_fmaf(RX[2][cx], sc_next, -v[1]);
            } else {
                v[0] = RX[0][cx] * sc_next;
                v[1] = RX[1][cx] * sc_next;
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (cx == 0) T0[r] = v[r];
                else if (cx == 1) X[s][r][1] = v[r];
                else X[s][r][3] = v[r];
            }
        } else if (m >= 4 && m < 4 + NR) {                   // second stage, row r: column differences
            const int r = m - 4;
            X[s][r][0] = T0[r] - X[s][r][1];
            X[s][r][2] = X[s][r][3] - X[s][r][1];
        } else if constexpr (PAR == 0) {
            if (m == 7) {                                    // taps: the row sum w0 + w2 per kx ...
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const float lo = RA[0][kx], hi = RA[2][kx];
                    const int q = kx == 0 ? 2 : (kx == 1 ? 3 : 0);    // column variants {w2, ., w0, w1} <- kx {2, ., 0, 1}
                    A[s][0][q] = hi;
                    A[s][2][q] = lo;
                    A[s][1][q] = lo + hi;
                }
            } else if (m == 8) {                             // ... and the column sums
#pragma unroll
                for (int r = 0; r < 3; ++r) A[s][r][1] = A[s][r][0] + A[s][r][2];
            }
        } else if (m == 6) {                                 // odd rows: one tap row, one column sum
            A[s][0][0] = RA[0][2];
            A[s][0][2] = RA[0][0];
            A[s][0][3] = RA[0][1];
            A[s][0][1] = RA[0][0] + RA[0][2];
        }
    };
    load_raw(smem, 0, 0);
#pragma unroll
    for (int m = 0; m < NM; ++m) xform(m, 0);

    // ---- pipeline, as k_convt_fused: the operands of k-step g + 1 are fetched and transformed under the MFMAs of k-step
    // g, across chunk boundaries too (the chunk barrier sits in front of the LAST k-step of a chunk, whose operands are in
    // registers already).  Chunk k + 1 is complete at the barrier of chunk k; chunk k + 2 then goes into the buffer of
    // chunk k, which nobody reads any more: four DMA instructions behind the barrier, the rest in the next k-step.
    for (int k = 0; k < nchunks; ++k) {
        const float* sb = smem + (k & 1) * BUF;
        const float* sbn = smem + ((k + 1) & 1) * BUF;
        const int c0 = k * KC, c0n = min(k + 1, nchunks - 1) * KC;
#pragma unroll
        for (int cp = 0; cp < KC / 2; ++cp) {
            const int cur = cp & 1, nxt = cur ^ 1;
            if (cp == KC / 2 - 1) {
                __builtin_amdgcn_s_waitcnt(0x0F70);
                __syncthreads();
                load_raw(sbn, c0n, 0);
            } else {
                load_raw(sb, c0, cp + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                constexpr int CV[5] = {0, 1, 2, 1, 3}, CW[5] = {0, 1, 2, 3, 3};
                const int rp = m / 5, q = m % 5;
                acc[rp][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[cur][PAR ? 0 : rp][CW[q]], X[cur][rp][CV[q]], acc[rp][q],
                                                                  0, 0, 0);
                xform(m, nxt);
                if (m >= NM - 5 && m < NM - 1) {
                    const int u = m - (NM - 5);                           // 0 .. 3
                    if (cp == 0 && 4 + u < N_DMA) dma1(k + 1, 4 + u);
                    else if (cp == KC / 2 - 1) dma1(k + 2, u);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);

    // ---- epilogue: lane = tile, registers = channels.  Per output row of this parity the five column products give four
    // neighbouring output columns 4 tx .. 4 tx + 3.
    const int64_t plane_out = (int64_t)p.OH * p.OW;
    const int Y0 = 2 * j0 + 4 * ty_l, X0 = 2 * i0 + 4 * tx_l;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int n = sr_mfma32_row(r, half, n0 + wn * 32);
        const float os = p.oscale ? p.oscale[(int64_t)b * p.N + n] : 1.0f;
        const float ob = p.obias ? p.obias[n] : 0.0f;
        float* o = p.out + ((int64_t)b * p.N + n) * plane_out + (int64_t)Y0 * p.OW + X0;
#pragma unroll
        for (int yr = 0; yr < 2; ++yr) {
            float v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                if constexpr (PAR == 0) v[q] = acc[yr ? 2 : 0][q][r] + acc[1][q][r];
                else v[q] = acc[yr][q][r];
            }
            float* orow = o + (int64_t)(2 * yr + PAR) * p.OW;
            orow[0] = (v[0] + v[1]) * os + ob;
            orow[1] = v[3] * os + ob;
            orow[2] = (v[2] + v[1]) * os + ob;
            orow[3] = v[4] * os + ob;
        }
    }
#endif
}

__global__ __launch_bounds__(256) void k_convt_wino(const ConvtWinoParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int bid = blockIdx.x;
    if (bid < p.half_blocks) convt_wino_body<0>(p, smem, bid);
    else convt_wino_body<1>(p, smem, bid - p.half_blocks);
}

}  // namespace

bool sr_convt_wino_eligible(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t ldw, const void* in) {
    if (B <= 0 || C <= 0 || N <= 0 || IH <= 0 || IW <= 0) return false;
    if (IW % PW != 0 || IH % PH != 0 || C % KC != 0 || C > 2048 || N % NB != 0) return false;
    // buffer addressing: byte offsets inside one sample / the weight tensor below 2^31 - 16
    if (C * IH * IW >= (1LL << 29) - 4 || 9 * C * ldw >= (1LL << 29) - 4) return false;
    if (2 * B * (IW / PW) * (IH / PH) * (N / NB) > 0x7FFFFFFFLL) return false;
    return sr_aligned16(in);
}

int sr_convt_wino_launch(float* out, const float* in, const float* wt, int64_t ldw, const float* iscale,
                         const float* oscale, const float* obias, int64_t B, int64_t C, int64_t N, int64_t IH,
                         int64_t IW, hipStream_t st) {
    ConvtWinoParams p;
    p.in = in; p.wt = wt; p.iscale = iscale; p.oscale = oscale; p.obias = obias; p.out = out;
    p.B = (int)B; p.C = (int)C; p.N = (int)N; p.ldw = (int)ldw;
    p.IH = (int)IH; p.IW = (int)IW; p.OH = 2 * (int)IH + 1; p.OW = 2 * (int)IW + 1;
    p.tiles_x = (int)(IW / PW); p.tiles_y = (int)(IH / PH); p.tiles_n = (int)(N / NB);
    p.half_blocks = p.tiles_x * p.tiles_y * p.tiles_n * p.B;
    const int lds = (STY + (int)C) * 4;
    if (!sr_allow_dynamic_lds<k_convt_wino>(160 * 1024)) return SR_EINVAL;
    hipLaunchKernelGGL(k_convt_wino, dim3(2u * (unsigned)p.half_blocks), dim3(256), lds, st, p);
    return sr_launch_status();
}
