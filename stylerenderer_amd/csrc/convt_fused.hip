// Stride-2 transposed 3x3 convolution, all four output phases in ONE workgroup (interior of the map), exact fp32
// (v_mfma_f32_32x32x2_f32).
//
// out[2j + py, 2i + px] = sum over the taps (ky, kx) with ky = py (mod 2), kx = px (mod 2) of
// in[j - (ky >> 1), i - (kx >> 1)] * W[ky][kx]: nine (tap -> phase, input shift) pairs over only four
// distinct input shifts.  Run as four launches (sr_convt_phases_launch, csrc/conv_mfma.hip) every phase re-stages the same
// halo patch and the 1- and 2-tap phases are operand-fetch bound (80 TFLOP/s).  Here a wave keeps the 2x2 MFMA tiles
// of ALL four phases (16 accumulator tiles = 256 registers, one wave per SIMD), so per k-step the 36
// MFMAs share 8 input operands and 18 weight operands, and the halo patch is staged once.
// Workgroup = 32x4 input positions (-> 64x8 output pixels) x 128 output channels, K chunks of 8 input
// channels, double-buffered LDS-DMA as in k_conv_mfma (staging: csrc/convt_stage.h).  The last output row / column
// (grid row H, column W) are left to the strip launches of the per-phase kernel.
#include "convt_fused.h"

#include "convt_stage.h"

namespace {

struct TFused {
    static constexpr int BN = 128;                          // output channels per workgroup
    static constexpr int KC = CONVT_KC;
    static constexpr int PW = CONVT_PW, PH = 4;
    static constexpr int LEAD = CONVT_LEAD;
    static constexpr int EWP = CONVT_EWP;                   // LEAD + 33 columns
    static constexpr int EH = PH + 1;
    static constexpr int PLANE = EH * EWP;                  // 180
    static constexpr int W_FLOATS = 9 * KC * BN;            // [tap][c][128] = 9216
    static constexpr int W_INSTR = W_FLOATS / 256;          // 36 = 9 per wave
    static constexpr int I_INSTR = (KC * PLANE / 4 + 63) / 64;   // 6
    static constexpr int I_FLOATS = I_INSTR * 256;          // 1536
    static constexpr int BUF = W_FLOATS + I_FLOATS;         // taps, then the halo patch: 10752 floats = 42 KB
    static constexpr int W_PER_WAVE = 9, I_PER_WAVE = 2;    // 36 / 8 instruction slots (surplus -> pad zone)
    static constexpr int PAD = 2 * BUF;
    static constexpr int STY = PAD + 4 * 256;
};

#ifdef CONVT_TIMING
// debug build only (scripts/build_variant.sh): per-workgroup time stamps of wave 0
__device__ long long g_convt_stamps[8 * 16384];
#define CONVT_STAMP(i) do { if (threadIdx.x == 0) { g_convt_stamps[(blockIdx.x & 16383) * 8 + (i)] = wall_clock64(); } } while (0)
#else
#define CONVT_STAMP(i)
#endif

// KS: K slices (round 5).  With few tiles and a long channel loop (the 32^2 x 512-channel layer at batch 4: 128
// workgroups walking 64 chunks each) slice s of p.ks walks the channels [s * c_per_slice, (s + 1) * c_per_slice): the
// same loop over k = 0 .. n - 1 with the bases of the two buffer resources and of the style row moved, raw sums to
// partial[s] in the layout of `out`; k_convt_fused_reduce adds the slices in order and applies scale / bias.
template <bool KS>
__global__ __launch_bounds__(256) void k_convt_fused(const ConvParams p) {
#if __HIP_DEVICE_COMPILE__   // buffer-resource builtins: device pass only (the host pass needs just the stub)
    using G = TFused;
    constexpr int BN = G::BN;
    CONVT_STAMP(0);
#ifdef CONVT_TIMING
    const long long convt_c0 = clock64();
#endif
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const sty = smem + G::STY;

    const SrTile tile = sr_tile_decode(sr_xcd_chunk(blockIdx.x, gridDim.x), p.tiles_n, p.tiles_x, p.tiles_y);
    const int b = KS ? tile.rest % p.B : tile.rest;
    const int slice = KS ? tile.rest / p.B : 0;
    const int c_beg = KS ? slice * p.c_per_slice : 0;          // first channel of this workgroup's K range
    const int c_cnt = KS ? p.c_per_slice : p.C;
    const int n0 = tile.n_t * BN, j0 = tile.ty * G::PH, i0 = tile.tx * G::PW;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int wco = wave & 1, wpx = wave >> 1;

    // ---- DMA descriptors: byte offsets inside the weight tensor / this sample for chunk 0 (csrc/convt_stage.h)
    int w_off[G::W_PER_WAVE];
#pragma unroll
    for (int i = 0; i < G::W_PER_WAVE; ++i) {
        const int j = wave + 4 * i;
        const int row = 2 * j + half;                       // [tap * KC + c]
        const int t = row / G::KC, c = row % G::KC;
        const int col = min(n0 + l31 * 4, p.ldw - 4);
        w_off[i] = j < G::W_INSTR ? ((t * p.C + c) * p.ldw + col) * 4 : SR_BUF_OOB;
    }
    int i_off[G::I_PER_WAVE];
#pragma unroll
    for (int i = 0; i < G::I_PER_WAVE; ++i) i_off[i] = convt_patch_offset<G::PLANE, G::I_INSTR>(p, wave + 4 * i, lane, j0, i0);
    const int plane_in = p.IH * p.IW;
    const __amdgpu_buffer_rsrc_t r_w = uniform_rsrc(p.wt + (int64_t)c_beg * p.ldw, (9 * p.C - c_beg) * p.ldw * 4);
    const __amdgpu_buffer_rsrc_t r_in = uniform_rsrc(p.in + ((int64_t)b * p.C + c_beg) * plane_in, c_cnt * plane_in * 4);
    const int nchunks = c_cnt / G::KC;

    // DMA instruction i (0 .. 10) of chunk k (clamped to the last chunk: a surplus fetch lands in a free buffer)
    auto dma1 = [&](int k, int i) {
        const int kc = min(k, nchunks - 1), c0 = kc * G::KC;
        float* dst = smem + (k & 1) * G::BUF;
        if (i < G::I_PER_WAVE) {                             // the halo patch first: it may come from HBM
            const int j = wave + 4 * i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                r_in, (lptr_t)(j < G::I_INSTR ? dst + G::W_FLOATS + j * 256 : smem + G::PAD + wave * 256), 16, i_off[i],
                c0 * plane_in * 4, 0, 0);
        } else {                                             // then the (L2-resident) weights
            const int ii = i - G::I_PER_WAVE, j = wave + 4 * ii;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r_w, (lptr_t)(j < G::W_INSTR ? dst + j * 256 : smem + G::PAD + wave * 256),
                                                     16, w_off[ii], c0 * p.ldw * 4, 0, 0);
        }
    };
    constexpr int N_DMA = G::W_PER_WAVE + G::I_PER_WAVE;    // 11 per wave and chunk

    // accumulators: [phase py*2+px][channel tile][pixel tile]
    f32x16 acc[4][2][2];
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ph][i][j][r] = 0.0f;

    int a_off[2], b_off[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        a_off[t] = half * BN + wco * 64 + t * 32 + l31;
        const int py = wpx * 2 + t;                          // pixel tile t = input row py of the patch
        b_off[t] = G::W_FLOATS + half * G::PLANE + (py + 1) * G::EWP + l31 + G::LEAD + 1;
    }

    // ---- pipeline.  One wave per SIMD: nobody else hides LDS latency or DMA issue, so
    //  * the 26 operands of k-step g + 1 are fetched (and the 8 input operands style-scaled) under the 36 MFMAs
    //    of k-step g — across chunk boundaries too: the chunk barrier sits in front of the LAST k-step of a
    //    chunk, whose operands are already in registers, and the first k-step of the next chunk is fetched
    //    under it (no MFMA ever waits for an LDS round trip behind a barrier);
    //  * the 11 DMA instructions of a chunk are spread over three k-steps, one per 8 MFMAs.
    // Chunk k + 1 is complete at the barrier of chunk k (issued a whole chunk earlier); chunk k + 2 then goes
    // into the buffer of chunk k, which nobody reads any more.
#pragma unroll
    for (int i = 0; i < N_DMA; ++i) dma1(0, i);
#pragma unroll
    for (int i = 0; i < 4; ++i) dma1(1, i);
    for (int c = tid; c < c_cnt; c += 256) sty[c] = p.iscale ? p.iscale[(int64_t)b * p.C + c_beg + c] : 1.0f;
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();

    float A[2][9][2], X[2][4][2];                        // [set][tap][channel tile], [set][dy*2+dx][pixel tile]
    float sc_next;
    auto load_set = [&](const float* sb, int c0, int cp, int set) {
#pragma unroll
        for (int sh = 0; sh < 4; ++sh)
#pragma unroll
            for (int t = 0; t < 2; ++t)
                X[set][sh][t] = sb[(2 * cp) * G::PLANE + b_off[t] - (sh >> 1) * G::EWP - (sh & 1)];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int t = 0; t < 2; ++t) A[set][tap][t] = sb[(tap * G::KC + 2 * cp) * BN + a_off[t]];
        sc_next = sty[c0 + 2 * cp + half];
    };
    load_set(smem, 0, 0, 0);
#pragma unroll
    for (int sh = 0; sh < 4; ++sh) { X[0][sh][0] *= sc_next; X[0][sh][1] *= sc_next; }
    CONVT_STAMP(1);

    for (int k = 0; k < nchunks; ++k) {
        const float* sb = smem + (k & 1) * G::BUF;
        const float* sbn = smem + ((k + 1) & 1) * G::BUF;
        const int c0 = k * G::KC, c0n = min(k + 1, nchunks - 1) * G::KC;
#pragma unroll
        for (int cp = 0; cp < G::KC / 2; ++cp) {
            const int cur = cp & 1, nxt = cur ^ 1;
            if (cp == G::KC / 2 - 1) {
                // chunk k + 1 landed (every wave drained its own DMAs), all reads of chunk k retired
                __builtin_amdgcn_s_waitcnt(0x0F70);
                __syncthreads();
                load_set(sbn, c0n, 0, nxt);
            } else {
                load_set(sb, c0, cp + 1, nxt);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int tap = ky * 3 + kx, ph = (ky & 1) * 2 + (kx & 1), sh = (ky >> 1) * 2 + (kx >> 1);
                    acc[ph][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[cur][tap][0], X[cur][sh][0], acc[ph][0][0], 0, 0, 0);
                    acc[ph][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[cur][tap][0], X[cur][sh][1], acc[ph][0][1], 0, 0, 0);
                    acc[ph][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[cur][tap][1], X[cur][sh][0], acc[ph][1][0], 0, 0, 0);
                    acc[ph][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[cur][tap][1], X[cur][sh][1], acc[ph][1][1], 0, 0, 0);
                    // style onto the 8 input operands of the next k-step (not its 18 weights): one multiply per
                    // tap from the second tap on (eight MFMAs cover the LDS latency of the fetch above)
                    if (tap >= 1) X[nxt][(tap - 1) >> 1][(tap - 1) & 1] *= sc_next;
                    // DMA: chunk k + 2 starts behind the barrier (4 instructions), the rest of chunk k + 1 follows in
                    // the first two k-steps of the next iteration... seen from this iteration: cp 0 / 1 finish
                    // chunk k + 1, the last k-step starts chunk k + 2
                    if ((tap & 1) == 1) {
                        const int u = tap >> 1;                               // 0 .. 3
                        if (cp == 0) dma1(k + 1, 4 + u);
                        else if (cp == 1 && 8 + u < N_DMA) dma1(k + 1, 8 + u);
                        else if (cp == G::KC / 2 - 1) dma1(k + 2, u);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);
    CONVT_STAMP(2);

    // ---- epilogue: lane = input column i, registers = channels; phases (py, 0) and (py, 1) are the
    // neighbouring output columns 2i, 2i + 1 of output row 2j + py
    const int64_t plane_out = (int64_t)p.OH * p.OW;
#pragma unroll
    for (int pt = 0; pt < 2; ++pt) {
        const int j = j0 + wpx * 2 + pt, i = i0 + l31;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = sr_mfma32_row(r, half, n0 + wco * 64 + ct * 32);
                if (n < p.N) {
                    const float os = (!KS && p.oscale) ? p.oscale[(int64_t)b * p.N + n] : 1.0f;
                    const float ob = (!KS && p.obias) ? p.obias[n] : 0.0f;
                    float* o = (KS ? p.partial + (int64_t)slice * p.B * p.N * plane_out : p.out) +
                               ((int64_t)b * p.N + n) * plane_out + (int64_t)(2 * j) * p.OW + 2 * i;
                    o[0] = acc[0][ct][pt][r] * os + ob;
                    o[1] = acc[1][ct][pt][r] * os + ob;
                    o[p.OW] = acc[2][ct][pt][r] * os + ob;
                    o[p.OW + 1] = acc[3][ct][pt][r] * os + ob;
                }
            }
    }
    CONVT_STAMP(3);
#ifdef CONVT_TIMING
    if (threadIdx.x == 0) g_convt_stamps[(blockIdx.x & 16383) * 8 + 5] = clock64() - convt_c0;
#endif
#endif
}

// interior outputs (rows < 2 IH, columns < 2 IW) = the slices of k_convt_fused<true> added in order, then scale / bias
__global__ __launch_bounds__(256) void k_convt_fused_reduce(const ConvParams p) {
    const int iw2 = 2 * p.IW, ih2 = 2 * p.IH;
    const int64_t plane_out = (int64_t)p.OH * p.OW, planes = (int64_t)p.B * p.N;
    const int64_t total = planes * ih2 * (iw2 / 4);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / ((int64_t)ih2 * (iw2 / 4));
        const int q = (int)(i - row * (int64_t)ih2 * (iw2 / 4));
        const int Y = q / (iw2 / 4), X = (q - Y * (iw2 / 4)) * 4;
        const int64_t at = row * plane_out + (int64_t)Y * p.OW + X;
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int s = 0; s < p.ks; ++s) {
            const float* src = p.partial + (int64_t)s * planes * plane_out + at;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += src[k];
        }
        const float os = p.oscale ? p.oscale[row] : 1.0f, ob = p.obias ? p.obias[row % p.N] : 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) p.out[at + k] = acc[k] * os + ob;
    }
}

}  // namespace

#ifdef CONVT_TIMING
extern "C" int sr_debug_convt_stamps(long long* host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_convt_stamps), (size_t)n * sizeof(long long));
}
#endif

bool sr_convt_fused_eligible(int64_t C, int64_t IH, int64_t IW, int64_t ldw, const void* in) {
    // buffer addressing: byte offsets inside one sample / the weight tensor below 2^31 - 16
    if (C * IH * IW >= (1LL << 29) - 4 || 9 * C * ldw >= (1LL << 29) - 4) return false;
    return IH % TFused::PH == 0 && IW % TFused::PW == 0 && C % TFused::KC == 0 && C <= 2048 && sr_aligned16(in);
}

int64_t sr_convt_fused_blocks(int64_t B, int64_t N, int64_t IH, int64_t IW) {
    return (IW / TFused::PW) * (IH / TFused::PH) * ((N + TFused::BN - 1) / TFused::BN) * B;
}

int sr_convt_fused_slices(int64_t fused_blocks, int64_t C, int64_t IH, int64_t IW) {
    if (IW % TFused::PW || IH % TFused::PH) return 1;
    for (int ks = 2; ks <= 4; ks *= 2)
        if (C % (ks * TFused::KC) == 0 && C / ks >= 64 && fused_blocks * ks >= 192) return ks;
    return 1;
}

int sr_convt_fused_launch(ConvParams p, int ks, hipStream_t st) {
    if (ks > 1) { p.ks = ks; p.c_per_slice = p.C / ks; }
    p.tiles_x = p.IW / TFused::PW;
    p.tiles_y = p.IH / TFused::PH;
    p.tiles_n = (p.N + TFused::BN - 1) / TFused::BN;
    const int64_t blocks = (int64_t)p.tiles_x * p.tiles_y * p.tiles_n * p.B * p.ks;
    if (blocks > 0x7FFFFFFFLL) return SR_ERANGE;
    if (p.ks > 1) {
        const int lds = (TFused::STY + p.c_per_slice) * 4;
        hipLaunchKernelGGL(k_convt_fused<true>, dim3((unsigned)blocks), dim3(256), lds, st, p);
        const int64_t total = (int64_t)p.B * p.N * 2 * p.IH * (2 * p.IW / 4);
        hipLaunchKernelGGL(k_convt_fused_reduce, dim3(sr_stream_grid(total, 256)), dim3(256), 0, st, p);
        return sr_launch_status();
    }
    const int lds = (TFused::STY + p.C) * 4;
    hipLaunchKernelGGL(k_convt_fused<false>, dim3((unsigned)blocks), dim3(256), lds, st, p);
    return sr_launch_status();
}
