// upfirdn2d for gfx950: zero-insert upsample -> pad/crop -> 2-D FIR -> decimate.
//
// Replaces the reference's upfirdn2d_op and its six tiled "modes" + large fallback
// (reference op/upfirdn2d_kernel.cu:79-257; mode table op/upfirdn2d.cpp:50-75).  MI355X-first design:
//   * k_fir4_tile — the shape that carries all the bytes in the generator (Blur after the
//     stride-2 transposed conv and its gradient: up = down = 1, 4x4 taps; reference layers.py:272-275):
//     a 32x64 output tile per 256-thread workgroup, the 35x67 input halo tile staged once in LDS
//     (9.5 KiB, rows padded to 68 floats so every lane's 8-float window is two aligned
//     ds_read_b128), each lane producing a 2x4 output micro-tile from a register sliding window and
//     writing 16-byte stores.  HBM traffic = 4*(N_in + N_out) bytes, the algorithmic minimum.
//   * k_fir4_band_fwd / k_fir4_band_nba_bwd — the same blur with the up-sampling layers' tail (noise, bias, LeakyReLU) and
//     its one-pass backward on the large maps, tiled by bands of whole rows: every HBM access but a band's first and
//     last three floats is an aligned 16-byte one although rows of 2^k + 1 floats are not aligned.
//   * k_upfirdn_generic — any up/down/kernel/pad (ToRGB skip upsample up=2, its gradient down=2,
//     odd kernels, crops): one output per lane, consecutive lanes on consecutive columns
//     (coalesced), polyphase tap skipping instead of multiplying inserted zeros.
// Taps are accumulated ky-major then kx in fp32 with separate multiply and add
// (-ffp-contract=off), the order the oracle (oracle/ops_np.py) fixes, so HIP == oracle bitwise.
#include "common.h"

#include <cstdlib>
#include <type_traits>

namespace {

struct UfdParams {
    int in_h, in_w, out_h, out_w, kh, kw;
    int up_x, up_y, down_x, down_y, pad_x0, pad_y0;
};

__device__ __forceinline__ int floor_div(int a, int b) {
    int q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}

// ------------------------------------------------------------------------------ generic
__global__ __launch_bounds__(256) void k_upfirdn_generic(float* __restrict__ out,
                                                         const float* __restrict__ x,
                                                         const float* __restrict__ k, UfdParams p,
                                                         int64_t total) {
    extern __shared__ float s_k[];      // flipped kernel
    for (int i = threadIdx.x; i < p.kh * p.kw; i += blockDim.x) {
        const int ky = i / p.kw, kx = i % p.kw;
        s_k[i] = k[(p.kh - 1 - ky) * p.kw + (p.kw - 1 - kx)];
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t plane_out = (int64_t)p.out_h * p.out_w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t plane = i / plane_out;
        const int rem = (int)(i - plane * plane_out);
        const int oy = rem / p.out_w, ox = rem - oy * p.out_w;
        const float* src = x + plane * (int64_t)p.in_h * p.in_w;
        // tap ky touches upsampled row  oy*down - pad0 + ky ; only multiples of `up` hold data
        const int my = oy * p.down_y - p.pad_y0, mx = ox * p.down_x - p.pad_x0;
        int ky0 = (-my) % p.up_y;   // first ky with (my + ky) % up == 0
        if (ky0 < 0) ky0 += p.up_y;
        int kx0 = (-mx) % p.up_x;
        if (kx0 < 0) kx0 += p.up_x;
        float acc = 0.0f;
        for (int ky = ky0; ky < p.kh; ky += p.up_y) {
            const int iy = (my + ky) / p.up_y;          // exact: divisible by construction
            if (iy < 0 || iy >= p.in_h) continue;
            for (int kx = kx0; kx < p.kw; kx += p.up_x) {
                const int ix = (mx + kx) / p.up_x;
                if (ix < 0 || ix >= p.in_w) continue;
                const float prod = src[(int64_t)iy * p.in_w + ix] * s_k[ky * p.kw + kx];
                acc = acc + prod;
            }
        }
        out[i] = acc;
    }
}

// ------------------------------------------------------------------------------ 4x4, up=down=1
constexpr int T_OH = 32, T_OW = 64, T_K = 4;
constexpr int T_IH = T_OH + T_K - 1;        // 35
constexpr int T_IW = T_OW + T_K - 1;        // 67
constexpr int T_LD = 68;                    // LDS row pitch (floats), multiple of 4
// Aligned staging (ALN): when the input rows are 16-byte aligned (in_w % 4 == 0, aligned base) and the window starts two
// columns left of a tile boundary (pad_x0 == 2: the gradient of the up-sampling layers' blur, the blur in front of the
// discriminator's stride-2 convolutions), the window is widened to start FOUR columns left — 72 columns = 18 aligned
// 16-byte groups per row, 630 vector loads per tile instead of 2 380 scalar ones with their index arithmetic; the FIR then
// reads its 8-float window at column lx + 2 (8-byte aligned: four ds_read_b64).
constexpr int A_LD = 72, A_G = A_LD / 4;    // pitch / 16-byte groups per row of the widened window

typedef const float __attribute__((address_space(4)))* cptr_t;

// The sixteen taps are wave-uniform: scalar loads into SGPRs (constant address space) instead of sixteen vector registers
// per lane — with the row-sliding window below the kernels fit 64 registers (eight waves per SIMD).
#define FIR4_LOAD_TAPS(kf, k)                                   \
    float kf[16];                                               \
    {                                                           \
        const cptr_t kc_ = (cptr_t)(uintptr_t)(k);              \
        _Pragma("unroll") for (int i_ = 0; i_ < 16; ++i_) kf[i_] = kc_[15 - i_];   /* flipped */ \
    }

// 2 x 4 outputs per lane from rows ly .. ly+4 of the staged tile.  Row t is tap row ky = t of output row 0 and ky = t - 1
// of output row 1: walking t upwards visits every accumulator's taps ky-major then kx — the bit-exact order of the
// oracle (multiply and add separate) — with one 8-float window row live at a time.
template <int LD, int COFF>
__device__ __forceinline__ void fir4_rows(const float* s_in, const float (&kf)[16], int lx, int ly, float (&acc)[2][4]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        float win[8];
        const float* row = s_in + (ly + t) * LD + lx + COFF;
        if (COFF % 4 == 0) {
            const float4 a = *reinterpret_cast<const float4*>(row);
            const float4 b = *reinterpret_cast<const float4*>(row + 4);
            win[0] = a.x; win[1] = a.y; win[2] = a.z; win[3] = a.w;
            win[4] = b.x; win[5] = b.y; win[6] = b.z; win[7] = b.w;
        } else {
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float2 a = *reinterpret_cast<const float2*>(row + 2 * h);
                win[2 * h] = a.x;
                win[2 * h + 1] = a.y;
            }
        }
#ifdef SR_FIR_SEP_EXPERIMENT
        // timing experiment: separable taps, fused multiply-adds (8 per output instead of 16 mul + 16 add)
        float hrow[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float h = win[c] * kf[0];
            h = __builtin_fmaf(win[c + 1], kf[1], h);
            h = __builtin_fmaf(win[c + 2], kf[2], h);
            h = __builtin_fmaf(win[c + 3], kf[3], h);
            hrow[c] = h;
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int ky = t - r;
            if (ky < 0 || ky > 3) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = ky == 0 ? hrow[c] * kf[4] : __builtin_fmaf(hrow[c], kf[4 + ky], acc[r][c]);
        }
#else
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int ky = t - r;
            if (ky < 0 || ky > 3) continue;
#pragma unroll
            for (int kx = 0; kx < 4; ++kx)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float prod = win[c + kx] * kf[ky * 4 + kx];
                    acc[r][c] = acc[r][c] + prod;
                }
        }
#endif
    }
}

__device__ __forceinline__ void fir4_store_row(float* q, int ox, int out_w, const float (&v)[4]) {
    if (ox + 3 < out_w && ((reinterpret_cast<uintptr_t>(q) & 15) == 0)) {
        *reinterpret_cast<float4*>(q) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (ox + c < out_w) q[c] = v[c];
    }
}

// NBA: the StyledConv tail (reference model.py:26-32: NoiseInjection + FusedLeakyReLU) applied to the
// blurred value before it is stored — y = lrelu((f + nw * noise[b, p]) + bias[c]) * gain, the same
// operation order as k_nba_fwd — which saves one full read + write of the activation per layer.
struct FirNba {
    const float* noise;       // [B or 1, 1, out_h, out_w] or NULL
    const float* noise_w;     // 1 float (device) when noise != NULL
    const float* bias;        // [C] or NULL
    int64_t noise_bstride;
    int channels;
    float alpha, gain;
};

template <bool NBA, bool ALN>
__global__ __launch_bounds__(256) void k_fir4_tile(float* __restrict__ out,
                                                   const float* __restrict__ x,
                                                   const float* __restrict__ k, int in_h, int in_w,
                                                   int out_h, int out_w, int pad_x0, int pad_y0,
                                                   int tiles_x, int tiles_y, FirNba nba) {
    constexpr int LD = ALN ? A_LD : T_LD;
    __shared__ __attribute__((aligned(16))) float s_in[T_IH * LD];
    int bid = blockIdx.x;
    const int tx_i = bid % tiles_x;
    bid /= tiles_x;
    const int ty_i = bid % tiles_y;
    const int64_t plane = bid / tiles_y;
    const int oy0 = ty_i * T_OH, ox0 = tx_i * T_OW;
    const int iy0 = oy0 - pad_y0, ix0 = ox0 - pad_x0;
    const float* src = x + plane * (int64_t)in_h * in_w;
    FIR4_LOAD_TAPS(kf, k)

    if (ALN) {
        // (pad_x0 == 2) window columns ox0 - 4 .. ox0 + 67 as 18 aligned groups per row; a group is inside or outside
        constexpr int NG = T_IH * A_G, ST = (NG + 255) / 256;
        float4 stage[ST];
#pragma unroll
        for (int j = 0; j < ST; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int r = i / A_G, g = i - r * A_G;
            const int gy = iy0 + r, gx = ox0 - 4 + 4 * g;
            const bool ok = i < NG && gy >= 0 && gy < in_h && gx >= 0 && gx < in_w;
            const float4 v = *reinterpret_cast<const float4*>(src + (ok ? (int64_t)gy * in_w + gx : 0));
            stage[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < ST; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < NG) reinterpret_cast<float4*>(s_in)[i] = stage[j];
        }
    } else {
        // stage the halo tile: consecutive lanes read consecutive columns of one row (coalesced).  All ten
        // loads of a lane are issued before the first LDS write (unconditional loads from clamped addresses,
        // masked afterwards): one memory round trip per tile instead of ten dependent ones.
        constexpr int T_STAGE = (T_IH * T_LD + 255) / 256;
        float stage[T_STAGE];
#pragma unroll
        for (int j = 0; j < T_STAGE; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int r = i / T_LD, c = i - r * T_LD;
            const int gy = iy0 + r, gx = ix0 + c;
            const bool ok = i < T_IH * T_LD && c < T_IW && gy >= 0 && gy < in_h && gx >= 0 && gx < in_w;
            const float v = src[ok ? (int64_t)gy * in_w + gx : 0];
            stage[j] = ok ? v : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < T_STAGE; ++j) {
            const int i = threadIdx.x + 256 * j;
            if (i < T_IH * T_LD) s_in[i] = stage[j];
        }
    }
    __syncthreads();

    const int lx = (threadIdx.x & 15) * 4;       // 4 output columns per lane
    const int ly = (threadIdx.x >> 4) * 2;       // 2 output rows per lane
    float acc[2][4];
    fir4_rows<LD, ALN ? 2 : 0>(s_in, kf, lx, ly, acc);

    float* dst = out + plane * (int64_t)out_h * out_w;
    float nw = 0.0f, bb = 0.0f;
    const float* nz = nullptr;
    if (NBA) {
        const int64_t b = plane / nba.channels;
        if (nba.noise) {
            nw = nba.noise_w[0];
            nz = nba.noise + b * nba.noise_bstride;
        }
        if (nba.bias) bb = nba.bias[plane - b * nba.channels];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + ly + r;
        if (oy >= out_h) continue;
        const int ox = ox0 + lx;
        if (NBA) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v = acc[r][c];
                if (nz && ox + c < out_w) v = v + nw * nz[(int64_t)oy * out_w + ox + c];
                v += bb;
                acc[r][c] = ((v > 0.0f) ? v : v * nba.alpha) * nba.gain;
            }
        }
        fir4_store_row(dst + (int64_t)oy * out_w + ox, ox, out_w, acc[r]);
    }
}

// ------------------------------------------------------------------------------ backward of blur + tail, one pass
// Gradient of  y = lrelu((blur(x) + w * noise) + bias) * gain  (k_fir4_tile<true>) w.r.t. x, with the reductions of
// the tail's backward, in ONE pass over the two full-size tensors it needs (gy, y) — the two-kernel form
// (k_nba_bwd: read gy, y, write gpre;  k_fir4_tile<false>: read gpre, write gx) moves five tensors, this one three.
// The halo tile of gpre = lrelu'(y) * gy * gain is computed while it is staged (same expression as k_nba_bwd, so gx
// is bit-identical to the two-kernel form); every gpre element belongs to exactly one tile's "owned" 32 x 64 corner
// of its 35 x 67 window, where it enters the three sums
//     sum gpre (bias gradient), sum gpre * noise (noise strength), sum gpre * y0 (demodulation row-dot; y0 = the
//     pre-activation value of the forward pass rebuilt from y, see k_nba_bwd<true>)
// as one partial triple per workgroup; the finish kernels of csrc/fused_elem.hip add them in a fixed order.
struct FirNbaBwd {
    const float* fw;          // forward output y [planes, in_h, in_w]
    const float* noise;       // [B or 1, 1, in_h, in_w] or NULL
    const float* noise_w;     // 1 float (device) when noise != NULL
    const float* bias;        // [C] or NULL
    float* partial;           // [planes * tiles] pairs (sum gpre, sum gpre * noise)
    float* dot_partial;       // [planes * tiles]
    int64_t noise_bstride;
    int channels;
    float alpha, gain, inv_pos, inv_neg;
};

struct FirSums {
    float b, n, d;
};

__device__ __forceinline__ float fir4_gpre(float g, float o, float nzv, bool ok, bool owned, const FirNbaBwd& q, float nw,
                                           float bb, FirSums& s) {
    const float v = ok ? ((o > 0.0f) ? g : g * q.alpha) * q.gain : 0.0f;
    if (owned) {
        const float y0 = ((o > 0.0f) ? o * q.inv_pos : o * q.inv_neg) - nw * nzv - bb;
        s.b += v;
        s.n += v * nzv;
        s.d += v * y0;
    }
    return v;
}

template <bool ALN>
__global__ __launch_bounds__(256) void k_fir4_nba_bwd(float* __restrict__ out, const float* __restrict__ gy,
                                                      const float* __restrict__ k, int in_h, int in_w, int out_h,
                                                      int out_w, int pad_x0, int pad_y0, int tiles_x, int tiles_y,
                                                      FirNbaBwd q) {
    constexpr int LD = ALN ? A_LD : T_LD;
    __shared__ __attribute__((aligned(16))) float s_in[T_IH * LD];
    __shared__ float s_red[12];
    int bid = blockIdx.x;
    const int tile = bid % (tiles_x * tiles_y);
    const int tx_i = bid % tiles_x;
    bid /= tiles_x;
    const int ty_i = bid % tiles_y;
    const int64_t plane = bid / tiles_y;
    const int oy0 = ty_i * T_OH, ox0 = tx_i * T_OW;
    const int iy0 = oy0 - pad_y0, ix0 = ox0 - pad_x0;
    const float* src = gy + plane * (int64_t)in_h * in_w;
    const float* fws = q.fw + plane * (int64_t)in_h * in_w;
    const int64_t b = plane / q.channels;
    const float* nz = q.noise ? q.noise + b * q.noise_bstride : nullptr;
    const float nw = q.noise ? q.noise_w[0] : 0.0f;
    const float bb = q.bias ? q.bias[plane - b * q.channels] : 0.0f;
    FIR4_LOAD_TAPS(kf, k)

    FirSums sums{0.0f, 0.0f, 0.0f};
    if (ALN) {
        // window columns ox0 - 4 .. ox0 + 67; owned = rows 0..31, window columns 2..65 (image columns ox0 - 2 .. ox0 + 61)
        constexpr int NG = T_IH * A_G, ST = (NG + 255) / 256;
        float4 sg[ST], so[ST], sn[ST];
#pragma unroll
        for (int j = 0; j < ST; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int r = i / A_G, g = i - r * A_G;
            const int y = iy0 + r, x = ox0 - 4 + 4 * g;
            const bool ok = i < NG && y >= 0 && y < in_h && x >= 0 && x < in_w;
            const int64_t o = ok ? (int64_t)y * in_w + x : 0;
            sg[j] = *reinterpret_cast<const float4*>(src + o);
            so[j] = *reinterpret_cast<const float4*>(fws + o);
            sn[j] = nz ? *reinterpret_cast<const float4*>(nz + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < ST; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int r = i / A_G, g = i - r * A_G;
            const int y = iy0 + r, x = ox0 - 4 + 4 * g;
            const bool ok = i < NG && y >= 0 && y < in_h && x >= 0 && x < in_w;
            const bool own_r = ok && r < T_OH;
            const int c0 = 4 * g;
            float4 v;
            v.x = fir4_gpre(sg[j].x, so[j].x, sn[j].x, ok, own_r && c0 >= 2 && c0 < 66, q, nw, bb, sums);
            v.y = fir4_gpre(sg[j].y, so[j].y, sn[j].y, ok, own_r && c0 + 1 >= 2 && c0 + 1 < 66, q, nw, bb, sums);
            v.z = fir4_gpre(sg[j].z, so[j].z, sn[j].z, ok, own_r && c0 + 2 >= 2 && c0 + 2 < 66, q, nw, bb, sums);
            v.w = fir4_gpre(sg[j].w, so[j].w, sn[j].w, ok, own_r && c0 + 3 >= 2 && c0 + 3 < 66, q, nw, bb, sums);
            if (i < NG) reinterpret_cast<float4*>(s_in)[i] = v;
        }
    } else {
        constexpr int T_STAGE = (T_IH * T_LD + 255) / 256;
        float sg[T_STAGE], so[T_STAGE], sn[T_STAGE];
#pragma unroll
        for (int j = 0; j < T_STAGE; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int r = i / T_LD, c = i - r * T_LD;
            const int y = iy0 + r, x = ix0 + c;
            const bool ok = i < T_IH * T_LD && c < T_IW && y >= 0 && y < in_h && x >= 0 && x < in_w;
            const int64_t o = ok ? (int64_t)y * in_w + x : 0;
            sg[j] = src[o];
            so[j] = fws[o];
            sn[j] = nz ? nz[o] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < T_STAGE; ++j) {
            const int i = threadIdx.x + 256 * j;
            const int r = i / T_LD, c = i - r * T_LD;
            const int y = iy0 + r, x = ix0 + c;
            const bool ok = i < T_IH * T_LD && c < T_IW && y >= 0 && y < in_h && x >= 0 && x < in_w;
            const float v = fir4_gpre(sg[j], so[j], sn[j], ok, ok && r < T_OH && c < T_OW, q, nw, bb, sums);
            if (i < T_IH * T_LD) s_in[i] = v;
        }
    }
    sums.b = sr_wave_sum(sums.b);
    sums.n = sr_wave_sum(sums.n);
    sums.d = sr_wave_sum(sums.d);
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { s_red[wave] = sums.b; s_red[4 + wave] = sums.n; s_red[8 + wave] = sums.d; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t slot = plane * (int64_t)(tiles_x * tiles_y) + tile;
        q.partial[slot * 2] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        q.partial[slot * 2 + 1] = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
        q.dot_partial[slot] = (s_red[8] + s_red[9]) + (s_red[10] + s_red[11]);
    }

    const int lx = (threadIdx.x & 15) * 4, ly = (threadIdx.x >> 4) * 2;
    float acc[2][4];
    fir4_rows<LD, ALN ? 2 : 0>(s_in, kf, lx, ly, acc);
    float* dst = out + plane * (int64_t)out_h * out_w;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int oy = oy0 + ly + r;
        if (oy >= out_h) continue;
        const int ox = ox0 + lx;
        fir4_store_row(dst + (int64_t)oy * out_w + ox, ox, out_w, acc[r]);
    }
}

// ------------------------------------------------------------------------------ whole-row bands (up-sampling layers)
// The two kernels above on the maps of the up-sampling layers (2^k + 1 wide on one side, 2^k on the other), tiled by
// BANDS of whole rows instead of 32 x 64 tiles.  A plane of an NCHW tensor is contiguous, so a band of whole rows of the
// (2^k + 1)-wide map is ONE contiguous span of memory: it is moved with 16-byte accesses from / to the span's address
// rounded down to 16 bytes, whatever the residue of its rows, and the at most three floats in front of and behind the
// aligned part are moved one by one by the band that owns them.  No workgroup owns a one-pixel edge column or row, and
// the 2^k-wide side (noise, gy, y, the forward's output) is aligned as it stands.
//   lanes: lanes_x = 2^k / 4 per row (four columns each), 256 / lanes_x lane rows of B_RPL = 4 output rows each
//          -> rmax = 4 * (256 / lanes_x) rows per band (16 at 256, 32 at 128, 64 at 64);
//   bands: ceil(rows / rmax) per plane, the rows spread evenly over them (band_rows).
// The arithmetic is that of fir4_rows and of the tiled kernels' epilogues, tap for tap.
constexpr int B_RPL = 4;                    // output rows per lane
constexpr int B_ST = 5;                     // 16-byte groups a lane has in flight per staging trip (one trip up to 257 wide)
constexpr int B_MIN_W = 64, B_MAX_W = 1024; // 2^k-side widths the band kernels take (profiles/fir_band_notes.md)

__device__ __forceinline__ void band_rows(int rows, int bands, int i, int& r0, int& rb) {
    const int base = rows / bands, rem = rows - base * bands;
    r0 = i * base + (i < rem ? i : rem);
    rb = base + (i < rem ? 1 : 0);
}

// B_RPL x 4 accumulators from window row t (tap row ky = t - r of output row r): fir4_rows' order for every accumulator
template <int NW>
__device__ __forceinline__ void band_taps(const float (&win)[NW], const float (&kf)[16], int t, float (&acc)[B_RPL][4]) {
#pragma unroll
    for (int r = 0; r < B_RPL; ++r) {
        const int ky = t - r;
        if (ky < 0 || ky > 3) continue;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float prod = win[c + kx] * kf[ky * 4 + kx];
                acc[r][c] = acc[r][c] + prod;
            }
    }
}

// Forward, pad 1: input [planes, in_h, in_w] -> output [planes, in_h - 1, in_w - 1], in_w - 1 = 4 * lanes_x.  The band's
// input rows r0 - 1 .. r0 + rb + 1 are one span of the tensor; LDS slot 4 + i holds the element i floats behind the
// span's start rounded down to a multiple of four floats (x is 16-byte aligned), elements of other planes (= rows
// outside the image) as zeros.  The LDS pitch is the global pitch: columns -1 and in_w have no slots, the first and last lane of a row
// select them to zero.  `total`: elements of the tensor — no load before its first or past its last element.
__global__ __launch_bounds__(256, 6) void k_fir4_band_fwd(float* __restrict__ out, const float* __restrict__ x,
                                                       const float* __restrict__ k, int in_h, int in_w, int lanes_x,
                                                       int bands, int64_t total, FirNba nba) {
    extern __shared__ __attribute__((aligned(16))) float s_band[];
    const int out_h = in_h - 1, out_w = in_w - 1;
    const int band = blockIdx.x % bands;
    const int64_t plane = blockIdx.x / bands;
    int r0, rb;
    band_rows(out_h, bands, band, r0, rb);
    const int pe = in_h * in_w;                                     // < 2^30 (sr_blur_noise_bias_act)
    const int64_t p0 = plane * (int64_t)pe;
    const int res = (int)((p0 + (int64_t)(r0 - 1) * in_w) & 3);
    const int e0 = (r0 - 1) * in_w - res;                           // LDS slot 4 + i = plane element e0 + i, e0 + p0 = 0 mod 4
    const int ng = (res + (rb + 3) * in_w + 3) >> 2;
    // loads stay inside the tensor: plane elements e_lo .. e_hi + 3 are its first and its last whole 16-byte group
    const int64_t last_full = (total & ~(int64_t)3) - 4;
    const int e_lo = (int)(-p0 > -(int64_t)(1 << 30) ? -p0 : -(int64_t)(1 << 30));
    const int e_hi = (int)(last_full - p0 < (int64_t)(1 << 30) ? last_full - p0 : (int64_t)(1 << 30));
    const float* xp = x + p0;
    FIR4_LOAD_TAPS(kf, k)

    // the lane's outputs: rows r0 + ly .. + 3, columns ox .. ox + 3; their noise travels with the staging loads
    const int gyi = threadIdx.x / lanes_x, gx = threadIdx.x - gyi * lanes_x;
    const int ly = gyi * B_RPL, ox = gx * 4;
    const int64_t b = plane / nba.channels;
    const float* nz = nba.noise ? nba.noise + b * nba.noise_bstride : nullptr;
    const float nw = nz ? nba.noise_w[0] : 0.0f;
    const float bb = nba.bias ? nba.bias[plane - b * nba.channels] : 0.0f;
    float4 nzv[B_RPL];
    if (nz) {
#pragma unroll
        for (int r = 0; r < B_RPL; ++r) {
            const int oy = min(r0 + ly + r, out_h - 1);
            nzv[r] = *reinterpret_cast<const float4*>(nz + (int64_t)oy * out_w + ox);
        }
    }

    for (int base = 0; base < ng; base += 256 * B_ST) {
        float4 st[B_ST];
#pragma unroll
        for (int j = 0; j < B_ST; ++j) {
            const int e = e0 + 4 * (base + (int)threadIdx.x + 256 * j);
            st[j] = *reinterpret_cast<const float4*>(xp + (e < e_lo ? e_lo : (e > e_hi ? e_hi : e)));
        }
#pragma unroll
        for (int j = 0; j < B_ST; ++j) {
            const int i = base + (int)threadIdx.x + 256 * j;
            if (i >= ng) continue;
            const int e = e0 + 4 * i;
            float4 v = st[j];
            if (e > e_hi) {                                         // the tensor's last, partial group: element by element
                const int64_t t = p0 + e;
                v.x = t < total ? x[t] : 0.0f;
                v.y = t + 1 < total ? x[t + 1] : 0.0f;
                v.z = t + 2 < total ? x[t + 2] : 0.0f;
                v.w = 0.0f;
            }
            // outside the plane = a padding row (or another plane's data, or the clamped load's)
            v.x = (unsigned)e < (unsigned)pe ? v.x : 0.0f;
            v.y = (unsigned)(e + 1) < (unsigned)pe ? v.y : 0.0f;
            v.z = (unsigned)(e + 2) < (unsigned)pe ? v.z : 0.0f;
            v.w = (unsigned)(e + 3) < (unsigned)pe ? v.w : 0.0f;
            *reinterpret_cast<float4*>(s_band + 4 + 4 * i) = v;
        }
    }
    __syncthreads();
    if (ly >= rb) return;

    float acc[B_RPL][4];
#pragma unroll
    for (int r = 0; r < B_RPL; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
    const float* w0 = s_band + 4 + res + ly * in_w + ox - 1;         // window row 0, image column ox - 1
#pragma unroll
    for (int t = 0; t < B_RPL + 3; ++t) {
        float win[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) win[c] = w0[t * in_w + c];
        if (gx == 0) win[0] = 0.0f;                                  // column -1
        if (gx == lanes_x - 1) win[6] = 0.0f;                        // column in_w
        band_taps(win, kf, t, acc);
    }

    float* dst = out + plane * (int64_t)out_h * out_w;
#pragma unroll
    for (int r = 0; r < B_RPL; ++r) {
        if (ly + r >= rb) continue;
        float nr[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (nz) { nr[0] = nzv[r].x; nr[1] = nzv[r].y; nr[2] = nzv[r].z; nr[3] = nzv[r].w; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v = acc[r][c];
            if (nz) v = v + nw * nr[c];
            v += bb;
            acc[r][c] = ((v > 0.0f) ? v : v * nba.alpha) * nba.gain;
        }
        *reinterpret_cast<float4*>(dst + (int64_t)(r0 + ly + r) * out_w + ox) =
            make_float4(acc[r][0], acc[r][1], acc[r][2], acc[r][3]);
    }
}

// Backward (k_fir4_nba_bwd), gradient pad 2: gy, y [planes, in_h, in_w] (in_w = 4 * lanes_x, aligned rows) -> gradient
// [planes, in_h + 1, in_w + 1].  A band owns rb rows of the gradient; it stages gpre rows r0 - 2 .. r0 + rb at pitch
// in_w + 8 (four zero columns on either side: aligned 16-byte LDS stores, the window at an 8-byte aligned column - 2) and
// owns — for the three sums — the gpre rows r0 .. r0 + rb - 1 that exist: every row belongs to exactly one band.  The
// rb output rows then go through LDS at the global pitch and leave as one flat span (see above): no 16-byte store
// straddles two bands.  One partial triple per band, in the layout of k_fir4_nba_bwd with chunks = bands.
__global__ __launch_bounds__(256) void k_fir4_band_nba_bwd(float* __restrict__ out, const float* __restrict__ gy,
                                                           const float* __restrict__ k, int in_h, int in_w, int lanes_x,
                                                           int bands, FirNbaBwd q) {
    extern __shared__ __attribute__((aligned(16))) float s_band[];
    __shared__ float s_red[12];
    const int out_h = in_h + 1, out_w = in_w + 1, ld = in_w + 8;
    const int band = blockIdx.x % bands;
    const int64_t plane = blockIdx.x / bands;
    int r0, rb;
    band_rows(out_h, bands, band, r0, rb);
    const float* src = gy + plane * (int64_t)in_h * in_w;
    const float* fws = q.fw + plane * (int64_t)in_h * in_w;
    const int64_t b = plane / q.channels;
    const float* nz = q.noise ? q.noise + b * q.noise_bstride : nullptr;
    const float nw = q.noise ? q.noise_w[0] : 0.0f;
    const float bb = q.bias ? q.bias[plane - b * q.channels] : 0.0f;
    FIR4_LOAD_TAPS(kf, k)

    for (int i = threadIdx.x; i < 2 * (rb + 3); i += 256)            // the zero columns left and right of every row
        *reinterpret_cast<float4*>(s_band + (i >> 1) * ld + ((i & 1) ? 4 + in_w : 0)) = make_float4(0.f, 0.f, 0.f, 0.f);
    const int ng = (rb + 3) * lanes_x;
    FirSums sums{0.0f, 0.0f, 0.0f};
    for (int base = 0; base < ng; base += 256 * B_ST) {
        float4 sg[B_ST], so[B_ST], sn[B_ST];
#pragma unroll
        for (int j = 0; j < B_ST; ++j) {
            const int i = base + (int)threadIdx.x + 256 * j;
            const int wr = i / lanes_x, g = i - wr * lanes_x;
            const int y = r0 - 2 + wr;
            const bool ok = i < ng && y >= 0 && y < in_h;
            const int64_t o = ok ? (int64_t)y * in_w + 4 * g : 0;
            sg[j] = *reinterpret_cast<const float4*>(src + o);
            so[j] = *reinterpret_cast<const float4*>(fws + o);
            sn[j] = nz ? *reinterpret_cast<const float4*>(nz + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < B_ST; ++j) {
            const int i = base + (int)threadIdx.x + 256 * j;
            const int wr = i / lanes_x, g = i - wr * lanes_x;
            const int y = r0 - 2 + wr;
            const bool ok = i < ng && y >= 0 && y < in_h;
            const bool own = ok && y >= r0 && y < r0 + rb;
            float4 v;
            v.x = fir4_gpre(sg[j].x, so[j].x, sn[j].x, ok, own, q, nw, bb, sums);
            v.y = fir4_gpre(sg[j].y, so[j].y, sn[j].y, ok, own, q, nw, bb, sums);
            v.z = fir4_gpre(sg[j].z, so[j].z, sn[j].z, ok, own, q, nw, bb, sums);
            v.w = fir4_gpre(sg[j].w, so[j].w, sn[j].w, ok, own, q, nw, bb, sums);
            if (i < ng) *reinterpret_cast<float4*>(s_band + wr * ld + 4 + 4 * g) = v;
        }
    }
    sums.b = sr_wave_sum(sums.b);
    sums.n = sr_wave_sum(sums.n);
    sums.d = sr_wave_sum(sums.d);
    {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) { s_red[wave] = sums.b; s_red[4 + wave] = sums.n; s_red[8 + wave] = sums.d; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t slot = plane * (int64_t)bands + band;
        q.partial[slot * 2] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
        q.partial[slot * 2 + 1] = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
        q.dot_partial[slot] = (s_red[8] + s_red[9]) + (s_red[10] + s_red[11]);
    }

    const int gyi = threadIdx.x / lanes_x, gx = threadIdx.x - gyi * lanes_x;
    const int ly = gyi * B_RPL, ox = gx * 4;
    const bool active = ly < rb;
    float acc[B_RPL][4];
#pragma unroll
    for (int r = 0; r < B_RPL; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
    if (active) {
        const float* w0 = s_band + ly * ld + 4 + ox - 2;             // window row 0, gpre column ox - 2: 8-byte aligned
#pragma unroll
        for (int t = 0; t < B_RPL + 3; ++t) {
            float win[8];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float2 a = *reinterpret_cast<const float2*>(w0 + t * ld + 2 * h);
                win[2 * h] = a.x;
                win[2 * h + 1] = a.y;
            }
            band_taps(win, kf, t, acc);
        }
    }
    // the last column (in_w = 4 * lanes_x) has no lane of the 4-column layout: one output per row, by the last rb lanes
    const int er = (int)threadIdx.x - (256 - rb);
    float edge = 0.0f;
    if (er >= 0) {
#pragma unroll
        for (int ky = 0; ky < 4; ++ky)
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const float prod = s_band[(er + ky) * ld + 4 + in_w - 2 + kx] * kf[ky * 4 + kx];
                edge = edge + prod;
            }
    }
    __syncthreads();                                                 // every window is read: the LDS takes the output rows
    const int64_t a0 = (plane * out_h + r0) * (int64_t)out_w;        // the band's first element in the tensor
    const int res = (int)(a0 & 3);
    if (active) {
#pragma unroll
        for (int r = 0; r < B_RPL; ++r) {
            if (ly + r >= rb) continue;
#pragma unroll
            for (int c = 0; c < 4; ++c) s_band[res + (ly + r) * out_w + ox + c] = acc[r][c];
        }
    }
    if (er >= 0) s_band[res + er * out_w + in_w] = edge;
    __syncthreads();
    const int end = res + rb * out_w;                                // LDS slots res .. end - 1 = tensor a0 .. of this band
    float* dst = out + (a0 - res);                                   // 16-byte aligned
    for (int j = 4 * (int)threadIdx.x; j < end; j += 4 * 256) {
        const float4 v = *reinterpret_cast<const float4*>(s_band + j);
        if (j >= res && j + 3 < end) {
            *reinterpret_cast<float4*>(dst + j) = v;
        } else {                                                     // the span's head and tail: this band's floats only
            if (j >= res && j < end) dst[j] = v.x;
            if (j + 1 >= res && j + 1 < end) dst[j + 1] = v.y;
            if (j + 2 >= res && j + 2 < end) dst[j + 2] = v.z;
            if (j + 3 >= res && j + 3 < end) dst[j + 3] = v.w;
        }
    }
}

// ------------------------------------------------------------------------------ 4x4 taps, up = 2 or down = 2
// The two resampling shapes of the networks: down = 2 (the blur in front of ResBlock.skip's 1x1 stride-2
// convolution evaluated only at the pixels that convolution reads, and the gradient of the ToRGB skip
// up-sampling) and up = 2 (the ToRGB skip up-sampling and the gradient of the former).  Same scheme as
// k_fir4_tile: the input window of a 32 x 32 output tile is staged once in LDS with coalesced row loads, each
// lane produces four consecutive outputs of one row.  Taps are visited ky-major then kx, multiply and add
// separate (-ffp-contract=off), inserted zeros are skipped (not multiplied): the order of k_upfirdn_generic and
// of the numpy oracle, so all three agree bit for bit.
constexpr int R_OH = 32, R_OW = 32;

template <int UP, int DOWN>
__global__ __launch_bounds__(256) void k_fir4_resample(float* __restrict__ out, const float* __restrict__ x,
                                                       const float* __restrict__ k, int in_h, int in_w,
                                                       int out_h, int out_w, int pad_x0, int pad_y0,
                                                       int tiles_x, int tiles_y,
                                                       const float* __restrict__ addend) {
    static_assert((UP == 1 && DOWN == 2) || (UP == 2 && DOWN == 1), "one of the two resampling shapes");
    // input rows / columns a tile can touch: (R - 1) * DOWN + 4 taps, every UP-th of them holds data
    constexpr int SPAN_H = ((R_OH - 1) * DOWN + 4 + UP - 1) / UP + 1;
    constexpr int SPAN_W = ((R_OW - 1) * DOWN + 4 + UP - 1) / UP + 1;
    constexpr int LDW = SPAN_W | 1;                                   // odd pitch: rows on different banks
    __shared__ float s_in[SPAN_H * LDW];
    __shared__ float s_k[16];
    int bid = blockIdx.x;
    const int tx_i = bid % tiles_x;
    bid /= tiles_x;
    const int ty_i = bid % tiles_y;
    const int64_t plane = bid / tiles_y;
    const int oy0 = ty_i * R_OH, ox0 = tx_i * R_OW;
    // first upsampled coordinate of the tile, and the first input row / column at or after it
    const int my0 = oy0 * DOWN - pad_y0, mx0 = ox0 * DOWN - pad_x0;
    const int iy_lo = floor_div(my0 + UP - 1, UP), ix_lo = floor_div(mx0 + UP - 1, UP);
    const float* src = x + plane * (int64_t)in_h * in_w;
    if (threadIdx.x < 16) {
        const int ky = threadIdx.x >> 2, kx = threadIdx.x & 3;
        s_k[threadIdx.x] = k[(3 - ky) * 4 + (3 - kx)];
    }
    for (int i = threadIdx.x; i < SPAN_H * SPAN_W; i += 256) {
        const int r = i / SPAN_W, c = i - r * SPAN_W;
        const int gy = iy_lo + r, gx = ix_lo + c;
        const bool ok = gy >= 0 && gy < in_h && gx >= 0 && gx < in_w;
        s_in[r * LDW + c] = ok ? src[(int64_t)gy * in_w + gx] : 0.0f;
    }
    __syncthreads();
    float kf[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) kf[i] = s_k[i];
    const int ly = threadIdx.x >> 3, lx = (threadIdx.x & 7) * 4;
    const int oy = oy0 + ly;
    if (oy >= out_h) return;
    const int my = oy * DOWN - pad_y0;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (UP == 2) {
        // Same taps in the same order as the loop below, without its 64 parity tests: of the four tap rows the two with
        // (my + ky) even hold data (ky = ky0, ky0 + 2), and since ox0 + lx is a multiple of four the column parity is the
        // same for every lane — output c reads the taps kx = ((c + PX) & 1), + 2 at compile-time offsets from one base
        // column.  Rows / columns outside the map are zeros in the staged window: adding their 0 * tap leaves the sum as
        // skipping them does.
        const int ky0 = my & 1;
        const int mx = ox0 + lx - pad_x0;
        const int px = mx & 1;
        const int cbase = ((mx - px) >> 1) - ix_lo;
        auto rows = [&](auto pxc) {
            constexpr int PX = decltype(pxc)::value;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int ky = ky0 + 2 * j;
                const float* row = s_in + (((my + ky) >> 1) - iy_lo) * LDW + cbase;
                const float* kr = s_k + ky * 4;
                const float k0 = kr[0], k1 = kr[1], k2 = kr[2], k3 = kr[3];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int kx = ((c + PX) & 1) + 2 * i;
                        const float kv = kx == 0 ? k0 : (kx == 1 ? k1 : (kx == 2 ? k2 : k3));
                        const float prod = row[(PX + c + kx) >> 1] * kv;
                        acc[c] = acc[c] + prod;
                    }
            }
        };
        if (px) rows(std::integral_constant<int, 1>{});
        else rows(std::integral_constant<int, 0>{});
    } else
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
        const int m = my + ky;
        if (UP == 2 && (m & 1)) continue;                               // an inserted zero row
        const int iy = (UP == 2 ? (m >> 1) : m);                        // arithmetic shift: exact for even m
        if (iy < 0 || iy >= in_h) continue;
        const float* row = s_in + (iy - iy_lo) * LDW;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int mxc = (ox0 + lx + c) * DOWN - pad_x0 + kx;
                if (UP == 2 && (mxc & 1)) continue;
                const int ix = (UP == 2 ? (mxc >> 1) : mxc);
                if (ix < 0 || ix >= in_w) continue;
                const float prod = row[ix - ix_lo] * kf[ky * 4 + kx];
                acc[c] = acc[c] + prod;
            }
    }
    const int64_t o = plane * (int64_t)out_h * out_w + (int64_t)oy * out_w + ox0 + lx;
    float* q = out + o;
    // optional second operand of a following addition (ToRGB: rgb + upsample(skip), reference model.py:66-68)
    // rows of 4-float groups on 16-byte addresses (every map of the networks): one 16-byte access per lane instead of
    // four 4-byte ones at a 16-byte stride — the 256^2 gradient of the discriminator's skip branch is 400 MB of traffic
    const bool vec = (out_w & 3) == 0 && ox0 + lx + 3 < out_w && ((reinterpret_cast<uintptr_t>(out) & 15) == 0) &&
                     (!addend || (reinterpret_cast<uintptr_t>(addend) & 15) == 0);
    if (vec) {
        float4 r = make_float4(acc[0], acc[1], acc[2], acc[3]);
        if (addend) {
            const float4 a = *reinterpret_cast<const float4*>(addend + o);
            r.x = r.x + a.x; r.y = r.y + a.y; r.z = r.z + a.z; r.w = r.w + a.w;
        }
        *reinterpret_cast<float4*>(q) = r;
        return;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (ox0 + lx + c < out_w) q[c] = addend ? acc[c] + addend[o + c] : acc[c];
}

// aligned staging of k_fir4_tile / k_fir4_nba_bwd (see A_LD); SR_FIR_ALIGNED=0 keeps the scalar staging (A/B)
inline bool fir4_aligned_enabled() {
    static const bool enabled = [] {
        const char* e = std::getenv("SR_FIR_ALIGNED");
        return !(e && e[0] == '0');
    }();
    return enabled;
}

inline bool fir4_aligned(const float* x, int in_w, int pad_x0) {
    return fir4_aligned_enabled() && pad_x0 == 2 && in_w % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// whole-row bands (k_fir4_band_*) for a map whose 2^k side is w4 wide and whose kernel writes `rows` rows per plane;
// bands == 0: the shape is not theirs
struct FirBand {
    int lanes_x, rmax, bands;
};

inline FirBand fir4_band_geom(int w4, int rows) {
    FirBand g{0, 0, 0};
    if (w4 % 4 != 0 || w4 < B_MIN_W || w4 > B_MAX_W || rows <= 0) return g;
    g.lanes_x = w4 / 4;
    g.rmax = B_RPL * (256 / g.lanes_x);
    g.bands = (rows + g.rmax - 1) / g.rmax;
    return g;
}

// SR_FIR_BAND=0 keeps the tiled kernels everywhere (A/B); SR_FIR_ALIGNED=0 does so too (it asks for the scalar staging)
inline bool fir4_band_enabled() {
    static const bool enabled = [] {
        const char* e = std::getenv("SR_FIR_BAND");
        return !(e && e[0] == '0');
    }();
    return enabled && fir4_aligned_enabled();
}

}  // namespace

extern "C" int sr_upfirdn2d(float* out, const float* x, const float* k, int64_t major, int in_h,
                            int in_w, int out_h, int out_w, int kh, int kw, int up_x, int up_y,
                            int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                            sr_stream_t stream) {
    if (major < 0 || in_h < 0 || in_w < 0 || kh <= 0 || kw <= 0 || up_x <= 0 || up_y <= 0 ||
        down_x <= 0 || down_y <= 0)
        return SR_EINVAL;
    // floor division like Python's // (reference op/upfirdn2d.py:103-104)
    auto fdiv = [](int a, int b) { int q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; };
    const int eh = fdiv(in_h * up_y + pad_y0 + pad_y1 - kh, down_y) + 1;
    const int ew = fdiv(in_w * up_x + pad_x0 + pad_x1 - kw, down_x) + 1;
    if (eh != out_h || ew != out_w) return SR_EINVAL;
    if (major == 0 || out_h <= 0 || out_w <= 0) return SR_OK;
    if (!out || !x || !k) return SR_EINVAL;
    hipStream_t st = sr_stream(stream);
    if (up_x == 1 && up_y == 1 && down_x == 1 && down_y == 1 && kh == 4 && kw == 4) {
        const int tiles_x = (out_w + T_OW - 1) / T_OW, tiles_y = (out_h + T_OH - 1) / T_OH;
        const int64_t blocks = (int64_t)tiles_x * tiles_y * major;
        if (blocks < 0x7FFFFFFFLL) {
            if (fir4_aligned(x, in_w, pad_x0))
                hipLaunchKernelGGL((k_fir4_tile<false, true>), dim3((unsigned)blocks), dim3(256), 0, st, out, x, k, in_h,
                                   in_w, out_h, out_w, pad_x0, pad_y0, tiles_x, tiles_y, FirNba{});
            else
                hipLaunchKernelGGL((k_fir4_tile<false, false>), dim3((unsigned)blocks), dim3(256), 0, st, out, x, k, in_h,
                                   in_w, out_h, out_w, pad_x0, pad_y0, tiles_x, tiles_y, FirNba{});
            return sr_launch_status();
        }
    }
    if (kh == 4 && kw == 4 && up_x == up_y && down_x == down_y &&
        ((up_x == 1 && down_x == 2) || (up_x == 2 && down_x == 1))) {
        const int tiles_x = (out_w + R_OW - 1) / R_OW, tiles_y = (out_h + R_OH - 1) / R_OH;
        const int64_t blocks = (int64_t)tiles_x * tiles_y * major;
        if (blocks < 0x7FFFFFFFLL) {
            if (down_x == 2)
                hipLaunchKernelGGL((k_fir4_resample<1, 2>), dim3((unsigned)blocks), dim3(256), 0, st, out, x, k, in_h,
                                   in_w, out_h, out_w, pad_x0, pad_y0, tiles_x, tiles_y, (const float*)nullptr);
            else
                hipLaunchKernelGGL((k_fir4_resample<2, 1>), dim3((unsigned)blocks), dim3(256), 0, st, out, x, k, in_h,
                                   in_w, out_h, out_w, pad_x0, pad_y0, tiles_x, tiles_y, (const float*)nullptr);
            return sr_launch_status();
        }
    }
    UfdParams p{in_h, in_w, out_h, out_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0};
    const int64_t total = major * (int64_t)out_h * out_w;
    hipLaunchKernelGGL(k_upfirdn_generic, dim3(sr_stream_grid(total, 256)), dim3(256),
                       (size_t)kh * kw * sizeof(float), st, out, x, k, p, total);
    return sr_launch_status();
}

extern "C" int sr_upsample2_add(float* out, const float* x, const float* k, const float* addend, int64_t major,
                                int in_h, int in_w, int out_h, int out_w, int pad0, int pad1, sr_stream_t stream) {
    if (major < 0 || in_h < 0 || in_w < 0) return SR_EINVAL;
    if (in_h * 2 + pad0 + pad1 - 4 + 1 != out_h || in_w * 2 + pad0 + pad1 - 4 + 1 != out_w) return SR_EINVAL;
    if (major == 0 || out_h <= 0 || out_w <= 0) return SR_OK;
    if (!out || !x || !k || !addend) return SR_EINVAL;
    const int tiles_x = (out_w + R_OW - 1) / R_OW, tiles_y = (out_h + R_OH - 1) / R_OH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * major;
    if (blocks >= 0x7FFFFFFFLL) return SR_ERANGE;
    hipLaunchKernelGGL((k_fir4_resample<2, 1>), dim3((unsigned)blocks), dim3(256), 0, sr_stream(stream), out, x, k, in_h,
                       in_w, out_h, out_w, pad0, pad0, tiles_x, tiles_y, addend);
    return sr_launch_status();
}

extern "C" int sr_blur_noise_bias_act(float* y, const float* x, const float* k, const float* noise,
                                      const float* noise_w, const float* bias, float alpha, float gain, int64_t n,
                                      int64_t c, int in_h, int in_w, int out_h, int out_w, int pad0, int pad1,
                                      int64_t noise_bstride, sr_stream_t stream) {
    if (n < 0 || c < 0 || in_h < 0 || in_w < 0) return SR_EINVAL;
    if (in_h + pad0 + pad1 - 4 + 1 != out_h || in_w + pad0 + pad1 - 4 + 1 != out_w) return SR_EINVAL;
    if (n * c == 0 || out_h <= 0 || out_w <= 0) return SR_OK;
    if (!y || !x || !k || (noise && !noise_w)) return SR_EINVAL;
    const int tiles_x = (out_w + T_OW - 1) / T_OW, tiles_y = (out_h + T_OH - 1) / T_OH;
    const int64_t blocks = (int64_t)tiles_x * tiles_y * n * c;
    if (blocks >= 0x7FFFFFFFLL) return SR_ERANGE;
    const FirNba nba{noise, noise_w, bias, noise_bstride, (int)c, alpha, gain};
    if (fir4_band_enabled() && pad0 == 1 && pad1 == 1 && al16(x) && al16(y) &&
        (!noise || (al16(noise) && noise_bstride % 4 == 0))) {
        const FirBand g = fir4_band_geom(out_w, out_h);
        if (g.bands > 0 && (int64_t)g.bands * n * c < 0x7FFFFFFFLL && (int64_t)in_h * in_w < (1 << 30)) {
            const size_t lds = ((size_t)(g.rmax + 3) * in_w + 16) * sizeof(float);
            hipLaunchKernelGGL(k_fir4_band_fwd, dim3((unsigned)(g.bands * n * c)), dim3(256), lds, sr_stream(stream), y, x,
                               k, in_h, in_w, g.lanes_x, g.bands, n * c * (int64_t)in_h * in_w, nba);
            return sr_launch_status();
        }
    }
    if (fir4_aligned(x, in_w, pad0))
        hipLaunchKernelGGL((k_fir4_tile<true, true>), dim3((unsigned)blocks), dim3(256), 0, sr_stream(stream), y, x, k,
                           in_h, in_w, out_h, out_w, pad0, pad0, tiles_x, tiles_y, nba);
    else
        hipLaunchKernelGGL((k_fir4_tile<true, false>), dim3((unsigned)blocks), dim3(256), 0, sr_stream(stream), y, x, k,
                           in_h, in_w, out_h, out_w, pad0, pad0, tiles_x, tiles_y, nba);
    return sr_launch_status();
}

// finish kernels of csrc/fused_elem.hip (bias / noise-strength / row-dot partials -> results, fixed order)
int sr_nba_finish_launch(float* gbias, float* gnoise_w, float* rowdot, const float* partial, const float* dot_partial,
                         float* chan_nw, int64_t n, int64_t c, int chunks, bool has_noise, hipStream_t st);

extern "C" int64_t sr_blur_nba_bwd_scratch_floats(int64_t n, int64_t c, int out_h, int out_w) {
    if (n <= 0 || c <= 0 || out_h <= 0 || out_w <= 0) return 3;
    const int64_t tiles = (int64_t)((out_w + T_OW - 1) / T_OW) * ((out_h + T_OH - 1) / T_OH);
    const int64_t bands = fir4_band_geom(out_w - 1, out_h).bands;      // one partial triple per tile or per band
    return 3 * n * c * (tiles > bands ? tiles : bands) + c + 2;
}

// gx [n, c, out_h, out_w] = blur^T( lrelu'(y) * gy * gain ) with `k` the FORWARD blur kernel and pad0 / pad1 the
// forward's padding (the gradient pads by 3 - pad0 in front), plus gbias [c], gnoise_w [1] (both optional: NULL = the
// parameters are frozen) and rowdot [n * c] (see FirNbaBwd).  gy, y: [n, c, in_h, in_w], the forward's OUTPUT extent.
extern "C" int sr_blur_nba_bwd(float* gx, float* gbias, float* gnoise_w, float* rowdot, const float* gy, const float* y,
                               const float* k_flipped, const float* noise, const float* noise_w, const float* bias,
                               float alpha, float gain, int64_t n, int64_t c, int in_h, int in_w, int out_h, int out_w,
                               int pad0, int64_t noise_bstride, float* scratch, sr_stream_t stream) {
    if (n < 0 || c < 0 || in_h < 0 || in_w < 0) return SR_EINVAL;
    // forward: in = out + 2 * pad - 3 with pad0 == pad1 (the up-sampling layers: 257 -> 256, pad 1)
    if (out_h + 2 * pad0 - 3 != in_h || out_w + 2 * pad0 - 3 != in_w || pad0 < 0 || pad0 > 3) return SR_EINVAL;
    if (n * c == 0 || in_h == 0 || in_w == 0) return SR_OK;
    if (!gx || !rowdot || !gy || !y || !k_flipped || !scratch || (noise && !noise_w) || gain == 0.0f || alpha == 0.0f)
        return SR_EINVAL;
    const int tiles_x = (out_w + T_OW - 1) / T_OW, tiles_y = (out_h + T_OH - 1) / T_OH;
    const int gpad = 3 - pad0;
    const bool vec = al16(gy) && al16(y) && (!noise || (al16(noise) && noise_bstride % 4 == 0));
    // whole-row bands on the up-sampling layers' maps, else 32 x 64 tiles
    FirBand band{0, 0, 0};
    if (fir4_band_enabled() && pad0 == 1 && vec && al16(gx)) band = fir4_band_geom(in_w, out_h);
    const int chunks = band.bands > 0 ? band.bands : tiles_x * tiles_y;
    const int64_t blocks = (int64_t)chunks * n * c;
    if (blocks >= 0x7FFFFFFFLL) return SR_ERANGE;
    // every gpre element must lie in some tile's owned corner: the tiles start at -gpad and cover chunks * 32 / 64
    if (tiles_y * T_OH - gpad < in_h || tiles_x * T_OW - gpad < in_w) return SR_EINVAL;
    hipStream_t st = sr_stream(stream);
    float* dot_partial = scratch + 2 * n * c * (int64_t)chunks;
    float* chan_nw = dot_partial + n * c * (int64_t)chunks;
    const FirNbaBwd q{y, noise, noise_w, bias, scratch, chunks == 1 ? rowdot : dot_partial, noise_bstride, (int)c, alpha,
                      gain, 1.0f / gain, 1.0f / (alpha * gain)};
    const bool aln = fir4_aligned(gy, in_w, gpad) && vec;
    if (band.bands > 0)
        hipLaunchKernelGGL(k_fir4_band_nba_bwd, dim3((unsigned)blocks), dim3(256),
                           (size_t)(band.rmax + 3) * (in_w + 8) * sizeof(float), st, gx, gy, k_flipped, in_h, in_w,
                           band.lanes_x, band.bands, q);
    else if (aln)
        hipLaunchKernelGGL(k_fir4_nba_bwd<true>, dim3((unsigned)blocks), dim3(256), 0, st, gx, gy, k_flipped, in_h, in_w,
                           out_h, out_w, gpad, gpad, tiles_x, tiles_y, q);
    else
        hipLaunchKernelGGL(k_fir4_nba_bwd<false>, dim3((unsigned)blocks), dim3(256), 0, st, gx, gy, k_flipped, in_h, in_w,
                           out_h, out_w, gpad, gpad, tiles_x, tiles_y, q);
    const int rc = sr_launch_status();
    if (rc != SR_OK) return rc;
    return sr_nba_finish_launch(gbias, gnoise_w, chunks == 1 ? nullptr : rowdot, scratch, dot_partial, chan_nw, n, c,
                                chunks, noise != nullptr, st);
}
