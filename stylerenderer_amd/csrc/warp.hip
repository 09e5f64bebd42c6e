// Pillow-exact bilinear affine warp of uint8 images (sr_warp_affine_u8, include/stylerenderer_amd.h).
//
// Pillow's Image.transform(size, AFFINE, a, BILINEAR) is plain float64 arithmetic per output pixel: the sample point
// a * (x + .5, y + .5), minus half a pixel, floor and fraction, four taps, three lerps v = a + (b - a) * d, truncation to
// a byte.  This file is compiled with -ffp-contract=off, so every product and sum below is rounded on its own, in the
// order written, exactly as the host definition (op/warp.py) and Pillow's C evaluate them.  fp32 does not reproduce it.
//
//   k_warp_affine  one workgroup = a 64 x 16 tile of output pixels (a rotated footprint of the tile stays compact in
//                  the source); a lane owns 4 consecutive pixels of one row, lanes run along x, so a wave covers
//                  64 pixels x 4 rows.  Taps are byte gathers.  With PACK the lane's 4 * C bytes leave as C dwords
//                  (uint8 HWC) or as one float4 per channel (float32 CHW); without it (rows or base not aligned) as
//                  single bytes / floats.  The matrix is wave-uniform: scalar loads.
//
// No tap can leave the image: each of the three border rules ends in an index inside [0, W) x [0, H).
#include "common.h"

namespace {

constexpr int TX = 16, TY = 16, PX = 4;       // lanes along x, rows, pixels per lane
constexpr double LIM = 1073741824.0;          // 2^30: floor(xf) is clamped to +-LIM before it becomes an int

struct WArgs {
    const uint8_t* in;      // [N, H, W, C]
    void* out;              // FORM 0: uint8 [N, oh, ow, C]; FORM 1: float32 [N, C, oh, ow]
    const double* m;        // [N, 6] (m_stride 6) or [6] (m_stride 0)
    int m_stride;
    int H, W, oh, ow;
    int fill;
};

// border 0: replicate, 1: reflect (period 2 * size), 2: constant (clamps; the fill is decided by the sample point)
template <int BORDER>
__device__ __forceinline__ int border_index(int i, int size) {
    if ((unsigned)i < (unsigned)size) return i;
    if (BORDER == 1) {
        const int period = 2 * size;
        int m = i % period;
        if (m < 0) m += period;
        return m < size ? m : period - 1 - m;
    }
    return i < 0 ? 0 : size - 1;
}

// floor and fraction of one coordinate; the integer part is clamped so that it (and + 1) fits an int.  fmax / fmin
// drop a NaN, so a matrix that is not a number still yields an index inside the image.
__device__ __forceinline__ int split(double f, double* frac) {
    const double fl = floor(f);
    *frac = f - fl;
    return (int)fmin(fmax(fl, -LIM), LIM);
}

// (uint8) v.  The empty asm keeps the converted value apart from the byte packing that follows (see clip8 in
// resample.hip: the compiler's fused convert-and-pack forms have been wrong on this target).
__device__ __forceinline__ uint32_t byte_of(double v) {
    int b = (int)v & 255;
    asm("" : "+v"(b));
    return (uint32_t)b;
}

// dataset.to_unit_tensor: (v / 255 - 0.5) / 0.5 in float32, each operation correctly rounded
__device__ __forceinline__ float unit(uint32_t v) { return ((float)v / 255.0f - 0.5f) / 0.5f; }

template <int C, int BORDER, int FORM, bool PACK>
__global__ __launch_bounds__(TX* TY) void k_warp_affine(WArgs a) {
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x / TX;
    const int x4 = (blockIdx.x * TX + tx) * PX, y = blockIdx.y * TY + ty, n = blockIdx.z;
    if (x4 >= a.ow || y >= a.oh) return;
    const double* m = a.m + (int64_t)n * a.m_stride;
    const double a0 = m[0], a1 = m[1], a2 = m[2], a3 = m[3], a4 = m[4], a5 = m[5];
    const uint8_t* img = a.in + (int64_t)n * a.H * a.W * C;
    const double ys = (double)y + 0.5;
    const int valid = min(PX, a.ow - x4);
    uint32_t px[PX][C];
#pragma unroll
    for (int q = 0; q < PX; ++q) {
        const double xs = (double)(x4 + q) + 0.5;
        const double xin = a0 * xs + a1 * ys + a2;
        const double yin = a3 * xs + a4 * ys + a5;
        double dx, dy;
        const int x0 = split(xin - 0.5, &dx), y0 = split(yin - 0.5, &dy);
        const bool inside = xin >= 0.0 && xin < (double)a.W && yin >= 0.0 && yin < (double)a.H;
        if (q >= valid || (BORDER == 2 && !inside)) {
#pragma unroll
            for (int c = 0; c < C; ++c) px[q][c] = (uint32_t)a.fill;
            continue;
        }
        const int64_t cx0 = (int64_t)border_index<BORDER>(x0, a.W) * C, cx1 = (int64_t)border_index<BORDER>(x0 + 1, a.W) * C;
        const uint8_t* r0 = img + (int64_t)border_index<BORDER>(y0, a.H) * a.W * C;
        const uint8_t* r1 = img + (int64_t)border_index<BORDER>(y0 + 1, a.H) * a.W * C;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double p00 = (double)r0[cx0 + c], p01 = (double)r0[cx1 + c];
            const double p10 = (double)r1[cx0 + c], p11 = (double)r1[cx1 + c];
            const double v1 = p00 + (p01 - p00) * dx;
            const double v2 = p10 + (p11 - p10) * dx;
            px[q][c] = byte_of(v1 + (v2 - v1) * dy);
        }
    }
    if (FORM == 0) {
        uint8_t* dst = static_cast<uint8_t*>(a.out) + (((int64_t)n * a.oh + y) * a.ow + x4) * C;
        if (PACK && valid == PX) {
            uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
            for (int w = 0; w < C; ++w) {           // dword w holds bytes 4w .. 4w + 3 of the lane's PX * C
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v |= px[(4 * w + k) / C][(4 * w + k) % C] << (8 * k);
                d4[w] = v;
            }
        } else {
#pragma unroll
            for (int q = 0; q < PX; ++q)
                if (q < valid) {
#pragma unroll
                    for (int c = 0; c < C; ++c) dst[q * C + c] = (uint8_t)px[q][c];
                }
        }
    } else {
        float* out = static_cast<float*>(a.out);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float* dst = out + (((int64_t)n * C + c) * a.oh + y) * a.ow + x4;
            if (PACK && valid == PX) {
                *reinterpret_cast<float4*>(dst) = make_float4(unit(px[0][c]), unit(px[1][c]), unit(px[2][c]), unit(px[3][c]));
            } else {
#pragma unroll
                for (int q = 0; q < PX; ++q)
                    if (q < valid) dst[q] = unit(px[q][c]);
            }
        }
    }
}

template <int C, int BORDER, int FORM>
void launch3(const WArgs& a, bool pack, dim3 grid, hipStream_t s) {
    if (pack) hipLaunchKernelGGL((k_warp_affine<C, BORDER, FORM, true>), grid, dim3(TX * TY), 0, s, a);
    else hipLaunchKernelGGL((k_warp_affine<C, BORDER, FORM, false>), grid, dim3(TX * TY), 0, s, a);
}

template <int C, int BORDER>
void launch2(const WArgs& a, int form, bool pack, dim3 grid, hipStream_t s) {
    if (form == 0) launch3<C, BORDER, 0>(a, pack, grid, s);
    else launch3<C, BORDER, 1>(a, pack, grid, s);
}

template <int C>
void launch1(const WArgs& a, int border, int form, bool pack, dim3 grid, hipStream_t s) {
    if (border == 0) launch2<C, 0>(a, form, pack, grid, s);
    else if (border == 1) launch2<C, 1>(a, form, pack, grid, s);
    else launch2<C, 2>(a, form, pack, grid, s);
}

}  // namespace

extern "C" int sr_warp_affine_u8(void* out, const uint8_t* in, const double* matrix, int64_t matrix_stride, int64_t N,
                                 int64_t H, int64_t W, int64_t C, int64_t oh, int64_t ow, int border, int fill,
                                 int out_form, sr_stream_t stream) {
    if (N < 0 || H < 1 || W < 1 || (C != 1 && C != 3 && C != 4) || oh < 1 || ow < 1 || border < 0 || border > 2 ||
        fill < 0 || fill > 255 || (out_form != 0 && out_form != 1) || (matrix_stride != 0 && matrix_stride != 6))
        return SR_EINVAL;
    if (N == 0) return SR_OK;
    if (!out || !in || !matrix || (reinterpret_cast<uintptr_t>(matrix) & 7)) return SR_EINVAL;
    if (N > 65535 || H > (1 << 24) || W > (1 << 24) || oh >= (1 << 20) || ow * C >= (1ll << 30)) return SR_ERANGE;
    WArgs a;
    a.in = in, a.out = out, a.m = matrix, a.m_stride = (int)matrix_stride;
    a.H = (int)H, a.W = (int)W, a.oh = (int)oh, a.ow = (int)ow;
    a.fill = fill;
    // a lane's 4 pixels start at byte 4 * C * k of a row: dword stores need dword-aligned rows, float4 stores 16 bytes
    const uintptr_t o = reinterpret_cast<uintptr_t>(out);
    const bool pack = out_form == 0 ? ((o & 3) == 0 && (ow * C) % 4 == 0) : ((o & 15) == 0 && ow % 4 == 0);
    const dim3 grid((unsigned)sr_ceil_div(ow, TX * PX), (unsigned)sr_ceil_div(oh, TY), (unsigned)N);
    if (C == 1) launch1<1>(a, border, out_form, pack, grid, sr_stream(stream));
    else if (C == 3) launch1<3>(a, border, out_form, pack, grid, sr_stream(stream));
    else launch1<4>(a, border, out_form, pack, grid, sr_stream(stream));
    return sr_launch_status();
}
