// Pillow-exact resampling of uint8 images (sr_resample_u8, include/stylerenderer_amd.h).
//
// Pillow's 8-bit resampler is two separable passes of integer arithmetic on 22-bit fixed-point coefficients: every
// output byte is clip(0, 255, (2^21 + sum_t pixel[first + t] * k[t]) >> 22) in int32, horizontal pass first into a uint8
// intermediate, then vertical.  Integer sums do not depend on their order, so these kernels equal Pillow (and the host
// restatement in op/resample.py) on every byte.  The tables come from the host; nothing here evaluates a filter.
//
//   k_resample_h  one workgroup = 64 output pixels x 4 rows, one wave per row.  A wave stages the contiguous input span
//                 of its row that the 64 pixels read ([first(x0), first(x63) + count(x63)) pixels) into LDS with aligned
//                 dword loads; one lane then computes one output pixel's channels from LDS bytes.  The coefficient table
//                 is stored TRANSPOSED [ksize, ow], so that a wave's read of tap t is one contiguous run.  A span that
//                 does not fit the LDS budget (a reduction by several hundred) reads global memory directly.
//   k_resample_v  a row is a flat run of bytes: a lane owns 4 consecutive bytes, walks the tap rows (coefficients are
//                 wave-uniform: scalar loads) and stores one packed dword (bytes / floats when the rows are not
//                 dword-aligned or the float32 CHW form is asked for).
//
// Either pass is skipped when its axis keeps its size; with both skipped the vertical kernel runs with an identity tap
// (the window copy).  The last pass that runs writes the requested form.  Only the window is computed: the horizontal
// pass makes the rows the window's vertical taps read, and of those only the window's columns.
// pixel * k: |k| < 2^23 in every table of the five filters seen so far (op/resample.py checks each table it builds), so
// the product is v_mad_i32_i24 at full rate; the M24 = false instantiations take the 32-bit multiply.
#include "common.h"

namespace {

constexpr int PBITS = 22;
constexpr int HALF = 1 << (PBITS - 1);
constexpr int HT_W = 64, HT_R = 4;          // horizontal tile: output pixels x rows per 256-lane workgroup
constexpr int VB = 256;
constexpr int LDS_BUDGET = 48 * 1024;

template <bool M24>
__device__ __forceinline__ int mad(int p, int k, int acc) {
    return (M24 ? __mul24(p, k) : p * k) + acc;
}

// The empty asm keeps the clipped value apart from the byte packing that follows it.  Left together, hipcc (ROCm 7)
// turns shift + clamp + pack of two values into v_ashr_pk_u8_i32 and ORs bytes 2 and 3 into its result as if the upper
// half were zero; on the MI355X it was not (whatever the register held before came through), and bytes 2 and 3 of
// every packed dword were wrong while bytes 0 and 1 were right.
__device__ __forceinline__ int clip8(int v) {
    v >>= PBITS;
    v = v < 0 ? 0 : (v > 255 ? 255 : v);
    asm("" : "+v"(v));
    return v;
}

// dataset.to_unit_tensor: (v / 255 - 0.5) / 0.5 in float32, each operation correctly rounded
__device__ __forceinline__ float unit(int v) { return ((float)v / 255.0f - 0.5f) / 0.5f; }

struct HArgs {
    const uint8_t* in;      // [N, H, W, C]
    void* out;              // FORM 0: uint8 [N, rows, out_pitch bytes]; FORM 1: float32 [N, C, rows, oww]
    const int* kT;          // [ksize, ow]
    const int* b;           // [ow, 2] (first, count)
    int64_t in_bytes;
    int H, W, ow;
    int row0, rows;         // input rows row0 .. row0 + rows are resampled
    int ox0, oww;           // output columns ox0 .. ox0 + oww
    int out_pitch;
    int lds_pitch;          // dwords per staged row
};

template <int C, bool M24, bool STAGE, int FORM>
__global__ __launch_bounds__(HT_W* HT_R) void k_resample_h(HArgs a) {
    extern __shared__ uint32_t lds[];
    const int tx = threadIdx.x & (HT_W - 1), ty = threadIdx.x / HT_W;
    const int x = blockIdx.x * HT_W + tx, r = blockIdx.y * HT_R + ty, n = blockIdx.z;
    const bool row_ok = r < a.rows;
    const uint8_t* grow = a.in + ((int64_t)n * a.H + (a.row0 + (row_ok ? r : 0))) * (int64_t)a.W * C;
    const uint8_t* src = grow;
    int base_px = 0, mis = 0;
    if (STAGE) {
        const int xf = a.ox0 + blockIdx.x * HT_W;
        const int xl = min(xf + HT_W - 1, a.ox0 + a.oww - 1);
        const int p0 = a.b[2 * xf], p1 = a.b[2 * xl] + a.b[2 * xl + 1];
        const uint8_t* first = grow + (int64_t)p0 * C;
        mis = (int)(reinterpret_cast<uintptr_t>(first) & 3);
        const uint8_t* start = first - mis;
        const int ndw = (mis + (p1 - p0) * C + 3) >> 2;
        const uint8_t* lo = a.in;
        const uint8_t* hi = a.in + a.in_bytes;
        uint32_t* mine = lds + ty * a.lds_pitch;
        if (row_ok)
            for (int i = tx; i < ndw; i += HT_W) {
                const uint8_t* p = start + 4 * i;
                uint32_t v;
                if (p >= lo && p + 4 <= hi) {
                    v = *reinterpret_cast<const uint32_t*>(p);
                } else {        // the first / last dword of the tensor: only its bytes
                    v = 0;
                    for (int q = 0; q < 4; ++q)
                        if (p + q >= lo && p + q < hi) v |= (uint32_t)p[q] << (8 * q);
                }
                mine[i] = v;
            }
        __syncthreads();
        src = reinterpret_cast<const uint8_t*>(mine);
        base_px = p0;
    }
    if (!row_ok || x >= a.oww) return;
    const int X = a.ox0 + x;
    const int xmin = a.b[2 * X], cnt = a.b[2 * X + 1];
    const uint8_t* px = src + mis + (int64_t)(xmin - base_px) * C;
    const int* kp = a.kT + X;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = HALF;
    for (int t = 0; t < cnt; ++t) {
        const int k = kp[(int64_t)t * a.ow];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = mad<M24>(px[t * C + c], k, acc[c]);
    }
    if (FORM == 0) {
        uint8_t* dst = static_cast<uint8_t*>(a.out) + ((int64_t)n * a.rows + r) * a.out_pitch + (int64_t)x * C;
        bool packed = false;
        if constexpr (C == 4) {
            if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
                *reinterpret_cast<uint32_t*>(dst) = (uint32_t)clip8(acc[0]) | (uint32_t)clip8(acc[1]) << 8 |
                                                    (uint32_t)clip8(acc[2]) << 16 | (uint32_t)clip8(acc[3]) << 24;
                packed = true;
            }
        }
        if (!packed) {
#pragma unroll
            for (int c = 0; c < C; ++c) dst[c] = (uint8_t)clip8(acc[c]);
        }
    } else {
        float* dst = static_cast<float*>(a.out);
#pragma unroll
        for (int c = 0; c < C; ++c) dst[(((int64_t)n * C + c) * a.rows + r) * a.oww + x] = unit(clip8(acc[c]));
    }
}

struct VArgs {
    const uint8_t* in;      // rows of in_pitch bytes, images in_img bytes apart; row 0 is source row row0
    void* out;              // OUT 0 / 1: uint8 [N, ohw, row_bytes]; OUT 2: float32 [N, C, ohw, oww]
    const int* k;           // [oh, ksize]; NULL: identity (output row y = input row oy0 + y)
    const int* b;           // [oh, 2]
    int64_t in_img;
    int in_pitch, in_off;   // in_off: byte offset of the window's first column in a row
    int ksize, row0;
    int oy0, ohw;
    int row_bytes, oww, C;
};

// AIN: rows of `in` can be read as aligned dwords up to the end of the lane's dword.  OUT 0: byte stores, 1: one packed
// dword per lane (row_bytes a multiple of 4, aligned base), 2: float32 CHW.
template <bool M24, bool AIN, int OUT>
__global__ __launch_bounds__(VB) void k_resample_v(VArgs a) {
    const int byte0 = (blockIdx.x * VB + threadIdx.x) * 4;
    if (byte0 >= a.row_bytes) return;
    const int y = blockIdx.y, n = blockIdx.z;
    const int valid = min(4, a.row_bytes - byte0);
    int ymin = a.oy0 + y, cnt = 1;
    const int* kp = nullptr;
    if (a.k) {
        ymin = a.b[2 * (a.oy0 + y)];
        cnt = a.b[2 * (a.oy0 + y) + 1];
        kp = a.k + (int64_t)(a.oy0 + y) * a.ksize;
    }
    const uint8_t* src = a.in + (int64_t)n * a.in_img + (int64_t)(ymin - a.row0) * a.in_pitch + a.in_off + byte0;
    int acc[4] = {HALF, HALF, HALF, HALF};
    for (int t = 0; t < cnt; ++t) {
        const int k = kp ? kp[t] : (1 << PBITS);
        uint32_t v;
        if (AIN) {
            v = *reinterpret_cast<const uint32_t*>(src);
        } else {
            v = 0;
            for (int q = 0; q < valid; ++q) v |= (uint32_t)src[q] << (8 * q);
        }
        src += a.in_pitch;
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = mad<M24>((int)((v >> (8 * q)) & 255u), k, acc[q]);
    }
    if (OUT == 1) {
        uint8_t* dst = static_cast<uint8_t*>(a.out) + ((int64_t)n * a.ohw + y) * a.row_bytes + byte0;
        *reinterpret_cast<uint32_t*>(dst) = (uint32_t)clip8(acc[0]) | (uint32_t)clip8(acc[1]) << 8 |
                                            (uint32_t)clip8(acc[2]) << 16 | (uint32_t)clip8(acc[3]) << 24;
    } else if (OUT == 0) {
        uint8_t* dst = static_cast<uint8_t*>(a.out) + ((int64_t)n * a.ohw + y) * a.row_bytes + byte0;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < valid) dst[q] = (uint8_t)clip8(acc[q]);
    } else {
        float* dst = static_cast<float*>(a.out);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < valid) {
                const int bi = byte0 + q;
                const int x = a.C == 3 ? bi / 3 : (a.C == 4 ? bi >> 2 : bi);
                const int c = bi - x * a.C;
                dst[(((int64_t)n * a.C + c) * a.ohw + y) * a.oww + x] = unit(clip8(acc[q]));
            }
    }
}

template <int C, bool M24, bool STAGE>
void launch_h2(const HArgs& a, int form, dim3 grid, size_t lds, hipStream_t s) {
    if (form == 0)
        hipLaunchKernelGGL((k_resample_h<C, M24, STAGE, 0>), grid, dim3(HT_W * HT_R), lds, s, a);
    else
        hipLaunchKernelGGL((k_resample_h<C, M24, STAGE, 1>), grid, dim3(HT_W * HT_R), lds, s, a);
}

template <int C>
void launch_h1(const HArgs& a, int form, bool m24, bool stage, dim3 grid, size_t lds, hipStream_t s) {
    if (m24 && stage) launch_h2<C, true, true>(a, form, grid, lds, s);
    else if (m24) launch_h2<C, true, false>(a, form, grid, lds, s);
    else if (stage) launch_h2<C, false, true>(a, form, grid, lds, s);
    else launch_h2<C, false, false>(a, form, grid, lds, s);
}

template <bool M24, bool AIN>
void launch_v1(const VArgs& a, int out, dim3 grid, hipStream_t s) {
    if (out == 0) hipLaunchKernelGGL((k_resample_v<M24, AIN, 0>), grid, dim3(VB), 0, s, a);
    else if (out == 1) hipLaunchKernelGGL((k_resample_v<M24, AIN, 1>), grid, dim3(VB), 0, s, a);
    else hipLaunchKernelGGL((k_resample_v<M24, AIN, 2>), grid, dim3(VB), 0, s, a);
}

inline int64_t round4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// rows of the source the window's vertical taps read: [r0, r1); false when the table does not fit the source
bool vertical_rows(const int32_t* bv, int64_t H, int64_t ksize, int64_t oy0, int64_t ohw, int64_t* r0, int64_t* r1) {
    *r0 = bv[2 * oy0];
    *r1 = (int64_t)bv[2 * (oy0 + ohw - 1)] + bv[2 * (oy0 + ohw - 1) + 1];
    if (*r0 < 0 || *r1 > H || *r1 <= *r0) return false;
    for (int64_t y = oy0; y < oy0 + ohw; ++y) {
        const int64_t lo = bv[2 * y], cnt = bv[2 * y + 1];
        if (cnt < 1 || (ksize && cnt > ksize) || lo < *r0 || lo + cnt > *r1) return false;
    }
    return true;
}

bool bad_shape(int64_t N, int64_t H, int64_t W, int64_t C, int64_t oh, int64_t ow, int64_t oy0, int64_t ox0, int64_t ohw,
               int64_t oww) {
    return N < 0 || H < 1 || W < 1 || (C != 1 && C != 3 && C != 4) || oh < 1 || ow < 1 || oy0 < 0 || ox0 < 0 || ohw < 1 ||
           oww < 1 || oy0 + ohw > oh || ox0 + oww > ow;
}

}  // namespace

extern "C" int64_t sr_resample_u8_scratch_bytes(int64_t N, int64_t H, int64_t W, int64_t C, int64_t oh, int64_t ow,
                                                const int32_t* bounds_v_host, int64_t oy0, int64_t ox0, int64_t ohw,
                                                int64_t oww) {
    if (bad_shape(N, H, W, C, oh, ow, oy0, ox0, ohw, oww)) return -1;
    if (oh == H || ow == W || N == 0) return 0;
    if (!bounds_v_host) return -1;
    int64_t r0, r1;
    if (!vertical_rows(bounds_v_host, H, 0, oy0, ohw, &r0, &r1)) return -1;
    return N * (r1 - r0) * round4(oww * C);
}

extern "C" int sr_resample_u8(void* out, const uint8_t* in, int64_t N, int64_t H, int64_t W, int64_t C, int64_t oh,
                              int64_t ow, const int32_t* coeffs_h_t, const int32_t* bounds_h, const int32_t* bounds_h_host,
                              int64_t ksize_h, const int32_t* coeffs_v, const int32_t* bounds_v,
                              const int32_t* bounds_v_host, int64_t ksize_v, int64_t oy0, int64_t ox0, int64_t ohw,
                              int64_t oww, int out_form, int mul24, uint8_t* scratch, sr_stream_t stream) {
    if (bad_shape(N, H, W, C, oh, ow, oy0, ox0, ohw, oww) || (out_form != 0 && out_form != 1)) return SR_EINVAL;
    if (N == 0) return SR_OK;
    const bool do_h = ow != W, do_v = oh != H;
    if (!out || !in) return SR_EINVAL;
    if (do_h != (coeffs_h_t != nullptr) || do_v != (coeffs_v != nullptr)) return SR_EINVAL;
    if (do_h && (!bounds_h || !bounds_h_host || ksize_h < 1)) return SR_EINVAL;
    if (do_v && (!bounds_v || !bounds_v_host || ksize_v < 1)) return SR_EINVAL;
    if (do_h && do_v && !scratch) return SR_EINVAL;
    if (N > 65535 || ohw > 65535 || H > (1 << 24) || W * C >= (1ll << 30) || ow * ksize_h >= (1ll << 31) ||
        oww * C >= (1ll << 30))
        return SR_ERANGE;
    hipStream_t s = sr_stream(stream);
    const bool m24 = mul24 != 0;

    int64_t r0 = oy0, r1 = oy0 + ohw;
    if (do_v && !vertical_rows(bounds_v_host, H, ksize_v, oy0, ohw, &r0, &r1)) return SR_EINVAL;
    const int64_t rows = r1 - r0, mid_pitch = round4(oww * C);
    if (sr_ceil_div(rows, HT_R) > 65535) return SR_ERANGE;

    if (do_h) {
        // the widest span of one tile decides the LDS row; the table must stay inside the source row
        int64_t span = 0;
        for (int64_t x = ox0; x < ox0 + oww; ++x) {
            const int64_t lo = bounds_h_host[2 * x], cnt = bounds_h_host[2 * x + 1];
            if (lo < 0 || cnt < 1 || cnt > ksize_h || lo + cnt > W) return SR_EINVAL;
            if (x > ox0 && (lo < bounds_h_host[2 * (x - 1)] ||
                            lo + cnt < (int64_t)bounds_h_host[2 * (x - 1)] + bounds_h_host[2 * (x - 1) + 1]))
                return SR_EINVAL;
        }
        for (int64_t xf = ox0; xf < ox0 + oww; xf += HT_W) {
            const int64_t xl = (xf + HT_W - 1 < ox0 + oww - 1) ? xf + HT_W - 1 : ox0 + oww - 1;
            const int64_t w = (int64_t)bounds_h_host[2 * xl] + bounds_h_host[2 * xl + 1] - bounds_h_host[2 * xf];
            if (w > span) span = w;
        }
        const int64_t lds_pitch = (span * C + 3 + 3) / 4 + 1;
        const bool stage = lds_pitch * 4 * HT_R <= LDS_BUDGET;
        HArgs a;
        a.in = in;
        a.out = do_v ? static_cast<void*>(scratch) : out;
        a.kT = coeffs_h_t;
        a.b = bounds_h;
        a.in_bytes = N * H * W * C;
        a.H = (int)H, a.W = (int)W, a.ow = (int)ow;
        a.row0 = (int)r0, a.rows = (int)rows;
        a.ox0 = (int)ox0, a.oww = (int)oww;
        a.out_pitch = (int)(do_v ? mid_pitch : oww * C);
        a.lds_pitch = (int)lds_pitch;
        const dim3 grid((unsigned)sr_ceil_div(oww, HT_W), (unsigned)sr_ceil_div(rows, HT_R), (unsigned)N);
        const size_t lds = stage ? (size_t)lds_pitch * 4 * HT_R : 0;
        const int form = do_v ? 0 : out_form;
        if (C == 1) launch_h1<1>(a, form, m24, stage, grid, lds, s);
        else if (C == 3) launch_h1<3>(a, form, m24, stage, grid, lds, s);
        else launch_h1<4>(a, form, m24, stage, grid, lds, s);
        const int rc = sr_launch_status();
        if (rc != SR_OK || !do_v) return rc;
    }

    VArgs v;
    v.out = out;
    v.k = coeffs_v;
    v.b = bounds_v;
    v.ksize = (int)ksize_v;
    v.oy0 = (int)oy0, v.ohw = (int)ohw;
    v.row_bytes = (int)(oww * C), v.oww = (int)oww, v.C = (int)C;
    if (do_h) {             // from the intermediate: row 0 is source row r0, only the window's columns
        v.in = scratch;
        v.in_img = rows * mid_pitch;
        v.in_pitch = (int)mid_pitch, v.in_off = 0, v.row0 = (int)r0;
    } else {
        v.in = in;
        v.in_img = H * W * C;
        v.in_pitch = (int)(W * C), v.in_off = (int)(ox0 * C), v.row0 = 0;
    }
    const bool ain = (reinterpret_cast<uintptr_t>(v.in) & 3) == 0 && v.in_pitch % 4 == 0 && v.in_off % 4 == 0 &&
                     v.in_img % 4 == 0;
    const int om = out_form == 1 ? 2 : ((reinterpret_cast<uintptr_t>(out) & 3) == 0 && v.row_bytes % 4 == 0 ? 1 : 0);
    const dim3 grid((unsigned)sr_ceil_div(sr_ceil_div(v.row_bytes, 4), VB), (unsigned)ohw, (unsigned)N);
    if (m24 && ain) launch_v1<true, true>(v, om, grid, s);
    else if (m24) launch_v1<true, false>(v, om, grid, s);
    else if (ain) launch_v1<false, true>(v, om, grid, s);
    else launch_v1<false, false>(v, om, grid, s);
    return sr_launch_status();
}
