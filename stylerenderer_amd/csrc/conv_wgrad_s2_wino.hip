// Stride-2 3x3 weight gradient in the polyphase minimal-filtering domain: 25 instead of 36 matrix products per 2 x 2
// tile of the base grid, exact fp32 MFMA.
//
//   dW[ky][kx][u][v] = sum_{b, j, i}  (uscale[b,u] * U[b, u, 2j + ky, 2i + kx]) * (vscale[b,v] * V[b, v, j, i])
//
// Per dimension two V samples v0, v1 meet five U samples s0 .. s4:
//   dw0 = v0 (s0 - s2) + (v0 + v1) s2,   dw1 = v0 s1 + v1 s3,   dw2 = v1 (s4 - s2) + (v0 + v1) s2
// i.e. five products  u^ = (s0 - s2, s1, s4 - s2, s3, s2)  x  v^ = (v0, v0, v1, v1, v0 + v1)  into four slots
// (0, 1, 2, 1, 3); both dimensions: 25 products into 16 accumulator tiles, dW[ky][kx] = sum of A[a][b] over
// a in S(ky), b in S(kx) with S(0) = {0, 3}, S(1) = {1}, S(2) = {2, 3}.  All constants are 0 or +-1.
//
// k_wgrad_s2p: a workgroup of four waves (one per SIMD: the 16 accumulator tiles are 256 registers) owns 32 U x 128 V
// channels, a wave 32 x 32 of them with all 16 accumulators, and walks the 16 x 2 half patches (8 tiles) of its K
// slice.  A matrix instruction takes two tiles as its K pair, so a half patch is 4 steps x 25 = 100 MFMAs per wave
// and barrier.  Per half patch, pipelined over three stages with one barrier each:
//   n + 2: the raw U window (5 rows x 36 floats per channel) arrives by 16-byte buffer-addressed LDS-DMA, the same
//          staging instruction as k_wgrad_s2_dma's row group (the rows are not 16-byte aligned; the DMA does not mind)
//   n + 1: each thread transforms ONE (tile, U channel) item, uscale folded into the row stage, and writes the 25
//          values in MFMA operand layout [tile][product][channel]; the raw V pixels arrive by DMA
//   n:     the MFMAs; v^ is four raw reads, four scale multiplies and five adds per lane and step, no LDS of its own
// The non-MFMA work is pinned one or two instructions behind each MFMA; nothing in the loop waits on memory except
// the stage barrier.  One 16-position slab per K slice: ks * 16 <= the ks * 2 * 9 the direct plan reserves.
// k_wgrad_s2p_finish adds the slices in slice order, combines 16 -> 9 in a fixed order and applies the output layout.
#include "wgrad_tile.h"
#include "conv_wgrad_s2_wino.h"
#include "wgrad_style_finish.h"

namespace {

__device__ const float g_s2p_one[1] = {1.f};

struct S2pParams {
    const float* U;
    const float* V;
    const float* uscale;
    const float* vscale;
    float* partial;       // [ks][16][CU][CV]
    int B, CU, CV, UH, UW, GH, GW;
    int tiles_x, tiles_y, tiles_u, tiles_v;     // 16 x 4 patches, 32 / 128 channel tiles
    int pps;                                    // patches per K slice
};

namespace s2p {
constexpr int RP = sr_s2_window::RP;      // 36 floats per staged window row (33 used)
constexpr int UPL = sr_s2_window::UPL;    // 181: odd channel pitch of the raw window
constexpr int URAW = sr_s2_window::BLOCK; // 5792 floats, one raw buffer
constexpr int VPL = 8 * 32 + 1;           // 257: row l holds the 32 pixels of channels l, l + 16, ..., l + 112
constexpr int VBUF = 16 * VPL;            // 4112
constexpr int TP = 25 * 32;               // 800: tile pitch of u^ [tile][product][channel]
constexpr int UHAT = 8 * TP;              // 6400
constexpr int OFF_V = sr_s2_window::OFF_V; // 11584
constexpr int OFF_UH = OFF_V + 2 * VBUF;  // 19808
constexpr int LDS_FLOATS = OFF_UH + 2 * UHAT;     // 32608
constexpr int LDS_BYTES = LDS_FLOATS * 4;         // 130432
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
// product index -> accumulator slot and v^ index, per dimension
__device__ constexpr int slot_of(int i) { return i == 0 ? 0 : i == 1 ? 1 : i == 2 ? 2 : i == 3 ? 1 : 3; }
__device__ constexpr int vsel_of(int i) { return i < 2 ? 0 : i < 4 ? 1 : 2; }
}  // namespace s2p

__global__ __launch_bounds__(256) void k_wgrad_s2p(const S2pParams p) {
#if __HIP_DEVICE_COMPILE__
    using namespace s2p;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const SrWgradTile wt = sr_wgrad_tile(blockIdx.x, p.tiles_u, p.tiles_v, 32, 128);
    const int slice = wt.slice, u0 = wt.u0, v0 = wt.v0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;

    const int nhp = 2 * p.tiles_x * p.tiles_y * p.B;        // half patches: index = 2 * patch + row group
    const int first = slice * p.pps * 2;
    int last = first + p.pps * 2;
    if (last > nhp) last = nhp;
    if (first >= last) return;                              // (the plan leaves no empty slice)
    const int plane_u = p.UH * p.UW, plane_v = p.GH * p.GW;
    const int tiles_xy = p.tiles_x * p.tiles_y;

    const __amdgpu_buffer_rsrc_t r_u = uniform_rsrc(p.U, p.B * p.CU * plane_u * 4);
    const __amdgpu_buffer_rsrc_t r_v = uniform_rsrc(p.V, p.B * p.CV * plane_v * 4);
    // U: 45 lanes = 5 rows x 9 float4.  V: lane = (channel l + 16 k: k = lane >> 3, row = (lane >> 2) & 1, float4 = lane & 3)
    const int u_lane_off = sr_s2_window::lane_off(lane, p.UW);
    const int v_lane_off = ((lane >> 3) * 16 * plane_v + ((lane >> 2) & 1) * p.GW + 4 * (lane & 3)) * 4;
    const bool u_lane = lane < sr_s2_window::LANES;
    const float* usc = p.uscale ? p.uscale : g_s2p_one;
    const float* vsc = p.vscale ? p.vscale : g_s2p_one;
    const int us_on = p.uscale ? 1 : 0, vs_on = p.vscale ? 1 : 0;

    // wave-uniform decode of a half patch (clamped to the slice: past its end the last one is staged again)
    auto clamp_hp = [&](int hp) { return hp < last ? hp : last - 1; };
    auto sample_of = [&](int hp) { return (hp >> 1) / tiles_xy; };
    auto origin_u = [&](int hp) {       // byte offset of the window's first float at channel u0
        const int g = hp & 1;
        const SrWgradPatch pt = sr_wgrad_patch(hp >> 1, p.tiles_x, p.tiles_y);
        return ((pt.b * p.CU + u0) * plane_u + (pt.ty * 8 + g * 4) * p.UW + pt.tx * 32) * 4;
    };
    auto origin_v = [&](int hp) {
        const int g = hp & 1;
        const SrWgradPatch pt = sr_wgrad_patch(hp >> 1, p.tiles_x, p.tiles_y);
        return ((pt.b * p.CV + v0) * plane_v + (pt.ty * 4 + g * 2) * p.GW + pt.tx * 16) * 4;
    };
    // (readfirstlane: a soffset the compiler keeps in a VGPR turns the DMA into a waterfall loop)
    // DMA item i of this wave (compile-time i): 0..7 = U channel wave + 4 i; 8..11 = V row wave + 4 (i - 8)
    auto dma_u = [&](int i, int org, float* dst) {
        const int ch = wave + 4 * i;
        if (u_lane)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r_u, (lptr_t)(dst + ch * UPL), 16, u_lane_off,
                                                     __builtin_amdgcn_readfirstlane(org + ch * plane_u * 4), 0, 0);
    };
    auto dma_v = [&](int i, int org, float* dst) {
        const int l = wave + 4 * i;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r_v, (lptr_t)(dst + l * VPL), 16, v_lane_off,
                                                 __builtin_amdgcn_readfirstlane(org + l * plane_v * 4), 0, 0);
    };
    auto load_us = [&](int hp) { return usc[((int64_t)sample_of(hp) * p.CU + u0 + l31) * us_on]; };
    auto load_vs = [&](int hp) { return vsc[((int64_t)sample_of(hp) * p.CV + v0 + wave * 32 + l31) * vs_on]; };

    // this thread's transform item: tile tid >> 5 (= 2 wave + half), channel l31
    const int xr_base = l31 * UPL + 4 * (tid >> 5);
    const int xw_base = (tid >> 5) * TP + l31;
    // operand addresses: u^ of tile 2 step + half, V of channel wave * 32 + l31 = (l31 & 15) + 16 (2 wave + (l31 >> 4))
    const int a_base = half * TP + l31;
    const int b_base = (l31 & 15) * VPL + (2 * wave + (l31 >> 4)) * 32 + 2 * half;

    float raw[25], tr[25];
    auto xf_read = [&](const float* src, int k) { raw[k] = src[xr_base + (k / 5) * RP + (k % 5)]; };      // k = row * 5 + col
    // row stage of column x, op q of 5: tr[i * 5 + x], rows (s0 - s2, s1, s4 - s2, s3, s2), uscale folded in
    auto xf_row = [&](int x, int q, float s) {
        if (q == 0) tr[4 * 5 + x] = raw[2 * 5 + x] * s;
        if (q == 1) tr[0 * 5 + x] = raw[0 * 5 + x] * s - tr[4 * 5 + x];
        if (q == 2) tr[1 * 5 + x] = raw[1 * 5 + x] * s;
        if (q == 3) tr[2 * 5 + x] = raw[4 * 5 + x] * s - tr[4 * 5 + x];
        if (q == 4) tr[3 * 5 + x] = raw[3 * 5 + x] * s;
    };
    // column stage + store of product (i, j)
    auto xf_col_store = [&](float* dst, int i, int j) {
        float v;
        if (j == 0) v = tr[i * 5 + 0] - tr[i * 5 + 2];
        else if (j == 1) v = tr[i * 5 + 1];
        else if (j == 2) v = tr[i * 5 + 4] - tr[i * 5 + 2];
        else if (j == 3) v = tr[i * 5 + 3];
        else v = tr[i * 5 + 2];
        dst[xw_base + (i * 5 + j) * 32] = v;
    };

    f32x16 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    // ---- prologue: raw U of half patches 0 and 1, V of 0; transform 0
    {
        const int o0 = origin_u(first), o1 = origin_u(clamp_hp(first + 1)), ov = origin_v(first);
#pragma unroll
        for (int i = 0; i < 8; ++i) dma_u(i, o0, smem);
#pragma unroll
        for (int i = 0; i < 8; ++i) dma_u(i, o1, smem + URAW);
#pragma unroll
        for (int i = 0; i < 4; ++i) dma_v(i, ov, smem + OFF_V);
    }
    float us_next = load_us(clamp_hp(first + 1));      // scale of the item transformed in the next stage
    float vs_cur = load_vs(first);
    {
        const float us0 = load_us(first);
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
#pragma unroll
        for (int k = 0; k < 25; ++k) xf_read(smem, k);
#pragma unroll
        for (int k = 0; k < 25; ++k) xf_row(k / 5, k % 5, us0);
#pragma unroll
        for (int k = 0; k < 25; ++k) xf_col_store(smem + OFF_UH, k / 5, k % 5);
    }

    const int count = last - first;
    for (int n = 0; n < count; ++n) {
        // "my DMAs landed" + "my LDS accesses retired", then the barrier: u^ and V of n complete, raw U of n + 1 landed
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const int cur = n & 1;
        const float* uh = smem + OFF_UH + cur * UHAT;
        const float* vb = smem + OFF_V + cur * VBUF;
        const float* ur = smem + (cur ^ 1) * URAW;           // raw U of n + 1: transformed in this stage
        float* uh_o = smem + OFF_UH + (cur ^ 1) * UHAT;
        float* ur_o = smem + cur * URAW;                     // raw U of n + 2 arrives here
        float* vb_o = smem + OFF_V + (cur ^ 1) * VBUF;       // V of n + 1
        const int hp_u = clamp_hp(first + n + 2), hp_v = clamp_hp(first + n + 1);
        const int org_u = origin_u(hp_u), org_v = origin_v(hp_v);
        const float us_x = us_next, vs = vs_cur;
        float us_ld = 1.0f, vs_ld = 1.0f;

        float a[25], vr[4], vh[9], vhn[9];
        auto fetch_v = [&](int step, int k) { vr[k] = vb[b_base + (k >> 1) * 16 + 4 * step + (k & 1)]; };
        // v^ [y][x] over (row 0, row 1, sum) x (col 0, col 1, sum), vscale folded in; op q of 9
        auto make_vh = [&](float* o, int q) {
            if (q < 4) o[(q >> 1) * 3 + (q & 1)] = vr[q] * vs;
            if (q == 4) o[2] = o[0] + o[1];
            if (q == 5) o[5] = o[3] + o[4];
            if (q == 6) o[6] = o[0] + o[3];
            if (q == 7) o[7] = o[1] + o[4];
            if (q == 8) o[8] = o[6] + o[7];
        };
        // operands of step 0: V first (v^ needs them first), then u^ in MFMA order (counted lgkmcnt waits)
#pragma unroll
        for (int k = 0; k < 4; ++k) fetch_v(0, k);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 25; ++k) a[k] = uh[a_base + k * 32];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 9; ++q) make_vh(vh, q);
        __builtin_amdgcn_sched_barrier(0);

#pragma unroll
        for (int step = 0; step < 4; ++step) {
#pragma unroll
            for (int m = 0; m < 25; ++m) {
                const int i = m / 5, j = m % 5;
                const int t = slot_of(i) * 4 + slot_of(j);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m], vh[vsel_of(i) * 3 + vsel_of(j)], acc[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                // ---- behind MFMA (step, m): its own operand register is free again
                if (step < 3) {
                    a[m] = uh[a_base + (2 * (step + 1)) * TP + m * 32];
                    if (m < 4) fetch_v(step + 1, m);
                    if (m >= 12 && m < 21) make_vh(vhn, m - 12);
                }
                if (step == 0) {
                    if (m < 8) dma_u(m, org_u, ur_o);
                    else if (m < 12) dma_v(m - 8, org_v, vb_o);
                    else if (m == 21) us_ld = load_us(hp_u);
                    else if (m == 22) vs_ld = load_vs(hp_v);
                }
                if (step == 1) xf_read(ur, m);
                if (step == 2) xf_row(m / 5, m % 5, us_x);
                if (step == 3) xf_col_store(uh_o, i, j);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (step < 3) {
#pragma unroll
                for (int q = 0; q < 9; ++q) vh[q] = vhn[q];
            }
        }
        us_next = us_ld;
        vs_cur = vs_ld;
    }
    // surplus fetches are still landing in this workgroup's LDS: drain them before the wave can retire
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // partial[slice][position][u][v]; C/D layout: column (v) = lane & 31, row (u) = (r & 3) + 8 (r >> 2) + 4 half
    float* dst = p.partial + (int64_t)slice * 16 * p.CU * p.CV;
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = sr_mfma32_row(r, half, u0);
            const int v = v0 + wave * 32 + l31;
            dst[((int64_t)t * p.CU + u) * p.CV + v] = acc[t][r];
        }
#endif
}

struct S2pFinish {
    const float* partial;
    float* out;
    int ks, CU, CV;
    int64_t slab, su, sv;
};

// One lane per (tap, u, v): the up to four positions of the tap are summed over the slices in slice order, each in
// its own accumulator (independent loads in flight), then combined as (A[a0][b0] + A[a0][b1]) + (A[a1][b0] + A[a1][b1]).
__global__ __launch_bounds__(256) void k_wgrad_s2p_finish(const S2pFinish p) {
    const int64_t plane = (int64_t)p.CU * p.CV;
    const int64_t total = 9 * plane;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int t = (int)(i / plane);
        const int64_t uv = i - (int64_t)t * plane;
        const int u = (int)(uv / p.CV), v = (int)(uv % p.CV);
        const int ky = t / 3, kx = t % 3;
        // S(0) = {0, 3}, S(1) = {1}, S(2) = {2, 3}
        const int a0 = ky, a1 = ky == 1 ? -1 : 3, b0 = kx, b1 = kx == 1 ? -1 : 3;
        const float* src = p.partial + uv;
        float s00 = 0.f, s01 = 0.f, s10 = 0.f, s11 = 0.f;
        for (int s = 0; s < p.ks; ++s) {
            const float* q = src + (int64_t)s * 16 * plane;
            s00 += q[(a0 * 4 + b0) * plane];
            if (b1 >= 0) s01 += q[(a0 * 4 + b1) * plane];
            if (a1 >= 0) s10 += q[(a1 * 4 + b0) * plane];
            if (a1 >= 0 && b1 >= 0) s11 += q[(a1 * 4 + b1) * plane];
        }
        p.out[t * p.slab + u * p.su + v * p.sv] = (s00 + s01) + (s10 + s11);
    }
}

}  // namespace

bool sr_wgrad_s2_wino_eligible(int64_t B, int64_t CU, int64_t CV, int64_t UH, int64_t UW, int64_t GH, int64_t GW, int d0) {
    return B > 0 && CU % 32 == 0 && CV % 128 == 0 && GW % 16 == 0 && GH % 4 == 0 && d0 == 0 && UH >= 2 * GH + 1 &&
           UW >= 2 * GW + 1 && B * CU * UH * UW < (1LL << 29) && B * CV * GH * GW < (1LL << 29);
}

int64_t sr_wgrad_s2_wino_scratch_floats(int64_t ks, int64_t CU, int64_t CV) { return ks * 16 * CU * CV; }

int sr_wgrad_s2_wino_launch(const float* U, const float* V, const float* uscale, const float* vscale, float* partial,
                            int64_t B, int64_t CU, int64_t CV, int64_t UH, int64_t UW, int64_t GH, int64_t GW, int ks,
                            int pps, hipStream_t st) {
    S2pParams p;
    p.U = U; p.V = V; p.uscale = uscale; p.vscale = vscale; p.partial = partial;
    p.B = (int)B; p.CU = (int)CU; p.CV = (int)CV; p.UH = (int)UH; p.UW = (int)UW; p.GH = (int)GH; p.GW = (int)GW;
    p.tiles_x = (int)(GW / 16); p.tiles_y = (int)(GH / 4); p.tiles_u = (int)(CU / 32); p.tiles_v = (int)(CV / 128);
    p.pps = pps;
    if (!sr_allow_dynamic_lds<k_wgrad_s2p>(s2p::LDS_BYTES)) return SR_EINVAL;
    hipLaunchKernelGGL(k_wgrad_s2p, dim3((unsigned)(p.tiles_u * p.tiles_v * ks)), dim3(256), s2p::LDS_BYTES, st, p);
    return sr_launch_status();
}

int sr_wgrad_s2_wino_finish(const WgradOut& out, const float* partial, int ks, int64_t CU, int64_t CV, hipStream_t st) {
    S2pFinish r;
    r.partial = partial; r.out = out.dwt; r.ks = ks; r.CU = (int)CU; r.CV = (int)CV;
    r.slab = out.slab; r.su = out.su; r.sv = out.sv;
    hipLaunchKernelGGL(k_wgrad_s2p_finish, dim3(sr_stream_grid(9 * CU * CV, 256)), dim3(256), 0, st, r);
    return sr_launch_status();
}

int sr_wgrad_s2_wino_style_finish(float* dwt, float* gis, const float* partial, const float* iscale, const float* wt,
                                  int64_t ldw, int sps, int64_t B, int64_t CU, int64_t CV, float* part, hipStream_t st) {
    SrStyleFinish f;
    f.partial = partial; f.iscale = iscale; f.wt = wt; f.dwt = dwt; f.part = part;
    f.B = (int)B; f.sps = sps; f.CU = (int)CU; f.CV = (int)CV; f.C = (int)CV; f.N = (int)CU; f.ldw = (int)ldw;
    return sr_wgrad_style_finish_launch<SrPullS2p, true>(f, gis, st);
}
