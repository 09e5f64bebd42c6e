// Weight gradient of the (modulated) convolution on the gfx950 matrix cores, exact fp32 MFMA.
//
//   D[tap][u][v] = sum_{b, p in grid}  (uscale[b,u] * U[b, u, p*IS + d0 + tap]) * (vscale[b,v] * V[b, v, p])
//
// U is the operand read through the tap window, V the operand on the base grid:
//   * regular conv  y = conv(x, W):      U = x (u = input channel),  V = dL/dy (v = output channel)
//   * transposed conv (upsampling, out[2y+ky] += x[y] W[ky]):  U = dL/dy read with stride 2, V = x
// The modulation of reference layers.py:295-299 enters as the per-(sample, channel) scales, so the
// per-sample weight gradients [B, Cout, Cin, k, k] the reference's grouped convolution would
// produce are never materialised: the batch is part of the K (pixel) dimension.
//
// GEMM per tap:  D[u][v] = sum_k A[u][k] * Bm[k][v],  k = pixel.  A workgroup owns a (UT x VT) tile
// of channels for ALL taps of the window (each staged U halo patch feeds every tap), a wave owns
// 32 x 32 x taps = 9 accumulator tiles (144 registers).  K is split over workgroups
// (grid = channel tiles x K slices ~ 2 x 256 CUs); slices write fp32 partial slabs that a second
// kernel sums in a fixed order (deterministic; no float atomics) while applying the output layout.
//
// Data movement: one 64-pixel patch per stage, LDS double buffered.  A staging instruction covers
// 64 consecutive floats of ONE channel plane (coalesced 256 B), so its per-lane source offset
// depends only on the lane (computed once per patch) and the channel only adds a wave-uniform
// stride.  The loads of patch i+1 are software-pipelined INTO the MFMA stream of patch i: a few
// global loads per pixel pair, written to the other LDS buffer four pixel pairs later (counted
// vmcnt, ~a dozen staging registers in flight), so the matrix pipe never waits for memory.
// (4-byte LDS-DMA was measured at ~90 cycles per instruction per CU — 62 TFLOP/s here — and
// 16-byte DMA needs 16-byte aligned planes, which halo rows are not: profiles/r01_notes.md.)
// Planes have an ODD pitch: the 32 lanes of an operand fetch (32 channels, same pixel) hit 32
// different banks.
// The modulation scales are fetched per patch as two small LDS rows and multiplied onto the
// operands after the ds_read (never onto freshly loaded registers: no wait on memory in the loop).
//
// This file: k_wgrad_mfma, the tiling (sr_wgrad_tiles) and the launch of the direct path.  The other paths, the
// reduce kernels and the dispatch live in their own files.
#include "wgrad_tile.h"
#include "conv_wgrad_mfma.h"

namespace {

// NG = number of 4-wave groups per workgroup.  With NG = 2 (512 threads) the two groups share
// the staged patch and split its pixel pairs (rows), each with its own accumulators and its own
// partial slab: two waves per SIMD cover each other's LDS / barrier stalls while the 133 KB
// double buffer still fits one workgroup per CU.
template <int IS, int TY, int TX, int PW, int PH, int PB, int UT, int VT, int NG>
struct WG {
    static constexpr int NWAVE = 4 * NG, THREADS = 256 * NG;
    static constexpr int PHG = PH / NG;                     // patch rows per group
    static_assert(NG == 1 || (PB == 1 && PH % NG == 0), "row split needs a single-sample patch");
    static constexpr int NT = TY * TX;
    static constexpr int EH = (PH - 1) * IS + TY;
    static constexpr int EW = (PW - 1) * IS + TX;
    static constexpr int NU = PB * EH * EW;                 // floats of one U channel plane
    static constexpr int USLOT = (NU + 63) / 64;            // staging instructions per U plane
    static constexpr int UPL = USLOT * 64 + 1;              // odd plane pitch
    static constexpr int NPIX = PB * PH * PW;               // 64
    static constexpr int VPL = NPIX + 1;
    static constexpr int WU = UT / 32, WV = VT / 32;
    static constexpr int SC = PB * (UT + VT);               // scale rows: [pb][UT] then [pb][VT]
    static constexpr int SC_ITEMS = (SC + THREADS - 1) / THREADS;   // one float per thread per item
    static constexpr int OFF_V = UT * UPL;
    static constexpr int OFF_S = OFF_V + VT * VPL;
    static constexpr int BUF = ((OFF_S + SC_ITEMS * THREADS + 3) / 4) * 4;
    static constexpr int LDS_BYTES = 2 * BUF * 4;
    // staging items of ONE wave per stage: its U channels x slots, its V channels, the scale rows
    static constexpr int U_ITEMS = (UT / NWAVE) * USLOT, V_ITEMS = VT / NWAVE;
    static constexpr int ITEMS = U_ITEMS + V_ITEMS + SC_ITEMS;
    static constexpr int KSTEPS = NPIX / 2 / NG;            // pixel pairs per stage and group
#ifndef SR_WGRAD_LAG
#define SR_WGRAD_LAG 4
#endif
    static constexpr int LAG = SR_WGRAD_LAG;                // pixel pairs between a load and its LDS write
    static constexpr int PER_STEP = (ITEMS + (KSTEPS - LAG) - 1) / (KSTEPS - LAG);
    static_assert(PER_STEP * (KSTEPS - LAG) >= ITEMS, "staging must finish inside the stage");
};

template <int IS, int TY, int TX, int PW, int PH, int PB, int UT, int VT, int NG>
__global__ __launch_bounds__(256 * NG) void k_wgrad_mfma(const WgradParams p) {
    using G = WG<IS, TY, TX, PW, PH, PB, UT, VT, NG>;
    static_assert(G::WU * G::WV == 4, "4 waves per workgroup");
    static_assert(G::NPIX == 64, "one V plane = one staging instruction");
    static_assert(PW % 2 == 0, "pixel pairs run along x");
    extern __shared__ __attribute__((aligned(16))) float smem[];      // the ONLY LDS object

    const SrWgradTile wt = sr_wgrad_tile(blockIdx.x, p.tiles_u, p.tiles_v, UT, VT);
    const int slice = wt.slice, u0 = wt.u0, v0 = wt.v0;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int grp = wave >> 2, w4 = wave & 3;            // group = which rows of the patch
    const int wu = w4 / G::WV, wv = w4 % G::WV;
    const int a_base = (wu * 32 + l31) * G::UPL + half * IS + grp * G::PHG * IS * G::EW;
    const int b_base = G::OFF_V + (wv * 32 + l31) * G::VPL + half + grp * G::PHG * PW;

    const int npatch = p.tiles_x * p.tiles_y * p.tiles_b;
    const int first = slice * p.patches_per_slice;
    int last = first + p.patches_per_slice;
    if (last > npatch) last = npatch;
    const int plane_u = p.UH * p.UW, plane_v = p.GH * p.GW;

    // ---- per-lane, patch-invariant decode of the staging slots
    int u_r[G::USLOT], u_c[G::USLOT], u_pb[G::USLOT];      // window row / col / sample of slot float
#pragma unroll
    for (int s = 0; s < G::USLOT; ++s) {
        const int f = s * 64 + lane;
        u_c[s] = f % G::EW;
        u_r[s] = (f / G::EW) % G::EH;
        u_pb[s] = (f < G::NU) ? f / (G::EW * G::EH) : -1;
    }
    const int v_px = lane % PW, v_py = (lane / PW) % PH, v_pb = lane / (PW * PH);
    // LDS write bases of this lane (channel `wave`, slot 0); items add immediates
    const int uw_base = wave * G::UPL + lane;
    const int vw_base = G::OFF_V + wave * G::VPL + lane;

    // ---- per-patch state, refreshed by prepare(): clamped per-lane offsets + validity
    int u_off[G::USLOT];
    bool u_ok[G::USLOT];
    int v_off;
    bool v_ok;
    int pat_b0 = 0;
    auto prepare = [&](int patch) {
        const SrWgradPatch pt = sr_wgrad_patch(patch, p.tiles_x, p.tiles_y);
        const int gy0 = pt.ty * PH, gx0 = pt.tx * PW, b0 = pt.b * PB;
        const int iy0 = gy0 * IS + p.dy0, ix0 = gx0 * IS + p.dx0;
        pat_b0 = b0;
#pragma unroll
        for (int s = 0; s < G::USLOT; ++s) {
            const int gy = iy0 + u_r[s], gx = ix0 + u_c[s], b = b0 + u_pb[s];
            u_ok[s] = u_pb[s] >= 0 && b < p.B && gy >= 0 && gy < p.UH && gx >= 0 && gx < p.UW;
            u_off[s] = u_ok[s] ? (b * p.CU) * plane_u + gy * p.UW + gx : 0;
        }
        const int gy = gy0 + v_py, gx = gx0 + v_px, b = b0 + v_pb;
        v_ok = b < p.B && gy < p.GH && gx < p.GW;
        v_off = v_ok ? (b * p.CV) * plane_v + gy * p.GW + gx : 0;
    };

    // Staging item k of this wave (k is a compile-time constant wherever these are called):
    //   k <  U_ITEMS            : U channel wave + 4*(k / USLOT), slot k % USLOT
    //   k <  U_ITEMS + V_ITEMS  : V channel wave + 4*(k - U_ITEMS)
    //   else                    : 256 floats of the scale rows (one per thread)
    // Every load is unconditional: the address is a wave-uniform channel base (SGPR) plus a
    // clamped per-lane offset; masks are applied when the value is written to LDS.
    auto item_load = [&](int k) -> float {
        if (k < G::U_ITEMS) {
            const int cu = k / G::USLOT, s = k % G::USLOT;
            const int u = min(u0 + wave + G::NWAVE * cu, p.CU - 1);
            return (p.U + (int64_t)u * plane_u)[u_off[s]];
        }
        if (k < G::U_ITEMS + G::V_ITEMS) {
            const int v = min(v0 + wave + G::NWAVE * (k - G::U_ITEMS), p.CV - 1);
            return (p.V + (int64_t)v * plane_v)[v_off];
        }
        const int e = (k - G::U_ITEMS - G::V_ITEMS) * G::THREADS + tid;
        float val = 1.0f;
        if (e < PB * UT) {
            const int pb = e / UT, u = e % UT;
            if (p.uscale && pat_b0 + pb < p.B && u0 + u < p.CU) val = p.uscale[(int64_t)(pat_b0 + pb) * p.CU + u0 + u];
        } else if (e < G::SC) {
            const int pb = (e - PB * UT) / VT, v = (e - PB * UT) % VT;
            if (p.vscale && pat_b0 + pb < p.B && v0 + v < p.CV) val = p.vscale[(int64_t)(pat_b0 + pb) * p.CV + v0 + v];
        }
        return val;
    };
    auto item_store = [&](int k, float val, float* dst) {
        if (k < G::U_ITEMS) {
            const int cu = k / G::USLOT, s = k % G::USLOT;
            const bool ok = u_ok[s] && (u0 + wave + G::NWAVE * cu < p.CU);
            dst[uw_base + G::NWAVE * cu * G::UPL + s * 64] = ok ? val : 0.0f;
        } else if (k < G::U_ITEMS + G::V_ITEMS) {
            const int cv = k - G::U_ITEMS;
            const bool ok = v_ok && (v0 + wave + G::NWAVE * cv < p.CV);
            dst[vw_base + G::NWAVE * cv * G::VPL] = ok ? val : 0.0f;
        } else {
            dst[G::OFF_S + (k - G::U_ITEMS - G::V_ITEMS) * G::THREADS + tid] = val;
        }
    };

    f32x16 acc[G::NT];
#pragma unroll
    for (int t = 0; t < G::NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    if (first < last) {
        // first patch of the slice: straight load -> write, eight items at a time
        prepare(first);
#pragma unroll
        for (int k0 = 0; k0 < G::ITEMS; k0 += 8) {
            float t8[8];
#pragma unroll
            for (int d = 0; d < 8; ++d)
                if (k0 + d < G::ITEMS) t8[d] = item_load(k0 + d);
#pragma unroll
            for (int d = 0; d < 8; ++d)
                if (k0 + d < G::ITEMS) item_store(k0 + d, t8[d], smem);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    int buf = 0;
    float stg[G::ITEMS];         // staged values; live ranges span LAG pixel pairs (~a dozen registers)
    for (int patch = first; patch < last; ++patch) {
        __syncthreads();     // buffer `buf` completely written; the other buffer no longer read
        // the staging stream is branch-free (a per-step branch makes the compiler's vmcnt
        // bookkeeping conservative and collapses the pipeline): after the last patch it simply
        // re-stages that patch into the idle buffer
        prepare(patch + 1 < last ? patch + 1 : patch);
        const float* sb = smem + buf * G::BUF;
        float* so = smem + (buf ^ 1) * G::BUF;
        float a_sc[PB], b_sc[PB];
#pragma unroll
        for (int pb = 0; pb < PB; ++pb) {
            a_sc[pb] = sb[G::OFF_S + pb * UT + wu * 32 + l31];
            b_sc[pb] = sb[G::OFF_S + PB * UT + pb * VT + wv * 32 + l31];
        }
        // MFMA operands are register double-buffered: the ds_reads of pixel pair s+1 are issued
        // BEFORE the MFMA block of pair s (one wave per SIMD: nobody else would hide the LDS
        // latency), and multiplied by the modulation scales at the top of the next iteration.
        float a_raw[G::NT], b_raw;
        auto fetch_operands = [&](int step) {
            const int qx = step % (PW / 2), py = (step / (PW / 2)) % G::PHG, pb = step / ((PW / 2) * G::PHG);
            b_raw = sb[b_base + (pb * PH + py) * PW + 2 * qx];
            const int ua = a_base + (pb * G::EH + py * IS) * G::EW + 2 * qx * IS;
#pragma unroll
            for (int ty = 0; ty < TY; ++ty)
#pragma unroll
                for (int tx = 0; tx < TX; ++tx) a_raw[ty * TX + tx] = sb[ua + ty * G::EW + tx];
        };
        fetch_operands(0);
#pragma unroll
        for (int step = 0; step < G::KSTEPS; ++step) {
            // next patch: PER_STEP loads per pixel pair, written to the other LDS buffer LAG pixel
            // pairs later — all in the MFMA shadow
#ifndef SR_ABL_W_NODMA
#pragma unroll
            for (int d = 0; d < G::PER_STEP; ++d) {
                const int k = step * G::PER_STEP + d;
                if (k < G::ITEMS) stg[k] = item_load(k);
                const int w = (step - G::LAG) * G::PER_STEP + d;
                if (w >= 0 && w < G::ITEMS) item_store(w, stg[w], so);
            }
#endif
            const int pb = step / ((PW / 2) * G::PHG);
            const float bv = b_raw * b_sc[pb];
            float av[G::NT];
#pragma unroll
            for (int t = 0; t < G::NT; ++t) av[t] = a_raw[t] * a_sc[pb];
            if (step + 1 < G::KSTEPS) fetch_operands(step + 1);
            __builtin_amdgcn_sched_barrier(0);      // the reads go out BEFORE the MFMA block
#pragma unroll
            for (int t = 0; t < G::NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv, acc[t], 0, 0, 0);
            // keep the software pipeline as written (the scheduler would otherwise hoist every
            // staging load to the top of the stage)
            __builtin_amdgcn_sched_barrier(0);
        }
        buf ^= 1;
    }

    // partial[slice][tap][u][v]; C/D layout: column (v) = lane & 31, row (u) = (r&3) + 8*(r>>2) + 4*half
    float* dst = p.partial + ((int64_t)slice * NG + grp) * G::NT * p.UP * p.VP;
#pragma unroll
    for (int t = 0; t < G::NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int u = sr_mfma32_row(r, half, u0 + wu * 32);
            const int v = v0 + wv * 32 + l31;
            dst[((int64_t)t * p.UP + u) * p.VP + v] = acc[t][r];
        }
}

template <int IS, int TY, int TX, int PW, int PH, int PB, int UT, int VT>
int launch_wgrad_one(const WgradParams& p, dim3 grid, hipStream_t st) {
    constexpr int NG = sr_wgrad_groups(PB);
    using G = WG<IS, TY, TX, PW, PH, PB, UT, VT, NG>;
    static_assert(G::LDS_BYTES <= 160 * 1024, "LDS budget");
    constexpr auto kern = k_wgrad_mfma<IS, TY, TX, PW, PH, PB, UT, VT, NG>;
    if (!sr_allow_dynamic_lds<kern>(G::LDS_BYTES)) return SR_EINVAL;
    hipLaunchKernelGGL(kern, grid, dim3(G::THREADS), G::LDS_BYTES, st, p);
    return sr_launch_status();
}

template <int TY, int TX>
int launch_wgrad_s1(const WgradParams& p, const SrWgradTiles& pl, dim3 grid, hipStream_t st) {
    if (pl.pw == 32) return launch_wgrad_one<1, TY, TX, 32, 2, 1, 64, 64>(p, grid, st);
    if (pl.pw == 16) return launch_wgrad_one<1, TY, TX, 16, 4, 1, 64, 64>(p, grid, st);
    if (pl.pw == 8) return launch_wgrad_one<1, TY, TX, 8, 8, 1, 64, 64>(p, grid, st);
    return launch_wgrad_one<1, TY, TX, 4, 4, 4, 64, 64>(p, grid, st);
}

template <int TY, int TX>
int launch_wgrad_s2(const WgradParams& p, const SrWgradTiles& pl, dim3 grid, hipStream_t st) {
    if (pl.pw == 16) return launch_wgrad_one<2, TY, TX, 16, 4, 1, 32, 128>(p, grid, st);
    return launch_wgrad_one<2, TY, TX, 8, 8, 1, 32, 128>(p, grid, st);
}

}  // namespace

SrWgradTiles sr_wgrad_tiles(int stride, int B, int CU, int CV, int GH, int GW) {
    SrWgradTiles pl;
    if (stride == 1) {
        if (GW > 16) { pl.pw = 32; pl.ph = 2; pl.pb = 1; }
        else if (GW > 8) { pl.pw = 16; pl.ph = 4; pl.pb = 1; }
        else if (GW > 4) { pl.pw = 8; pl.ph = 8; pl.pb = 1; }
        else { pl.pw = 4; pl.ph = 4; pl.pb = 4; }
        pl.ut = 64; pl.vt = 64;
    } else {
        // the stride-2 window patch is 4x larger: narrower U tile, and never more than 5 DMA
        // slots per plane
        if (GW > 8) { pl.pw = 16; pl.ph = 4; pl.pb = 1; }
        else { pl.pw = 8; pl.ph = 8; pl.pb = 1; }
        pl.ut = 32; pl.vt = 128;
    }
    pl.tiles_x = (GW + pl.pw - 1) / pl.pw;
    pl.tiles_y = (GH + pl.ph - 1) / pl.ph;
    pl.tiles_b = (B + pl.pb - 1) / pl.pb;
    pl.tiles_u = (CU + pl.ut - 1) / pl.ut;
    pl.tiles_v = (CV + pl.vt - 1) / pl.vt;
    const int npatch = pl.tiles_x * pl.tiles_y * pl.tiles_b;
    const int tiles_uv = pl.tiles_u * pl.tiles_v;
    // one 512-thread workgroup per CU (two 256-thread ones for the multi-sample patch type)
    const int target = (pl.pb == 1 ? 1 : 2) * SR_NUM_CU;
    int ks = (target + tiles_uv - 1) / tiles_uv;
    if (ks > npatch) ks = npatch;
    if (ks < 1) ks = 1;
    pl.pps = (npatch + ks - 1) / ks;
    pl.ks = (npatch + pl.pps - 1) / pl.pps;
    return pl;
}

int64_t sr_wgrad_direct_floats(const SrWgradTiles& t, int ksize) {
    return (int64_t)t.ks * sr_wgrad_groups(t.pb) * ksize * ksize * (t.tiles_u * t.ut) * (int64_t)(t.tiles_v * t.vt) + 4;
}

WgradParams sr_wgrad_params(const float* U, const float* V, const float* uscale, const float* vscale, float* partial,
                            int64_t B, int CU, int CV, int UH, int UW, int GH, int GW, int d0, const SrWgradTiles& t) {
    WgradParams p;
    p.U = U; p.V = V; p.uscale = uscale; p.vscale = vscale;
    p.partial = partial;
    p.B = (int)B; p.CU = CU; p.CV = CV; p.UH = UH; p.UW = UW; p.GH = GH; p.GW = GW;
    p.dy0 = p.dx0 = d0;
    p.tiles_x = t.tiles_x; p.tiles_y = t.tiles_y; p.tiles_b = t.tiles_b;
    p.tiles_u = t.tiles_u; p.tiles_v = t.tiles_v; p.ks = t.ks; p.patches_per_slice = t.pps;
    p.UP = t.tiles_u * t.ut; p.VP = t.tiles_v * t.vt;
    return p;
}

int sr_wgrad_direct_launch(const WgradParams& p, const SrWgradTiles& t, int ksize, int stride, hipStream_t st) {
    if (p.B == 0) return SR_OK;
    const dim3 grid((unsigned)(t.tiles_u * t.tiles_v * t.ks));
    if (ksize == 3 && stride == 1) return launch_wgrad_s1<3, 3>(p, t, grid, st);
    if (ksize == 3 && stride == 2) return launch_wgrad_s2<3, 3>(p, t, grid, st);
    if (ksize == 1 && stride == 1) return launch_wgrad_s1<1, 1>(p, t, grid, st);
    return launch_wgrad_s2<1, 1>(p, t, grid, st);
}
