// Weight-gradient dispatch of the dense convolutions: which kernel serves a call is decided ONCE, by make_wgrad_plan
// (DESIGN.md 4.0 has the table), and the C entry points sr_conv2d_wgrad_scratch_floats, sr_conv2d_wgrad_path_floats,
// sr_conv2d_wgrad_path and sr_conv2d_wgrad_mfma size, report and launch from that plan.  Host code only: every path
// lives in its own file behind an *_eligible / *_floats / *_launch header, and nothing is launched from here directly.
#include "common.h"
#include "conv_split_bf16.h"
#include "conv_wgrad_bf16x3.h"
#include "conv_wgrad_mfma.h"
#include "conv_wgrad_reduce.h"
#include "conv_wgrad_s2_dma.h"
#include "conv_wgrad_s2_wino.h"
#include "conv_wgrad_small3.h"
#include "conv_wgrad_wino.h"
#include "conv_wino.h"
#include "wgrad_style_finish.h"

#include <algorithm>
#include <cstdlib>

namespace {

// One weight-gradient call as the dispatch sees it: the shape and, for the alignment rules, the buffers (NULL =
// alignment unknown, assume aligned).  wgrad_call() derives the kernels' view: U is the operand read through the tap
// window, V the one on the base grid G; a regular convolution has (U, V) = (x, gy), the transposed one (gy, x).
struct WgradCall {
    int64_t B, C, N, IH, IW, OH, OW;
    int ksize, stride, pad, transposed;
    const void *x, *gy;
    int GH = 0, GW = 0, UH = 0, UW = 0, CU = 0, CV = 0, d0 = 0;
    bool valid = false;     // one of the geometries the kernels serve (SR_EINVAL otherwise)
    bool is3x3(int s, int pd) const { return ksize == 3 && stride == s && pad == pd; }
    bool derive() {
        if (B < 0 || C <= 0 || N <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return false;
        if (!(ksize == 3 || ksize == 1) || !(stride == 1 || stride == 2)) return false;
        if (!transposed) {
            if (OH != (IH + 2 * pad - ksize) / stride + 1 || OW != (IW + 2 * pad - ksize) / stride + 1) return false;
            GH = (int)OH; GW = (int)OW; UH = (int)IH; UW = (int)IW; CU = (int)C; CV = (int)N; d0 = -pad;
        } else {
            if (!is3x3(2, 0) || OH != 2 * IH + 1 || OW != 2 * IW + 1) return false;
            GH = (int)IH; GW = (int)IW; UH = (int)OH; UW = (int)OW; CU = (int)N; CV = (int)C; d0 = 0;
        }
        return true;
    }
};

// k_wgrad_s2p takes an eligible stride-2 call from this much direct work on, 18 B CU CV GH GW: measured (DESIGN.md 4.2h,
// profiles/s2wgrad_wino_notes.md) a tie at 4.83e9 and 5 - 8 % ahead at 7.25e9; below, its longer prologue per slice loses.
// Must stay above 3.63e9: tests pin k_wgrad_s2_dma's results bit for bit up to (3, 64 -> 256, 129^2) = 3.62e9.
constexpr double SR_WGRAD_S2_WINO_MIN_WORK = 6.0e9;
static_assert(SR_WGRAD_S2_WINO_MIN_WORK > 3.63e9, "k_wgrad_s2_dma keeps the shapes the tests pin bit for bit");

struct WgradPlan {
    int path = SR_WGRAD_PATH_INVALID;
    int64_t sized = -1;                      // sr_conv2d_wgrad_scratch_floats of the call
    int64_t needs = -1;                      // sr_conv2d_wgrad_path_floats: what the chosen path writes, <= sized
    SrWgradTiles tiles = {};                 // tiling and K slices of k_wgrad_mfma / k_wgrad_s2_dma / k_wgrad_s2p
};

// THE path list: every path goes through candidate(), in priority order; the first one taken serves the call.
//   reach   the SHAPE can get here: with some buffer alignment, and below or above a launch-size bar.  SR_WGRAD_SMALL,
//           SR_WINOGRAD and SR_CONV_SPLIT_BF16 count as they stand; SR_WGRAD_S2_WINO and SR_WGRAD_DMA move no size.
//           `sized` is the largest `floats` within reach,
//   take    THIS call takes it (its buffers, the switches now) unless an earlier candidate did
//   floats  what the path writes to the scratch
// (the *_floats of a path are asked only within its reach: outside it some are undefined)
WgradPlan make_wgrad_plan(const WgradCall& c) {
    WgradPlan w;
    if (!c.valid) return w;
    const int64_t B = c.B, C = c.C, N = c.N, IH = c.IH, IW = c.IW;
    auto candidate = [&](int path, bool reach, bool take, int64_t floats) {
        if (!reach) return;
        w.sized = std::max(w.sized, floats);
        if (w.path != SR_WGRAD_PATH_INVALID || !take) return;
        w.path = path; w.needs = floats;
    };
    // the streaming kernel takes every call of its shape: nothing else is in reach there, the direct kernel included
    const bool small = sr_wgrad_small3_eligible(C, N, c.ksize, c.stride, c.pad, c.transposed);
    candidate(SR_WGRAD_PATH_SMALL3, small, true, small ? sr_wgrad_small3_floats(B, IH, IW) : 0);
    if (small) return w;
    const SrWgradTiles& pl = w.tiles = sr_wgrad_tiles(c.stride, (int)B, c.CU, c.CV, c.GH, c.GW);
    const int64_t direct = sr_wgrad_direct_floats(pl, c.ksize);
    if (!c.transposed && c.is3x3(1, 1)) {
        const bool reach = sr_winograd_enabled() && sr_wgrad_wino_eligible(B, C, N, IH, IW, nullptr, nullptr);
        candidate(SR_WGRAD_PATH_WINO, reach, sr_wgrad_wino_eligible(B, C, N, IH, IW, c.x, c.gy),
                  reach ? sr_wgrad_wino_scratch_floats(B, C, N, IH, IW) : 0);
    } else if (!c.transposed && c.ksize == 1 && c.stride == 1) {
        // opt-in spike (SR_CONV_SPLIT_BF16=1): split-bf16 matrix paths, same partial-slab layout and reduce
        candidate(SR_WGRAD_PATH_BF16_1X1, sr_wgrad_bf16x3_enabled('w'),
                  c.pad == 0 && B > 0 && sr_wgrad_bf16x3_eligible(B, C, N, IH * IW, c.x, c.gy),
                  sr_wgrad_bf16x3_scratch_floats(B, C, N, IH * IW));
    } else if (c.ksize == 3 && c.stride == 2) {
        candidate(SR_WGRAD_PATH_BF16_S2, sr_wgrad_bf16x3_enabled('g'),
                  c.pad == 0 && sr_wgrad_s2_bf16x3_eligible(B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, c.transposed ? c.x : c.gy),
                  sr_wgrad_s2_bf16x3_scratch_floats(B, c.CU, c.CV, c.GH, c.GW));
        // The polyphase 25-product kernel walks the direct plan's K slices and writes ONE slab of 16 positions per slice
        // where the direct kernels write two of 9: ks * 16 <= ks * 18, so it adds nothing to `sized` (stated, and checked
        // here: callers size their buffers from the direct plan).  SR_WGRAD_S2_WINO: 0 never, force ignores the work bar.
        const bool s2p = sr_wgrad_s2_wino_eligible(B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, c.d0);
        const int sw = sr_env_char("SR_WGRAD_S2_WINO");
        const double work = 18.0 * (double)B * c.CU * c.CV * c.GH * c.GW;
        const int64_t floats = sr_wgrad_s2_wino_scratch_floats(pl.ks, c.CU, c.CV);
        if (s2p && floats > std::max(w.sized, direct)) std::abort();     // one 16-position slab per slice always fits
        candidate(SR_WGRAD_PATH_S2_WINO, s2p, sw != '0' && (sw == 'f' || work >= SR_WGRAD_S2_WINO_MIN_WORK), floats);
        // the direct kernel's tiling, slabs and bits with LDS-DMA staging: its scratch is the direct figure
        candidate(SR_WGRAD_PATH_S2_DMA, true,
                  sr_wgrad_s2_dma_eligible(pl, B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, c.d0), direct);
    }
    candidate(SR_WGRAD_PATH_DIRECT, true, true, direct);        // the fallback: takes what nobody else does
    return w;
}

// Style gradient from the per-sample slabs (wgrad_style_finish.h): the two transform-domain paths, where
// the plan the call takes anyway cuts K into whole slices per sample.  Nothing is re-planned: a call whose slices
// straddle samples keeps the plain finish and the caller its row-dot pass.
struct StylePlan {
    int sps = 0;                 // whole K slices per sample; 0: not on this path
    int64_t part = -1;           // floats of the style-gradient partials
};
StylePlan make_style_plan(const WgradCall& c, const WgradPlan& w) {
    StylePlan s;
    if (c.B <= 0 || c.B > SR_STYLE_FINISH_MAX_B) return s;
    if (w.path == SR_WGRAD_PATH_WINO) {
        s.sps = sr_wgrad_wino_slices_per_sample(c.B, c.C, c.N, c.IH, c.IW);
        if (s.sps > 0) s.part = sr_wgrad_style_part_floats(c.B, c.C, c.N, false);
    } else if (w.path == SR_WGRAD_PATH_S2_WINO && c.transposed) {
        // one sample per patch row of the plan (pb = 1): sample b owns patches [b * per, (b + 1) * per)
        const SrWgradTiles& pl = w.tiles;
        const int per = pl.tiles_x * pl.tiles_y;
        if (pl.pb == 1 && per % pl.pps == 0 && (int64_t)pl.ks * pl.pps == (int64_t)per * c.B) {
            s.sps = per / pl.pps;
            s.part = sr_wgrad_style_part_floats(c.B, c.CU, c.CV, true);
        }
    }
    return s;
}

WgradCall wgrad_call(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize, int stride,
                     int pad, int transposed, const void* x, const void* gy) {
    WgradCall c{B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, x, gy};
    c.valid = c.derive();
    return c;
}

}  // namespace

extern "C" int64_t sr_conv2d_wgrad_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t IH,
                                                  int64_t IW, int64_t OH, int64_t OW, int ksize,
                                                  int stride, int pad, int transposed) {
    return make_wgrad_plan(wgrad_call(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, nullptr, nullptr)).sized;
}

extern "C" int64_t sr_conv2d_wgrad_path_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH,
                                               int64_t OW, int ksize, int stride, int pad, int transposed, const float* x,
                                               const float* gy) {
    return make_wgrad_plan(wgrad_call(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, x, gy)).needs;
}

extern "C" int sr_conv2d_wgrad_path(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                                    int ksize, int stride, int pad, int transposed, const float* x, const float* gy) {
    return make_wgrad_plan(wgrad_call(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, x, gy)).path;
}

extern "C" int sr_conv2d_wgrad_mfma(float* dwt, const float* x, const float* gy, const float* xscale,
                                    const float* gscale, int64_t B, int64_t C, int64_t N, int64_t IH,
                                    int64_t IW, int64_t OH, int64_t OW, int ksize, int stride, int pad,
                                    int transposed, float* scratch, sr_stream_t stream) {
    const WgradCall c = wgrad_call(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, x, gy);
    const WgradPlan w = make_wgrad_plan(c);
    if (w.path == SR_WGRAD_PATH_INVALID) return SR_EINVAL;
    if (!dwt || !x || !gy || !scratch) return SR_EINVAL;
    if (B * C * IH * IW >= (1LL << 31) || B * N * OH * OW >= (1LL << 31)) return SR_ERANGE;
    hipStream_t st = sr_stream(stream);
    // U / V and their scales
    const float *U = transposed ? gy : x, *V = transposed ? x : gy;
    const float *uscale = transposed ? gscale : xscale, *vscale = transposed ? xscale : gscale;
    // dwt is [taps][C][N]: a regular convolution has (u, v) = (c, n), the transposed one (u, v) = (n, c)
    const WgradOut out{dwt, (int64_t)c.CU * c.CV, transposed ? 1 : c.CV, transposed ? c.CU : 1};
    const SrWgradTiles& pl = w.tiles;
    int ks = 0, UP = 0, VP = 0, rc = SR_OK;
    switch (w.path) {
    case SR_WGRAD_PATH_SMALL3:
        return sr_wgrad_small3_launch(dwt, x, gy, xscale, gscale, B, C, N, IH, IW, scratch, st);
    case SR_WGRAD_PATH_WINO:
        return sr_wgrad_wino_launch(dwt, x, gy, xscale, gscale, B, C, N, IH, IW, scratch, st);
    case SR_WGRAD_PATH_BF16_1X1:
        rc = sr_wgrad_bf16x3_launch(x, gy, xscale, gscale, scratch, B, C, N, IH * IW, &ks, &UP, &VP, st);
        return rc != SR_OK ? rc : sr_wgrad_reduce_launch(out, scratch, ks, 1, UP, VP, c.CU, c.CV, st);
    case SR_WGRAD_PATH_BF16_S2:
        rc = sr_wgrad_s2_bf16x3_launch(U, V, uscale, vscale, scratch, B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, &ks, &UP, &VP, st);
        return rc != SR_OK ? rc : sr_wgrad_reduce_launch(out, scratch, ks, 9, UP, VP, c.CU, c.CV, st);
    case SR_WGRAD_PATH_S2_WINO:
        rc = sr_wgrad_s2_wino_launch(U, V, uscale, vscale, scratch, B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, pl.ks, pl.pps, st);
        return rc != SR_OK ? rc : sr_wgrad_s2_wino_finish(out, scratch, pl.ks, c.CU, c.CV, st);
    default: {  // SR_WGRAD_PATH_S2_DMA, SR_WGRAD_PATH_DIRECT: one kernel argument, one slab per slice and group
        const WgradParams p = sr_wgrad_params(U, V, uscale, vscale, scratch, B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, c.d0, pl);
        rc = w.path == SR_WGRAD_PATH_S2_DMA ? sr_wgrad_s2_dma_launch(p, pl, st) : sr_wgrad_direct_launch(p, pl, ksize, stride, st);
        if (rc != SR_OK) return rc;
        return sr_wgrad_reduce_launch(out, scratch, B > 0 ? pl.ks * sr_wgrad_groups(pl.pb) : 0, ksize * ksize, p.UP, p.VP, c.CU,
                                      c.CV, st);
    }
    }
}

extern "C" int64_t sr_conv2d_wgrad_style_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH,
                                                int64_t OW, int ksize, int stride, int pad, int transposed, const float* x,
                                                const float* gy) {
    const WgradCall c = wgrad_call(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, x, gy);
    return make_style_plan(c, make_wgrad_plan(c)).part;
}

extern "C" int sr_conv2d_wgrad_style(float* dwt, float* gis, const float* x, const float* gy, const float* iscale,
                                     const float* gscale, const float* wt, int64_t ldw, int64_t B, int64_t C, int64_t N,
                                     int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize, int stride, int pad,
                                     int transposed, float* scratch, float* part, sr_stream_t stream) {
    const WgradCall c = wgrad_call(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, x, gy);
    const WgradPlan w = make_wgrad_plan(c);
    const StylePlan s = make_style_plan(c, w);
    if (s.sps <= 0) return SR_EINVAL;
    if (!dwt || !gis || !x || !gy || !iscale || !wt || !scratch || !part || ldw < N) return SR_EINVAL;
    if (B * C * IH * IW >= (1LL << 31) || B * N * OH * OW >= (1LL << 31)) return SR_ERANGE;
    hipStream_t st = sr_stream(stream);
    if (w.path == SR_WGRAD_PATH_WINO)
        return sr_wgrad_wino_style_launch(dwt, gis, x, gy, iscale, gscale, wt, ldw, B, C, N, IH, IW, scratch, part, st);
    // SR_WGRAD_PATH_S2_WINO, transposed: U = gy with the demodulation, V = x WITHOUT the style (it enters in the finish)
    const SrWgradTiles& pl = w.tiles;
    const int rc = sr_wgrad_s2_wino_launch(gy, x, gscale, nullptr, scratch, B, c.CU, c.CV, c.UH, c.UW, c.GH, c.GW, pl.ks, pl.pps, st);
    return rc != SR_OK ? rc : sr_wgrad_s2_wino_style_finish(dwt, gis, scratch, iscale, wt, ldw, s.sps, B, c.CU, c.CV, part, st);
}
