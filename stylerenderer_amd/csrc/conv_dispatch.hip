// Forward dispatch of the dense convolutions: which kernel serves a call is decided ONCE, by make_conv_plan (DESIGN.md
// 4.0 has the table), and the C entry points sr_conv2d_mfma[_ex] / sr_conv2d_nba[_ex] and the path, scratch and Winograd
// queries size, report and launch from that plan.  Host code only: every path lives in its own file behind an
// *_eligible / *_launch header, and nothing is launched from here directly.
#include "common.h"
#include "conv1x1_gemm.h"
#include "conv_mfma.h"
#include "conv_s2_bf16x3.h"
#include "conv_s2_wino.h"
#include "conv_split_bf16.h"
#include "conv_wino.h"
#include "convt_fused.h"
#include "convt_wino.h"

#include <algorithm>

namespace {

// One dense-convolution call as the dispatch sees it: the shape and, for the alignment rules, the buffers.  A NULL
// buffer means "alignment unknown, assume aligned" (as the *_eligible functions of the other files treat it).
struct ConvCall {
    int64_t B, C, N, IH, IW, OH, OW;
    int ksize, stride, pad, transposed;
    const void *in, *out, *wt;
    int64_t ldw;
    bool is3x3(int s, int pd) const { return ksize == 3 && stride == s && pad == pd; }
};

// Polyphase 25-product form of the non-transposed stride-2 3x3 convolution (csrc/conv_s2_wino.hip).
// The kernel has no K slices: launches with fewer workgroups stay on k_conv_mfma, whose split-K serves them (the
// threshold k_convt_fused uses for the same reason; measurements in DESIGN.md 4.1y).
constexpr int64_t S2_WINO_MIN_BLOCKS = 192;

bool convt_interior(int path) {
    return path == SR_CONV_PATH_CONVT_BF16 || path == SR_CONV_PATH_CONVT_WINO || path == SR_CONV_PATH_CONVT_FUSED_KS ||
           path == SR_CONV_PATH_CONVT_FUSED;
}

// 25-product form of the transposed stride-2 3x3 convolution's interior (csrc/convt_wino.hip).  The kernel has no K
// slices, so the bar is on the direct flops 18 B C N IH IW of the launch: smaller launches keep k_convt_fused, its K
// slices and the tap-split form.  Floor: the row ("t3s2", (8, 512, 512, 32, 32)) of tests/conv_plan_cases.py (3.87e10) is
// launched by the GPU suite as a k_convt_fused shape and stays there.  Measured, the new kernel is ahead on every row from
// 1.93e10 up (0.67 .. 0.86 of k_convt_fused's time), so the bar sits just above its floor; the generator's
// launches at batch 16 start at 7.73e10.
constexpr double CONVT_WINO_MIN_FLOPS = 4.0e10;
static_assert(CONVT_WINO_MIN_FLOPS > 18.0 * 8 * 512 * 512 * 32 * 32, "the t3s2 row of tests/conv_plan_cases.py stays on k_convt_fused");

struct ConvPlan {
    int path = SR_CONV_PATH_DIRECT; // the direct kernel (per-phase launches when transposed) takes what nobody else does
    bool strips = false;            // transposed: sr_convt_strips_launch follows the interior kernel
    int ks = 1, c_per_slice = 0;    // K slices of the fused / tap-split launch (c_per_slice: tap-split only)
    bool taps_gemm = false;         // tap-split in its flattened-pixel GEMM form
    int64_t floats = 0;             // scratch of the chosen path (direct: what its split-K would use)
    int64_t sized = 0;              // sr_conv2d_scratch_floats of the call
    int code() const { return path | (strips ? SR_CONV_PATH_STRIPS : 0); }
};

// THE path list: every path of a call's geometry goes through candidate(), in priority order.
//   reach   the SHAPE can get here: with some buffer alignment, below or above a launch-size bar, and with the on / off
//           switches (SR_CONV_S2_WINO, SR_CONVT_WINO, SR_CONVT_FUSED, SR_CONVT_FUSED_KS, SR_CONVT_STRIPS, SR_CONV1X1_GEMM) in either
//           position — they are read per call, the scratch may be sized before one flips.  SR_WINOGRAD, SR_CONVT_TAPS and
//           SR_CONV_SPLIT_BF16 count as they stand.  `sized` is the largest `floats` within reach,
//   take    THIS call takes it (its buffers, the switches now) unless an earlier candidate did
//   floats  scratch the path cannot run without — so with a scratch (of `sized` floats: the interface has no other
//           size) whatever is taken fits, and without one only paths that need none are taken
ConvPlan make_conv_plan(const ConvCall& c, bool have_scratch) {
    ConvPlan plan;
    const int64_t B = c.B, C = c.C, N = c.N, IH = c.IH, IW = c.IW, OH = c.OH, OW = c.OW;
    if (B <= 0 || C <= 0 || N <= 0 || OH <= 0 || OW <= 0) return plan;
    plan.sized = plan.floats = sr_conv_direct_floats(B, C, N, IH, IW, OH, OW, c.transposed);
    auto candidate = [&](int path, bool reach, bool take, int64_t floats, int ks = 1) {
        if (!reach) return;
        plan.sized = std::max(plan.sized, floats);
        if (plan.path != SR_CONV_PATH_DIRECT || !take || (floats > 0 && !have_scratch)) return;
        plan.path = path; plan.floats = floats; plan.ks = ks;
    };
    if (!c.transposed && c.is3x3(1, 1)) {
        if (sr_winograd_enabled() && sr_wino_eligible(B, C, N, IH, IW, nullptr, nullptr))
            candidate(SR_CONV_PATH_WINO, true, sr_wino_eligible(B, C, N, IH, IW, c.in, c.out),
                      sr_wino_scratch_floats(C, N) + sr_wino_partial_floats(B, C, N, IH, IW));
    } else if (!c.transposed && c.is3x3(2, 0)) {
        // opt-in spike (SR_CONV_SPLIT_BF16=1): split-bf16 matrix path for the down-sampling convolution and the data
        // gradient of the up-sampling one
        candidate(SR_CONV_PATH_S2_BF16, sr_wgrad_bf16x3_enabled('c') && sr_conv_s2_bf16x3_eligible(B, C, N, IH, IW, OH, OW),
                  true, sr_conv_s2_bf16x3_scratch_floats(C, N));
        const int sw = sr_env_char("SR_CONV_S2_WINO");      // =0 keeps k_conv_mfma, =force ignores the workgroup bar (tests)
        candidate(SR_CONV_PATH_S2_WINO, sr_conv_s2_wino_eligible(B, C, N, IH, IW, OH, OW, nullptr, nullptr),
                  sw != '0' && sr_conv_s2_wino_eligible(B, C, N, IH, IW, OH, OW, c.in, c.out) &&
                      (sw == 'f' || sr_conv_s2_wino_blocks(B, N, OH, OW) >= S2_WINO_MIN_BLOCKS),
                  sr_conv_s2_wino_scratch_floats(C, N));
    } else if (!c.transposed && c.ksize == 1 && c.stride == 1) {
        // no window: a plain GEMM with both operands K-major (csrc/conv1x1_gemm.hip) where its tiles fill the chip
        candidate(SR_CONV_PATH_GEMM1X1, true,
                  c.pad == 0 && sr_conv1x1_gemm_eligible(B, C, N, c.ldw, IH * IW, c.in, c.wt, c.out), 0);
    } else if (c.transposed && c.is3x3(2, 0)) {
        // opt-in spike (SR_CONV_SPLIT_BF16=1): the interior of the map on the bf16 matrix cores (three-way operand
        // split); it keeps the tap-split form out, the border stays on the exact-fp32 kernels
        const bool bf = sr_wgrad_bf16x3_enabled('t') && sr_convt_bf16x3_eligible(B, C, N, IH, IW);
        // SR_CONVT_WINO: =0 never takes k_convt_wino, =force takes it for any eligible size (tests), unset applies the
        // flop bar; SR_CONVT_FUSED=0 ("per-phase launches") keeps it out too
        const int sw = sr_env_char("SR_CONVT_FUSED"), wsw = sr_env_char("SR_CONVT_WINO");
        const bool wino_ok = sw != '0' && wsw != '0' && sr_convt_wino_eligible(B, C, N, IH, IW, c.ldw, c.in);
        const bool wino_forced = wino_ok && wsw == 'f' && !bf;
        // small problems: nine shifted 1x1 convolutions in one launch + one reduction (k_conv_mfma<..., TAP9>)
        if (sr_convt_taps_wanted(B, C, N, IH, IW)) {
            int ks;
            sr_convt_taps_plan((int)IH, (int)IW, (int)B, (int)N, (int)C, ks, plan.c_per_slice);
            candidate(SR_CONV_PATH_CONVT_TAPS, true, !bf && !wino_forced, (int64_t)ks * 9 * B * N * (IH + 1) * (IW + 1), ks);
        }
        candidate(SR_CONV_PATH_CONVT_BF16, bf, true, sr_convt_bf16x3_scratch_floats(C, N));
        // interior of the map in 25 of 36 products (k_convt_wino) for the large launches
        candidate(SR_CONV_PATH_CONVT_WINO, sr_convt_wino_eligible(B, C, N, IH, IW, c.ldw, nullptr),
                  wino_ok && (wsw == 'f' || 18.0 * (double)B * (double)C * (double)N * (double)IH * (double)IW >=
                                                CONVT_WINO_MIN_FLOPS), 0);
        // interior of the map: all four phases in one workgroup (k_convt_fused); SR_CONVT_FUSED=0 keeps the per-phase
        // launches, =1 takes it whatever the size
        const bool fused_ok = sw != '0' && IW >= 16 && sr_convt_fused_eligible(C, IH, IW, c.ldw, c.in);
        // the fused kernel has no split-K: when its workgroups cover less than ~3/4 of the CUs AND the channel loop is
        // long (C > 256: 64 chunks, ~0.38 ms whatever the batch), each one walks the whole loop alone and the per-phase
        // launches, which split K, are faster — in-graph, scripts/bench_convt_small.py: 32^2 512->512 at batch 1 / 2 / 4
        // 0.23 / 0.26 / 0.35 ms against 0.38 / 0.39 / 0.40 fused (batch 8: 0.56 against 0.43, fused stays);
        // 64^2 512->256 at batch 1 / 2 0.26 / 0.33 against 0.39; 128^2 256->128 (32 chunks) is fused from batch 1 on
        const int64_t blocks = sr_convt_fused_blocks(B, N, IH, IW);
        const bool pays = blocks >= 192 || C <= 256;
        // few tiles, long channel loop: K slices inside the fused kernel (SR_CONVT_FUSED_KS=0: the per-phase launches)
        const int ks = pays ? 1 : sr_convt_fused_slices(blocks, C, IH, IW);
        candidate(SR_CONV_PATH_CONVT_FUSED_KS, ks > 1, fused_ok && !sr_env_off("SR_CONVT_FUSED_KS"),
                  ks * B * N * (2 * IH + 1) * (2 * IW + 1), ks);
        candidate(SR_CONV_PATH_CONVT_FUSED, true, fused_ok && (pays || sw == '1'), 0);
        // behind an interior kernel the output row 2*IH and column 2*IW run as two three-tap launches + one reduction
        // (SR_CONVT_STRIPS=0: the four thin per-phase launches and their split-K reductions)
        const int64_t strip = sr_convt_strip_floats(B, N, IH, IW);
        plan.sized = std::max(plan.sized, strip);
        if (convt_interior(plan.path) && have_scratch && !sr_env_off("SR_CONVT_STRIPS")) {
            plan.strips = true;
            plan.floats = std::max(plan.floats, strip);
        }
    }
    if (plan.path == SR_CONV_PATH_CONVT_TAPS)
        plan.taps_gemm = sr_convt_taps_gemm_eligible(B, C, N, IW, c.ldw, plan.c_per_slice, c.wt);
    return plan;
}

// The geometries the matrix-core kernels serve (SR_EINVAL otherwise).
bool conv_call_valid(const ConvCall& c) {
    if (c.B < 0 || c.C <= 0 || c.N <= 0 || c.IH <= 0 || c.IW <= 0 || c.OH <= 0 || c.OW <= 0) return false;
    if (c.transposed) return c.is3x3(2, 0) && c.OH == 2 * c.IH + 1 && c.OW == 2 * c.IW + 1;
    return (c.ksize == 3 || c.ksize == 1) && (c.stride == 1 || c.stride == 2) &&
           c.OH == (c.IH + 2 * c.pad - c.ksize) / c.stride + 1 && c.OW == (c.IW + 2 * c.pad - c.ksize) / c.stride + 1;
}

}  // namespace

extern "C" int64_t sr_conv2d_scratch_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW,
                                            int64_t OH, int64_t OW, int ksize, int stride, int pad,
                                            int transposed) {
    const ConvCall c{B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, nullptr, nullptr, nullptr, 0};
    return make_conv_plan(c, true).sized;
}

extern "C" int sr_conv2d_path(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW, int ksize,
                              int stride, int pad, int transposed, const float* in, const float* out, const float* wt,
                              int64_t wt_ld, int have_scratch) {
    const ConvCall c{B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, in, out, wt, wt_ld};
    return conv_call_valid(c) ? make_conv_plan(c, have_scratch != 0).code() : SR_CONV_PATH_INVALID;
}

extern "C" int64_t sr_conv2d_path_floats(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                                         int ksize, int stride, int pad, int transposed, const float* in, const float* out,
                                         const float* wt, int64_t wt_ld, int have_scratch) {
    const ConvCall c{B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, in, out, wt, wt_ld};
    return conv_call_valid(c) ? make_conv_plan(c, have_scratch != 0).floats : -1;
}

// 1 when a stride-1 3x3 convolution call with these sizes AND these buffers runs the Winograd kernel (and therefore
// writes / reads the Winograd-domain weights at the head of its scratch), 0 when it takes the direct kernel.
extern "C" int sr_conv2d_uses_winograd(int64_t B, int64_t C, int64_t N, int64_t IH, int64_t IW, const float* in,
                                       const float* out) {
    return make_conv_plan(ConvCall{B, C, N, IH, IW, IH, IW, 3, 1, 1, 0, in, out, nullptr, 0}, true).path == SR_CONV_PATH_WINO;
}

extern "C" int sr_conv2d_mfma_ex(float* out, const float* in, const float* wt, const float* iscale,
                              const float* oscale, const float* obias, int64_t B, int64_t C,
                              int64_t N, int64_t wt_ld, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                              int ksize, int stride, int pad, int transposed, int flags, float* scratch,
                              sr_stream_t stream) {
    const ConvCall c{B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed, in, out, wt, wt_ld};
    if (B < 0 || C <= 0 || N <= 0 || IH <= 0 || IW <= 0 || OH <= 0 || OW <= 0) return SR_EINVAL;
    if (wt_ld < N || wt_ld % 4 != 0 || !sr_aligned16(wt)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!out || !in || !wt) return SR_EINVAL;
    // 32-bit element offsets inside the kernel
    if (B * C * IH * IW >= (1LL << 31) || B * N * OH * OW >= (1LL << 40) ||
        (int64_t)ksize * ksize * C * wt_ld >= (1LL << 31))
        return SR_ERANGE;
    if (!conv_call_valid(c)) return SR_EINVAL;
    const ConvPlan plan = make_conv_plan(c, scratch != nullptr);
    hipStream_t st = sr_stream(stream);
    ConvParams p;
    p.in = in; p.wt = wt; p.iscale = iscale; p.oscale = oscale; p.obias = obias; p.out = out;
    p.B = (int)B; p.C = (int)C; p.N = (int)N; p.ldw = (int)wt_ld;
    p.IH = (int)IH; p.IW = (int)IW; p.OH = (int)OH; p.OW = (int)OW;
    p.partial = scratch;
    p.partial_floats = scratch ? plan.sized : 0;
    for (int i = 0; i < 9; ++i) p.wmap[i] = 0;
    p.ks = 1; p.c_per_slice = (p.C + 15) / 16 * 16;
    p.tap_first = 0; p.tap_step = 1; p.tap_count = 9;
    int rc = SR_OK;
    switch (plan.path) {
    case SR_CONV_PATH_WINO:
        return sr_wino_conv3x3(out, in, wt, wt_ld, iscale, oscale, obias, B, C, N, IH, IW, scratch, st, nullptr,
                               (flags & SR_CONV_U_READY) != 0);
    case SR_CONV_PATH_S2_BF16:
        return sr_conv_s2_bf16x3_launch(out, in, wt, wt_ld, iscale, oscale, obias, B, C, N, IH, IW, OH, OW, scratch, st);
    case SR_CONV_PATH_S2_WINO:
        return sr_conv_s2_wino_launch(out, in, wt, wt_ld, iscale, oscale, obias, B, C, N, IH, IW, OH, OW, scratch, st);
    case SR_CONV_PATH_GEMM1X1:
        return sr_conv1x1_gemm_launch(out, in, wt, wt_ld, iscale, oscale, obias, B, C, N, IH * IW, st);
    case SR_CONV_PATH_CONVT_TAPS:
        return sr_convt_taps_launch(p, plan.ks, plan.c_per_slice, plan.taps_gemm, st);
    case SR_CONV_PATH_CONVT_BF16:
        rc = sr_convt_bf16x3_launch(out, in, wt, wt_ld, iscale, oscale, obias, B, C, N, IH, IW, scratch, st);
        break;
    case SR_CONV_PATH_CONVT_WINO:
        rc = sr_convt_wino_launch(out, in, wt, wt_ld, iscale, oscale, obias, B, C, N, IH, IW, st);
        break;
    case SR_CONV_PATH_CONVT_FUSED_KS:
    case SR_CONV_PATH_CONVT_FUSED:
        for (int i = 0; i < 9; ++i) p.wmap[i] = i;
        rc = sr_convt_fused_launch(p, plan.ks, st);
        break;
    default:    // SR_CONV_PATH_DIRECT
        if (transposed) break;
        return sr_conv_direct_launch(p, ksize, stride, pad, st);
    }
    // transposed 3x3 stride 2, no padding: out[2y + ky, 2x + kx] += in[y, x] * W[ky][kx]; the interior is done or left to
    // the per-phase launches, the border follows
    if (rc != SR_OK) return rc;
    if (plan.strips) return sr_convt_strips_launch(p, st);
    return sr_convt_phases_launch(p, convt_interior(plan.path), st);
}

extern "C" int sr_conv2d_mfma(float* out, const float* in, const float* wt, const float* iscale,
                              const float* oscale, const float* obias, int64_t B, int64_t C,
                              int64_t N, int64_t wt_ld, int64_t IH, int64_t IW, int64_t OH, int64_t OW,
                              int ksize, int stride, int pad, int transposed, float* scratch,
                              sr_stream_t stream) {
    return sr_conv2d_mfma_ex(out, in, wt, iscale, oscale, obias, B, C, N, wt_ld, IH, IW, OH, OW, ksize, stride, pad,
                             transposed, 0, scratch, stream);
}

// Modulated 3x3 stride-1 convolution with the StyledConv tail fused into the store (Winograd kernel only).
// SR_EINVAL when the shape is not taken by the Winograd path: the caller then runs sr_conv2d_mfma followed
// by sr_noise_bias_act.
extern "C" int sr_conv2d_nba_ex(float* out, const float* in, const float* wt, const float* iscale, const float* oscale,
                                const float* noise, const float* noise_w, const float* abias, float alpha, float gain,
                                int64_t B, int64_t C, int64_t N, int64_t wt_ld, int64_t H, int64_t W,
                                int64_t noise_bstride, int flags, float* scratch, sr_stream_t stream) {
    if (B < 0 || C <= 0 || N <= 0 || H <= 0 || W <= 0) return SR_EINVAL;
    if (wt_ld < N || wt_ld % 4 != 0 || !sr_aligned16(wt)) return SR_EINVAL;
    if (B == 0) return SR_OK;
    if (!out || !in || !wt || !scratch || (noise && !noise_w)) return SR_EINVAL;
    if (!sr_conv2d_uses_winograd(B, C, N, H, W, in, out)) return SR_EINVAL;
    const WinoNba nba{noise, noise_w, abias, noise_bstride, alpha, gain};
    return sr_wino_conv3x3(out, in, wt, wt_ld, iscale, oscale, nullptr, B, C, N, H, W, scratch, sr_stream(stream), &nba,
                           (flags & SR_CONV_U_READY) != 0);
}

extern "C" int sr_conv2d_nba(float* out, const float* in, const float* wt, const float* iscale, const float* oscale,
                             const float* noise, const float* noise_w, const float* abias, float alpha, float gain,
                             int64_t B, int64_t C, int64_t N, int64_t wt_ld, int64_t H, int64_t W,
                             int64_t noise_bstride, float* scratch, sr_stream_t stream) {
    return sr_conv2d_nba_ex(out, in, wt, iscale, oscale, noise, noise_w, abias, alpha, gain, B, C, N, wt_ld, H, W,
                            noise_bstride, 0, scratch, stream);
}
