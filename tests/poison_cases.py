"""The table of tests/test_poison_gpu.py: one case per kernel family and memory-relevant shape, each a builder that returns
(callable, inputs, inplace).  The GPU test calls `callable(*inputs)` once plainly and once with every tensor of `inputs`
embedded in a guarded buffer and every allocation of the wrappers poisoned (tests/poison.py).

  * `inputs`: a list of tensors (on the device; None and non-tensors pass through unchanged).  A tensor that requires grad
    keeps the flag when embedded.  A callable that differentiates calls torch.autograd.grad itself, so that the backward
    allocations happen inside the poisoned region; it returns a tensor or a flat tuple / list of tensors (None allowed).
  * `inplace`: the positions in `inputs` the call is meant to modify (those are cloned for the plain run).
  * `env`: switches set for both runs; every switch of conv_plan_cases.SWITCHES that is not named is unset.
  * `waive`: (output position, reason) — that ONE output is by design only partly written by the call under test; it is
    then compared with the plain run bit for bit instead of being required finite.  Never more than one case in ten.

The shapes are the ones the suite's float64 comparisons already use: the tables are imported where they are module
level names, and copied from the parametrize lists of the named tests where they are not.  Nothing here computes a
reference."""
import math
import os
import re

import numpy as np
import torch

from conv_plan_cases import FORWARD, SWITCHES as PLAN_SWITCHES, WGRAD, case_id, conv_args
from test_conv_gpu import CASES as CONV_CASES, GENERIC, TAPS
from test_conv_s2_wino_gpu import SMALL as S2_WINO_SMALL
from test_convt_wino_gpu import SHAPES as CONVT_WINO_SHAPES
from test_dispatch_edges_gpu import AFF, REDUCE, SMALLCONV, SMALLCONV_DX
from test_wgrad_s2_wino_gpu import SMALL as WGRAD_S2_WINO_SMALL

DEV = "cuda"
SQRT2 = 2 ** 0.5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# every environment switch a case may set: unset before each case, then the case's own
SWITCHES = sorted(set(PLAN_SWITCHES) | {
    "SR_CONV_S2_WINO", "SR_WGRAD_S2_WINO", "SR_CONVT_WINO", "SR_CONVT_TAPS", "SR_CONVT_FUSED", "SR_CONVT_FUSED_KS",
    "SR_CONVT_STRIPS", "SR_WINOGRAD", "SR_WINO_SPLIT", "SR_U_CACHE", "SR_CONV1X1_GEMM", "SR_WGRAD_SMALL", "SR_WGRAD_DMA",
    "SR_FIR_ALIGNED", "SR_BLUR_BWD_FUSED", "SR_RASTER_TILED", "SR_RASTER_LEVELS", "SR_RASTER_PYRAMID", "SR_PRUNE_GRADS",
    "SR_CONV_SPLIT_BF16", "SR_CONV_ROT", "SR_WGW_WAVES", "SR_CONVT_TAPS_GEMM"})

# ---- coverage ---------------------------------------------------------------------------------------------------------
WRAPPER_MODULES = ["conv", "conv_generic", "fused_act", "fused_elem", "smallconv", "smallmm", "style", "style_bank",
                   "weight_prep", "weight_bank", "bankmm", "upfirdn2d", "share", "rasterize"]

# the stream-taking functions those modules call through op._dispatch.native (found by searching them for `native(`;
# tests/test_poison_cpu.py repeats the search and compares)
REQUIRED = [
    # conv
    "sr_conv2d_mfma_ex", "sr_conv2d_wgrad_mfma", "sr_conv2d_nba_ex", "sr_noise_bias_act_bwd_dot", "sr_blur_nba_bwd",
    "sr_conv1x1_add",
    # conv_generic
    "sr_conv2d_generic", "sr_conv2d_generic_dgrad", "sr_conv2d_generic_wgrad",
    # fused_act
    "sr_fused_bias_act", "sr_fused_act_bwd",
    # fused_elem
    "sr_noise_bias_act", "sr_noise_bias_act_bwd", "sr_noise_bias_act_affine", "sr_noise_bias_act_affine_bwd",
    "sr_noise_bias_act_affine_bwd2", "sr_blur_noise_bias_act", "sr_rowdot", "sr_rowdot_bwd", "sr_rowdot_div",
    # smallconv
    "sr_smallconv_fwd", "sr_smallconv_dx_add", "sr_smallconv_dw_bias", "sr_modrows_fwd", "sr_modrows_bwd",
    # smallmm, style
    "sr_linear_fwd", "sr_linear_bwd_x", "sr_linear_bwd_w", "sr_demod_fwd", "sr_demod_bwd",
    # weight_prep, weight_bank
    "sr_weight_prep", "sr_weight_prep_bwd", "sr_weight_adjoint", "sr_weight_prep_batch", "sr_weight_adjoint_batch",
    # bankmm (style_bank launches through it)
    "sr_bank_nt", "sr_bank_nn", "sr_bank_tn",
    # upfirdn2d, share
    "sr_upfirdn2d", "sr_upsample2_add", "sr_share_rows",
    # rasterize
    "sr_rasterize_forward_f32", "sr_rasterize_forward_f64", "sr_rasterize_backward_f32", "sr_rasterize_backward_f64",
    "sr_rasterize_grad_f32", "sr_rasterize_grad_f64", "sr_rasterize_forward_levels_f32", "sr_rasterize_grad_levels_f32",
]


def native_calls(source):
    """The sr_* names a wrapper module's source launches through `native(...)`: `native(x).sr_name(`, `run = native(x)`
    followed by `run.sr_name(`, and `getattr(native(x), "sr_name_" + suf)` (suf: f32 | f64)."""
    found = set(re.findall(r"native\([^()]*\)\s*\.\s*(sr_\w+)", source))
    for var in set(re.findall(r"(\w+)\s*=\s*native\(", source)):
        found |= set(re.findall(r"\b%s\.(sr_\w+)" % re.escape(var), source))
    for stem in re.findall(r"getattr\(\s*native\([^()]*\)\s*,\s*\"(sr_\w+_)\"\s*\+\s*suf\s*\)", source):
        found |= {stem + "f32", stem + "f64"}
    return found


# ---- the table --------------------------------------------------------------------------------------------------------
class Case:
    __slots__ = ("id", "build", "env", "waive")

    def __init__(self, id, build, env=None, waive=None):
        self.id, self.build, self.env, self.waive = id, build, dict(env or {}), waive


CASES = []


def case(id, env=None, waive=None):
    def deco(build):
        CASES.append(Case(id, build, env, waive))
        return build
    return deco


def add(id, build, env=None, waive=None):
    CASES.append(Case(id, build, env, waive))


class Rand:
    """Deterministic inputs: standard normal values from a seeded host generator, moved to the device."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, *shape, grad=False, scale=1.0):
        t = (torch.randn(*shape, generator=self.g) * scale).to(DEV)
        return t.requires_grad_() if grad else t

    def pos(self, *shape, grad=False):
        t = (torch.rand(*shape, generator=self.g) + 0.5).to(DEV)
        return t.requires_grad_() if grad else t


def _seed(*v):
    return sum((i + 1) * int(x) for i, x in enumerate(v)) % (2 ** 31)


def _blur(gain=4.0):
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
    return (k1[None, :] * k1[:, None] / 64.0 * gain).to(DEV)


def _dims(shape):
    return "B%d-C%d-N%d-%dx%d" % tuple(shape[:5])


# ---- dense convolutions: forward ----------------------------------------------------------------------------------------
def conv_forward(b, c, n, ih, iw, k, stride, pad, tr, scaled=True, offset=0):
    """offset: the input as a contiguous view 4 * offset bytes into its buffer — not 16-byte aligned, which the
    vector-staging kernels refuse (the direct kernel's scalar staging serves it)."""
    def build():
        from stylerenderer_amd.op.conv import conv2d_mfma

        r = Rand(_seed(b, c, n, ih, iw, k, stride))
        x, wt = r(b * c * ih * iw + offset), r(k * k, c, n, scale=1.0 / (k * c ** 0.5))
        isc, osc, bias = (r(b, c), r(b, n), r(n)) if scaled else (None, None, None)
        return (lambda x, wt, isc, osc, bias: conv2d_mfma(x[offset:].view(b, c, ih, iw), wt, isc, osc, bias, k, stride, pad,
                                                          bool(tr))), [x, wt, isc, osc, bias], ()
    return build


def conv_wgrad(b, c, n, ih, iw, k, stride, pad, tr, scaled=True):
    def build():
        from stylerenderer_amd.op.conv import conv2d_wgrad_mfma, conv_out_size

        r = Rand(_seed(b, c, n, ih, iw, k, stride, 7))
        oh, ow = conv_out_size(ih, iw, k, stride, pad, tr)
        x, gy = r(b, c, ih, iw), r(b, n, oh, ow)
        xs, gs = (r(b, c), r(b, n)) if scaled else (None, None)
        return (lambda x, gy, xs, gs: conv2d_wgrad_mfma(x, gy, xs, gs, k, stride, pad, bool(tr))), [x, gy, xs, gs], ()
    return build


for row in FORWARD:
    if row[-1]:
        a = conv_args(row[0], row[1])
        add("plan-fwd-" + case_id(row), conv_forward(*a[:5], *a[7:]), row[2])
for row in WGRAD:
    if row[-1]:
        a = conv_args(row[0], row[1])
        # (the streaming from-RGB form in the wrapper takes unscaled 1x1 operands only: scaled here = the MFMA path)
        add("plan-wgrad-" + case_id(row), conv_wgrad(*a[:5], *a[7:]), row[2])

# every geometry of test_conv_gpu.CASES (odd extents, channel tails, one-pixel maps): forward and weight gradient on the
# natural dispatch, and the Winograd / vector-staging shapes again from an input that is not 16-byte aligned
for s in CONV_CASES:
    tag = "%s-k%d-s%d%s" % (_dims(s), s[5], s[6], "-convT" if s[8] else "")
    add("conv-" + tag, conv_forward(*s))
    add("wgrad-" + tag, conv_wgrad(*s, scaled=(s[0] + s[1]) % 2 == 0))
for s in ((1, 8, 64, 8, 32, 3, 1, 1, False), (2, 16, 64, 129, 129, 3, 2, 0, False), (2, 8, 130, 32, 32, 3, 2, 0, True),
          (4, 64, 256, 64, 64, 1, 1, 0, False)):
    add("conv-offset-input-%s-k%d-s%d%s" % (_dims(s), s[5], s[6], "-convT" if s[8] else ""), conv_forward(*s, offset=1))

# stride-2 polyphase Winograd, forward and weight gradient, and the up-sampling one (tests' SMALL / SHAPES tables)
for s in S2_WINO_SMALL:
    add("s2-wino-" + _dims(s), conv_forward(*s, 3, 2, 0, False), {"SR_CONV_S2_WINO": "force"})
for s in WGRAD_S2_WINO_SMALL:
    add("wgrad-s2-wino-%s-%s" % (_dims(s), "convT" if s[5] else "conv"), conv_wgrad(*s[:5], 3, 2, 0, s[5]),
        {"SR_WGRAD_S2_WINO": "force"})
for s in CONVT_WINO_SHAPES:
    add("convt-wino-" + _dims(s), conv_forward(*s, 3, 2, 0, True), {"SR_CONVT_WINO": "force"})

# transposed convolution: the tap-split launch and the per-phase launches, border strips, K slices (test_conv_gpu)
BORDER_STRIPS = [(2, 8, 130, 32, 32), (1, 16, 6, 8, 64), (3, 24, 64, 12, 32), (1, 64, 128, 64, 64)]
K_SLICES = [(2, 320, 512, 32, 32), (4, 512, 256, 32, 32)]
for s in TAPS:
    for mode in ("1", "0"):
        add("convt-taps%s-%s" % (mode, _dims(s)), conv_forward(*s, 3, 2, 0, True), {"SR_CONVT_TAPS": mode})
for s in BORDER_STRIPS:
    add("convt-strips-" + _dims(s), conv_forward(*s, 3, 2, 0, True), {"SR_CONVT_TAPS": "0", "SR_CONVT_FUSED": "1"})
for s in K_SLICES:
    add("convt-kslices-" + _dims(s), conv_forward(*s, 3, 2, 0, True), {"SR_CONVT_TAPS": "0"})

# split-K reduce forms of the weight gradient (test_dispatch_edges_gpu.REDUCE) and the streaming from-RGB form
for s in REDUCE:
    add("wgrad-reduce-" + _dims(s), conv_wgrad(*s, 1, 1, 0, False, scaled=False))
add("wgrad-from-rgb-B4-C3-N128-32x32", conv_wgrad(4, 3, 128, 32, 32, 1, 1, 0, False, scaled=False))
add("wgrad-from-rgb-B2-C3-N128-256x256", conv_wgrad(2, 3, 128, 256, 256, 1, 1, 0, False, scaled=False))

# the 1x1 GEMM (forced at the shapes of test_conv1x1_gemm_vs_float64_and_window_kernel) and conv1x1_add
for s in [(2, 32, 128, 16, 32), (3, 48, 256, 8, 16), (1, 16, 128, 32, 64)]:
    add("conv1x1-gemm-" + _dims(s), conv_forward(*s, 1, 1, 0, False), {"SR_CONV1X1_GEMM": "force"})


def conv1x1_add_case(b, c, n, h, w):
    def build():
        from stylerenderer_amd.op import conv as C

        r = Rand(_seed(b, c, n, h, w, 11))
        x, wt = r(b, c, h, w, grad=True), r(1, c, n, grad=True)
        osc, addend, gy = r(b, n), r(b, n, h, w, grad=True), r(b, n, h, w)

        def run(x, wt, osc, addend, gy):
            y = C.conv1x1_add(x, wt, osc, addend)
            return (y,) + tuple(torch.autograd.grad(y, [x, wt, addend], gy))
        return run, [x, wt, osc, addend, gy], ()
    return build


for hw in ((64, 64), (64, 62)):       # 256 tiles: the GEMM with the addend in its store; 248: the two operators
    add("conv1x1-add-B4-C64-N256-%dx%d" % hw, conv1x1_add_case(4, 64, 256, *hw))


# generic geometry (test_conv_gpu.GENERIC): forward, data gradient, weight gradient, transposed forward


def generic_case(b, c, n, h, w, kh, kw, st, pd):
    def build():
        from stylerenderer_amd.op import conv_generic as cg

        r = Rand(7)
        x, wt, bias = r(b, c, h, w, grad=True), r(n, c, kh, kw, grad=True, scale=(c * kh * kw) ** -0.5), r(n, grad=True)
        wt_t = r(c, n, kh, kw, scale=(c * kh * kw) ** -0.5)

        def run(x, wt, bias, wt_t):
            y = cg.conv2d_generic(x, wt, bias, st, pd)
            grads = torch.autograd.grad(y.square().sum(), [x, wt, bias])
            return (y,) + tuple(grads) + (cg.conv_transpose2d_generic(x.detach(), wt_t, stride=st, padding=pd),)
        return run, [x, wt, bias, wt_t], ()
    return build


for s in GENERIC:
    add("generic-B%d-C%d-N%d-%dx%d-k%dx%d-s%s-p%s" % s, generic_case(*s))


# ---- frozen-weight scratch: the Winograd-domain weight block kept between calls ---------------------------------------
@case("frozen-weight-scratch-B2-C64-N128-16x32", {"SR_U_CACHE": "1"})
def _frozen():
    from stylerenderer_amd.op import conv as cv

    b, c, n, h, w = 2, 64, 128, 16, 32
    r = Rand(3)
    x, wt, isc, osc = r(b, c, h, w), r(9, c, n, scale=1.0 / (3 * c ** 0.5)), r(b, c), r(b, n)
    wt._sr_frozen = True

    def run(x, wt, isc, osc):
        first = cv.conv2d_mfma(x, wt, isc, osc, None, 3, 1, 1)
        (entry,) = wt._sr_scratch.values()
        assert entry.ready, "the first call took the Winograd kernel and wrote the weight block"
        second = cv.conv2d_mfma(x, wt, isc, osc, None, 3, 1, 1)          # SR_CONV_U_READY: reads the kept block
        assert torch.equal(first, second)
        return first, second
    return run, [x, wt, isc, osc], ()


# ---- through autograd -------------------------------------------------------------------------------------------------
def convfn_case(geom, b, c, n, h, w):
    def build():
        from stylerenderer_amd.op import conv as cv

        k = cv._GEOM[geom][0]
        r = Rand(_seed(b, c, n, h, w, k))
        x, wt = r(b, c, h, w, grad=True), r(k * k, c, n, grad=True, scale=1.0 / (k * c ** 0.5))
        isc, osc, bias = r(b, c, grad=True), r(b, n, grad=True), r(n, grad=True)
        oh, ow = cv.conv_out_size(h, w, *cv._GEOM[geom][:4])
        gy = r(b, n, oh, ow)

        def run(x, wt, isc, osc, bias, gy):
            y = cv.conv2d(x, wt, isc, osc, bias, geom)
            return (y,) + tuple(torch.autograd.grad(y, [x, wt, isc, osc, bias], gy))
        return run, [x, wt, isc, osc, bias, gy], ()
    return build


for geom, s in (("c3", (2, 16, 64, 8, 32)), ("c3", (2, 5, 7, 16, 16)), ("c3s2", (2, 10, 5, 33, 33)),
                ("t3s2", (2, 8, 130, 32, 32)), ("c1", (2, 16, 5, 32, 32))):
    add("autograd-convfn-%s-%s" % (geom, _dims(s)), convfn_case(geom, *s))


def nba_node_case(up, b, c, n, h, w, shared_noise, second_order=False):
    def build():
        from stylerenderer_amd.op import conv as cv

        r = Rand(_seed(b, c, n, h, w, up, 5))
        oh, ow = (2 * h, 2 * w) if up else (h, w)
        x, wt, s = r(b, c, h, w, grad=True), r(9, c, n, grad=True, scale=1.0 / (3 * c ** 0.5)), r(b, c, grad=True)
        noise, nw, ab, proj = r(1 if shared_noise else b, 1, oh, ow), r(1, grad=True), r(n, grad=True), r(b, n, oh, ow)
        kernel = _blur()
        if second_order:
            wsq = (torch.rand(c, n, generator=r.g) / c).to(DEV).requires_grad_()
        else:
            wsq = r.pos(b, n, grad=True)                                     # the demodulation scale itself

        def run(x, wt, s, wsq, noise, nw, ab, proj, kernel):
            d = torch.rsqrt((s * s) @ wsq + 1e-8) if second_order else wsq   # (second order: linked to s outside the node)
            if up:
                y = cv.upconv_nba(x, wt, s, d, kernel, (1, 1), noise, nw, ab)
            else:
                assert cv.conv_nba_supported(x, wt, noise)
                y = cv.conv2d_nba(x, wt, s, d, noise, nw, ab)
            if second_order:
                (gs,) = torch.autograd.grad((y * proj).sum(), s, create_graph=True)
                (g2,) = torch.autograd.grad((gs * gs).sum(), wt)
                return y, gs, g2
            return (y,) + tuple(torch.autograd.grad((y * proj).sum(), [x, wt, s, wsq, nw, ab]))
        return run, [x, wt, s, wsq, noise, nw, ab, proj, kernel], ()
    return build


add("autograd-conv-nba-B2-C16-N64-8x32", nba_node_case(False, 2, 16, 64, 8, 32, False))
add("autograd-conv-nba-kslices-B1-C128-N64-8x32", nba_node_case(False, 1, 128, 64, 8, 32, True))
add("autograd-upconv-nba-B2-C16-N64-8x32", nba_node_case(True, 2, 16, 64, 8, 32, False))
add("autograd-upconv-nba-257-B1-C8-N8-128x128", nba_node_case(True, 1, 8, 8, 128, 128, True))
add("double-backward-conv-nba-B2-C16-N64-8x32", nba_node_case(False, 2, 16, 64, 8, 32, False, second_order=True))
add("double-backward-upconv-nba-B2-C16-N64-8x32", nba_node_case(True, 2, 16, 64, 8, 32, False, second_order=True))


# ---- fused tails --------------------------------------------------------------------------------------------------------
def fused_bias_act_case(shape, act, grad, use_b):
    def build():
        from stylerenderer_amd.op.fused_act import fused_bias_act

        r = Rand(_seed(*shape, act, grad))
        x, b, ref = r(*shape), (r(shape[1]) if use_b else r(0)), (r(*shape) if grad == 1 else r(0))
        return (lambda x, b, ref: fused_bias_act(x, b, ref, act, grad, 0.2, SQRT2)), [x, b, ref], ()
    return build


for shape, code, use_b in (((1, 5, 33, 31), (3, 0), True), ((2, 3, 7), (3, 1), True), ((16, 512), (3, 2), False),
                           ((2, 8, 64, 64), (1, 0), True)):
    add("fused-bias-act-%s-act%d-grad%d" % ("x".join(map(str, shape)), *code), fused_bias_act_case(shape, *code, use_b))


def act_backward_case(shape):
    def build():
        from stylerenderer_amd.op.fused_act import _act_backward

        r = Rand(_seed(*shape, 15))
        return (lambda gy, out: _act_backward(gy, out, 0.2, SQRT2)), [r(*shape), r(*shape)], ()
    return build


for shape in ((3, 5, 40, 36), (16, 512), (2, 3, 7, 9)):
    add("fused-act-bwd-" + "x".join(map(str, shape)), act_backward_case(shape))


def nba_case(shape, shared):
    def build():
        from stylerenderer_amd.op.fused_elem import noise_bias_act

        r = Rand(_seed(*shape, shared))
        x, noise = r(*shape, grad=True), r(1 if shared else shape[0], 1, *shape[2:])
        nw, bias, gy = r(1, grad=True), r(shape[1], grad=True), r(*shape)

        def run(x, noise, nw, bias, gy):
            y = noise_bias_act(x, noise, nw, bias)
            return (y,) + tuple(torch.autograd.grad(y, [x, nw, bias], gy))
        return run, [x, noise, nw, bias, gy], ()
    return build


for shape, shared in (((2, 6, 8, 8), True), ((3, 5, 16, 12), False), ((2, 4, 4, 4), True)):
    add("noise-bias-act-%s-%s" % ("x".join(map(str, shape)), "noise1" if shared else "bnoise"), nba_case(shape, shared))


def tail_backward_case(b, n, oh, shared, frozen, one_pass):
    """The activation backward with row-dots (sr_noise_bias_act_bwd_dot) and the one-pass up-sampling tail
    (sr_blur_nba_bwd: activation backward, its three reductions and the blur's gradient onto the (oh + 1)-wide map)."""
    def build():
        from stylerenderer_amd.op import conv as cv
        from stylerenderer_amd.op.upfirdn2d import flipped

        r = Rand(5 + oh)
        gy, out = r(b, n, oh, oh), r(b, n, oh, oh)
        noise = None if shared is None else r(1 if shared else b, 1, oh, oh)
        nw, ab, kernel = (r(1) if noise is not None else None), r(n), _blur()

        def run(gy, out, noise, nw, ab, kernel):
            if one_pass:
                return cv._blur_nba_bwd(gy, out, flipped(kernel), 1, (b, n, oh + 1, oh + 1), noise, nw, ab, 0.2, SQRT2,
                                        not frozen)
            return cv._nba_bwd_dot(gy, out, noise, nw, ab, 0.2, SQRT2, not frozen)
        return run, [gy, out, noise, nw, ab, kernel], ()
    return build


for b, n, oh, shared, frozen in ((2, 8, 256, False, False), (3, 5, 16, True, False), (1, 6, 64, False, True),
                                 (2, 4, 96, None, False)):
    tag = "B%d-N%d-%d-%s%s" % (b, n, oh, {None: "nonoise", True: "noise1", False: "bnoise"}[shared], "-frozen" * frozen)
    add("nba-bwd-dot-" + tag, tail_backward_case(b, n, oh, shared, frozen, False))
    add("blur-nba-bwd-" + tag, tail_backward_case(b, n, oh, shared, frozen, True))

# the StyledMapConv tail: forward, backward, second backward (test_dispatch_edges_gpu.AFF)


def affine_case(b, c, h, w, per_sample):
    def build():
        from stylerenderer_amd.op.fused_elem import noise_bias_act_affine

        r = Rand(b * 7 + c * 3 + h)
        x, amap = r(b, c, h, w, grad=True), r(b, 4, h, w)
        amap[:, 1] = 0.5 + amap[:, 1].abs()
        amap.requires_grad_()
        noise, nw, bias = r(b if per_sample else 1, 1, h, w), r(1, grad=True), r(c, grad=True)
        gy, Px, Pm, Pb, Pnw = r(b, c, h, w, grad=True), r(b, c, h, w), r(b, 4, h, w), r(c), r(1)

        def run(x, amap, noise, nw, bias, gy, Px, Pm, Pb, Pnw):
            y = noise_bias_act_affine(x, amap[:, 1:3], noise, nw, bias, 0.2, SQRT2)
            gx, gm, gb, gnw = torch.autograd.grad(y, [x, amap, bias, nw], gy, create_graph=True)
            q = (gx * Px).sum() + (gm * Pm).sum() + (gb * Pb).sum() + (gnw * Pnw).sum()
            d_gy, d_x, d_m = torch.autograd.grad(q, [gy, x, amap])
            return y, gx, gm, gb, gnw, d_gy, d_x, d_m
        return run, [x, amap, noise, nw, bias, gy, Px, Pm, Pb, Pnw], ()
    return build


for s in AFF:
    add("affine-tail-B%d-C%d-%dx%d-%s" % (s[:4] + ("bnoise" if s[4] else "noise1",)), affine_case(*s))


# ---- row-dots and small matrix products ---------------------------------------------------------------------------------
def rowdot_case(b, c, h, w):
    def build():
        from stylerenderer_amd.op.fused_elem import rowdot

        r = Rand(_seed(b, c, h, w, 91))
        a, bb, s = r(b, c, h, w, grad=True), r(b, c, h, w, grad=True), r(b, c, grad=True)

        def run(a, bb, s):
            dots, out = rowdot(a, bb, s)
            plain = rowdot(a, bb)
            return (dots, out, plain) + tuple(torch.autograd.grad(dots.sum() + (out * a.detach()).sum(), [a, bb, s]))
        return run, [a, bb, s], ()
    return build


for hw in ((20, 24), (17, 17), (65, 65), (257, 257)):
    add("rowdot-B3-C7-%dx%d" % hw, rowdot_case(3, 7, *hw))


def rowdot_div_case(shape):
    def build():
        from stylerenderer_amd.op.fused_elem import rowdot_div

        r = Rand(sum(shape))
        a, bb, d = r(*shape), r(*shape), r.pos(*shape[:2])

        def run(a, bb, d):
            with torch.no_grad():
                return rowdot_div(a, bb, d)
        return run, [a, bb, d], ()
    return build


for shape in ((2, 8, 16, 16), (1, 64, 128, 128), (3, 5, 9, 9)):
    add("rowdot-div-" + "x".join(map(str, shape)), rowdot_div_case(shape))

# ToRGB 1x1 convolution (test_dispatch_edges_gpu.SMALLCONV / SMALLCONV_DX)


def smallconv_case(b, c, n, h, w, with_bias):
    def build():
        from stylerenderer_amd.op.smallconv import SmallConvFwd

        r = Rand(b * 1000 + c * 10 + n)
        x, ws, gy = r(b, c, h, w, grad=True), r(b, n, c, grad=True), r(b, n, h, w)
        bias = r(n, grad=True) if with_bias else None

        def run(x, ws, gy, bias):
            y = SmallConvFwd.apply(x, ws, bias)
            return (y,) + tuple(torch.autograd.grad(y, [x, ws] + ([bias] if bias is not None else []), gy))
        return run, [x, ws, gy, bias], ()
    return build


def smallconv_fork_case(b, c, n, h, w, fused):
    def build():
        from stylerenderer_amd.op.smallconv import SmallConvFork

        r = Rand(b * 100 + c + n)
        x, ws, gy, probe = r(b, c, h, w, grad=True), r(b, n, c), r(b, n, h, w), r(b, c, h, w)

        def run(x, ws, gy, probe):
            same, rgb = SmallConvFork.apply(x, ws, None)
            loss = (same * probe).sum() + (rgb * gy).sum()
            return rgb, torch.autograd.grad(loss, x, create_graph=not fused)[0]
        return run, [x, ws, gy, probe], ()
    return build


for s in SMALLCONV:
    add("smallconv-%s-%s" % (_dims(s), "bias" if s[5] else "nobias"), smallconv_case(*s))
for s in SMALLCONV_DX:
    add("smallconv-dx-addend-" + _dims(s), smallconv_fork_case(*s, True))
for s in SMALLCONV_DX[1:4:2]:
    add("smallconv-dx-plain-" + _dims(s), smallconv_fork_case(*s, False))


def modrows_case(b, n, c):
    def build():
        from stylerenderer_amd.op import smallconv

        r = Rand(b * 100 + c)
        w, s, up = r(n, c, grad=True), r(b, c, grad=True), r(b, n, c)

        def run(w, s, up):
            got = smallconv.modulated_rows(w, s, 0.173)
            return (got,) + tuple(torch.autograd.grad(got, [w, s], up))
        return run, [w, s, up], ()
    return build


for s in ((1, 3, 512), (4, 3, 128), (5, 4, 36)):
    add("modrows-B%d-N%d-C%d" % s, modrows_case(*s))


# ---- style path ---------------------------------------------------------------------------------------------------------
def equal_linear_case(b, k, n, act, bias, strided):
    def build():
        from stylerenderer_amd.op import style

        r = Rand(b * 1000 + n)
        xfull, w, gy = r(b, 3, k, grad=True), r(n, k, grad=True), r(b, n)
        b0 = r(n, grad=True) if bias else None

        def run(xfull, w, b0, gy):
            x_in = xfull[:, 1] if strided else xfull[:, 1].contiguous()
            assert style.linear_supported(x_in, w)
            y = style.equal_linear(x_in, w, b0, 1.0 / math.sqrt(k), 0.7, act)
            return (y,) + tuple(torch.autograd.grad(y, [t for t in (xfull, w, b0) if t is not None], gy))
        return run, [xfull, w, b0, gy], ()
    return build


for s in ((16, 512, 512, True, True, False), (5, 64, 24, False, True, True), (3, 16, 130, False, False, False),
          (1, 512, 128, True, True, True)):
    add("equal-linear-B%d-K%d-N%d%s%s%s" % (s[:3] + ("-act" * s[3], "-bias" * s[4], "-strided" * s[5])),
        equal_linear_case(*s))


def smallmm_case(b, k, n):
    def build():
        from stylerenderer_amd.op import smallmm

        r = Rand(b + k + n)
        a, w, g = r(b, k), r(n, k), r(b, n)

        def run(a, w, g):
            assert smallmm.supported(k, a, w, g)
            return smallmm.mm_nt(a, w), smallmm.mm_nn(g, w), smallmm.mm_tn(g, a)
        return run, [a, w, g], ()
    return build


add("smallmm-B5-K64-N24", smallmm_case(5, 64, 24))
add("smallmm-B3-K16-N130", smallmm_case(3, 16, 130))


def demod_case(b, ci, co):
    def build():
        from stylerenderer_amd.op import style

        r = Rand(b + ci + co)
        s, gd = r(b, ci, grad=True), r(b, co)
        wsq = (torch.rand(ci, co, generator=r.g) / ci).to(DEV).requires_grad_()

        def run(s, wsq, gd):
            d = style.demod_scale(s, wsq, 1e-8)
            return (d,) + tuple(torch.autograd.grad(d, [s, wsq], gd))
        return run, [s, wsq, gd], ()
    return build


for s in ((16, 512, 512), (3, 24, 8), (1, 130, 64)):
    add("demod-B%d-Ci%d-Co%d" % s, demod_case(*s))


def weight_prep_case(shape, want_sq):
    def build():
        from stylerenderer_amd.op.weight_prep import weight_prep

        r = Rand(sum(shape))
        w = r(*shape, grad=True)
        co, ci, k = shape[-4], shape[-3], shape[-1]
        a, bsq = r(k * k, ci, co), r(ci, co)

        def run(w, a, bsq):
            wt, wsq = weight_prep(w, 0.37, want_sq)
            loss = (wt * a).sum() + ((wsq * wsq * bsq).sum() if want_sq else 0.0)
            return (wt, wsq) + tuple(torch.autograd.grad(loss, [w]))
        return run, [w, a, bsq], ()
    return build


for shape in ((1, 24, 16, 3, 3), (6, 10, 3, 3), (3, 16, 1, 1), (1, 64, 130, 1, 1)):
    add("weight-prep-%s-sq" % "x".join(map(str, shape)), weight_prep_case(shape, True))
add("weight-prep-6x10x3x3-nosq", weight_prep_case((6, 10, 3, 3), False))


def adjoint_case(taps, c, n, flip):
    def build():
        from stylerenderer_amd.op.weight_prep import adjoint

        r = Rand(taps + c + n)
        wt, a = r(taps, c, n, grad=True), r(taps, n, c)
        padded = torch.zeros(taps, c, (n + 3) // 4 * 4 + 4, device=DEV)
        padded[:, :, :n] = wt.detach()

        def run(wt, a, padded):
            got = adjoint(wt, flip)
            return got, torch.autograd.grad((got * a).sum(), wt)[0], adjoint(padded[:, :, :n], flip)
        return run, [wt, a, padded], ()
    return build


for s in ((9, 40, 24, True), (9, 3, 128, False), (1, 130, 6, False)):
    add("weight-adjoint-T%d-C%d-N%d-%s" % (s[:3] + ("flip" if s[3] else "noflip",)), adjoint_case(*s))


@case("weight-bank-batched-prep-and-adjoint")
def _weight_bank():
    from stylerenderer_amd.op import weight_bank as wb

    r = Rand(3)
    shapes = [(64, 32, 3), (6, 20, 3), (130, 12, 1), (3, 64, 1), (128, 128, 3), (7, 5, 3), (512, 64, 1)]
    ws = [r(co, ci, k, k) for co, ci, k in shapes]
    scales = [0.5 + 0.1 * i for i in range(len(ws))]
    sqs = [i % 2 == 0 for i in range(len(ws))]
    flips = [w.shape[2] == 3 and i % 3 != 0 for i, w in enumerate(ws)]

    def run(*ws):
        outs = wb.prep_batch(list(ws), scales, sqs)
        adjs = wb.adjoint_batch([wt for wt, _ in outs], flips)
        return [wt for wt, _ in outs] + [wsq for _, wsq in outs if wsq is not None] + list(adjs)
    return run, ws, ()


def bank_modulation_case(batch):
    def build():
        from stylerenderer_amd.op import bankmm

        g = torch.Generator().manual_seed(0)
        rows, widths, nrow, k = [0, 1, 1, 2, 3, 3, 3, 5], [64, 128, 32, 64, 512, 256, 8, 128], 6, 128
        x = torch.randn(batch, nrow, k, generator=g).to(DEV).requires_grad_()
        ws = [torch.randn(n, k, generator=g).to(DEV).requires_grad_() for n in widths]
        bs = [torch.randn(n, generator=g).to(DEV).requires_grad_() for n in widths]
        cs = [torch.randn(batch, n, generator=g).to(DEV) for n in widths]
        nw = len(widths)

        def run(x, *rest):
            ws, bs, cs = list(rest[:nw]), list(rest[nw:2 * nw]), rest[2 * nw:]
            assert bankmm.modulation_supported(x, ws, bs)
            flat, outs = bankmm.modulation(x, rows, ws, bs, 0.37, 1.5)          # sr_bank_nt
            f = sum(((o * o) * c).sum() for o, c in zip(outs, cs))
            grads = torch.autograd.grad(f, [x] + ws + bs)                       # sr_bank_nn (x), sr_bank_tn (weights)
            return (flat,) + tuple(outs) + tuple(grads)
        return run, [x] + ws + bs + cs, ()
    return build


def bank_demod_case(batch):
    def build():
        from stylerenderer_amd.op import bankmm

        g = torch.Generator().manual_seed(3)
        widths, read, couts = [64, 32, 128, 64, 16], [0, 2, 3], [128, 64, 256]
        a = (torch.rand(sum(batch * w for w in widths), generator=g) + 0.1).to(DEV).requires_grad_()
        ms = [torch.rand(widths[i], co, generator=g).to(DEV).requires_grad_() for i, co in zip(read, couts)]
        offs, o = [], 0
        for w in widths:
            offs.append(o)
            o += batch * w

        def run(a, *ms):
            ms = list(ms)
            assert bankmm.demod_supported(ms)
            flat, qs = bankmm.demod_products(a, batch, [offs[i] for i in read], ms)      # sr_bank_nn
            f = (torch.rsqrt(flat + 1e-8) * torch.linspace(0.5, 1.5, flat.numel(), device=DEV)).sum()
            return (flat,) + tuple(qs) + tuple(torch.autograd.grad(f, [a] + ms))          # sr_bank_nt, sr_bank_tn
        return run, [a] + ms, ()
    return build


for batch in (1, 4):
    add("bank-mm-modulation-B%d" % batch, bank_modulation_case(batch))
    add("bank-mm-demod-B%d" % batch, bank_demod_case(batch))


def share_rows_case(b, d, k):
    def build():
        from stylerenderer_amd.op.share import share_rows_

        g = Rand(b + d + k)(b, d)
        return (lambda g: share_rows_(g, k)), [g], (0,)
    return build


for s in ((4, 1000, 300), (3, 37, 37), (16, 4099, 1)):
    add("share-rows-B%d-D%d-K%d" % s, share_rows_case(*s))


def adam_flat_case(total):
    def build():
        from stylerenderer_amd.op._dispatch import native

        r = Rand(total)
        p, g, m, v = r(total), r(total), r(total, scale=0.1), r(total).square()
        step = torch.full((), 3.0, device=DEV)

        def run(p, g, m, v, step):
            native(p).sr_adam_flat(p, g, m, v, total, 2e-3, 0.9, 0.99, 1e-8, step)
            return p, m, v
        return run, [p, g, m, v, step], (0, 2, 3)
    return build


for total in (1000, 4097, 257 * 257 * 3):
    add("adam-flat-%d" % total, adam_flat_case(total))


# ---- FIR ----------------------------------------------------------------------------------------------------------------
def upfirdn_case(shape, kernel, up, down, pad, offset=0):
    """upfirdn2d and its gradient (the adjoint resampling with the flipped taps); offset: the input as a contiguous view
    4 * offset bytes into its buffer (the scalar staging of the 4x4 tile kernel)."""
    def build():
        from stylerenderer_amd.op.upfirdn2d import upfirdn2d

        r = Rand(_seed(*shape, up, down, offset))
        n = math.prod(shape)
        buf = r(n + offset)

        def run(buf, k):
            x = buf[offset:].view(shape).requires_grad_()
            y = upfirdn2d(x, k, up=up, down=down, pad=pad)
            gy = torch.linspace(-1.0, 1.0, y.numel(), device=DEV).view(y.shape)
            return y, torch.autograd.grad(y, x, gy)[0]
        return run, [buf, kernel()], ()
    return build


def _k3():
    k1 = torch.tensor([1.0, 2.0, 1.0])
    return (k1[None, :] * k1[:, None] / 16.0).to(DEV)


for wdt in (17, 33, 65, 257):                       # the blur behind the up-sampling convolution: 2^k + 1 -> 2^k
    add("fir-blur-%d-scalar-fwd-aligned-bwd" % wdt, upfirdn_case((2, 3, wdt, wdt), _blur, 1, 1, (1, 1)))
add("fir-blur-36x40-pad2-aligned", upfirdn_case((2, 3, 36, 40), lambda: _blur(1.0), 1, 1, (2, 1)))
add("fir-blur-36x40-pad2-offset-scalar", upfirdn_case((2, 3, 36, 40), lambda: _blur(1.0), 1, 1, (2, 1), offset=1))
add("fir-blur-256-pad2-aligned", upfirdn_case((1, 2, 256, 256), _blur, 1, 1, (2, 2)))
add("fir-blur-36x40-staging-off", upfirdn_case((2, 3, 36, 40), lambda: _blur(1.0), 1, 1, (2, 1)), {"SR_FIR_ALIGNED": "0"})
for shape in ((2, 3, 70, 45), (1, 2, 33, 129), (1, 1, 5, 3), (1, 2, 257, 257)):
    tag = "x".join(map(str, shape))
    add("fir-down2-%s" % tag, upfirdn_case(shape, lambda: _blur(1.0), 1, 2, (1, 1)))
    add("fir-up2-%s" % tag, upfirdn_case(shape, _blur, 2, 1, (2, 1)))
add("fir-down2-negative-pad-2x3x70x45", upfirdn_case((2, 3, 70, 45), lambda: _blur(1.0), 1, 2, (-1, 3)))
add("fir-generic-3x3-taps-2x3x17x17", upfirdn_case((2, 3, 17, 17), _k3, 1, 1, (1, 1)))
add("fir-generic-up3-down2-1x2x33x65", upfirdn_case((1, 2, 33, 65), _blur, 3, 2, (2, 1)))


def upsample2_add_case(b, c, h, w):
    def build():
        from stylerenderer_amd.op.upfirdn2d import upsample2_add

        r = Rand(b + c * 10 + h * 100 + w)
        skip, addend, G = r(b, c, h, w, grad=True), r(b, c, 2 * h, 2 * w, grad=True), r(b, c, 2 * h, 2 * w)

        def run(skip, addend, G, k):
            y = upsample2_add(skip, k, (2, 1), addend)
            return (y,) + tuple(torch.autograd.grad(y, [skip, addend], G))
        return run, [skip, addend, G, _blur()], ()
    return build


for s in ((2, 3, 8, 8), (1, 3, 7, 5), (2, 5, 16, 12), (1, 2, 33, 9)):
    add("upsample2-add-%dx%dx%dx%d" % s, upsample2_add_case(*s))


def skip_down_case(b, c, h, w):
    def build():
        from stylerenderer_amd.op.upfirdn2d import skip_down

        r = Rand(b + c * 10 + h * 100 + w)
        oh, ow = (h - 2) // 2 + 1, (w - 2) // 2 + 1
        x, P1, P2 = r(b, c, h, w, grad=True), r(b, c, h, w), r(b, c, oh, ow)

        def run(x, P1, P2, k):
            same, down = skip_down(x, k, (1, 1))
            return down, torch.autograd.grad((same * P1).sum() + (down * P2).sum(), x)[0]
        return run, [x, P1, P2, _blur(1.0)], ()
    return build


for s in ((2, 4, 16, 16), (1, 3, 9, 7), (1, 3, 10, 6), (2, 2, 64, 32)):
    add("skip-down-%dx%dx%dx%d" % s, skip_down_case(*s))


def blur_nba_case(shape, shared):
    def build():
        from stylerenderer_amd.op.fused_elem import blur_noise_bias_act

        b, c, h, w = shape
        r = Rand(_seed(*shape, 3))
        x, noise = r(b, c, h, w, grad=True), r(1 if shared else b, 1, h - 1, w - 1)
        nw, bias, gy = r(1, grad=True), r(c, grad=True), r(b, c, h - 1, w - 1)

        def run(x, noise, nw, bias, gy, k):
            y = blur_noise_bias_act(x, k, (1, 1), noise, nw, bias)
            return (y,) + tuple(torch.autograd.grad(y, [x, nw, bias], gy))
        return run, [x, noise, nw, bias, gy, _blur()], ()
    return build


for shape, shared in (((2, 5, 33, 33), False), ((3, 4, 9, 17), True), ((1, 6, 65, 65), False), ((1, 3, 257, 257), True)):
    add("blur-noise-bias-act-%dx%dx%dx%d" % shape, blur_nba_case(shape, shared))


# ---- rasteriser -----------------------------------------------------------------------------------------------------------
def _golden_mesh(name, dtype=torch.float32):
    g = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    v = torch.from_numpy(g["v"]).to(DEV, dtype).requires_grad_()
    tex = torch.from_numpy(g["tex"]).to(DEV, dtype).requires_grad_()
    tri = torch.from_numpy(g["tri"].astype(np.int64)).to(DEV)
    return g, v, tex, tri


def raster_flat_case(name, dtype, env_tiled=False):
    def build():
        import stylerenderer_amd.op as op
        import importlib

        R = importlib.import_module("stylerenderer_amd.op.rasterize")
        g, v, tex, tri = _golden_mesh(name, dtype)
        res = g["index"].shape[1]
        go = torch.from_numpy(g["grad_out"]).to(DEV, dtype)

        def run(v, tex, tri, go):
            out = op.rasterize(v, tex, tri, res)
            gv, gt = torch.autograd.grad(out, [v, tex], go)
            chw = op.rasterize(v.detach(), tex.detach(), tri, res, channel_major=True)
            idx, coeff, zbuf = R.forward_with_depth(v.detach(), tri, res, res, False, 1e-6)
            return out, gv, gt, chw, idx, coeff, zbuf, R.backward(v.detach(), idx, False, 1e-6)
        return run, [v, tex, tri, go], ()
    return build


add("raster-flat-f32-raster_ellipsoid_32", raster_flat_case("raster_ellipsoid_32", torch.float32))
add("raster-flat-f32-tiled-raster_ellipsoid_64", raster_flat_case("raster_ellipsoid_64", torch.float32),
    {"SR_RASTER_TILED": "1"})
add("raster-flat-f64-raster_ellipsoid_32", raster_flat_case("raster_ellipsoid_32", torch.float64))


def raster_nonsquare_case(h, w, persp, dtype):
    """raster_nonsquare_cases.ab_mesh over the whole x = -1 .. 1 span of an h x w image: with h > w samples alias into
    later rows (k_resolve_alias, k_grad_pix_alias, k_grad_big_alias), with w > h rows are dropped."""
    def build():
        import importlib

        import stylerenderer_amd.op as op
        from raster_nonsquare_cases import ab_mesh

        R = importlib.import_module("stylerenderer_amd.op.rasterize")
        vh, trih = ab_mesh(h, w, persp, on_image=False)
        r = Rand(_seed(h, w, persp))
        v = torch.from_numpy(vh).to(DEV, dtype).requires_grad_()
        tex = r(2, vh.shape[1], 6).to(dtype).requires_grad_()
        tri = torch.from_numpy(trih).to(DEV)
        go = r(2, h, w, 6).to(dtype)

        def run(v, tex, tri, go):
            out = op.rasterize(v, tex, tri, h, w, persp)
            gv, gt = torch.autograd.grad(out, [v, tex], go)
            chw = op.rasterize(v.detach(), tex.detach(), tri, h, w, persp, channel_major=True)
            idx, coeff, zbuf = R.forward_with_depth(v.detach(), tri, h, w, persp, 1e-6)
            return out, gv, gt, chw, idx, coeff, zbuf, R.backward(v.detach(), idx, persp, 1e-6)
        return run, [v, tex, tri, go], ()
    return build


for _h, _w in ((20, 12), (12, 20)):
    add("raster-nonsquare-f32-orthographic-%dx%d" % (_h, _w), raster_nonsquare_case(_h, _w, False, torch.float32))
    add("raster-nonsquare-f32-perspective-%dx%d" % (_h, _w), raster_nonsquare_case(_h, _w, True, torch.float32))
    add("raster-nonsquare-f64-orthographic-%dx%d" % (_h, _w), raster_nonsquare_case(_h, _w, False, torch.float64))


@case("raster-levels-f32-raster_ellipsoid_64")
def _raster_levels():
    from stylerenderer_amd.op.rasterize import rasterize_pyramid

    g, v, tex, tri = _golden_mesh("raster_ellipsoid_64")
    sizes = [(4, 4), (8, 8), (16, 16), (24, 40), (64, 64)]
    r = Rand(64)
    ups = [r(v.shape[0], 3, h, w) for h, w in sizes]

    def run(v, tex, tri, *ups):
        maps = rasterize_pyramid(v, tex, tri, sizes, channel_major=True)      # sr_rasterize_forward_levels_f32
        f = sum((m * u).sum() for m, u in zip(maps, ups))
        return tuple(maps) + tuple(torch.autograd.grad(f, [v, tex]))          # sr_rasterize_grad_levels_f32
    return run, [v, tex, tri] + ups, ()


def overflow_mesh(persp):
    """The inputs of test_ops_gpu.test_rasterize_tiled_path_list_overflow_wide_boxes_and_tile_borders: > 2 048 small
    triangles in one 32x32 tile (list overflow), boxes over two to four tiles, boxes wider than 64 pixels, exact ties,
    an image edge (80) that is no multiple of the tile."""
    rng = np.random.RandomState(11)
    res = 80
    tris = []

    def put(cx, cy, size, z):
        a = rng.rand() * 2 * np.pi
        pts = [(cx + size * np.cos(a + k * 2.1), cy + size * np.sin(a + k * 2.1)) for k in range(3)]
        tris.append([(x, y, z + 0.01 * rng.randn()) for x, y in pts])

    for _ in range(6000):
        put(32 + 32 * rng.rand(), 32 * rng.rand(), 0.6 + 1.5 * rng.rand(), -2.0 - rng.rand())
    for _ in range(300):
        put(rng.choice([31.5, 63.5]) + rng.randn(), rng.choice([31.5, 63.5]) + rng.randn(), 1.0 + 2 * rng.rand(), -2.5)
    for _ in range(40):
        y = 80 * rng.rand()
        tris.append([(20.0, y, -3.0), (75.0, y + 0.6, -3.0), (47.0, y + 1.2, -3.0)])
    for _ in range(12):
        put(80 * rng.rand(), 80 * rng.rand(), 10 + 25 * rng.rand(), -3.5)
    for _ in range(60):
        tris.append(tris[int(rng.randint(0, 3000))])
    pix = np.asarray(tris, np.float64)
    ndc = np.empty_like(pix)
    ndc[..., 0] = (pix[..., 0] + 0.5) * 2 / res - 1
    ndc[..., 1] = 1 - (pix[..., 1] + 0.5) * 2 / res
    ndc[..., 2] = pix[..., 2]
    if persp:
        ndc[..., 0] *= -ndc[..., 2]
        ndc[..., 1] *= -ndc[..., 2]
    v1 = ndc.reshape(-1, 3).astype(np.float32)
    nf = pix.shape[0]
    tri = np.arange(3 * nf, dtype=np.int64).reshape(nf, 3)
    flip = rng.rand(nf) < 0.5
    tri[flip] = tri[flip][:, ::-1]
    return np.stack([v1, v1 * np.float32(0.97)], 0), tri, res


def raster_overflow_case(persp):
    def build():
        import importlib

        R = importlib.import_module("stylerenderer_amd.op.rasterize")
        v, tri, res = overflow_mesh(persp)
        v, tri = torch.from_numpy(v).to(DEV), torch.from_numpy(tri).to(DEV)
        return (lambda v, tri: R.forward_with_depth(v, tri, res, res, persp, 1e-6)), [v, tri], ()
    return build


for persp in (False, True):
    add("raster-tiled-list-overflow-%s" % ("perspective" if persp else "orthographic"), raster_overflow_case(persp),
        {"SR_RASTER_TILED": "1"})


@case("vertex-normals-forward-and-backward")
def _vertex_normals():
    from stylerenderer_amd import utils_3d
    from stylerenderer_amd.op import morph

    g, v, _, tri = _golden_mesh("raster_ellipsoid_32")
    v = v.detach()
    gn = Rand(12)(*v.shape)

    def run(v, tri, gn):
        return utils_3d.mesh_point_normal(v, tri), morph.vertex_normals_backward(v, tri, gn)
    return run, [v, tri, gn], ()
