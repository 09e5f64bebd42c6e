"""Shape-selected kernel variants on both sides of their dispatch thresholds, each against a float64 CPU reference of the
same operation, with the variant that ran asserted from the profiler's kernel names.

Bars are per element against the float64 sum of absolute products (mag) of that element, as in test_conv_vs_float64:
a float32 sum of K products carries at most (K' + 1) * 2^-24 * mag of round-off, K' the longest serial chain of the
kernel's summation order.  Where two variants differ only in template arguments and the profiler's names do not carry
them (util.kernel_ran), the rule and the value it gives for the case are stated beside the case."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conv_plan_cases import FORWARD, STRIPS, SWITCHES, WGRAD, case_id, conv_args
from util import bits_equal, kernel_ran, launched_kernels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24                  # float32 unit round-off


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _check(got, want, mag, bar, what):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    ratio = float(((got - want).abs() / (mag + 1e-30)).max())
    assert ratio <= bar, "%s: error %.3e of the absolute-product sum (bar %.1e)" % (what, ratio, bar)


# ---- ToRGB 1x1 convolution (csrc/fused_elem.hip sr_smallconv_*) -------------------------------------------------------
# forward: 16 waves iff ceil(hw / 256) * B < 1024 && C >= 64, else 4
# weight gradient: chunks = ceil(hw / 4096) (one chunk is stored directly, more go through k_smallconv_dw_finish),
#                  CH = 4 channels per workgroup iff C % 4 == 0; the bias sum covers B * chunks entries (k_smallconv_gb_finish)
SMALLCONV = [
    # (B, C, N, H, W, bias)   forward waves | dw chunks, CH | bias entries
    (1, 128, 1, 64, 64, True),      # 16 (16 blocks)        | 1, 4  | 1
    (1, 100, 2, 64, 64, False),     # 16, C % 16 != 0       | 1, 4  | -
    (2, 70, 4, 32, 32, True),       # 16, waves 14, 15 idle | 1, 1  | 2
    (15, 64, 3, 128, 128, True),    # 16 (960 blocks)       | 4, 4  | 60
    (16, 64, 4, 128, 128, True),    # 4 (1024 blocks)       | 4, 4  | 64
    (16, 63, 2, 128, 128, False),   # 4 (C < 64)            | 4, 1  | -
    (4, 64, 1, 256, 256, True),     # 4 (1024 blocks)       | 16, 4 | 64
    (8, 6, 3, 256, 256, True),      # 4 (C < 64)            | 16, 1 | 128
]


@pytest.mark.parametrize("case", SMALLCONV, ids=lambda c: "B%d-C%d-N%d-%dx%d-%s" % (c[:5] + ("bias" if c[5] else "nobias",)))
def test_smallconv_forward_and_gradients_vs_float64(case):
    from stylerenderer_amd.op.smallconv import SmallConvFwd

    b, c, n, h, w, with_bias = case
    g = _gen(b * 1000 + c * 10 + n)
    x, ws, gy = torch.randn(b, c, h, w, generator=g), torch.randn(b, n, c, generator=g), torch.randn(b, n, h, w, generator=g)
    bias = torch.randn(n, generator=g) if with_bias else None
    xd, wd = x.to(DEV).requires_grad_(), ws.to(DEV).requires_grad_()
    bd = bias.to(DEV).requires_grad_() if with_bias else None

    def run():
        y = SmallConvFwd.apply(xd, wd, bd)
        grads = torch.autograd.grad(y, [xd, wd] + ([bd] if with_bias else []), gy.to(DEV))
        return (y,) + tuple(grads)

    got, names = launched_kernels(run)
    wide = math.ceil(h * w / 256) * b < 1024 and c >= 64
    chunks = math.ceil(h * w / 4096)
    assert kernel_ran(names, "k_smallconv_fwd", "<%d, %d>" % (n, 16 if wide else 4)), names
    assert kernel_ran(names, "k_smallconv_dx"), names
    assert kernel_ran(names, "k_smallconv_dw", "<%d, %d>" % (n, 4 if c % 4 == 0 else 1)), names
    assert kernel_ran(names, "k_smallconv_dw_finish") == (chunks > 1), names
    assert kernel_ran(names, "k_smallconv_gb_finish") == with_bias, names

    X, W, G = x.double(), ws.double(), gy.double()
    y = torch.einsum("bjc,bchw->bjhw", W, X)
    y_mag = torch.einsum("bjc,bchw->bjhw", W.abs(), X.abs())
    if with_bias:
        y = y + bias.double()[None, :, None, None]
        y_mag = y_mag + bias.double().abs()[None, :, None, None]
    # forward: chains of ceil(C / waves) <= 16 products (2 roundings each), <= 15 wave partials, the bias: < 50 -> 3e-6
    _check(got[0], y, y_mag, 3e-6, "out")
    # data gradient: N <= 4 products and 3 adds: 7 roundings -> 8 * 2^-24
    _check(got[1], torch.einsum("bjc,bjhw->bchw", W, G), torch.einsum("bjc,bjhw->bchw", W.abs(), G.abs()), 8 * U, "dx")
    # weight gradient: <= 4 float4 steps of 4 products per lane, 6 + 2 levels of wave / workgroup sums, <= 16 chunks
    # summed over the finish wave's 6 levels: < 30 roundings -> 2e-6
    _check(got[2], torch.einsum("bjhw,bchw->bjc", G, X), torch.einsum("bjhw,bchw->bjc", G.abs(), X.abs()), 2e-6, "dws")
    if with_bias:
        _check(got[3], G.sum((0, 2, 3)), G.abs().sum((0, 2, 3)), 2e-6, "gb")


# sr_smallconv_dx_add: groups = clamp(ceil(2048 / (ceil(hw4 / 256) * B)), 1, ceil(C / 8)), cgroup = ceil(ceil(C / groups) / 8) * 8
SMALLCONV_DX = [
    # (B, C, N, H, W)        groups x cgroup (last group)
    (2, 8, 3, 32, 32),       # 1 x 8
    (3, 6, 4, 16, 16),       # 1 x 8 (6: the addend's tail loop only)
    (1, 128, 3, 64, 64),     # 16 x 8
    (1, 100, 3, 64, 64),     # 13 x 8 (4)
    (4, 100, 2, 256, 256),   # 7 x 16 (4)
    (2, 69, 1, 32, 32),      # 9 x 8 (5)
]


def _dx_groups(b, c, hw):
    wgs = math.ceil(hw // 4 / 256) * b
    groups = min(max(math.ceil(2048 / wgs), 1), math.ceil(c / 8))
    cg = math.ceil(math.ceil(c / groups) / 8) * 8
    return math.ceil(c / cg), cg


def test_smallconv_dx_group_table():
    """The table above is what the C++ rule gives."""
    want = [(1, 8), (1, 8), (16, 8), (13, 8), (7, 16), (9, 8)]
    assert [_dx_groups(b, c, h * w) for b, c, n, h, w in SMALLCONV_DX] == want


@pytest.mark.parametrize("case", SMALLCONV_DX, ids=lambda c: "B%d-C%d-N%d-%dx%d" % c)
@pytest.mark.parametrize("fused", [True, False], ids=["addend", "plain"])
def test_smallconv_fork_dx_addend_vs_float64(case, fused):
    """SmallConvFork: the feature map's other gradient added inside k_smallconv_dx (first-order backward) or, with a
    recorded backward, the plain kernel plus a separate addition; both against float64."""
    from stylerenderer_amd.op.smallconv import SmallConvFork

    b, c, n, h, w = case
    g = _gen(b * 100 + c + n)
    x, ws = torch.randn(b, c, h, w, generator=g), torch.randn(b, n, c, generator=g)
    gy, probe = torch.randn(b, n, h, w, generator=g), torch.randn(b, c, h, w, generator=g)
    xd = x.to(DEV).requires_grad_()
    wd = ws.to(DEV)

    def run():
        same, rgb = SmallConvFork.apply(xd, wd, None)
        loss = (same * probe.to(DEV)).sum() + (rgb * gy.to(DEV)).sum()
        return torch.autograd.grad(loss, xd, create_graph=not fused)[0]

    gx, names = launched_kernels(run)
    assert kernel_ran(names, "k_smallconv_dx"), names
    W, G, P = ws.double(), gy.double(), probe.double()
    want = P + torch.einsum("bjc,bjhw->bchw", W, G)
    mag = P.abs() + torch.einsum("bjc,bjhw->bchw", W.abs(), G.abs())
    # N <= 4 products, 3 adds, then the addend: 8 roundings -> 10 * 2^-24
    _check(gx, want, mag, 10 * U, "dx + addend")


# ---- StyledMapConv tail (csrc/fused_elem.hip aff_cgroup, k_nba_aff_fwd / bwd / bwd2, k_plane_sum[_strided]) -----------
# wgs = ceil(hw / 1024) * B; groups = min(ceil(2048 / wgs), cap, C) with cap = 64 iff wgs * 16 < 256 else 16;
# cgroup = ceil(C / groups)
AFF = [
    # (B, C, H, W, per-sample noise)   groups x cgroup
    (2, 1, 32, 32, False),             # 1 x 1: no plane sum
    (4, 128, 64, 64, True),            # cap 16: 16 x 8
    (1, 128, 64, 64, False),           # cap 64: 64 x 2
    (1, 69, 32, 32, True),             # cap 64: 35 x 2, the last of 1 (35 groups: 9 + 9 + 9 + 8 per wave)
]


def _aff_groups(b, c, hw):
    wgs = math.ceil(hw / 1024) * b
    cap = 64 if wgs * 16 < 256 else 16
    cg = math.ceil(c / max(min(math.ceil(2048 / wgs), cap, c), 1))
    return math.ceil(c / cg), cg


def test_aff_group_table():
    assert [_aff_groups(b, c, h * w) for b, c, h, w, _ in AFF] == [(1, 1), (16, 8), (64, 2), (35, 2)]


def _aff_reference(t, slope, gain, absolute=False):
    """y, first-order gradients and the second-order pass of the tail in float64 (the sign mask m from the float64
    pre-activation, which the inputs keep away from zero).  absolute: the same sums over absolute values (the bars)."""
    A = (lambda v: v.abs()) if absolute else (lambda v: v)
    x, a, s, nz, nw, bias, gy = (A(t[k]) for k in ("x", "a", "s", "noise", "nw", "bias", "gy"))
    Px, Pa, Ps, Pb, Pnw = (A(t[k]) for k in ("Px", "Pa", "Ps", "Pb", "Pnw"))
    m = t["m"]
    bb = bias[None, :, None, None]
    v = x * a + s + nw * nz + bb
    r = gy * m
    out = {"y": m * v, "gx": r * a, "ga": (r * x).sum(1), "gs": r.sum(1), "gb": r.sum((0, 2, 3)),
           "gnw": (r * nz).sum().reshape(1)}
    out["d_gy"] = m * (Px * a + Pa[:, None] * x + Ps[:, None] + Pb[None, :, None, None] + Pnw * nz)
    out["d_x"] = r * Pa[:, None]
    out["d_a"] = (r * Px).sum(1)
    return out


@pytest.mark.parametrize("case", AFF, ids=lambda c: "B%d-C%d-%dx%d-%s" % (c[:4] + ("bnoise" if c[4] else "noise1",)))
def test_styled_map_tail_vs_float64(case):
    """Forward, first-order gradients (x, both map planes, bias, noise strength) and the second-order pass (gradients
    of the first-order results' projections w.r.t. gy, x and the scale plane), with smap2 a channel slice of a
    4-channel map as GeneratorWithMap hands it."""
    from stylerenderer_amd.op.fused_elem import noise_bias_act_affine

    b, c, h, w, per_sample = case
    slope, gain, lo = 0.2, math.sqrt(2.0), 1
    g = _gen(b * 7 + c * 3 + h)
    x = torch.randn(b, c, h, w, generator=g, dtype=torch.float64)
    amap = torch.randn(b, 4, h, w, generator=g, dtype=torch.float64)
    amap[:, lo] = 0.5 + amap[:, lo].abs()                          # the scale plane: |a| >= 0.5
    noise = torch.randn(b if per_sample else 1, 1, h, w, generator=g, dtype=torch.float64)
    nw, bias = torch.randn(1, generator=g, dtype=torch.float64), torch.randn(c, generator=g, dtype=torch.float64)
    a, s = amap[:, lo:lo + 1], amap[:, lo + 1:lo + 2]
    # keep the pre-activation at least 1e-2 from the kink, so that float32 and float64 take the same slope
    v = x * a + s + nw * noise + bias[None, :, None, None]
    x = x + torch.where(v.abs() < 1e-2, (torch.where(v < 0, -2e-2, 2e-2) - v) / a, torch.zeros_like(v))
    x, amap, noise, nw, bias = (t.float() for t in (x, amap, noise, nw, bias))
    gy = torch.randn(b, c, h, w, generator=g)
    Px, Pm = torch.randn(b, c, h, w, generator=g), torch.randn(b, 4, h, w, generator=g)
    Pb, Pnw = torch.randn(c, generator=g), torch.randn(1, generator=g)

    xd, md, nwd, bd, gyd = (t.to(DEV).requires_grad_() for t in (x, amap, nw, bias, gy))

    def run():
        y = noise_bias_act_affine(xd, md[:, lo:lo + 2], noise.to(DEV), nwd, bd, slope, gain)
        gx, gm, gb, gnw = torch.autograd.grad(y, [xd, md, bd, nwd], gyd, create_graph=True)
        q = ((gx * Px.to(DEV)).sum() + (gm * Pm.to(DEV)).sum() + (gb * Pb.to(DEV)).sum() + (gnw * Pnw.to(DEV)).sum())
        d_gy, d_x, d_m = torch.autograd.grad(q, [gyd, xd, md])
        return y, gx, gm, gb, gnw, d_gy, d_x, d_m

    (y, gx, gm, gb, gnw, d_gy, d_x, d_m), names = launched_kernels(run)
    groups, _ = _aff_groups(b, c, h * w)
    for k in ("k_nba_aff_fwd", "k_nba_aff_bwd", "k_nba_aff_bwd2", "k_plane_sum_strided"):
        assert kernel_ran(names, k), (k, names)
    assert kernel_ran(names, "k_plane_sum") == (groups > 1), names

    D = lambda t: t.double()  # noqa: E731
    t = {"x": D(x), "a": D(amap[:, lo:lo + 1]), "s": D(amap[:, lo + 1:lo + 2]), "noise": D(noise), "nw": D(nw),
         "bias": D(bias), "gy": D(gy), "Px": D(Px), "Pa": D(Pm[:, lo]), "Ps": D(Pm[:, lo + 1]), "Pb": D(Pb),
         "Pnw": D(Pnw)}
    v = t["x"] * t["a"] + t["s"] + t["nw"] * t["noise"] + t["bias"][None, :, None, None]
    t["m"] = torch.where(v > 0, 1.0, slope) * gain
    want, mag = _aff_reference(t, slope, gain), _aff_reference(t, slope, gain, absolute=True)
    # element-wise results: <= 8 roundings (10 * 2^-24); channel sums: chains of cgroup <= 8 plus a 4 x 16-deep plane
    # sum; bias / noise-strength sums over B * H * W: per-wave partials and the finish tree; all < 40 roundings -> 3e-6
    _check(y, want["y"], mag["y"], 10 * U, "y")
    _check(gx, want["gx"], mag["gx"], 10 * U, "gx")
    zero = torch.zeros(b, h, w, dtype=torch.float64)
    gm_want = torch.stack([zero, want["ga"], want["gs"], zero], 1)
    gm_mag = torch.stack([zero, mag["ga"], mag["gs"], zero], 1)
    _check(gm, gm_want, gm_mag, 3e-6, "g_map")
    _check(gb, want["gb"], mag["gb"], 3e-6, "g_bias")
    _check(gnw, want["gnw"], mag["gnw"], 3e-6, "g_noise_w")
    _check(d_gy, want["d_gy"], mag["d_gy"], 10 * U, "second order: d gy")
    _check(d_x, want["d_x"], mag["d_x"], 10 * U, "second order: d x")
    dm_want = torch.stack([zero, want["d_a"], zero, zero], 1)
    dm_mag = torch.stack([zero, mag["d_a"], zero, zero], 1)
    _check(d_m, dm_want, dm_mag, 3e-6, "second order: d map")


# ---- weight gradients (csrc/conv_wgrad_dispatch.hip and the conv_wgrad_*.hip it launches) -----------------------------
def _wgrad_reference(x, gy, xs, gs, k):
    def f(xx, gg, a, bsc):
        xx = xx * a[:, :, None, None] if a is not None else xx
        gg = gg * bsc[:, :, None, None] if bsc is not None else gg
        dw = torch.nn.grad.conv2d_weight(xx, (gg.shape[1], xx.shape[1], k, k), gg, padding=k // 2)
        return dw.permute(2, 3, 1, 0).reshape(k * k, xx.shape[1], gg.shape[1])

    D = lambda t: None if t is None else t.double()  # noqa: E731
    A = lambda t: None if t is None else t.double().abs()  # noqa: E731
    return f(D(x), D(gy), D(xs), D(gs)), f(A(x), A(gy), A(xs), A(gs))


def _wgrad_case(b, c, n, h, w, k, scaled, seed):
    from stylerenderer_amd.op.conv import conv2d_wgrad_mfma

    g = _gen(seed)
    x, gy = torch.randn(b, c, h, w, generator=g), torch.randn(b, n, h, w, generator=g)
    xs = torch.randn(b, c, generator=g) if scaled else None
    gs = torch.randn(b, n, generator=g) if scaled else None
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    got, names = launched_kernels(lambda: conv2d_wgrad_mfma(dev(x), dev(gy), dev(xs), dev(gs), ksize=k, stride=1,
                                                            pad=k // 2))
    want, mag = _wgrad_reference(x, gy, xs, gs, k)
    return got, want, mag, names


# wgrad_small_ok: 3x3 stride 1 pad 1, C <= 4, N <= 4; blocks = clamp(ceil(B * H * W / 1024), 1, 256) in a grid-stride loop
SMALL3 = ([(c, n, 2, 24, 20, (c + n) % 2 == 0) for c in range(1, 5) for n in range(1, 5)]    # 960 pixels: 1 block
          + [(3, 4, 4, 256, 256, s) for s in (False, True)]                                  # 256 * 1024: 256 blocks, one pass
          + [(4, 3, 5, 256, 256, s) for s in (False, True)])                                 # 256 blocks, 1.25 passes


@pytest.mark.parametrize("case", SMALL3, ids=lambda c: "C%d-N%d-B%d-%dx%d-%s" % (c[:5] + ("scaled" if c[5] else "plain",)))
def test_wgrad_small3_vs_float64(case):
    c, n, b, h, w, scaled = case
    got, want, mag, names = _wgrad_case(b, c, n, h, w, 3, scaled, c * 10 + n + b)
    assert kernel_ran(names, "k_wgrad_small3") and kernel_ran(names, "k_wgrad_small3_finish"), names
    # a lane's <= 5 grid-stride pixels (<= 4 roundings each with the operand scales), 6 + 2 levels of shuffle / LDS
    # folds, <= 64 slabs per finish lane + 2 levels: < 100 roundings -> 6e-6
    _check(got, want, mag, 6e-6, "dwt")


# launch_wgrad_reduce: k_wgrad_reduce_wave iff total = k*k * C * N <= 1024 && ks >= 32 (ks = K slices of make_plan times
# the two groups of a single-sample patch workgroup); 1x1 stride 1 on one 32-wide patch column per 2 rows
REDUCE = [
    # (B, C, N, H, W)     total, ks -> form
    (1, 32, 32, 16, 64),  # 1024, 32  -> wave
    (2, 8, 16, 64, 64),   # 128, 256  -> wave (lanes walk four slices each)
    (1, 32, 32, 14, 64),  # 1024, 28  -> plain
    (1, 32, 33, 16, 64),  # 1056, 32  -> plain
    (1, 8, 16, 8, 8),     # 128, 2    -> plain
]


@pytest.mark.parametrize("case", REDUCE, ids=lambda c: "B%d-C%d-N%d-%dx%d" % c)
def test_wgrad_split_k_reduce_forms_vs_float64(case):
    b, c, n, h, w = case
    wave = case in REDUCE[:2]
    got, want, mag, names = _wgrad_case(b, c, n, h, w, 1, False, b + c + n + h)
    assert kernel_ran(names, "k_wgrad_reduce_wave") == wave, names
    assert kernel_ran(names, "k_wgrad_reduce") == (not wave), names
    # MFMA steps of 2 products over one 64-pixel patch per slice (64 roundings), <= 256 slices in <= 4-deep lane chains
    # and 6 levels, or <= 32 slices in one chain: < 100 roundings -> 6e-6
    _check(got, want, mag, 6e-6, "dwt")


# ---- 1x1 convolution as a GEMM (csrc/conv1x1_gemm.hip): tiles (P / 128) * (N / 128) * B >= 256 -------------------------
@pytest.mark.parametrize("hw", [(64, 64), (64, 62)], ids=["256tiles-gemm", "248tiles-window"])
@pytest.mark.parametrize("with_addend", [False, True], ids=["plain", "add"])
def test_conv1x1_gemm_threshold_vs_float64(hw, with_addend):
    from stylerenderer_amd.op import conv as C

    b, c, n = 4, 64, 256
    h, w = hw
    gemm = (h * w // 128) * (n // 128) * b >= 256
    g = _gen(h * w + with_addend)
    x, wt, osc = torch.randn(b, c, h, w, generator=g), torch.randn(1, c, n, generator=g), torch.randn(b, n, generator=g)
    add, gy = torch.randn(b, n, h, w, generator=g), torch.randn(b, n, h, w, generator=g)
    xd, wd = x.to(DEV).requires_grad_(), wt.to(DEV).requires_grad_()

    def run():
        if with_addend:
            y = C.conv1x1_add(xd, wd, osc.to(DEV), add.to(DEV))
        else:
            y = C.conv2d(xd, wd, None, osc.to(DEV), None, "c1")
        return (y.detach(),) + tuple(torch.autograd.grad(y, [xd, wd], gy.to(DEV)))

    (y, gx, gw), names = launched_kernels(run)
    assert kernel_ran(names, "k_conv1x1_gemm") == gemm, names
    X, Wt, S, A, G = (t.double() for t in (x, wt[0], osc, add, gy))
    y_want = torch.einsum("cn,bchw->bnhw", Wt, X) * S[:, :, None, None]
    y_mag = torch.einsum("cn,bchw->bnhw", Wt.abs(), X.abs()) * S.abs()[:, :, None, None]
    if with_addend:
        y_want, y_mag = y_want + A, y_mag + A.abs()
    GS, GSa = G * S[:, :, None, None], G.abs() * S.abs()[:, :, None, None]
    # out: a chain of 64 products, the scale and the addend (< 2 * 64 + 2 roundings, the convolution tests' 2e-6 holds
    # the typical error far below); dx: 256 products (5e-6); dw: 4 patches of 64 pixels per slice and a 128-slice
    # reduce chain (< 300 roundings -> 2e-5)
    _check(y, y_want, y_mag, 2e-6, "out")
    _check(gx, torch.einsum("cn,bnhw->bchw", Wt, GS), torch.einsum("cn,bnhw->bchw", Wt.abs(), GSa), 5e-6, "dx")
    _check(gw, torch.einsum("bchw,bnhw->cn", X, GS)[None], torch.einsum("bchw,bnhw->cn", X.abs(), GSa)[None], 2e-5, "dw")


# ---- ToRGB skip and ResBlock fork (op/upfirdn2d.py UpsampleAdd, SkipDown) ----------------------------------------------
def _blur(factor):
    import ops_np

    return torch.from_numpy(ops_np.make_blur_kernel((1, 3, 3, 1), float(factor ** 2)))


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 3, 7, 5), (2, 5, 16, 12), (1, 2, 33, 9)], ids=str)
def test_upsample2_add_vs_float64(shape):
    """Generator skip (pad (2, 1), the 4x4 up-sampling FIR plus the image in one kernel): value, the gradients of both
    inputs and the second-order gradient through the skip gradient."""
    from stylerenderer_amd.op.upfirdn2d import _upfirdn2d_cpu, upsample2_add

    b, c, h, w = shape
    pad = (2, 1)
    k = _blur(2)
    g = _gen(b + c * 10 + h * 100 + w)
    skip, add = torch.randn(b, c, h, w, generator=g), torch.randn(b, c, 2 * h, 2 * w, generator=g)
    G, R = torch.randn(b, c, 2 * h, 2 * w, generator=g), torch.randn(b, c, h, w, generator=g)

    def run(dev, dt, kk):
        s, a, gg = (t.to(dev, dt).requires_grad_() for t in (skip, add, G))
        y = (upsample2_add(s, kk.to(dev, dt), pad, a) if dev != "cpu"
             else a + _upfirdn2d_cpu(s, kk.to(dt), 2, 1, pad))
        gs, ga = torch.autograd.grad(y, [s, a], gg, create_graph=True)
        (dg,) = torch.autograd.grad((gs * R.to(dev, dt)).sum(), gg)
        return y, gs, ga, dg

    (y, gs, ga, dg), names = launched_kernels(lambda: run(DEV, torch.float32, k))
    assert kernel_ran(names, "k_fir4_resample", "<2, 1>"), names
    want = run("cpu", torch.float64, k)
    skip_a, add_a, G_a, R_a = skip.abs(), add.abs(), G.abs(), R.abs()
    mag = add_a.double() + _upfirdn2d_cpu(skip_a.double(), k.abs().double(), 2, 1, pad)
    # up = 2: 4 nonzero taps (4 products, 3 adds) and the addend: 8 roundings -> 10 * 2^-24; the skip gradient is the
    # 16-tap down-sampling FIR: 31 roundings -> 32 * 2^-24; the addend's gradient is the cotangent itself
    _check(y, want[0].detach(), mag, 10 * U, "out")
    s_req = skip_a.double().requires_grad_()
    (gs_mag,) = torch.autograd.grad(_upfirdn2d_cpu(s_req, k.double(), 2, 1, pad), s_req, G_a.double())
    _check(gs, want[1].detach(), gs_mag, 32 * U, "g skip")
    _check(ga, want[2].detach(), G_a.double(), 0.0, "g addend")
    _check(dg, want[3].detach(), _upfirdn2d_cpu(R_a.double(), k.double(), 2, 1, pad), 10 * U, "second order")


@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (1, 3, 9, 7), (1, 3, 10, 6), (2, 2, 64, 32)], ids=str)
def test_skip_down_equals_two_consumers_and_float64(shape):
    """Discriminator ResBlock fork (pad (1, 1), down 2): SkipDown's backward is upsample2_add with its own g_pad; all
    gradients against the two-consumer form (x and upfirdn2d(x, down=2)) and against float64, to second order."""
    from stylerenderer_amd.op.upfirdn2d import _upfirdn2d_cpu, skip_down, upfirdn2d

    b, c, h, w = shape
    pad = (1, 1)
    k = _blur(1)
    g = _gen(b + c * 10 + h * 100 + w)
    x = torch.randn(b, c, h, w, generator=g)
    oh, ow = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    P1, P2, R = torch.randn(b, c, h, w, generator=g), torch.randn(b, c, oh, ow, generator=g), torch.randn(b, c, h, w, generator=g)

    def run(dev, dt, fused):
        xx, p2 = x.to(dev, dt).requires_grad_(), P2.to(dev, dt).requires_grad_()
        kk = k.to(dev, dt)
        if dev == "cpu":
            same, down = xx, _upfirdn2d_cpu(xx, kk, 1, 2, pad)
        elif fused:
            same, down = skip_down(xx, kk, pad)
        else:
            same, down = xx, upfirdn2d(xx, kk, down=2, pad=pad)
        loss = (same * P1.to(dev, dt)).sum() + (down * p2).sum()
        (gx,) = torch.autograd.grad(loss, xx, create_graph=True)
        (dp2,) = torch.autograd.grad((gx * R.to(dev, dt)).sum(), p2)
        return down, gx, dp2

    (down, gx, dp2), names = launched_kernels(lambda: run(DEV, torch.float32, True))
    assert kernel_ran(names, "k_fir4_resample", "<1, 2>") and kernel_ran(names, "k_fir4_resample", "<2, 1>"), names
    ref = run(DEV, torch.float32, False)
    want = run("cpu", torch.float64, False)
    for a, r, what in zip((down, gx, dp2), ref, ("down", "gx", "second order")):
        assert float((a - r).abs().max()) <= 1e-6 * float(r.abs().max()), what
    K, X = k.double().abs(), x.double().abs()
    p2_req = P2.double().abs().requires_grad_()
    # down 2: 16 taps, 31 roundings -> 32 * 2^-24; its transpose (4 taps) plus the other consumer's gradient: 10 * 2^-24
    _check(down, want[0].detach(), _upfirdn2d_cpu(X, K, 1, 2, pad), 32 * U, "down")
    xr = X.clone().requires_grad_()
    (gmag,) = torch.autograd.grad(_upfirdn2d_cpu(xr, K, 1, 2, pad), xr, p2_req.detach())
    _check(gx, want[1].detach(), gmag + P1.double().abs(), 10 * U, "gx")
    _check(dp2, want[2].detach(), _upfirdn2d_cpu(R.double().abs(), K, 1, 2, pad), 32 * U, "second order")


# ---- FIR staging (csrc/upfirdn2d.hip fir4_aligned: pad_x0 == 2, in_w % 4 == 0, 16-byte base; SR_FIR_ALIGNED=0 off) -----
_FIR_CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = sys.argv[2:]
import test_dispatch_edges_gpu as T
np.savez(sys.argv[1], **T._fir_outputs())
"""


def _fir_nba_params():
    g = _gen(6)
    return {"nw": torch.randn(1, generator=g, dtype=torch.float64), "bias": torch.randn(5, generator=g, dtype=torch.float64)}


def _fir_outputs(offset=0):
    """upfirdn2d (blur, pad 2) and sr_blur_nba_bwd (256 -> 257, pad 1) on fixed inputs; offset: the inputs as contiguous
    views 4 * offset bytes into their buffers."""
    from stylerenderer_amd.op.conv import _blur_nba_bwd
    from stylerenderer_amd.op.upfirdn2d import flipped, upfirdn2d

    def dev(t):
        buf = torch.empty(t.numel() + offset, device=DEV)
        buf[offset:] = t.reshape(-1).to(DEV)
        return buf[offset:].view(t.shape)

    g = _gen(5)
    x = torch.randn(2, 3, 36, 40, generator=g)
    k = _blur(1)
    out = {"fir": upfirdn2d(dev(x), k.to(DEV), pad=(2, 1)).cpu().numpy()}
    b, c, hh = 2, 5, 32
    gy, y = torch.randn(b, c, hh, hh, generator=g), torch.randn(b, c, hh, hh, generator=g)
    noise = torch.randn(1, 1, hh, hh, generator=g)
    nw, bias = _fir_nba_params()["nw"].float(), _fir_nba_params()["bias"].float()
    g257, gb, gnw, rdot = _blur_nba_bwd(dev(gy), dev(y), flipped(k.to(DEV)), 1, (b, c, hh + 1, hh + 1), noise.to(DEV),
                                        nw.to(DEV), bias.to(DEV), 0.2, math.sqrt(2.0))
    out.update(g257=g257.cpu().numpy(), gb=gb.cpu().numpy(), gnw=gnw.cpu().numpy(), rdot=rdot.cpu().numpy())
    out.update(x=x.numpy(), gy=gy.numpy(), y=y.numpy(), noise=noise.numpy())
    return out


def test_fir_aligned_and_scalar_staging_agree_with_the_oracle(tmp_path):
    import ops_np
    from stylerenderer_amd.op.upfirdn2d import _upfirdn2d_cpu

    aligned, names = launched_kernels(_fir_outputs)
    assert kernel_ran(names, "k_fir4_tile", "<false, true>") and kernel_ran(names, "k_fir4_nba_bwd", "<true>"), names
    shifted, names_s = launched_kernels(lambda: _fir_outputs(1))
    assert kernel_ran(names_s, "k_fir4_tile", "<false, false>") and kernel_ran(names_s, "k_fir4_nba_bwd", "<false>"), names_s
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, SR_FIR_ALIGNED="0")
    dst = str(tmp_path / "scalar.npz")
    run = subprocess.run([sys.executable, "-c", _FIR_CHILD, dst, here, root, os.path.join(root, "oracle")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    scalar = dict(np.load(dst))
    # the FIR outputs are bit for bit the same under both stagings; the bias / noise / row-dot sums are not (the two
    # stagings hand the owned pixels to different lanes: another summation order), so those are held to float64 below —
    # but a misaligned input takes the scalar staging and must reproduce it exactly
    for key in ("fir", "g257"):
        assert bits_equal(aligned[key], scalar[key]), key
        assert bits_equal(aligned[key], shifted[key]), key
    for key in ("gb", "gnw", "rdot"):
        assert bits_equal(scalar[key], shifted[key]), key
    # the blur itself: bit for bit the numpy oracle's order
    k = ops_np.make_blur_kernel((1, 3, 3, 1), 1.0)
    assert bits_equal(aligned["fir"], ops_np.upfirdn2d(aligned["x"], k, 1, 1, (2, 1)))
    # the fused backward: blur^T(lrelu'(y) * gy * gain) and its two sums, against float64
    gain = math.sqrt(2.0)
    m = torch.where(torch.from_numpy(aligned["y"]).double() > 0, 1.0, 0.2) * gain
    gpre = torch.from_numpy(aligned["gy"]).double() * m
    kd = torch.from_numpy(k).double()
    x257 = torch.zeros(gpre.shape[:2] + (gpre.shape[2] + 1, gpre.shape[3] + 1), dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(_upfirdn2d_cpu(x257, kd, 1, 1, (1, 1)), x257, gpre)
    (mag,) = torch.autograd.grad(_upfirdn2d_cpu(x257, kd.abs(), 1, 1, (1, 1)), x257, gpre.abs())
    # the slope product (2 roundings), then 16 taps (31): 40 * 2^-24
    _check(torch.from_numpy(aligned["g257"]), want, mag, 40 * U, "g257")
    nz = torch.from_numpy(aligned["noise"]).double()
    y = torch.from_numpy(aligned["y"]).double()
    nwb = {k: v.float().double() for k, v in _fir_nba_params().items()}      # the float32 values the device used
    # the row dot: sum over pixels of gpre times the blur's output, recovered from the activation output
    pre = torch.where(y > 0, y / gain, y / (0.2 * gain))
    blur = pre - nwb["nw"] * nz - nwb["bias"][None, :, None, None]
    blur_mag = pre.abs() + (nwb["nw"] * nz).abs() + nwb["bias"].abs()[None, :, None, None]
    # per-lane partials over a 32 x 32 tile, wave / workgroup trees, the finish over the tiles: < 30 roundings -> 2e-6
    for res in (aligned, scalar):
        _check(torch.from_numpy(res["gb"]), gpre.sum((0, 2, 3)), gpre.abs().sum((0, 2, 3)), 2e-6, "gb")
        _check(torch.from_numpy(res["gnw"]), (gpre * nz).sum().reshape(1), (gpre * nz).abs().sum().reshape(1), 2e-6, "gnw")
        _check(torch.from_numpy(res["rdot"]), (gpre * blur).sum((2, 3)), (gpre.abs() * blur_mag).sum((2, 3)), 2e-6, "rdot")


# ---- ToRGB path on contiguous inputs at a 4-byte storage offset -------------------------------------------------------
def _offset(t, offset=1):
    buf = torch.empty(t.numel() + offset, device=DEV)
    buf[offset:] = t.reshape(-1).to(DEV)
    return buf[offset:].view(t.shape)


def test_torgb_path_on_misaligned_contiguous_inputs():
    from stylerenderer_amd.layers import ModulatedConv2d
    from stylerenderer_amd.op.conv import conv2d_wgrad_mfma
    from stylerenderer_amd.op.smallconv import modulated_conv1x1_small

    b, c, n, h, w = 2, 64, 3, 16, 16
    g = _gen(77)
    x, wgt, s = torch.randn(b, c, h, w, generator=g), torch.randn(n, c, generator=g), torch.randn(b, c, generator=g)
    bias, gy = torch.randn(n, generator=g), torch.randn(b, n, h, w, generator=g)

    def small(xd):
        xd = xd.requires_grad_()
        wd, sd, bd = (t.to(DEV).requires_grad_() for t in (wgt, s, bias))
        y = modulated_conv1x1_small(xd, wd, sd, bd, scale=0.125)
        return [y.detach()] + list(torch.autograd.grad(y, [xd, wd, sd, bd], gy.to(DEV)))

    xo = _offset(x)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 4
    got, ref = small(xo), small(x.to(DEV))
    for a, r in zip(got, ref):
        assert torch.equal(a, r)
    X, W, S = x.double(), wgt.double() * 0.125, s.double()
    want = torch.einsum("jc,bc,bchw->bjhw", W, S, X) + bias.double()[None, :, None, None]
    mag = torch.einsum("jc,bc,bchw->bjhw", W.abs(), S.abs(), X.abs()) + bias.double().abs()[None, :, None, None]
    _check(got[0], want, mag, 3e-6, "modulated_conv1x1_small")

    torch.manual_seed(3)
    mod = ModulatedConv2d(c, n, 1, 16, demodulate=False).to(DEV)
    style = torch.randn(b, 16, generator=g)
    y_off, y_ref = mod(_offset(x), style.to(DEV)), mod(x.to(DEV), style.to(DEV))
    assert torch.equal(y_off, y_ref)
    lin = mod.modulation
    st = style.double() @ (lin.weight.detach().cpu().double() * lin.scale).t() + lin.bias.detach().cpu().double() * lin.lr_mul
    W = mod.weight.detach().cpu().double().view(n, c) * mod.scale
    want = torch.einsum("jc,bc,bchw->bjhw", W, st, X)
    mag = torch.einsum("jc,bc,bchw->bjhw", W.abs(), st.abs(), X.abs())
    _check(y_off, want, mag, 3e-6, "ModulatedConv2d(k=1)")

    # from-RGB weight gradient (1x1, C <= 4): the streaming weight-gradient kernel with the operands' roles swapped
    x3, g3 = torch.randn(b, 3, 32, 32, generator=g), torch.randn(b, 128, 32, 32, generator=g)
    for xo3, go3 in ((_offset(x3), g3.to(DEV)), (x3.to(DEV), _offset(g3)), (_offset(x3), _offset(g3))):
        dw = conv2d_wgrad_mfma(xo3, go3, ksize=1, stride=1, pad=0)
        assert torch.equal(dw, conv2d_wgrad_mfma(x3.to(DEV), g3.to(DEV), ksize=1, stride=1, pad=0))
    want, mag = _wgrad_reference(x3, g3, None, None, 1)
    _check(dw, want, mag, 2e-6, "from-RGB weight gradient")


def test_from_rgb_weight_gradient_at_256_vs_float64():
    """conv2d_wgrad_mfma 1x1 with 3 input channels at 256^2 (the discriminator's from-RGB layer): 16 chunks per row,
    k_smallconv_dw_finish, then the sum over the batch."""
    b, c, n, h, w = 2, 3, 128, 256, 256
    got, want, mag, names = _wgrad_case(b, c, n, h, w, 1, False, 256)
    # _dw(x, gy): the image is the "gradient" operand (N = 3), the 128 channels the rows (CH = 4)
    assert kernel_ran(names, "k_smallconv_dw", "<3, 4>") and kernel_ran(names, "k_smallconv_dw_finish"), names
    _check(got, want, mag, 2e-6, "dwt")


# ---- the dispatch queries and the launches agree (csrc/conv_dispatch.hip make_conv_plan, csrc/conv_wgrad_dispatch.hip) -----
# kernels that tell the paths apart: a path's launch runs exactly its own of these (no numeric assertions here: the
# float64 comparisons of the same shapes are in test_conv_gpu, test_conv_s2_wino_gpu and above).  k_conv_mfma is judged
# apart: it is the direct path's only kernel and no other non-transposed path runs it, but the transposed paths use its
# TAP9 / per-phase instantiations for the tap-split launch in patch form, the strips and the border.
def _forward_kernels(path):
    from stylerenderer_amd import _lib as P

    own = {P.CONV_PATH_DIRECT: set(), P.CONV_PATH_WINO: {"k_conv_wino"}, P.CONV_PATH_S2_WINO: {"k_conv_s2_wino"},
           P.CONV_PATH_GEMM1X1: {"k_conv1x1_gemm"}, P.CONV_PATH_CONVT_TAPS: {"k_convt_tap_reduce"},
           P.CONV_PATH_CONVT_FUSED: {"k_convt_fused"},
           P.CONV_PATH_CONVT_FUSED_KS: {"k_convt_fused", "k_convt_fused_reduce"}}[path & ~STRIPS]
    return own | ({"k_convt_strip_reduce"} if path & STRIPS else set())


FORWARD_KERNELS = ("k_conv_wino", "k_conv_s2_wino", "k_conv1x1_gemm", "k_convt_tap_reduce", "k_convt_fused",
                   "k_convt_fused_reduce", "k_convt_strip_reduce")
WGRAD_KERNELS = {"k_wgrad_mfma": 0, "k_wgrad_small3": 1, "k_wgrad_wino": 2, "k_wgrad_s2_dma": 5}      # SR_WGRAD_PATH_*


@pytest.mark.parametrize("row", [r for r in FORWARD if r[-1]], ids=case_id)
def test_forward_launch_runs_the_path_the_query_returns(row, monkeypatch):
    from stylerenderer_amd import _lib
    from stylerenderer_amd.op.conv import _wt_pitch, conv2d_mfma

    geom, shape, env, _, _, path, _ = row
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for kv in env.items():
        monkeypatch.setenv(*kv)
    b, c, n, ih, iw, oh, ow, k, stride, pad, tr = conv_args(geom, shape)
    x = torch.randn(b, c, ih, iw, device=DEV)
    wt, ldw = _wt_pitch(torch.randn(k * k, c, n, device=DEV))
    got = _lib.lib().sr_conv2d_path(b, c, n, ih, iw, oh, ow, k, stride, pad, tr, x.data_ptr(), None, wt.data_ptr(), ldw, 1)
    assert got == path                                   # the rule beside the row, now with real buffers
    _, names = launched_kernels(lambda: conv2d_mfma(x, wt, None, None, None, k, stride, pad, bool(tr)))
    assert {kn for kn in FORWARD_KERNELS if kernel_ran(names, kn)} == _forward_kernels(got), names
    if got == _lib.CONV_PATH_DIRECT or not tr:
        assert kernel_ran(names, "k_conv_mfma") == (got == _lib.CONV_PATH_DIRECT), names


@pytest.mark.parametrize("row", [r for r in WGRAD if r[-1]], ids=case_id)
def test_wgrad_launch_runs_the_path_the_query_returns(row, monkeypatch):
    from stylerenderer_amd import _lib
    from stylerenderer_amd.op.conv import conv2d_wgrad_mfma

    geom, shape, env, _, path, _ = row
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for kv in env.items():
        monkeypatch.setenv(*kv)
    b, c, n, ih, iw, oh, ow, k, stride, pad, tr = conv_args(geom, shape)
    x, gy = torch.randn(b, c, ih, iw, device=DEV), torch.randn(b, n, oh, ow, device=DEV)
    got = _lib.lib().sr_conv2d_wgrad_path(b, c, n, ih, iw, oh, ow, k, stride, pad, tr, x.data_ptr(), gy.data_ptr())
    assert got == path
    _, names = launched_kernels(lambda: conv2d_wgrad_mfma(x, gy, None, None, k, stride, pad, bool(tr)))
    assert {kn for kn in WGRAD_KERNELS if kernel_ran(names, kn)} == {kn for kn, v in WGRAD_KERNELS.items() if v == got}, names
