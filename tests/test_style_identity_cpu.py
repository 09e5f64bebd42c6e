"""The identity behind csrc/wgrad_style_finish.h, in float64 on the oracle's convolutions (oracle/ops_np.py).

For y = oscale * conv(iscale (.) x, W) and a cotangent g let P_b[t, c, n] = corr(x[b, c], oscale[b, n] * g[b, n])[t] be
the weight gradient of sample b WITHOUT the style.  Then
    dW[t, c, n] = sum_b iscale[b, c] * P_b[t, c, n]          gis[b, c] = sum_{t, n} W[t, c, n] * P_b[t, c, n]
where dW = d<g, y>/dW and gis = d<g, y>/d iscale (= sum_p x * dxu, the row-dot of the input with the unscaled data
gradient).  <g, y> is linear in W and in iscale, so both derivatives are exact evaluations of the oracle's forward at
unit vectors — no differencing.  2 samples, 3 -> 4 channels, 5 x 6 maps; the stride-1 padded 3x3 geometry and the
stride-2 transposed one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ops_np  # noqa: E402

B, C, N, H, W = 2, 3, 4, 5, 6


def _forward(x, wt, iscale, oscale, transposed):
    """y = oscale * conv(iscale * x, wt), wt [3, 3, C, N], through the oracle's per-sample-weight convolutions."""
    w = np.broadcast_to(wt.transpose(3, 2, 0, 1)[None], (B, N, C, 3, 3))                # [B, N, C, ky, kx]
    xs = x * iscale[:, :, None, None]
    y = ops_np._conv_transpose2d_f64(xs, w, 2) if transposed else ops_np._conv2d_f64(xs, w, 1, 1)
    return y * oscale[:, :, None, None]


def _per_sample_wgrad(x, g, oscale, transposed):
    """P [B, 3, 3, C, N] from the definition: the correlation of x[b, c] with oscale[b, n] * g[b, n] at tap (ky, kx)."""
    gs = g * oscale[:, :, None, None]
    p = np.zeros((B, 3, 3, C, N))
    for ky in range(3):
        for kx in range(3):
            if transposed:          # y[2i + ky, 2j + kx] += x[i, j] * w[ky, kx]
                win = gs[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2]
                p[:, ky, kx] = np.einsum("bchw,bnhw->bcn", x, win)
            else:                   # y[i, j] += xpad[i + ky, j + kx] * w[ky, kx]
                xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
                p[:, ky, kx] = np.einsum("bchw,bnhw->bcn", xp[:, :, ky:ky + H, kx:kx + W], gs)
    return p


@pytest.mark.parametrize("transposed", [False, True], ids=["c3", "t3s2"])
def test_weight_and_style_gradient_are_two_contractions_of_the_per_sample_weight_gradient(transposed):
    rng = np.random.RandomState(7 + int(transposed))
    x = rng.randn(B, C, H, W)
    wt = rng.randn(3, 3, C, N)
    iscale, oscale = rng.randn(B, C), rng.randn(B, N)
    oh, ow = (2 * H + 1, 2 * W + 1) if transposed else (H, W)
    g = rng.randn(B, N, oh, ow)
    loss = lambda w, s: float((g * _forward(x, w, s, oscale, transposed)).sum())  # noqa: E731
    p = _per_sample_wgrad(x, g, oscale, transposed)

    # the loss itself, as the full contraction: P is the weight gradient the oracle's forward implies
    full = np.einsum("bc,yxcn,byxcn->", iscale, wt, p)
    assert abs(full - loss(wt, iscale)) <= 1e-12 * np.abs(np.einsum("bc,yxcn,byxcn->bc", iscale, wt, p)).sum()

    # dW = d loss / d W, entry by entry (the loss is linear in W)
    dw = np.zeros_like(wt)
    for idx in np.ndindex(*wt.shape):
        e = np.zeros_like(wt)
        e[idx] = 1.0
        dw[idx] = loss(e, iscale)
    want_dw = np.einsum("bc,byxcn->yxcn", iscale, p)
    assert np.abs(dw - want_dw).max() <= 1e-12 * np.abs(want_dw).max()

    # gis = d loss / d iscale, entry by entry (linear in iscale) — and, by its definition, sum_p x * dxu
    gis = np.zeros_like(iscale)
    for idx in np.ndindex(*iscale.shape):
        e = np.zeros_like(iscale)
        e[idx] = 1.0
        gis[idx] = loss(wt, e)
    want_gis = np.einsum("yxcn,byxcn->bc", wt, p)
    assert np.abs(gis - want_gis).max() <= 1e-12 * np.abs(want_gis).max()

    # the same number from the maps, as the row-dot pass forms it: dxu = adjoint convolution of oscale * g with W
    wb = np.broadcast_to(wt.transpose(3, 2, 0, 1)[None], (B, N, C, 3, 3))
    gs = g * oscale[:, :, None, None]
    if transposed:      # adjoint of the stride-2 transposed convolution: the stride-2 convolution, channels swapped
        dxu = ops_np._conv2d_f64(gs, wb.transpose(0, 2, 1, 3, 4), 2, 0)
    else:               # adjoint of the padded 3x3 correlation: flipped taps, channels swapped
        dxu = ops_np._conv2d_f64(gs, wb.transpose(0, 2, 1, 3, 4)[..., ::-1, ::-1], 1, 1)
    rowdot = (x * dxu).sum((2, 3))
    assert np.abs(rowdot - want_gis).max() <= 1e-12 * np.abs(want_gis).max()
