"""CPU: the 25-product form of the stride-2 transposed 3x3 convolution (csrc/convt_wino.hip) — its algebra restated in
numpy, split into the even-row (15 products) and odd-row (10 products) halves the kernel's two workgroup kinds run, and
its place in the dispatch plan through the host-only queries.  No GPU is touched."""
import json

import numpy as np
import pytest

import make_golden_conv_plan as G
from conv_plan_cases import MISALIGNED, SWITCHES, conv_args
from stylerenderer_amd import _lib as P

BAR = 2e-6
STRIPS = P.CONV_PATH_STRIPS
WINO, FUSED, FUSED_KS, TAPS, DIRECT = (P.CONV_PATH_CONVT_WINO, P.CONV_PATH_CONVT_FUSED, P.CONV_PATH_CONVT_FUSED_KS,
                                       P.CONV_PATH_CONVT_TAPS, P.CONV_PATH_DIRECT)


# ---- the algebra ----------------------------------------------------------------------------------------------------
# per dimension, tile t: a = in[2t-1], b = in[2t], c = in[2t+1]; products p = 0 .. 4 pair the input variant IN[p] of
# (a-b, b, c-b, c) with the weight variant WT[p] of (w2, w0+w2, w0, w1):  m1, m2, m3, b w1, c w1
IN = (0, 1, 2, 1, 3)
WT = (0, 1, 2, 3, 3)
ROWS = {0: (0, 1, 2), 1: (3, 4)}          # row products of the even-row / odd-row half


def _xform_in(s):                         # three samples a, b, c along axis 0
    return np.stack([s[0] - s[1], s[1], s[2] - s[1], s[2]])


def _xform_w(g):                          # three taps along axis 0
    return np.stack([g[2], g[0] + g[2], g[0], g[1]])


def _direct(x, w):
    """float64 interior of the transposed convolution and its sum of absolute products: out[2j + ky, 2i + kx] +=
    x[j, i] w[ky, kx], rows < 2 IH and columns < 2 IW."""
    c, ih, iw = x.shape
    n = w.shape[1]
    out, mag = np.zeros((n, 2 * ih + 1, 2 * iw + 1)), np.zeros((n, 2 * ih + 1, 2 * iw + 1))
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    for ky in range(3):
        for kx in range(3):
            out[:, ky:ky + 2 * ih:2, kx:kx + 2 * iw:2] += np.einsum("cn,cyx->nyx", w64[:, :, ky, kx], x64)
            mag[:, ky:ky + 2 * ih:2, kx:kx + 2 * iw:2] += np.einsum("cn,cyx->nyx", np.abs(w64[:, :, ky, kx]), np.abs(x64))
    return out[:, :2 * ih, :2 * iw], mag[:, :2 * ih, :2 * iw]


def _wino(x, w, dtype):
    """The 25-product form in `dtype`, accumulated over the channels in channel order; the even-row half and the odd-row half
    are computed separately (nothing is shared but the input).  Returns (interior, products per tile and channel)."""
    c, ih, iw = x.shape
    n = w.shape[1]
    th, tw = ih // 2, iw // 2
    xp = np.zeros((c, ih + 1, iw + 1), dtype)                     # in[-1] = 0
    xp[:, 1:, 1:] = x
    # samples (ry, cx) of tile (ty, tx) = in[2 ty - 1 + ry, 2 tx - 1 + cx]
    d = np.stack([np.stack([xp[:, ry:ry + 2 * th:2, cx:cx + 2 * tw:2] for cx in range(3)]) for ry in range(3)])
    v = _xform_in(d)                                              # [row variant 4, cx, c, ty, tx]
    v = _xform_in(np.moveaxis(v, 1, 0))                           # [column variant 4, row variant 4, c, ty, tx]
    v = np.swapaxes(v, 0, 1).astype(dtype)
    u = _xform_w(np.moveaxis(w.astype(dtype), 2, 0))              # [row variant 4, c, n, kx]
    u = _xform_w(np.moveaxis(u, 3, 0))                            # [column variant 4, row variant 4, c, n]
    u = np.swapaxes(u, 0, 1).astype(dtype)
    out = np.zeros((n, 4 * th, 4 * tw), dtype)
    nprod = 0
    for par, rows in ROWS.items():
        acc = np.zeros((len(rows), 5, n, th, tw), dtype)
        for ch in range(c):
            for i, p in enumerate(rows):
                for q in range(5):
                    acc[i, q] = acc[i, q] + u[WT[p], WT[q], ch][:, None, None] * v[IN[p], IN[q], ch][None]
                    nprod += 1
        # output rows of this half: even (m1 + m2, m3 + m2) / odd (b w1, c w1); the same along the columns
        rowsum = (acc[0] + acc[1], acc[2] + acc[1]) if par == 0 else (acc[0], acc[1])
        for yr, r in enumerate(rowsum):
            y = 2 * yr + par
            out[:, y::4, 0::4] = r[0] + r[1]
            out[:, y::4, 1::4] = r[3]
            out[:, y::4, 2::4] = r[2] + r[1]
            out[:, y::4, 3::4] = r[4]
    return out, nprod / c


@pytest.mark.parametrize("shape", [(8, 64, 8, 32), (24, 128, 16, 64), (512, 64, 8, 32)], ids=str)
def test_25_product_form_in_numpy(shape):
    """(C, N, IH, IW).  Bar: that of the kernels, 2e-6 of the sum of absolute products."""
    c, n, ih, iw = shape
    rng = np.random.default_rng(c + n)
    x = rng.standard_normal((c, ih, iw)).astype(np.float32)
    w = rng.standard_normal((c, n, 3, 3)).astype(np.float32)
    want, mag = _direct(x, w)
    got, nprod = _wino(x, w, np.float32)
    assert nprod == 25 and got.shape == want.shape
    err = float((np.abs(got.astype(np.float64) - want) / mag).max())
    print("25-product form %s: error %.3e of the absolute-product sum (bar %.1e)" % (shape, err, BAR))
    assert err < BAR
    if c <= 24:                                                   # the identity itself, in float64
        exact, _ = _wino(x, w, np.float64)
        assert float(np.abs(exact - want).max()) < 1e-11 * float(mag.max())


# ---- the dispatch plan ----------------------------------------------------------------------------------------------
@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCHES + ["SR_CONVT_WINO"]:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _path(shape, env=None, in_ptr=None, have=1):
    return P.lib().sr_conv2d_path(*conv_args("t3s2", shape), in_ptr, None, None, 0, have)


BIG = (16, 512, 512, 32, 32)              # 7.73e10: the smallest of the generator's launches at batch 16
ROW = (8, 512, 512, 32, 32)               # 3.87e10: the row of conv_plan_cases.py that stays on k_convt_fused
SMALL = (1, 8, 64, 8, 32)


def test_path_on_both_sides_of_the_flop_bar(clean_env):
    assert _path(BIG) == WINO | STRIPS
    assert _path((16, 512, 256, 64, 64)) == WINO | STRIPS and _path((16, 256, 128, 128, 128)) == WINO | STRIPS
    assert _path((9, 512, 512, 32, 32)) == WINO | STRIPS          # 4.35e10
    assert _path(ROW) == FUSED | STRIPS                           # 3.87e10
    assert _path((4, 512, 256, 64, 64)) == FUSED | STRIPS         # 3.87e10: config[2]
    assert _path(SMALL) == TAPS


def test_switches(clean_env):
    clean_env.setenv("SR_CONVT_WINO", "0")
    assert _path(BIG) == FUSED | STRIPS
    clean_env.setenv("SR_CONVT_WINO", "force")
    assert _path(SMALL) == WINO | STRIPS and _path(ROW) == WINO | STRIPS and _path(BIG) == WINO | STRIPS
    clean_env.setenv("SR_CONVT_FUSED", "0")                       # "per-phase launches" keeps the new path out too
    assert _path(BIG) == DIRECT
    clean_env.delenv("SR_CONVT_WINO")
    assert _path(BIG) == DIRECT


@pytest.mark.parametrize("switch", [None, "force"])
def test_ineligible_calls_fall_to_the_rules_of_the_other_paths(clean_env, switch):
    def both(shape, in_ptr=None):
        if switch is None:
            clean_env.delenv("SR_CONVT_WINO", raising=False)
        else:
            clean_env.setenv("SR_CONVT_WINO", switch)
        got = _path(shape, in_ptr=in_ptr)
        clean_env.setenv("SR_CONVT_WINO", "0")
        return got, _path(shape, in_ptr=in_ptr)

    got, off = both(BIG, MISALIGNED)                              # k_convt_fused wants an aligned input as well
    assert got == off == DIRECT
    got, off = both((16, 512, 512, 64, 16))                       # IW % 32 = 16
    assert got == off and got & 0xFF != WINO
    got, off = both((16, 512, 480, 32, 32))                       # N % 64 = 32: k_convt_fused takes any N
    assert got == off == FUSED | STRIPS
    got, off = both((16, 516, 512, 32, 32))                       # C % 8 = 4
    assert got == off and got & 0xFF != WINO
    got, off = both((16, 512, 512, 36, 32))                       # IH % 8 = 4: k_convt_fused's patch is 4 rows high
    assert got == off == FUSED | STRIPS


def test_path_needs_no_scratch_and_strips_follow_only_with_one(clean_env):
    L = P.lib()
    args = conv_args("t3s2", BIG)
    assert _path(BIG, have=0) == WINO
    assert _path(BIG, have=1) == WINO | STRIPS
    assert L.sr_conv2d_path_floats(*args, None, None, None, 0, 0) == 0
    clean_env.setenv("SR_CONVT_STRIPS", "0")
    assert _path(BIG, have=1) == WINO
    assert L.sr_conv2d_path_floats(*args, None, None, None, 0, 1) == 0


@pytest.mark.parametrize("switch", [None, "force"])
def test_new_path_fits_the_recorded_scratch_sizes(clean_env, switch):
    """For every shape of the golden sweep the path taken — the new one wherever it applies — needs no more scratch than
    sr_conv2d_scratch_floats answered before this path existed (tests/golden/conv_plan_parent.json)."""
    with open(G.OUT) as f:
        sized = [v[0] for v in json.load(f)["unset"]]
    if switch is not None:
        clean_env.setenv("SR_CONVT_WINO", switch)
    L = P.lib()
    rows = G.shapes()
    taken = 0
    bad = []
    for r, s in zip(rows, sized):
        need = L.sr_conv2d_path_floats(*r[1:], None, None, None, 0, 1)
        taken += L.sr_conv2d_path(*r[1:], None, None, None, 0, 1) & 0xFF == WINO
        if not 0 <= need <= s:
            bad.append((r, need, s))
    assert not bad, "%d rows, first: %s" % (len(bad), bad[:3])
    if switch == "force":
        assert taken > 0                                          # the sweep does reach the new path
