"""Polyphase 25-product form of the non-transposed stride-2 3x3 convolution (csrc/conv_s2_wino.hip) against a float64
CPU convolution and against the direct kernel it replaces (k_conv_mfma<2, 3, 3, ...>).

Error measure and bar are those of test_conv_vs_float64: max |got - float64| / sum |a||b| < 2e-6.  The kernel is
selected by SR_CONV_S2_WINO (0 = off, force = ignore the workgroup threshold of 192) and by the call geometry;
which kernel ran is asserted from the profiler's kernel names."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from util import kernel_ran, launched_kernels

gpu = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-6
NEW, OLD = "k_conv_s2_wino", "k_conv_mfma"


def _inputs(b, c, n, ih, iw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, ih, iw, generator=g)
    w = torch.randn(n, c, 3, 3, generator=g)
    isc, osc, bias = torch.randn(b, c, generator=g), torch.randn(b, n, generator=g), torch.randn(n, generator=g)
    return x, w, isc, osc, bias


def _taps(w):
    n, c = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(9, c, n).contiguous()


def _ref(x, w, isc, osc, bias):
    """(float64 result, float64 sum of absolute products) of out = conv(x * isc, w, stride 2) * osc + bias."""
    xs, ax = x.double(), x.abs().double()
    if isc is not None:
        xs, ax = xs * isc.double()[:, :, None, None], ax * isc.abs().double()[:, :, None, None]
    y, mag = F.conv2d(xs, w.double(), stride=2), F.conv2d(ax, w.abs().double(), stride=2)
    if osc is not None:
        y, mag = y * osc.double()[:, :, None, None], mag * osc.abs().double()[:, :, None, None]
    if bias is not None:
        y, mag = y + bias.double()[None, :, None, None], mag + bias.abs().double()[None, :, None, None]
    return y, mag


def _run(x, wt, isc, osc, bias):
    from stylerenderer_amd.op.conv import conv2d_mfma

    return conv2d_mfma(x, wt, isc, osc, bias, 3, 2, 0, False)


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _rel(got, want, mag):
    return float(((got.detach().cpu().double() - want).abs() / (mag + 1e-30)).max())


_REF_CACHE = {}


def _case(b, c, n, ih, iw):
    """Inputs and float64 references of one shape for the three scale modes, computed once."""
    key = (b, c, n, ih, iw)
    if key not in _REF_CACHE:
        x, w, isc, osc, bias = _inputs(b, c, n, ih, iw, seed=b * 1000 + c * 10 + n + ih)
        modes = {"plain": (None, None, None), "iscale": (isc, None, None), "all": (isc, osc, bias)}
        _REF_CACHE[key] = (x, w, {m: (s, _ref(x, w, *s)) for m, s in modes.items()})
    return _REF_CACHE[key]


# ---- 1. smallest shapes under force ------------------------------------------------------------------------------------
SMALL = [
    (1, 4, 64, 17, 65),       # one tile, one chunk: prologue and epilogue only
    (1, 12, 128, 65, 65),     # odd chunk count, two channel blocks
    (3, 16, 64, 33, 129),     # non-square, several tiles per row
    (2, 64, 64, 129, 129),    # a longer K loop
]


@gpu
@pytest.mark.parametrize("mode", ["plain", "iscale", "all"])
@pytest.mark.parametrize("shape", SMALL)
def test_forced_small_shapes_vs_float64_and_bit_repeatable(shape, mode, monkeypatch):
    x, w, refs = _case(*shape)
    scales, (want, mag) = refs[mode]
    monkeypatch.setenv("SR_CONV_S2_WINO", "force")
    args = _dev(x, _taps(w), *scales)
    got, names = launched_kernels(lambda: _run(*args))
    assert kernel_ran(names, NEW) and not kernel_ran(names, OLD), names
    assert got.shape == want.shape
    err = _rel(got, want, mag)
    print("s2 wino %s %s: error %.3e of the absolute-product sum (bar %.1e)" % (shape, mode, err, BAR))
    assert err < BAR
    again = _run(*args)
    assert torch.equal(got, again)


# ---- 2. natural dispatch on both sides of the threshold ------------------------------------------------------------------
@gpu
def test_natural_dispatch_on_both_sides_of_the_workgroup_threshold(monkeypatch):
    # workgroups = B * (OW / 32) * (OH / 8) * (N / 64): 3 * 2 * 8 * 4 = 192 takes the new kernel, 3 * 2 * 8 * 3 = 144 does not
    monkeypatch.delenv("SR_CONV_S2_WINO", raising=False)
    for n, new in ((256, True), (192, False)):
        x, w, refs = _case(3, 8, n, 129, 129)
        scales, (want, mag) = refs["all"]
        args = _dev(x, _taps(w), *scales)
        got, names = launched_kernels(lambda: _run(*args))
        assert kernel_ran(names, NEW) == new and kernel_ran(names, OLD) == (not new), (n, names)
        err = _rel(got, want, mag)
        print("s2 natural N=%d (%s): error %.3e (bar %.1e)" % (n, NEW if new else OLD, err, BAR))
        assert err < BAR
        if new:
            monkeypatch.setenv("SR_CONV_S2_WINO", "0")
            off, names_off = launched_kernels(lambda: _run(*args))
            assert kernel_ran(names_off, OLD) and not kernel_ran(names_off, NEW), names_off
            assert _rel(off, want, mag) < BAR
            # the switch selects another kernel: the switched-off result is the old kernel's bit for bit (repeatable),
            # and not the new kernel's
            assert torch.equal(off, _run(*args))
            assert not torch.equal(off, got)
            monkeypatch.delenv("SR_CONV_S2_WINO", raising=False)


# ---- 3. ineligible neighbours under force ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("what, shape", [("OW = 31", (1, 4, 64, 17, 63)), ("C = 6", (1, 6, 64, 17, 65)),
                                         ("N = 48", (1, 4, 48, 17, 65)), ("offset input", (1, 4, 64, 17, 65))])
def test_ineligible_neighbours_fall_through_under_force(what, shape, monkeypatch):
    x, w, isc, osc, bias = _inputs(*shape, seed=11)
    want, mag = _ref(x, w, isc, osc, bias)
    xd, wt, isc, osc, bias = _dev(x, _taps(w), isc, osc, bias)
    if what == "offset input":
        flat = torch.empty(xd.numel() + 1, device=DEV)
        flat[1:] = xd.reshape(-1)
        xd = flat[1:].view(xd.shape)              # contiguous, 4 bytes behind a 16-byte boundary
        assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    monkeypatch.setenv("SR_CONV_S2_WINO", "force")
    got, names = launched_kernels(lambda: _run(xd, wt, isc, osc, bias))
    assert kernel_ran(names, OLD) and not kernel_ran(names, NEW), (what, names)
    monkeypatch.setenv("SR_CONV_S2_WINO", "0")
    off = _run(xd, wt, isc, osc, bias)
    assert torch.equal(got, off), what
    assert _rel(got, want, mag) < BAR


# ---- 4. the direct kernel's two halo stagings on a shape the new kernel would otherwise take -----------------------------
@gpu
def test_rotating_lead_equals_dword_staging_with_the_switch_off(monkeypatch):
    x, w, refs = _case(3, 8, 256, 129, 129)
    scales, _ = refs["all"]
    args = _dev(x, _taps(w), *scales)
    monkeypatch.setenv("SR_CONV_S2_WINO", "0")
    monkeypatch.setenv("SR_CONV_ROT", "1")
    a, names = launched_kernels(lambda: _run(*args))
    assert kernel_ran(names, OLD) and not kernel_ran(names, NEW), names
    monkeypatch.setenv("SR_CONV_ROT", "0")
    d = _run(*args)
    assert torch.equal(a, d)


# ---- 5. through autograd: the data gradient of the up-sampling convolution ---------------------------------------------------
# forward "t3s2" with B = 3, C = 256, N = 8.  From 64^2 the data gradient is case 2's launch (3, 8, 256, 129, 129) and
# takes the new kernel by itself; from 32^2 it has 48 workgroups and takes it under force only.
@gpu
@pytest.mark.parametrize("hw, switch", [(32, "force"), (64, None)])
def test_data_gradient_through_autograd(hw, switch, monkeypatch):
    from stylerenderer_amd.op.conv import ConvFn

    b, c, n = 3, 256, 8
    g = torch.Generator().manual_seed(77 + hw)
    x = torch.randn(b, c, hw, hw, generator=g)
    w = torch.randn(c, n, 3, 3, generator=g)                         # conv_transpose2d layout
    isc, osc = torch.randn(b, c, generator=g), torch.randn(b, n, generator=g)
    gy = torch.randn(b, n, 2 * hw + 1, 2 * hw + 1, generator=g)
    # float64: gx = isc * conv2d(gy * osc, w), and the same with absolute values
    want = F.conv2d(gy.double() * osc.double()[:, :, None, None], w.double(), stride=2) * isc.double()[:, :, None, None]
    mag = F.conv2d(gy.abs().double() * osc.abs().double()[:, :, None, None], w.abs().double(), stride=2) \
        * isc.abs().double()[:, :, None, None]
    wt = w.permute(2, 3, 0, 1).reshape(9, c, n).contiguous()
    xd, wd, iscd, oscd, gyd = _dev(x, wt, isc, osc, gy)

    def grad():
        xr = xd.clone().requires_grad_(True)
        y = ConvFn.apply(xr, wd, iscd, oscd, None, "t3s2")
        return torch.autograd.grad(y, xr, gyd)[0]

    if switch is None:
        monkeypatch.delenv("SR_CONV_S2_WINO", raising=False)
    else:
        monkeypatch.setenv("SR_CONV_S2_WINO", switch)
    on, names = launched_kernels(grad)
    assert kernel_ran(names, NEW), names
    monkeypatch.setenv("SR_CONV_S2_WINO", "0")
    off, names_off = launched_kernels(grad)
    assert not kernel_ran(names_off, NEW), names_off
    err_on, err_off = _rel(on, want, mag), _rel(off, want, mag)
    diff = _rel(on, off.detach().cpu().double(), mag)
    print("s2 wino gx %d^2: error %.3e, direct kernel %.3e, difference %.3e (bar %.1e)" % (hw, err_on, err_off, diff, BAR))
    assert err_on < BAR and err_off < BAR
    assert diff <= 2 * err_off


# ---- 6. the algebra on the CPU ----------------------------------------------------------------------------------------------
def _slot(a):
    return (0, 0, 1, 1, 2)[a]


@pytest.mark.parametrize("k", [8, 128])
def test_polyphase_algebra_in_numpy(k):
    """25 products into 9 slots and the output transform, accumulated over K channels in float32 in channel order, against
    a float64 direct convolution.  Bar: that of the kernels, 2e-6 of the sum of absolute products (a float32 chain of K
    terms plus the three adds of the output transform is far inside it for these K)."""
    rng = np.random.default_rng(k)
    th, tw, n = 2, 3, 5                                               # output tiles, output channels
    x = rng.standard_normal((k, 4 * th + 1, 4 * tw + 1)).astype(np.float32)
    w = rng.standard_normal((n, k, 3, 3)).astype(np.float32)
    want = np.zeros((n, 2 * th, 2 * tw))
    mag = np.zeros_like(want)
    for ky in range(3):
        for kx in range(3):
            patch = x[:, ky:ky + 4 * th:2, kx:kx + 4 * tw:2].astype(np.float64)
            want += np.einsum("nc,cyx->nyx", w[:, :, ky, kx].astype(np.float64), patch)
            mag += np.einsum("nc,cyx->nyx", np.abs(w[:, :, ky, kx]).astype(np.float64), np.abs(patch))

    def xform_in(s):                                                  # five samples along axis 0
        return np.stack([s[0] - s[2], s[1], s[4] - s[2], s[3], s[2]])

    def xform_w(g):                                                   # three taps along axis 0
        return np.stack([g[0], g[1], g[2], g[1], g[0] + g[2]])

    # U[a, b, n, c]
    u = xform_w(np.moveaxis(w, 2, 0))                                 # [a, n, c, kx]
    u = xform_w(np.moveaxis(u, 3, 0))                                 # [b, a, n, c]
    u = np.swapaxes(u, 0, 1).astype(np.float32)
    got = np.zeros((n, 2 * th, 2 * tw), np.float32)
    for ty in range(th):
        for tx in range(tw):
            d = x[:, 4 * ty:4 * ty + 5, 4 * tx:4 * tx + 5]            # [c, 5, 5]
            v = xform_in(np.moveaxis(d, 1, 0))                        # [a, c, 5]
            v = xform_in(np.moveaxis(v, 2, 0))                        # [b, a, c]
            v = np.swapaxes(v, 0, 1).astype(np.float32)               # [a, b, c]
            acc = np.zeros((3, 3, n), np.float32)
            nprod = 0
            for c in range(k):                                        # channel order, float32 accumulation
                for a in range(5):
                    for bb in range(5):
                        acc[_slot(a), _slot(bb)] = acc[_slot(a), _slot(bb)] + u[a, bb, :, c] * v[a, bb, c]
                        nprod += 1
            assert nprod == 25 * k
            for r in range(2):
                for s in range(2):
                    got[:, 2 * ty + r, 2 * tx + s] = (acc[r, s] + acc[2, s]) + (acc[r, 2] + acc[2, 2])
    err = float((np.abs(got.astype(np.float64) - want) / mag).max())
    print("polyphase algebra K=%d: error %.3e of the absolute-product sum" % (k, err))
    assert err < BAR
