"""Polyphase 25-product form of the stride-2 3x3 weight gradient (csrc/conv_wgrad_s2_wino.hip: k_wgrad_s2p +
k_wgrad_s2p_finish) against a float64 CPU sum and against the direct kernel it replaces (k_wgrad_s2_dma).

Error measure and bar are those of test_conv_s2_wino_gpu: max |got - float64| / sum |a||b| < 2e-6.  The path is selected
by SR_WGRAD_S2_WINO (0 = never, force = ignore the work bar T) and by the call geometry; which kernels ran is asserted
from the profiler's kernel names and compared with sr_conv2d_wgrad_path."""
import pytest
import torch

from util import kernel_ran, launched_kernels

gpu = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-6
NEW, NEW_FINISH, OLD, DIRECT = "k_wgrad_s2p", "k_wgrad_s2p_finish", "k_wgrad_s2_dma", "k_wgrad_mfma"
SWITCH = "SR_WGRAD_S2_WINO"
T_WORK = 6.0e9                # SR_WGRAD_S2_WINO_MIN_WORK of csrc/conv_wgrad_dispatch.hip: 18 B CU CV GH GW >= T takes the new path


def _out_size(ih, iw, pad, tr):
    return (2 * ih + 1, 2 * iw + 1) if tr else ((ih + 2 * pad - 3) // 2 + 1, (iw + 2 * pad - 3) // 2 + 1)


def _inputs(b, c, n, ih, iw, tr, seed, pad=0):
    g = torch.Generator().manual_seed(seed)
    oh, ow = _out_size(ih, iw, pad, tr)
    x = torch.randn(b, c, ih, iw, generator=g)
    gy = torch.randn(b, n, oh, ow, generator=g)
    return x, gy, torch.randn(b, c, generator=g), torch.randn(b, n, generator=g)


def _ref(x, gy, xs, gs, tr, pad=0):
    """(float64 dwt [9, C, N], float64 sum of absolute products) of the stride-2 3x3 weight gradient."""
    def f(xx, gg, a, bsc):
        xx = xx * a[:, :, None, None] if a is not None else xx
        gg = gg * bsc[:, :, None, None] if bsc is not None else gg
        u, v = (gg, xx) if tr else (xx, gg)                 # U: the (2G + 1)-wide map, V: the G-wide one
        if pad:
            u = torch.nn.functional.pad(u, (pad,) * 4)
        gh, gw = v.shape[2:]
        vm = v.permute(1, 0, 2, 3).reshape(v.shape[1], -1)                                   # [CV, K]
        taps = []
        for ky in range(3):
            for kx in range(3):
                um = u[:, :, ky:ky + 2 * gh:2, kx:kx + 2 * gw:2].permute(1, 0, 2, 3).reshape(u.shape[1], -1)
                d = um @ vm.t()                                                              # [CU, CV]
                taps.append(d.t() if tr else d)                                              # [C, N]
        return torch.stack(taps)

    D = lambda t: None if t is None else t.double()  # noqa: E731
    A = lambda t: None if t is None else t.double().abs()  # noqa: E731
    return f(D(x), D(gy), D(xs), D(gs)), f(A(x), A(gy), A(xs), A(gs))


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _run(x, gy, xs, gs, tr, pad=0):
    from stylerenderer_amd.op.conv import conv2d_wgrad_mfma

    return conv2d_wgrad_mfma(x, gy, xs, gs, 3, 2, pad, tr)


def _rel(got, want, mag):
    return float(((got.detach().cpu().double() - want).abs() / (mag + 1e-30)).max())


def _path(b, c, n, ih, iw, tr, pad=0):
    from stylerenderer_amd import _lib

    oh, ow = _out_size(ih, iw, pad, tr)
    return _lib.lib().sr_conv2d_wgrad_path(b, c, n, ih, iw, oh, ow, 3, 2, pad, int(tr), None, None)


_REF_CACHE = {}


def _case(b, c, n, ih, iw, tr):
    """Inputs and float64 references of one shape for the three scale modes, computed once."""
    key = (b, c, n, ih, iw, tr)
    if key not in _REF_CACHE:
        x, gy, xs, gs = _inputs(b, c, n, ih, iw, tr, seed=b * 1000 + c * 10 + n + ih)
        uonly = (None, gs) if tr else (xs, None)            # uscale = the scale of the windowed operand
        modes = {"plain": (None, None), "uscale": uonly, "both": (xs, gs)}
        _REF_CACHE[key] = (x, gy, {m: (s, _ref(x, gy, *s, tr)) for m, s in modes.items()})
    return _REF_CACHE[key]


# ---- 1. smallest shapes under force -------------------------------------------------------------------------------------
SMALL = [
    (1, 128, 32, 4, 16, True),        # one patch, one channel tile, non-square
    (2, 128, 64, 8, 32, True),        # patches in x, y and batch, two U tiles
    (5, 256, 128, 32, 32, True),      # 80 patches over 8 channel tiles: several patches per slice, ragged last slice
    (2, 32, 128, 33, 33, False),      # plain stride 2
    (3, 64, 256, 65, 65, False),
]


@gpu
@pytest.mark.parametrize("mode", ["plain", "uscale", "both"])
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "B%d-C%d-N%d-%dx%d-%s" % (s[:5] + ("convT" if s[5] else "conv",)))
def test_forced_small_shapes_vs_float64_and_bit_repeatable(shape, mode, monkeypatch):
    tr = shape[5]
    x, gy, refs = _case(*shape)
    scales, (want, mag) = refs[mode]
    args = _dev(x, gy, *scales) + (tr,)
    monkeypatch.setenv(SWITCH, "force")
    got, names = launched_kernels(lambda: _run(*args))
    assert kernel_ran(names, NEW) and kernel_ran(names, NEW_FINISH) and not kernel_ran(names, OLD), names
    assert len(names) == 2, names                           # main + finish, as the direct path
    assert got.shape == want.shape
    err = _rel(got, want, mag)
    again = _run(*args)
    monkeypatch.setenv(SWITCH, "0")
    old, names_old = launched_kernels(lambda: _run(*args))
    assert kernel_ran(names_old, OLD) and not kernel_ran(names_old, NEW), names_old
    err_old = _rel(old, want, mag)
    print("s2 wgrad %s %s: error %.3e of the absolute-product sum, k_wgrad_s2_dma %.3e (bar %.1e)"
          % (shape, mode, err, err_old, BAR))
    assert err < BAR and err_old < BAR
    assert torch.equal(got, again)


# ---- 2. natural dispatch on both sides of T ----------------------------------------------------------------------------------
@gpu
def test_natural_dispatch_on_both_sides_of_the_work_bar(monkeypatch):
    from stylerenderer_amd import _lib

    # work = 18 B CU CV GH GW with CU = 256, CV = 512, G = 32^2: B = 2 -> 4.83e9, B = 3 -> 7.25e9
    for b, new in ((2, False), (3, True)):
        shape = (b, 512, 256, 32, 32, True)
        assert (18.0 * b * 256 * 512 * 32 * 32 >= T_WORK) == new
        monkeypatch.delenv(SWITCH, raising=False)
        x, gy, refs = _case(*shape)
        scales, (want, mag) = refs["both"]
        args = _dev(x, gy, *scales) + (True,)
        path = _path(*shape)
        assert path == (_lib.WGRAD_PATH_S2_WINO if new else _lib.WGRAD_PATH_S2_DMA)
        got, names = launched_kernels(lambda: _run(*args))
        assert kernel_ran(names, NEW) == new and kernel_ran(names, OLD) == (not new), (b, names)
        err = _rel(got, want, mag)
        print("s2 wgrad natural B=%d (%s): error %.3e (bar %.1e)" % (b, NEW if new else OLD, err, BAR))
        assert err < BAR
        if new:
            monkeypatch.setenv(SWITCH, "0")
            assert _path(*shape) == _lib.WGRAD_PATH_S2_DMA
            off, names_off = launched_kernels(lambda: _run(*args))
            assert kernel_ran(names_off, OLD) and not kernel_ran(names_off, NEW), names_off
            assert _rel(off, want, mag) < BAR


# ---- 3. ineligible neighbours under force ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("what, shape, pad", [
    ("GW = 24", (2, 128, 32, 16, 24, True), 0), ("GH = 6", (2, 128, 32, 6, 16, True), 0),
    ("U channels 48", (2, 128, 48, 16, 16, True), 0), ("V channels 64", (2, 64, 32, 16, 16, True), 0),
    ("pad 1", (2, 32, 128, 32, 32, False), 1)])
def test_ineligible_neighbours_fall_through_under_force(what, shape, pad, monkeypatch):
    from stylerenderer_amd import _lib

    tr = shape[5]
    x, gy, xs, gs = _inputs(*shape, seed=11, pad=pad)
    want, mag = _ref(x, gy, xs, gs, tr, pad)
    args = _dev(x, gy, xs, gs) + (tr, pad)
    monkeypatch.setenv(SWITCH, "0")
    path_off = _path(*shape, pad=pad)
    off = _run(*args)
    monkeypatch.setenv(SWITCH, "force")
    assert _path(*shape, pad=pad) == path_off == _lib.WGRAD_PATH_DIRECT, what
    got, names = launched_kernels(lambda: _run(*args))
    assert kernel_ran(names, DIRECT) and not kernel_ran(names, NEW), (what, names)
    assert torch.equal(got, off), what
    assert _rel(got, want, mag) < BAR


# ---- 4. through autograd ----------------------------------------------------------------------------------------------------------
class _Recorder:
    """Stands in for op.conv.conv2d_wgrad_mfma: records every stride-2 3x3 call's operands."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, x, gy, xscale=None, gscale=None, ksize=3, stride=1, pad=1, transposed=False):
        out = self.real(x, gy, xscale, gscale, ksize, stride, pad, transposed)
        if ksize == 3 and stride == 2:
            self.calls.append((x.detach(), gy.detach(), xscale, gscale, bool(transposed)))
        return out

    def mag(self, cin, cout):
        """sum over the recorded calls of sum |a||b| in float64, as [9, Cin, Cout] of the layer's tap-major weight: a call
        of the adjoint geometry (second order) has the two channel roles swapped, the taps stay."""
        assert cin != cout
        total = 0.0
        for x, gy, xs, gs, tr in self.calls:
            cpu = lambda t: None if t is None else t.detach().cpu()  # noqa: E731
            m = _ref(cpu(x), cpu(gy), cpu(xs), cpu(gs), tr)[1]
            assert m.shape[1:] in ((cin, cout), (cout, cin)), m.shape
            total = total + (m if m.shape[1:] == (cin, cout) else m.transpose(1, 2))
        return total


def _layer_grads(layer, fwd, x, gy, second, monkeypatch):
    """weight.grad of out = fwd(x) against gy (first order), or of |d out / d x|^2 (second order), with the recorder's
    absolute-product sum laid out like weight.grad's [.., Cout, Cin, 3, 3]."""
    import stylerenderer_amd.op.conv as C

    rec = _Recorder(C.conv2d_wgrad_mfma)
    monkeypatch.setattr(C, "conv2d_wgrad_mfma", rec)
    layer.zero_grad()
    xr = x.clone().requires_grad_(True)
    out = fwd(xr)
    names = None
    if second:
        g1, = torch.autograd.grad(out, xr, gy, create_graph=True)
        _, names = launched_kernels(lambda: g1.pow(2).sum().backward())
    else:
        _, names = launched_kernels(lambda: out.backward(gy))
    monkeypatch.setattr(C, "conv2d_wgrad_mfma", rec.real)
    return rec, names


def _compare_layer(layer, weight, scale, fwd, x, gy, second, label, monkeypatch):
    res = {}
    for sw in ("force", "0"):
        monkeypatch.setenv(SWITCH, sw)
        rec, names = _layer_grads(layer, fwd, x, gy, second, monkeypatch)
        assert rec.calls, "no stride-2 weight gradient ran"
        assert kernel_ran(names, NEW) == (sw == "force") and kernel_ran(names, OLD) == (sw == "0"), (sw, names)
        res[sw] = (weight.grad.detach().clone(), rec)
    g_on, rec = res["force"]
    g_off = res["0"][0]
    assert torch.isfinite(g_on).all()
    # weight.grad[.., o, i, ky, kx] = scale * dwt[ky * 3 + kx, i, o] (no demodulation: the weight enters only through
    # the convolution), so its absolute-product sum is scale * the recorded calls'
    n, c = weight.shape[-4], weight.shape[-3]
    mag = scale * rec.mag(c, n).reshape(3, 3, c, n).permute(3, 2, 0, 1)
    diff = float(((g_on - g_off).reshape(mag.shape).cpu().double().abs() / (mag + 1e-30)).max())
    print("s2 wgrad %s %s order: |force - off| = %.3e of the absolute-product sum (bar %.1e)"
          % (label, "second" if second else "first", diff, BAR))
    assert diff < BAR


@gpu
@pytest.mark.parametrize("second", [False, True], ids=["first", "second"])
def test_upsampling_modulated_conv_through_autograd(second, monkeypatch):
    from stylerenderer_amd import layers, synth

    torch.manual_seed(5)
    conv = layers.ModulatedConv2d(128, 64, 3, 32, demodulate=False, upsample=True)
    synth.fill_state_dict(conv.state_dict(), salt=3)
    conv = conv.to(DEV)
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 128, 16, 16, generator=g).to(DEV)
    style = torch.randn(2, 32, generator=g).to(DEV)
    gy = torch.randn(2, 64, 33, 33, generator=g).to(DEV)
    _compare_layer(conv, conv.weight, conv.scale, lambda xr: conv(xr, style, skip_blur=True), x, gy, second,
                   "ModulatedConv2d up 128 -> 64, 16^2 -> 33^2", monkeypatch)


@gpu
@pytest.mark.parametrize("second", [False, True], ids=["first", "second"])
def test_downsampling_conv_layer_through_autograd(second, monkeypatch):
    from stylerenderer_amd import layers, synth

    layer = layers.ConvLayer(32, 128, 3, downsample=True, bias=False, activate=False)
    synth.fill_state_dict(layer.state_dict(), salt=4)
    layer = layer.to(DEV)
    conv = [m for m in layer if isinstance(m, layers.EqualConv2d)][0]
    g = torch.Generator().manual_seed(22)
    x = torch.randn(2, 32, 32, 32, generator=g).to(DEV)
    gy = torch.randn(2, 128, 16, 16, generator=g).to(DEV)
    _compare_layer(layer, conv.weight, conv.scale, lambda xr: layer(xr), x, gy, second,
                   "ConvLayer down 32 -> 128, 32^2 -> 16^2", monkeypatch)


# ---- 5. under capture ------------------------------------------------------------------------------------------------------------
@gpu
def test_forced_call_under_graph_capture(monkeypatch):
    x, gy, refs = _case(2, 128, 64, 8, 32, True)
    scales, _ = refs["both"]
    args = _dev(x, gy, *scales) + (True,)
    monkeypatch.setenv(SWITCH, "force")
    eager = _run(*args)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(*args)                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _run(*args)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
