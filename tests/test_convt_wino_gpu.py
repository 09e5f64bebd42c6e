"""25-product form of the stride-2 transposed 3x3 convolution's interior (csrc/convt_wino.hip, k_convt_wino) against a
float64 CPU transposed convolution and against the 36-product kernel it replaces (k_convt_fused).

Error measure and bar are those of test_conv_gpu: max |got - float64| / sum |a||b| < 2e-6 over the WHOLE output (interior
and the strips behind it).  The kernel is selected by SR_CONVT_WINO (0 = never, force = any eligible size; unset = the flop
bar of the dispatch plan); which kernel ran is asserted from the profiler's kernel names."""
import pytest
import torch
from torch.nn import functional as F

from util import kernel_ran, launched_kernels

gpu = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-6
NEW, OLD = "k_convt_wino", "k_convt_fused"
GUARD = 4096                                      # floats behind the output's end

SHAPES = [
    (1, 8, 64, 8, 32),        # one patch, one chunk
    (2, 24, 128, 16, 64),     # three chunks (prologue, steady state, epilogue of the pipeline), 2x2 patches, two channel blocks
    (1, 512, 64, 8, 32),      # the longest style row
    (3, 16, 64, 8, 32),       # an odd batch
]
MODES = ["plain", "iscale", "all"]


def _inputs(b, c, n, ih, iw, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(b, c, ih, iw, generator=g)
    w = torch.randn(c, n, 3, 3, generator=g)                          # conv_transpose2d layout
    isc, osc, bias = torch.randn(b, c, generator=g), torch.randn(b, n, generator=g), torch.randn(n, generator=g)
    return x, w, isc, osc, bias


def _taps(w):
    c, n = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(9, c, n).contiguous()


def _ref(x, w, isc, osc, bias):
    """(float64 result, float64 sum of absolute products) of out = conv_transpose2d(x * isc, w, stride 2) * osc + bias."""
    xs, ax = x.double(), x.abs().double()
    if isc is not None:
        xs, ax = xs * isc.double()[:, :, None, None], ax * isc.abs().double()[:, :, None, None]
    y, mag = F.conv_transpose2d(xs, w.double(), stride=2), F.conv_transpose2d(ax, w.abs().double(), stride=2)
    if osc is not None:
        y, mag = y * osc.double()[:, :, None, None], mag * osc.abs().double()[:, :, None, None]
    if bias is not None:
        y, mag = y + bias.double()[None, :, None, None], mag + bias.abs().double()[None, :, None, None]
    return y, mag


_REF_CACHE = {}


def _case(b, c, n, ih, iw):
    """Inputs and float64 references of one shape for the three scale modes, computed once."""
    key = (b, c, n, ih, iw)
    if key not in _REF_CACHE:
        x, w, isc, osc, bias = _inputs(b, c, n, ih, iw, seed=b * 1000 + c * 10 + n + ih)
        modes = {"plain": (None, None, None), "iscale": (isc, None, None), "all": (isc, osc, bias)}
        _REF_CACHE[key] = (x, w, {m: (s, _ref(x, w, *s)) for m, s in modes.items()})
    return _REF_CACHE[key]


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _rel(got, want, mag):
    return float(((got.detach().cpu().double() - want).abs() / (mag + 1e-30)).max())


def _run_guarded(x, wt, isc, osc, bias):
    """The transposed convolution into a NaN-filled output with a guard region behind its end: (output, guard)."""
    from stylerenderer_amd import _lib
    from stylerenderer_amd.op._dispatch import native

    b, c, ih, iw = x.shape
    n = wt.shape[2]
    oh, ow = 2 * ih + 1, 2 * iw + 1
    flat = torch.full((b * n * oh * ow + GUARD,), float("nan"), device=DEV)
    out = flat[:b * n * oh * ow].view(b, n, oh, ow)
    nscr = _lib.lib().sr_conv2d_scratch_floats(b, c, n, ih, iw, oh, ow, 3, 2, 0, 1)
    scratch = torch.empty(max(nscr, 1), device=DEV)
    native(x).sr_conv2d_mfma_ex(out, x, wt, isc, osc, bias, b, c, n, wt.stride(1), ih, iw, oh, ow, 3, 2, 0, 1, 0, scratch)
    return out, flat[b * n * oh * ow:]


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_forced_shapes_vs_float64_guarded_and_bit_repeatable(shape, mode, monkeypatch):
    x, w, refs = _case(*shape)
    scales, (want, mag) = refs[mode]
    args = _dev(x, _taps(w), *scales)
    monkeypatch.setenv("SR_CONVT_WINO", "force")
    (got, guard), names = launched_kernels(lambda: _run_guarded(*args))
    assert kernel_ran(names, NEW) and not kernel_ran(names, OLD), names
    assert got.shape == want.shape
    assert bool(torch.isfinite(got).all()), "an output element was not written"
    assert bool(torch.isnan(guard).all()), "a store behind the output's end"
    err = _rel(got, want, mag)
    again, _ = _run_guarded(*args)
    assert torch.equal(got, again)
    # the 36-product kernel on the same data (small launches take the tap-split form otherwise)
    monkeypatch.setenv("SR_CONVT_WINO", "0")
    monkeypatch.setenv("SR_CONVT_TAPS", "0")
    monkeypatch.setenv("SR_CONVT_FUSED", "1")
    (off, _), names_off = launched_kernels(lambda: _run_guarded(*args))
    assert kernel_ran(names_off, OLD) and not kernel_ran(names_off, NEW), names_off
    err_off = _rel(off, want, mag)
    diff = _rel(got, off.detach().cpu().double(), mag)
    print("convt wino %s %s: error %.3e, k_convt_fused %.3e, difference %.3e of the absolute-product sum (bar %.1e)"
          % (shape, mode, err, err_off, diff, BAR))
    assert err < BAR and err_off < BAR
    assert diff <= err + err_off                                  # the two agree to round-off


@gpu
def test_natural_dispatch_keeps_small_launches_on_the_fused_kernel(monkeypatch):
    """Below the flop bar (18 B C N IH IW = 3.0e8 here) nothing changes: the switch unset and the switch off are bit-identical."""
    from stylerenderer_amd.op.conv import conv2d_mfma

    x, w, refs = _case(2, 24, 128, 16, 64)
    scales, _ = refs["all"]
    args = _dev(x, _taps(w), *scales)
    monkeypatch.delenv("SR_CONVT_WINO", raising=False)
    a, names = launched_kernels(lambda: conv2d_mfma(*args, 3, 2, 0, True))
    assert not kernel_ran(names, NEW), names
    monkeypatch.setenv("SR_CONVT_WINO", "0")
    assert torch.equal(a, conv2d_mfma(*args, 3, 2, 0, True))


@gpu
def test_up_sampling_layer_through_autograd(monkeypatch):
    """UpConvNBAFn forward + backward under force against the same with the switch off: the image within the float64 bar of
    the convolution (the blur is a convex combination, the activation 1-Lipschitz times its gain), the gradients finite and
    equal within round-off (they depend on the forward only through the activation's sign and the rebuilt y0)."""
    from stylerenderer_amd.op.conv import UpConvNBAFn

    b, c, n, ih, iw = 2, 16, 64, 8, 32
    x, w, isc, osc, _ = _inputs(b, c, n, ih, iw, seed=5)
    g = torch.Generator().manual_seed(6)
    kernel = torch.tensor([1.0, 3.0, 3.0, 1.0])
    kernel = (kernel[:, None] * kernel[None, :])
    kernel = kernel / kernel.sum() * 4.0
    noise = torch.randn(b, 1, 2 * ih, 2 * iw, generator=g)
    noise_w, abias = torch.randn(1, generator=g), torch.randn(n, generator=g)
    gy = torch.randn(b, n, 2 * ih, 2 * iw, generator=g)
    xd, wd, iscd, oscd, kd, nd, nwd, abd, gyd = _dev(x, _taps(w), isc, osc, kernel, noise, noise_w, abias, gy)
    slope, gain = 0.2, 2.0 ** 0.5

    def step():
        leaves = [t.clone().requires_grad_(True) for t in (xd, wd, iscd, oscd)]
        y = UpConvNBAFn.apply(leaves[0], leaves[1], leaves[2], leaves[3], kd, (1, 1), nd, nwd, abd, slope, gain)
        return (y,) + torch.autograd.grad(y, leaves, gyd)

    monkeypatch.setenv("SR_CONVT_WINO", "force")
    on, names = launched_kernels(step)
    assert kernel_ran(names, NEW) and not kernel_ran(names, OLD), names
    monkeypatch.setenv("SR_CONVT_WINO", "0")
    off, names_off = launched_kernels(step)
    assert not kernel_ran(names_off, NEW), names_off
    # image: |d out| <= gain * blur(|d y|) <= gain * 4 * BAR * blur-mean(sum |a||b|); bound by the largest magnitude
    _, mag = _ref(x, w, isc, osc, None)
    bound = gain * 4.0 * 2 * BAR * float(mag.max())
    d_img = float((on[0].detach() - off[0].detach()).abs().max())
    print("up-sampling layer: image difference %.3e (bound %.3e)" % (d_img, bound))
    assert bool(torch.isfinite(on[0]).all()) and d_img <= bound
    for name, a, o in zip(("x", "wt", "iscale", "oscale"), on[1:], off[1:]):
        assert bool(torch.isfinite(a).all()), name
        scale = float(o.abs().max())
        d = float((a - o).abs().max())
        print("up-sampling layer: gradient %s difference %.3e of its largest value" % (name, d / scale))
        assert d <= 1e-4 * scale, name
