"""Weight gradient and style gradient of a modulated convolution from ONE weight-gradient kernel — host side of
sr_conv2d_wgrad_style (csrc/conv_wgrad_dispatch.hip; the finish kernels: csrc/wgrad_style_finish.h).

For y = gscale * conv(iscale * x, wt) and the cotangent gy the split-K weight-gradient kernels write per-slice partial
sums; where no slice straddles a sample, the finish kernel forms from them both
  dwt[t, c, n] = sum_b iscale[b, c] * P_b[t, c, n]      and      gis[b, c] = sum_{t, n} wt[t, c, n] * P_b[t, c, n]
(P_b: the weight gradient of sample b without the style), so the style gradient needs no pass over x and the data
gradient.  op.conv._conv_grads decides when to use it."""
import torch

from .. import _lib
from ._dispatch import native


def part_floats(x, gy, ksize=3, stride=1, pad=1, transposed=False):
    """Floats of the style-gradient partials if `wgrad_style` serves this call — its weight gradient takes a
    transform-domain kernel whose K slices do not straddle samples (sr_conv2d_wgrad_style_floats) — else -1: the call
    keeps sr_conv2d_wgrad_mfma and the row-dot pass."""
    if not (x.is_cuda and x.dtype == torch.float32 and gy.dtype == torch.float32 and x.dim() == 4 and gy.dim() == 4
            and x.is_contiguous() and gy.is_contiguous() and x.shape[0] == gy.shape[0]):
        return -1
    b, c, ih, iw = x.shape
    _, n, oh, ow = gy.shape
    return _lib.lib().sr_conv2d_wgrad_style_floats(b, c, n, ih, iw, oh, ow, ksize, stride, pad, int(bool(transposed)),
                                                   _lib.ptr(x), _lib.ptr(gy))


def wgrad_style(x, gy, iscale, gscale, wt, ldw, ksize=3, stride=1, pad=1, transposed=False, timed=None):
    """(dwt [k*k, C, N], gis [B, C]).  wt: the forward weight [k*k, C, ldw-pitched N]; `timed(launch)` brackets the
    launch (op.conv's PROFILE).  Only where `part_floats` >= 0: anything else is an error, not a fallback."""
    npart = part_floats(x, gy, ksize, stride, pad, transposed)
    if npart < 0:
        raise RuntimeError("wgrad_style: the call's weight-gradient plan has no whole K slices per sample")
    b, c, ih, iw = x.shape
    _, n, oh, ow = gy.shape
    for t, shape, name in ((iscale, (b, c), "iscale"), (gscale, (b, n), "gscale")):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32):
            raise RuntimeError("wgrad_style: %s must be contiguous float32 %s" % (name, shape))
    if (iscale is None or wt.dtype != torch.float32 or tuple(wt.shape[:2]) != (ksize * ksize, c) or wt.shape[2] < n
            or ldw < n or tuple(wt.stride()) != (c * ldw, ldw, 1)):
        raise RuntimeError("wgrad_style: needs iscale and the float32 forward weight [k*k, C, N] at row pitch ldw")
    tr = int(bool(transposed))
    nfl = _lib.lib().sr_conv2d_wgrad_scratch_floats(b, c, n, ih, iw, oh, ow, ksize, stride, pad, tr)
    scratch = torch.empty(nfl, dtype=torch.float32, device=x.device)
    part = torch.empty(npart, dtype=torch.float32, device=x.device)
    dwt = torch.empty((ksize * ksize, c, n), dtype=torch.float32, device=x.device)
    gis = torch.empty((b, c), dtype=torch.float32, device=x.device)

    def launch():
        native(x).sr_conv2d_wgrad_style(dwt, gis, x, gy, iscale, gscale, wt, ldw, b, c, n, ih, iw, oh, ow, ksize, stride,
                                        pad, tr, scratch, part)

    if timed is None:
        launch()
    else:
        timed(launch)
    return dwt, gis
