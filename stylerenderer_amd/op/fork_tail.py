"""Stride-1 styled layer whose output feeds both the next layer and ToRGB, as ONE autograd node (reference
model.py:206-219: conv -> noise -> bias -> LeakyReLU, then ToRGB beside the next layer).

    forward   (y, rgb) = (conv2d_nba(x, ...), conv1x1(y, ws) + rgb_bias)        the two launches of the separate nodes
    backward  (g_y, g_rgb) -> one pass (csrc/fused_elem.hip k_fork_nba_bwd) for what `SmallConvFork.backward` and the
              activation backward of `ConvNBAFn.backward` do in three launches and six passes over a full-size map:
              gy = g_y + Ws^T g_rgb is never written and y is read once.  Bit for bit the same gradients.

Every other backward (a recorded one, no ToRGB cotangent, a cotangent the kernel cannot read in place, no gradient wanted
for the ToRGB rows) runs the two nodes' own backward bodies in their order: `op.smallconv.fork_backward`, then
`op.conv._nba_backward`.  SR_FORK_TAIL=0 (read per call, `enabled`): the model builds the two nodes as before.
"""
import os

import torch

from .. import _lib
from . import conv as _conv
from . import smallconv as _smallconv
from ._dispatch import mark_inputs, native, wanted
from .fused_elem import noise_stride, param_grads


def enabled():
    return os.environ.get("SR_FORK_TAIL", "1") != "0"


class Head:
    """The ToRGB head handed to the layer in front of it: `n_rgb` output channels, `rows()` -> (ws [B, n_rgb, C],
    bias [n_rgb]) — called only where the combined node applies — and `rgb`, where that node leaves the head's image
    (None: the caller runs the head itself).  The layer's module still returns its activation alone."""
    __slots__ = ("n_rgb", "rows", "rgb")

    def __init__(self, n_rgb, rows):
        self.n_rgb, self.rows, self.rgb = n_rgb, rows, None


def supported(x, n, n_rgb, noise, oscale):
    """Whether the node serves a layer with input x [B, C, H, W] and n output channels whose convolution already takes the
    conv-NBA path (`op.conv.conv_nba_supported`, the caller's check): what the ToRGB kernels and the fused backward ask
    of the OUTPUT [B, n, H, W] on top of that."""
    b, _, h, w = x.shape
    return (oscale is not None and 1 <= n_rgb <= 4 and n % 4 == 0 and n <= 4096
            and (h * w) % 4 == 0 and b * n <= 65535)


def _fused_backward(g_y, g_rgb, out, ws, noise, noise_w, abias, slope, gain, want_params, want_rgb_bias):
    """(gpre, gb, gnw, rdot, dws, gb_rgb): `op.smallconv._dx` (+ addend), `_dw` and `op.conv._nba_bwd_dot` in one launch."""
    g_rgb, ws = _smallconv._aligned(g_rgb), ws.contiguous()
    b, n, h, w = out.shape
    nrgb = ws.size(1)
    inner = h * w
    gpre = torch.empty_like(out)
    gb, gnw = param_grads(out, noise, want_params)
    rdot = torch.empty((b, n), dtype=out.dtype, device=out.device)
    dws = torch.empty((b, nrgb, n), dtype=out.dtype, device=out.device)
    gb_rgb = torch.empty(nrgb, dtype=out.dtype, device=out.device) if want_rgb_bias else None
    scratch = torch.empty(_lib.lib().sr_fork_nba_bwd_scratch_floats(b, n, nrgb, inner), dtype=out.dtype, device=out.device)
    native(out).sr_fork_nba_bwd(gpre, gb, gnw, rdot, dws, gb_rgb, g_y, out, g_rgb, ws, noise, noise_w, abias, slope, gain,
                                b, n, nrgb, inner, noise_stride(noise, inner), scratch)
    return gpre, gb, gnw, rdot, dws, gb_rgb


class ConvNBAForkFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wt, iscale, oscale, noise, noise_w, abias, slope, gain, ws, rgb_bias):
        mark_inputs(ctx, x, wt, iscale, oscale, noise, noise_w, abias, slope, gain, ws, rgb_bias)
        out = _conv._nba_forward(x, wt, iscale, oscale, noise, noise_w, abias, slope, gain)
        rgb = _smallconv._fwd(out, ws, rgb_bias)
        ctx.save_for_backward(x, wt, iscale, oscale, noise, noise_w, abias, out, ws)
        ctx.cfg = (float(slope), float(gain))
        ctx.frozen = bool(getattr(wt, "_sr_frozen", False))
        ctx.adj = getattr(wt, "_sr_adj", None)
        ctx.set_materialize_grads(False)                 # an unused output's cotangent stays None (no zero-fill)
        return out, rgb

    @staticmethod
    def backward(ctx, g_y, g_rgb):
        saved, ws = ctx.saved_tensors[:8], ctx.saved_tensors[8]
        noise, noise_w, abias, out = saved[4:]
        slope, gain = ctx.cfg
        needs = wanted(ctx)
        if g_y is None and g_rgb is None:
            return (None,) * 11
        fused = (g_rgb is not None and not torch.is_grad_enabled() and needs[9] and slope != 0.0 and gain != 0.0
                 and out.data_ptr() % 16 == 0
                 and (g_y is None or (g_y.is_contiguous() and g_y.data_ptr() % 16 == 0 and g_y.dtype == out.dtype
                                      and g_y.shape == out.shape)))
        if not fused:
            gy, gws, gb_rgb = _smallconv.fork_backward(out, ws, (True, needs[9], needs[10]), g_y, g_rgb)
            return _conv._nba_backward(saved, ctx.cfg, ctx.frozen, ctx.adj, needs[:9], gy) + (gws, gb_rgb)
        want_p = bool(needs[6] or (noise is not None and needs[5]))
        gpre, gb, gnw, rdot, dws, gb_rgb = _fused_backward(g_y, g_rgb, out, ws, noise, noise_w, abias, slope, gain, want_p,
                                                           needs[10])
        return _conv._nba_grads(saved, ctx.frozen, ctx.adj, needs[:9], want_p, gpre, gb, gnw, rdot) + (dws, gb_rgb)


def conv2d_nba_fork(x, wt, iscale, oscale, noise, noise_w, abias, slope, gain, ws, rgb_bias):
    """(y, rgb): y = lrelu(oscale*conv3x3(iscale*x, wt) + noise_w*noise + abias) * gain, rgb = conv1x1(y, ws) + rgb_bias."""
    y, rgb = ConvNBAForkFn.apply(x, wt, iscale, oscale, noise, noise_w, abias, slope, gain, ws, rgb_bias)
    # The next layer consumes an alias (no kernel, forward or backward), as it consumes `SmallConvFork`'s first output:
    # under a recorded backward y collects more than two cotangents (the next layer's node, that layer's recorded
    # operators, this node's own recorded ToRGB weight gradient), and floating-point addition does not associate.  With
    # the alias the next layer's share is summed first and arrives as one cotangent, exactly as with the two nodes.
    return y.view_as(y), rgb
