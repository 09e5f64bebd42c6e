"""Dense convolution on the matrix cores — host side of csrc/conv_dispatch.hip (C ABI sr_conv2d_mfma; the kernels: csrc/conv_mfma.hip and its siblings).

Low-level operator used by layers.ModulatedConv2d / EqualConv2d for device tensors:

  conv2d_mfma(x, wt, iscale=None, oscale=None, obias=None, ksize=3, stride=1, pad=1, transposed=False)
    x [B,C,IH,IW] fp32, wt [k*k, C, N] (tap-major, N contiguous), iscale [B,C], oscale [B,N], obias [N]
    out[b,n] = oscale[b,n] * sum_{tap,c} wt[tap,c,n] * iscale[b,c] * x[b,c,window(tap)] + obias[n]

It replaces the F.conv2d / F.conv_transpose2d(groups=batch) calls of reference layers.py:301-322.
"""
import os
import threading

import torch

from .. import _lib
from ._dispatch import hold_for_capture, mark_inputs, native, require_f32, wanted
from . import weight_prep as _wp
from . import wgrad_style as _ws
from .fused_elem import noise_stride, param_grads, rowdot, rowdot_div


# Optional per-launch timing used by bench.py's roofline leg: when PROFILE is a list, every MFMA
# launch is bracketed by events on the launch stream and (kind, geometry, flops, start, end) appended.
PROFILE = None


def _timed(like, kind, geom, flops, launch):
    if PROFILE is None:
        return launch()
    stream = torch.cuda.current_stream(like.device)          # the launch stream: that of the operand's device
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    launch()
    e1.record(stream)
    PROFILE.append((kind, geom, flops, e0, e1))


def conv_out_size(ih, iw, ksize, stride, pad, transposed):
    if transposed:
        return (ih - 1) * stride + ksize - 2 * pad, (iw - 1) * stride + ksize - 2 * pad
    return (ih + 2 * pad - ksize) // stride + 1, (iw + 2 * pad - ksize) // stride + 1


def conv2d_mfma(x, wt, iscale=None, oscale=None, obias=None, ksize=3, stride=1, pad=1,
                transposed=False):
    require_f32(x, "conv2d_mfma")
    require_f32(wt, "conv2d_mfma weight")
    x = x.contiguous()
    b, c, ih, iw = x.shape
    taps, cw, n = wt.shape
    wt, ldw = _wt_pitch(wt)
    if taps != ksize * ksize or cw != c:
        raise RuntimeError("conv2d_mfma: weight must be [k*k, C, N]; got %s for C=%d k=%d"
                           % (tuple(wt.shape), c, ksize))
    oh, ow = conv_out_size(ih, iw, ksize, stride, pad, transposed)
    for t, shape, name in ((iscale, (b, c), "iscale"), (oscale, (b, n), "oscale"), (obias, (n,), "obias")):
        if t is not None:
            require_f32(t, "conv2d_mfma " + name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise RuntimeError("conv2d_mfma: %s must be contiguous %s" % (name, shape))
    out = torch.empty((b, n, oh, ow), dtype=x.dtype, device=x.device)
    gh, gw = (ih, iw) if transposed else (oh, ow)
    flops = 2.0 * b * gh * gw * c * n * ksize * ksize
    nscr = _lib.lib().sr_conv2d_scratch_floats(b, c, n, ih, iw, oh, ow, ksize, stride, pad, int(bool(transposed)))
    scratch, flags, entry = _conv_scratch(wt, nscr, (b, c, n, ih, iw, ksize, stride, pad, bool(transposed)), x)
    _timed(x, "conv", (ksize, stride, int(bool(transposed)), b, c, n, gh, gw), flops,
           lambda: native(x).sr_conv2d_mfma_ex(out, x, wt, iscale, oscale, obias, b, c, n, ldw, ih, iw, oh, ow, ksize,
                                               stride, pad, int(bool(transposed)), flags, scratch))
    _scratch_written(entry, b, c, n, ih, iw, x, out)
    return out


class _Scratch:
    """One persistent scratch of a frozen weight: `ready` says that its leading block HOLDS the Winograd-domain weights —
    set only after a call that (a) was executed, not merely recorded into a graph under capture, and (b) was served by
    the Winograd kernel for its actual buffers (sr_conv2d_uses_winograd: 16-byte alignment of input / output is part of
    the rule; a misaligned first call runs the direct kernel and writes no weights).  ADVICE r4: the entry used to count
    as ready from its creation."""
    __slots__ = ("buf", "ready")

    def __init__(self, buf):
        self.buf, self.ready = buf, False


def _conv_scratch(wt, nscr, key, like):
    """(scratch, flags, entry) of one convolution call.  Weights a frozen network prepared once (`wt._sr_frozen`: latent
    inversion, the LPIPS trunk) keep ONE scratch per call geometry of the stride-1 3x3 convolution: its leading block
    holds the Winograd-domain weights, which later calls reuse (SR_CONV_U_READY: one k_wino_weights launch less per
    convolution and step) once a call has really written them (`_Scratch.ready`, `_scratch_written`); the split-K
    region behind it is rewritten by every call.  The buffer lives as long as the prepared weight (a new weight
    version makes a new prepared tensor) and as any graph captured over it.
    One stream per frozen network: two streams convolving with the same prepared weight and geometry at the same time
    would share the split-K region (the loops that freeze a network — inversion, sampling — run on one stream)."""
    if nscr <= 0:
        return None, 0, None
    if not (getattr(wt, "_sr_frozen", False) and key[5:] == (3, 1, 1, False)) or os.environ.get("SR_U_CACHE", "1") == "0":
        return torch.empty(nscr, dtype=like.dtype, device=like.device), 0, None
    cache = wt.__dict__.setdefault("_sr_scratch", {})
    k = key + (os.environ.get("SR_WINOGRAD", "1"), os.environ.get("SR_WINO_SPLIT", "1"), wt._version, wt.data_ptr())
    hit = cache.get(k)
    if hit is None or hit.buf.numel() < nscr:
        if len(cache) >= 6:                      # a handful of geometries per weight (batch sizes of one loop)
            cache.clear()
        hit = cache[k] = _Scratch(torch.empty(nscr, dtype=like.dtype, device=like.device))
    hold_for_capture(hit.buf)
    return hit.buf, (1 if hit.ready else 0), hit


def _scratch_written(entry, b, c, n, h, w, x, out):
    """After a successful launch: the entry's weight block is valid from now on iff this call was executed (not
    captured) and took the Winograd kernel."""
    if entry is None or entry.ready:
        return
    if x.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    if _lib.lib().sr_conv2d_uses_winograd(b, c, n, h, w, _lib.ptr(x), _lib.ptr(out)):
        entry.ready = True


class _StyleRequest:
    """Set (per thread) by `_conv_grads` around ONE conv2d_wgrad_mfma call that is also to yield the style gradient: the
    forward weight in, gis [B, C] out (op.wgrad_style).  A request and not an argument: the call keeps the signature
    and the return value that WgradFn and everything wrapped around the function rely on."""
    __slots__ = ("wt", "gis")

    def __init__(self, wt):
        self.wt, self.gis = wt, None


_TLS = threading.local()


def conv2d_wgrad_mfma(x, gy, xscale=None, gscale=None, ksize=3, stride=1, pad=1, transposed=False):
    """dwt [k*k, C, N] = sum over batch and pixels of (xscale*x)[window] * (gscale*gy)."""
    require_f32(x, "conv2d_wgrad_mfma")
    require_f32(gy, "conv2d_wgrad_mfma grad")
    x = x.contiguous()
    gy = gy.contiguous()
    b, c, ih, iw = x.shape
    b2, n, oh, ow = gy.shape
    if b2 != b or (oh, ow) != conv_out_size(ih, iw, ksize, stride, pad, transposed):
        raise RuntimeError("conv2d_wgrad_mfma: shape mismatch x %s gy %s" % (tuple(x.shape), tuple(gy.shape)))
    for t, shape, name in ((xscale, (b, c), "xscale"), (gscale, (b, n), "gscale")):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous() or t.dtype != torch.float32):
            raise RuntimeError("conv2d_wgrad_mfma: %s must be contiguous float32 %s" % (name, shape))
    if (ksize == 1 and stride == 1 and pad == 0 and not transposed and c <= 4 and xscale is None and gscale is None
            and (ih * iw) % 4 == 0 and b * n <= 65535 and n <= 4096 and os.environ.get("SR_WGRAD_SMALL", "1") != "0"):
        # the discriminator's from-RGB layer (3 -> 128 channels, 1x1, reference model.py:304): on 64-channel MFMA tiles
        # that is 5 % useful work; it IS the streaming row-product kernel of ToRGB with the roles of the two operands
        # swapped — dws[b, c, n] = sum_p x[b, c, p] * gy[b, n, p] — followed by the sum over the batch.  (With operand
        # scales — the map heads' 3 -> 4 skip layers — the two extra element-wise launches cost what the kernel saves:
        # measured, left on the MFMA path.)
        from .smallconv import _dw

        return _dw(x, gy).sum(0).view(1, c, n)
    gh, gw = (ih, iw) if transposed else (oh, ow)
    flops = 2.0 * b * gh * gw * c * n * ksize * ksize
    req = getattr(_TLS, "style", None)
    if req is not None and req.gis is None:
        wtp, ldw = _wt_pitch(req.wt)
        dwt, req.gis = _ws.wgrad_style(
            x, gy, xscale, gscale, wtp, ldw, ksize, stride, pad, transposed,
            lambda launch: _timed(x, "wgrad", (ksize, stride, int(bool(transposed)), b, c, n, gh, gw), flops, launch))
        return dwt
    nfl = _lib.lib().sr_conv2d_wgrad_scratch_floats(b, c, n, ih, iw, oh, ow, ksize, stride, pad, int(bool(transposed)))
    if nfl < 0:
        raise RuntimeError("conv2d_wgrad_mfma: unsupported geometry")
    scratch = torch.empty(nfl, dtype=torch.float32, device=x.device)
    dwt = torch.empty((ksize * ksize, c, n), dtype=torch.float32, device=x.device)
    _timed(x, "wgrad", (ksize, stride, int(bool(transposed)), b, c, n, gh, gw), flops,
           lambda: native(x).sr_conv2d_wgrad_mfma(dwt, x, gy, xscale, gscale, b, c, n, ih, iw, oh, ow, ksize, stride, pad,
                                                  int(bool(transposed)), scratch))
    return dwt


# ------------------------------------------------------------------------------------------------
# Differentiable operators. Two mutually recursive autograd Functions close the algebra:
#   ConvFn   y  = oscale * conv(iscale * x, wt) + bias
#   WgradFn  dW = sum_b corr(iscale * x, oscale * g)
# d(ConvFn)/dx is a ConvFn with the adjoint geometry, d(ConvFn)/dwt is a WgradFn, and both
# derivatives of WgradFn are ConvFn's — so gradients of any order (path-length regulariser,
# R1: reference train.py:110-134) run on the same two MFMA kernels.
_ADJOINT = {"c3": "c3", "c3s2": "t3s2", "t3s2": "c3s2", "c1": "c1"}
_GEOM = {  # name -> (ksize, stride, pad, transposed)
    "c3": (3, 1, 1, False), "c3s2": (3, 2, 0, False), "t3s2": (3, 2, 0, True), "c1": (1, 1, 0, False),
    "c1s2": (1, 2, 0, False),
}


def adjoint_weight(wt, geom, frozen=False, banked=None):
    """Weights of the data-gradient convolution: channels swapped; taps reversed for the
    stride-1 3x3 correlation (the strided pair c3s2 <-> t3s2 keeps tap order).  `frozen`: the prepared weight
    belongs to a module frozen with op.weight_prep.freeze_prepared_weights — its adjoint is computed once.
    `banked`: (flip, adjoint) prepared together with `wt` by op.weight_bank for all layers of the pass — plain data,
    used when this backward is not itself being recorded (a recorded one needs the adjoint as a function of `wt`)."""
    if banked is not None and banked[0] == (geom == "c3") and not torch.is_grad_enabled():
        return banked[1]
    if frozen and not wt.requires_grad and not torch.is_grad_enabled():
        return _wp.adjoint_cached(wt, geom == "c3")
    return _wp.adjoint(wt, geom == "c3")


def _bc(s):
    return s[:, :, None, None]


def _input_grads(x, g, wt, iscale, oscale, geom, need_x, need_is, frozen=False, banked=None, fused=True):
    """(gx, gis) of y = oscale * conv(iscale * x, wt) for the cotangent g: the data gradient through the adjoint
    `ConvFn`, then the style gradient sum_p x*dxu and dx = iscale*dxu — in one sweep (csrc/fused_elem.hip) where
    `fused` and both are wanted.  `need_is` implies an `iscale`: `needs_input_grad` is False for a None input."""
    if not (need_x or need_is):
        return None, None
    if geom == "c1s2":
        inner = ConvFn.apply(g, adjoint_weight(wt, "c1", frozen, banked), oscale, None, None, "c1")
        dxu = torch.zeros_like(x)
        dxu[:, :, ::2, ::2] = inner
    else:
        dxu = ConvFn.apply(g, adjoint_weight(wt, geom, frozen, banked), oscale, None, None, _ADJOINT[geom])
    if fused and need_is and need_x:
        gis, gx = rowdot(x, dxu, iscale)
        return gx, gis
    gis = rowdot(x, dxu) if need_is else None
    gx = (dxu * _bc(iscale) if iscale is not None else dxu) if need_x else None
    return gx, gis


# How often `_conv_grads` formed a wanted style gradient in the weight gradient's finish / by the row-dot pass (tests)
STYLE_PATH_COUNTS = {"wgrad": 0, "rowdot": 0}


def _conv_grads(x, g, wt, iscale, oscale, geom, need_x, need_w, need_is, frozen=False, banked=None):
    """(gx, gw, gis) of y = oscale * conv(iscale * x, wt) for the cotangent g: the backward the three convolution nodes
    share.  Where the weight and the style gradient are both wanted, the pass is not itself recorded and the weight
    gradient's plan cuts K into whole slices per sample (`op.wgrad_style.part_floats`), the style gradient comes out of
    the weight gradient's finish kernel and the adjoint convolution applies the style in its store (its `oscale`):
    no row-dot pass over x and the data gradient.  SR_STYLE_FROM_WGRAD=0, and every other case: `_input_grads` and
    `WgradFn` as before, bit for bit."""
    if (need_w and need_is and iscale is not None and geom in ("c3", "t3s2") and not torch.is_grad_enabled()
            and os.environ.get("SR_STYLE_FROM_WGRAD", "1") != "0" and _ws.part_floats(x, g, *_GEOM[geom]) >= 0):
        STYLE_PATH_COUNTS["wgrad"] += 1
        gx = None
        if need_x:
            gx = ConvFn.apply(g, adjoint_weight(wt, geom, frozen, banked), oscale, iscale, None, _ADJOINT[geom])
        req = _TLS.style = _StyleRequest(wt)
        try:
            gw = conv2d_wgrad_mfma(x, g, iscale, oscale, *_GEOM[geom])
        finally:
            _TLS.style = None
        return gx, gw, req.gis
    if need_is:
        STYLE_PATH_COUNTS["rowdot"] += 1
    gx, gis = _input_grads(x, g, wt, iscale, oscale, geom, need_x, need_is, frozen, banked)
    gw = WgradFn.apply(x, g, iscale, oscale, geom) if need_w else None
    return gx, gw, gis


class ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wt, iscale, oscale, bias, geom):
        mark_inputs(ctx, x, wt, iscale, oscale, bias, geom)
        k, stride, pad, tr = _GEOM[geom]
        out = conv2d_mfma(x, wt, iscale, oscale, bias, k, stride, pad, tr)
        ctx.frozen = bool(getattr(wt, "_sr_frozen", False))
        ctx.adj = getattr(wt, "_sr_adj", None)
        ctx.geom = geom
        ctx.has = (iscale is not None, oscale is not None, bias is not None)
        ctx.save_for_backward(x, wt, iscale, oscale, bias, out if oscale is not None else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, wt, iscale, oscale, bias, out = ctx.saved_tensors
        need_x, need_w, need_is, need_os, need_b = wanted(ctx)[:5]      # minus what this pass would discard
        geom = ctx.geom
        g = g.contiguous()
        gos = gb = None
        gx, gw, gis = _conv_grads(x, g, wt, iscale, oscale, geom, need_x, need_w, need_is, ctx.frozen, ctx.adj)
        if need_os:
            y0 = out - bias[None, :, None, None] if bias is not None else out
            gos = rowdot_div(g, y0, oscale)
        if need_b:
            gb = g.sum((0, 2, 3))
        return gx, gw, gis, gos, gb, None


class WgradFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, g, iscale, oscale, geom):
        mark_inputs(ctx, x, g, iscale, oscale, geom)
        k, stride, pad, tr = _GEOM[geom]
        ctx.geom = geom
        ctx.save_for_backward(x, g, iscale, oscale)
        return conv2d_wgrad_mfma(x, g, iscale, oscale, k, stride, pad, tr)

    @staticmethod
    def backward(ctx, gg):
        """gg = d/d(dW) [k*k, C, N]."""
        x, g, iscale, oscale = ctx.saved_tensors
        need_x, need_g, need_is, need_os = wanted(ctx)[:4]
        geom = ctx.geom
        gg = gg.contiguous()
        g_g = gos = None
        gx, gis = _input_grads(x, g, gg, iscale, oscale, geom, need_x, need_is, fused=False)
        if need_g or need_os:
            dgu = ConvFn.apply(x, gg, iscale, None, None, geom)
            if need_os:
                gos = rowdot(g, dgu)
            if need_g:
                g_g = dgu * _bc(oscale) if oscale is not None else dgu
        return gx, g_g, gis, gos, None


# ------------------------------------------------------------------------------------------------
# Modulated 3x3 convolution + noise + bias + LeakyReLU as ONE node (non-upsampling StyledConv, reference
# model.py:11-32).  Forward: the Winograd kernel applies the tail in its store (the pre-activation tensor
# is never written).  Backward: the activation backward also emits sum_p g*y0 (the demodulation gradient,
# y0 rebuilt from the output), then the usual data / weight gradient kernels.  When the backward pass is
# itself recorded (create_graph) the VJP is re-derived from the two separate differentiable operators.
def _aliases(*tensors):
    """Fresh graph nodes for the saved inputs of a fused node.  The second-order fallback re-derives the VJP
    with autograd.grad; asking it for gradients w.r.t. the saved tensors themselves would also follow the
    history that links them OUTSIDE the node (the demodulation scale is a function of the style) and count
    those paths twice.  Gradients w.r.t. the aliases stop at the node boundary, and stay differentiable."""
    return [t.view_as(t) if t is not None else None for t in tensors]


def _recorded_backward(saved, needs, gy, rebuild):
    """Backward of a fused node while that backward is itself recorded (create_graph): the output is rebuilt from the
    separate differentiable operators — `rebuild(*aliases)` of `saved`, the node's leading inputs (None where one takes
    no gradient) — and its VJP taken for the inputs that `needs` one.  One gradient per forward input."""
    with torch.enable_grad():
        ins = _aliases(*saved)
        y = rebuild(*ins)
        sel = [t for t, nd in zip(ins, needs) if nd and t is not None]
        got = iter(torch.autograd.grad(y, sel, gy, create_graph=True, allow_unused=True)) if sel else iter(())
        grads = [next(got) if (nd and t is not None) else None for t, nd in zip(ins, needs)]
    return tuple(grads) + (None,) * (len(needs) - len(ins))


def conv_nba_shape_ok(x, n, noise):
    """Shape / layout part of `conv_nba_supported` (no weights needed): the library's dispatch takes the Winograd kernel
    for this input (sr_conv2d_path; the output is allocated by the caller, aligned), one grid row per (sample, channel)."""
    if x.device.type != "cuda" or x.dtype != torch.float32 or not x.is_contiguous():
        return False
    b, c, h, w = x.shape
    ok = b * n <= 65535 and _lib.lib().sr_conv2d_path(b, c, n, h, w, h, w, 3, 1, 1, 0, _lib.ptr(x), None, None, 0,
                                                      1) == _lib.CONV_PATH_WINO
    if noise is not None:
        ok = ok and noise.dtype == torch.float32 and noise.numel() in (h * w, b * h * w) and noise.data_ptr() % 16 == 0
    return ok


def conv_nba_supported(x, wt, noise):
    return wt.shape[0] == 9 and conv_nba_shape_ok(x, wt.shape[2], noise)


def _wt_pitch(wt):
    """(wt, row pitch): the kernels read weight rows as 16-byte vectors — row pitch a multiple of 4 floats (views of the
    padded buffers of op.weight_prep pass through untouched)."""
    taps, cw, n = wt.shape
    if (wt.stride(2) == 1 and wt.stride(1) % 4 == 0 and wt.stride(1) >= n and wt.stride(0) == cw * wt.stride(1)
            and wt.data_ptr() % 16 == 0):
        return wt, wt.stride(1)
    ldw = (n + 3) // 4 * 4
    return (torch.nn.functional.pad(wt, (0, ldw - n)) if ldw != n else wt.contiguous()), ldw


def _nba_forward(x, wt, iscale, oscale, noise, noise_w, abias, slope, gain):
    """The launch of `ConvNBAFn.forward` (and of op.fork_tail's node): convolution with the tail in its store."""
    b, c, h, w = x.shape
    n = wt.shape[2]
    wtp, ldw = _wt_pitch(wt)
    out = torch.empty((b, n, h, w), dtype=x.dtype, device=x.device)
    nscr = _lib.lib().sr_conv2d_scratch_floats(b, c, n, h, w, h, w, 3, 1, 1, 0)
    scratch, flags, entry = _conv_scratch(wt if wtp is wt else wtp, max(nscr, 1), (b, c, n, h, w, 3, 1, 1, False), x)
    flops = 2.0 * b * h * w * c * n * 9
    _timed(x, "conv", (3, 1, 0, b, c, n, h, w), flops,
           lambda: native(x).sr_conv2d_nba_ex(out, x, wtp, iscale, oscale, noise, noise_w, abias, float(slope),
                                              float(gain), b, c, n, ldw, h, w, noise_stride(noise, h * w), flags,
                                              scratch))
    _scratch_written(entry, b, c, n, h, w, x, out)
    return out


def _nba_backward(saved, cfg, frozen, adj, needs, gy):
    """The backward of `ConvNBAFn` for the cotangent gy: `saved` = (x, wt, iscale, oscale, noise, noise_w, abias, out),
    `needs` one flag per forward input.  Nine gradients."""
    from .fused_elem import _NBA

    x, wt, iscale, oscale, noise, noise_w, abias, out = saved
    slope, gain = cfg
    if torch.is_grad_enabled() and oscale is not None:
        # a recorded backward of the DEMODULATED layer needs the pre-activation as a function of its operands (the
        # demodulation gradient is sum_p g * y0): re-derived from the separate operators.  Without demodulation (the
        # discriminator's layers under R1, the LPIPS trunk) nothing below reads y0 — the operators of the plain
        # branch are differentiable themselves and record the same pass without convolving again
        return _recorded_backward(
            (x, wt, iscale, oscale, None, noise_w, abias), needs, gy,
            lambda xa, wa, sa, da, _, nwa, aba: _NBA.apply(ConvFn.apply(xa, wa, sa, da, None, "c3"), noise, nwa, aba,
                                                           slope, gain, out.detach()))
    want_p = bool(needs[6] or (noise is not None and needs[5]))
    if oscale is None:
        # no demodulation (the LPIPS trunk's plain convolution + bias + ReLU): nothing to row-dot — and with slope 0
        # the pre-activation cannot be rebuilt from the output anyway
        from .fused_elem import _NBABackward

        g, gb, gnw = _NBABackward.apply(gy, out, noise, slope, gain, want_p)
        rdot = None
    else:
        g, gb, gnw, rdot = _nba_bwd_dot(gy, out, noise, noise_w, abias, slope, gain, want_p)
    return _nba_grads(saved, frozen, adj, needs, want_p, g, gb, gnw, rdot)


def _nba_grads(saved, frozen, adj, needs, want_p, g, gb, gnw, rdot):
    """The nine gradients of `ConvNBAFn` from the activation backward's outputs: g (cotangent of the convolution), gb, gnw
    (bias / noise-strength gradients, where want_p) and rdot (demodulation row-dots, None without demodulation)."""
    x, wt, iscale, oscale, noise = saved[:5]
    gos = None
    gx, gw, gis = _conv_grads(x, g, wt, iscale, oscale, "c3", needs[0], needs[1], needs[2], frozen, adj)
    if needs[3] and oscale is not None:
        gos = rdot / oscale
    return (gx, gw, gis, gos, None, (gnw if noise is not None and want_p and needs[5] else None),
            (gb if want_p and needs[6] else None), None, None)


class ConvNBAFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wt, iscale, oscale, noise, noise_w, abias, slope, gain):
        mark_inputs(ctx, x, wt, iscale, oscale, noise, noise_w, abias, slope, gain)
        out = _nba_forward(x, wt, iscale, oscale, noise, noise_w, abias, slope, gain)
        ctx.save_for_backward(x, wt, iscale, oscale, noise, noise_w, abias, out)
        ctx.cfg = (float(slope), float(gain))
        ctx.frozen = bool(getattr(wt, "_sr_frozen", False))
        ctx.adj = getattr(wt, "_sr_adj", None)
        return out

    @staticmethod
    def backward(ctx, gy):
        return _nba_backward(ctx.saved_tensors, ctx.cfg, ctx.frozen, ctx.adj, wanted(ctx), gy)


def _nba_bwd_dot(gy, out, noise, noise_w, abias, slope, gain, want_params=True):
    """Activation backward + bias / noise-strength gradients + demodulation row-dots in one pass (want_params False:
    frozen bias / noise strength — their reduction launches are skipped, gb / gnw come back empty)."""
    gy = gy.contiguous()
    b, n, h, w = out.shape
    inner = h * w
    g = torch.empty_like(out)
    gb, gnw = param_grads(out, noise, want_params)
    rdot = torch.empty((b, n), dtype=out.dtype, device=out.device)
    scratch = torch.empty(_lib.lib().sr_noise_bias_act_bwd_dot_scratch_floats(b, n, inner), dtype=out.dtype,
                          device=out.device)
    native(out).sr_noise_bias_act_bwd_dot(g, gb, gnw, rdot, gy, out, noise, noise_w, abias, slope, gain, b, n, inner,
                                          noise_stride(noise, inner), scratch)
    return g, gb, gnw, rdot


def _blur_bwd_fused():
    """SR_BLUR_BWD_FUSED=0: the two-kernel backward of the up-sampling layer's tail (A/B measurements)."""
    import os

    return os.environ.get("SR_BLUR_BWD_FUSED", "1") != "0"


def _blur_nba_bwd(gy, out, k_flipped, p0, shape257, noise, noise_w, abias, slope, gain, want_params=True):
    """csrc/upfirdn2d.hip k_fir4_nba_bwd: gradient w.r.t. the blur's input plus what `_nba_bwd_dot` returns."""
    gy = gy.contiguous()
    b, n, oh, ow = out.shape
    g257 = torch.empty(shape257, dtype=out.dtype, device=out.device)
    gb, gnw = param_grads(out, noise, want_params, zero_empty=False)
    rdot = torch.empty((b, n), dtype=out.dtype, device=out.device)
    scratch = torch.empty(_lib.lib().sr_blur_nba_bwd_scratch_floats(b, n, shape257[2], shape257[3]), dtype=out.dtype,
                          device=out.device)
    native(out).sr_blur_nba_bwd(g257, gb, gnw, rdot, gy, out, k_flipped, noise, noise_w, abias, slope, gain, b, n, oh, ow,
                                shape257[2], shape257[3], p0, noise_stride(noise, oh * ow), scratch)
    return g257, gb, gnw, rdot


def upconv_nba_supported(x, wt, noise, oh, ow):
    b = x.shape[0]
    n = wt.shape[2]
    ok = (x.device.type == "cuda" and x.dtype == torch.float32 and wt.shape[0] == 9 and (oh * ow) % 4 == 0
          and b * n <= 65535)
    if noise is not None:
        ok = ok and noise.dtype == torch.float32 and noise.numel() in (oh * ow, b * oh * ow) and noise.data_ptr() % 16 == 0
    return ok


class UpConvNBAFn(torch.autograd.Function):
    """Upsampling StyledConv (reference model.py:11-32 with layers.py:304-311) as one node: stride-2 transposed
    convolution -> [blur + noise + bias + LeakyReLU] (one kernel).  Backward: the activation backward also
    yields the demodulation gradient — <blur^T g, y257> = <g, blur(y257)> = sum_p g * y0 with y0 rebuilt from
    the output — so neither the 257^2 convolution output nor a row-dot pass over it is needed."""

    @staticmethod
    def forward(ctx, x, wt, iscale, oscale, kernel, pad, noise, noise_w, abias, slope, gain):
        from .fused_elem import _BlurNBA

        mark_inputs(ctx, x, wt, iscale, oscale, kernel, pad, noise, noise_w, abias, slope, gain)
        y257 = conv2d_mfma(x, wt, iscale, oscale, None, 3, 2, 0, True)
        out = _BlurNBA.forward(_NoCtx(), y257, kernel, pad, noise, noise_w, abias, slope, gain)
        ctx.save_for_backward(x, wt, iscale, oscale, kernel, noise, noise_w, abias, out)
        ctx.cfg = (tuple(pad), float(slope), float(gain), tuple(y257.shape))
        ctx.frozen = bool(getattr(wt, "_sr_frozen", False))
        ctx.adj = getattr(wt, "_sr_adj", None)
        return out

    @staticmethod
    def backward(ctx, gy):
        from .fused_elem import _BlurNBA
        from .upfirdn2d import flipped, upfirdn2d_op

        x, wt, iscale, oscale, kernel, noise, noise_w, abias, out = ctx.saved_tensors
        pad, slope, gain, shape257 = ctx.cfg
        needs = wanted(ctx)
        if torch.is_grad_enabled():
            return _recorded_backward(
                (x, wt, iscale, oscale, None, None, None, noise_w, abias), needs, gy,
                lambda xa, wa, sa, da, _k, _p, _n, nwa, aba: _BlurNBA.apply(
                    ConvFn.apply(xa, wa, sa, da, None, "t3s2"), kernel, pad, noise, nwa, aba, slope, gain, out.detach()))
        want_p = bool(needs[8] or (noise is not None and needs[7]))
        p0 = pad[0]
        oh, ow = out.shape[2], out.shape[3]
        if (_blur_bwd_fused() and pad[0] == pad[1] and shape257[2] == oh + 3 - 2 * p0 and shape257[3] == ow + 3 - 2 * p0
                and tuple(kernel.shape) == (4, 4)):
            # activation backward, its three reductions and the blur's gradient in one pass over gy and out
            g257, gb, gnw, rdot = _blur_nba_bwd(gy, out, flipped(kernel), p0, shape257, noise, noise_w, abias, slope,
                                                gain, want_p)
        else:
            g, gb, gnw, rdot = _nba_bwd_dot(gy, out, noise, noise_w, abias, slope, gain, want_p)
            g257 = upfirdn2d_op(g.reshape(-1, oh, ow, 1), flipped(kernel), 1, 1, 1, 1, 3 - p0,
                                shape257[3] - ow + p0, 3 - p0, shape257[2] - oh + p0).view(shape257)
        gos = None
        gx, gw, gis = _conv_grads(x, g257, wt, iscale, oscale, "t3s2", needs[0], needs[1], needs[2], ctx.frozen, ctx.adj)
        if needs[3] and oscale is not None:
            gos = rdot / oscale
        return (gx, gw, gis, gos, None, None, None, (gnw if noise is not None and want_p and needs[7] else None),
                (gb if want_p and needs[8] else None), None, None)


class _NoCtx:
    """Stand-in context for calling an autograd Function's forward as a plain launcher."""

    def save_for_backward(self, *a):
        pass


def upconv_nba(x, wt, iscale, oscale, kernel, pad, noise, noise_w, abias, slope=0.2, gain=2 ** 0.5):
    return UpConvNBAFn.apply(x, wt, iscale, oscale, kernel, tuple(pad), noise, noise_w, abias, slope, gain)


def conv2d_nba(x, wt, iscale, oscale, noise, noise_w, abias, slope=0.2, gain=2 ** 0.5):
    """lrelu(oscale*conv3x3(iscale*x, wt) + noise_w*noise + abias) * gain in one node (see ConvNBAFn)."""
    return ConvNBAFn.apply(x, wt, iscale, oscale, noise, noise_w, abias, slope, gain)


class Conv1x1AddFn(torch.autograd.Function):
    """out = oscale * conv1x1(x, wt) + addend in one launch (csrc/conv1x1_gemm.hip, sr_conv1x1_add): the skip branch of the
    discriminator's ResBlock with the sum of the two branches in its store (reference model.py ResBlock.forward) — the
    separate addition was a read-read-write pass of the block's output.  Backward: the 1x1 operators of ConvFn (so any
    order of differentiation stays on them) and the cotangent itself for the addend."""

    @staticmethod
    def forward(ctx, x, wt, oscale, addend):
        mark_inputs(ctx, x, wt, oscale, addend)
        b, c, h, w = x.shape
        n = wt.shape[2]
        out = torch.empty((b, n, h, w), dtype=x.dtype, device=x.device)
        native(x).sr_conv1x1_add(out, x, wt, oscale, addend, b, c, n, wt.stride(1), h * w)
        ctx.frozen = bool(getattr(wt, "_sr_frozen", False))
        ctx.adj = getattr(wt, "_sr_adj", None)
        ctx.save_for_backward(x, wt, oscale)
        return out

    @staticmethod
    def backward(ctx, g):
        x, wt, oscale = ctx.saved_tensors
        need_x, need_w, _, need_a = wanted(ctx)[:4]
        g = g.contiguous()
        gx = gw = None
        if need_x:
            gx = ConvFn.apply(g, adjoint_weight(wt, "c1", ctx.frozen, ctx.adj), oscale, None, None, "c1")
        if need_w:
            gw = WgradFn.apply(x, g, None, oscale, "c1")
        return gx, gw, None, (g if need_a else None)


def conv1x1_add(x, wt, oscale, addend):
    """oscale * conv1x1(x, wt) + addend: fused where the GEMM-shaped kernel takes the shape, else the two operators.
    `oscale` is a constant table (no gradient flows to it)."""
    ok = (x.device.type == "cuda" and x.dtype == torch.float32 and addend.dtype == torch.float32 and x.is_contiguous()
          and addend.is_contiguous() and wt.dim() == 3 and wt.shape[0] == 1 and wt.stride(2) == 1
          and wt.stride(1) % 4 == 0 and (oscale is None or (oscale.is_contiguous() and not oscale.requires_grad))
          and tuple(addend.shape) == (x.shape[0], wt.shape[2], x.shape[2], x.shape[3]))
    if ok:
        b, c, h, w = x.shape
        ok = bool(_lib.lib().sr_conv1x1_add_supported(b, c, wt.shape[2], wt.stride(1), h * w, _lib.ptr(x), _lib.ptr(wt),
                                                      _lib.ptr(addend), _lib.ptr(addend)))
    if not ok:
        return ConvFn.apply(x, wt, None, oscale, None, "c1") + addend
    return Conv1x1AddFn.apply(x, wt, oscale, addend)


def conv2d(x, wt, iscale=None, oscale=None, bias=None, geom="c3"):
    """Differentiable (to any order) MFMA convolution; see ConvFn."""
    return ConvFn.apply(x, wt, iscale, oscale, bias, geom)
