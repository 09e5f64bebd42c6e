"""FID Inception-v3 kernels (C ABI sr_incep_* / sr_fstats_*, csrc/inception.hip).

    conv(x, w, segs)          relu(conv(x) + bias) with folded BatchNorm, fp32 MFMA implicit GEMM, output rows
                              split over up to three (tensor, channel offset) destinations   reference BasicConv2d
    pool(x, mode, out, coff)  max 3x3/2, average 3x3/1 pad 1 (count_include_pad=False), max 3x3/1 pad 1
    gap(x)                    [B, C, H, W] -> [B, C] mean over H, W                          AdaptiveAvgPool2d(1)
    resize299(x)              bilinear to 299^2, F.interpolate(align_corners=False) (k_ppl_prep, shift 0, scale 1)
    stats_update / stats_finalize   fp64 sum and Gram of float32 feature rows -> mean, covariance

Forward only, device float32 tensors only: stylerenderer_amd/inception.py keeps the composite torch form for CPU
tensors.
"""
import ctypes

import torch

from . import ppl as _ppl
from ._dispatch import native, require_f32

POOL = {"max3s2": 0, "avg3s1": 1, "max3s1": 2}


class FoldedConv:
    """One GEMM of the native trunk: weight [K, M] (K = C * kh * kw, (c, ky, kx) order), bias [M], geometry."""

    def __init__(self, w, b, kh, kw, stride, ph, pw):
        self.m, k = w.shape[0], w[0].numel()
        self.c = w.shape[1]
        self.wt = w.reshape(self.m, k).t().contiguous()
        self.bias = b.contiguous()
        self.kh, self.kw, self.stride, self.ph, self.pw = kh, kw, stride, ph, pw

    def out_hw(self, h, w):
        return (h + 2 * self.ph - self.kh) // self.stride + 1, (w + 2 * self.pw - self.kw) // self.stride + 1


def conv(x, f, segs=None):
    """x [B, C, H, W] -> relu(conv + bias).  segs: [(out, m0, coff), ...] with m0 the first GEMM row that goes to `out`
    at channel `coff`; None allocates and returns a [B, M, OH, OW] tensor."""
    require_f32(x, "inception conv")
    x = x.contiguous()
    b, c, h, w = x.shape
    if c != f.c:
        raise ValueError("inception conv: %d input channels, weight expects %d" % (c, f.c))
    oh, ow = f.out_hw(h, w)
    ret = None
    if segs is None:
        ret = torch.empty(b, f.m, oh, ow, dtype=x.dtype, device=x.device)
        segs = [(ret, 0, 0)]
    n = len(segs)
    for out, _m0, _coff in segs:
        if (out.dtype != torch.float32 or not out.is_contiguous() or out.device != x.device or out.dim() != 4
                or tuple(out.shape[2:]) != (oh, ow) or out.shape[0] != b):
            raise ValueError("inception conv: destination must be contiguous float32 [%d, *, %d, %d] on %s"
                             % (b, oh, ow, x.device))
    outs = (ctypes.c_void_p * n)(*[s[0].data_ptr() for s in segs])
    m0 = (ctypes.c_int64 * n)(*[s[1] for s in segs])
    coff = (ctypes.c_int64 * n)(*[s[2] for s in segs])
    ctot = (ctypes.c_int64 * n)(*[s[0].shape[1] for s in segs])
    native(x).sr_incep_conv(x, f.wt, f.bias, b, c, h, w, f.m, f.kh, f.kw, f.stride, f.ph, f.pw, n, outs, m0, coff, ctot)
    return ret


def pool(x, mode, out=None, coff=0):
    require_f32(x, "inception pool")
    x = x.contiguous()
    b, c, h, w = x.shape
    oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == "max3s2" else (h, w)
    ret = None
    if out is None:
        out = ret = torch.empty(b, c, oh, ow, dtype=x.dtype, device=x.device)
    if (not out.is_contiguous() or out.device != x.device or out.dim() != 4 or out.shape[0] != b
            or tuple(out.shape[2:]) != (oh, ow) or out.dtype != torch.float32):
        raise ValueError("inception pool: destination must be contiguous float32 [%d, *, %d, %d]" % (b, oh, ow))
    native(x).sr_incep_pool(out, x, b, c, h, w, POOL[mode], coff, out.shape[1])
    return ret


def gap(x):
    require_f32(x, "inception gap")
    x = x.contiguous()
    b, c, h, w = x.shape
    out = torch.empty(b, c, dtype=x.dtype, device=x.device)
    native(x).sr_incep_gap(out, x, b * c, h * w)
    return out


def resize299(x, size=(299, 299)):
    zero = torch.zeros(3, dtype=torch.float32, device=x.device)
    one = torch.ones(3, dtype=torch.float32, device=x.device)
    return _ppl.prep(x, zero, one, (0, 0, x.shape[2], x.shape[3]), size)


def stats_update(total, gram, shift, feat, first):
    """Adds the rows of feat [n, d] (device float32) to the fp64 accumulators total [d] / gram [d, d] / shift [d]."""
    require_f32(feat, "feature stats")
    feat = feat.contiguous()
    n, d = feat.shape
    native(feat).sr_fstats_update(total, gram, shift, feat, n, d, 1 if first else 0)


def stats_finalize(total, gram, shift, count):
    d = total.numel()
    mean = torch.empty(d, dtype=torch.float64, device=total.device)
    cov = torch.empty(d, d, dtype=torch.float64, device=total.device)
    native(total).sr_fstats_finalize(mean, cov, total, gram, shift, count, d)
    return mean, cov
