"""Perceptual path length kernels (C ABI sr_ppl_endpoints / sr_ppl_prep / sr_lpips_pair, csrc/ppl.hip).

    endpoints(a, b, t, mode, eps, n_ends)   latents at t (and t + eps) of every pair, interleaved   reference ppl.py:14-19, 102-112
    prep(img, shift, scale, window, size)   crop window -> bilinear resize -> ScalingLayer          reference ppl.py:159-165
    lpips_pair(feats, lins, div)            per-pair LPIPS distance of interleaved samples / div     networks_basic.py:62-85

Forward only, device float32 tensors only: the callers (stylerenderer_amd/ppl.py, lpips.PNetLin.pair_distance) keep
the composite torch form for everything else.
"""
import ctypes

import torch

from .. import _lib
from ._dispatch import native, require_f32

MODES = {"w": 0, "z": 1}


def endpoints(a, b, t, mode, eps=0.0, n_ends=2, in_stride=None):
    """Pair i = rows a[i * in_stride ...], b[i * in_stride ...] (flat float32 storage of `d` = a.shape[-1] values each)
    at t[i] (and t[i] + eps when n_ends = 2) -> [npairs * n_ends, d], row i * n_ends + e."""
    require_f32(a, "ppl endpoints")
    d = a.shape[-1]
    npairs = t.numel()
    in_stride = d if in_stride is None else in_stride
    t = t.reshape(-1).contiguous()
    out = torch.empty(npairs * n_ends, d, dtype=a.dtype, device=a.device)
    native(a).sr_ppl_endpoints(out, a, b, in_stride, t, npairs, d, MODES[mode], n_ends, float(eps))
    return out


def pair_endpoints(x, t, mode, eps):
    """The sampled [2B, D] tensor read as pairs (x[::2], x[1::2]) -> [2B, D]: row 2i at t[i], row 2i+1 at t[i] + eps."""
    x = x.contiguous()
    d = x.shape[1]
    return endpoints(x, x.view(-1)[d:], t, mode, eps, 2, in_stride=2 * d)


def crop_window(h, w, crop):
    """(y0, x0, ch, cw) of the reference's --crop (rows 3c:7c, columns 2c:6c, c = H // 8), or the whole image."""
    if not crop:
        return 0, 0, h, w
    c = h // 8
    y1, x1 = min(7 * c, h), min(6 * c, w)
    return 3 * c, 2 * c, y1 - 3 * c, x1 - 2 * c


def prep(img, shift, scale, window, size):
    """img [N, 3, H, W] -> [N, 3, size[0], size[1]]: window (y0, x0, ch, cw), bilinear to `size` when it differs from
    (ch, cw), then (x - shift_c) / scale_c."""
    require_f32(img, "ppl prep")
    img = img.contiguous()
    n, c, h, w = img.shape
    if c != 3:
        raise ValueError("ppl prep: expected 3 channels, got %d" % c)
    y0, x0, ch, cw = window
    oh, ow = size
    out = torch.empty(n, 3, oh, ow, dtype=img.dtype, device=img.device)
    shift = shift.reshape(-1).to(img.device, torch.float32).contiguous()
    scale = scale.reshape(-1).to(img.device, torch.float32).contiguous()
    native(img).sr_ppl_prep(out, img, shift, scale, n, h, w, y0, x0, ch, cw, oh, ow)
    return out


def lpips_pair(feats, lins, div):
    """feats: list of raw trunk features [2B, C_k, H_k, W_k] (pair i = samples 2i, 2i+1); lins: [C_k] heads.
    -> [B] = sum_k mean_hw sum_c lin_k (f0/n0 - f1/n1)^2, divided by `div`."""
    feats = [f.contiguous() for f in feats]
    lins = [l.reshape(-1).contiguous() for l in lins]
    for f, l in zip(feats, lins):
        require_f32(f, "lpips_pair")
        if (f.dim() != 4 or f.shape[0] % 2 or f.shape[0] != feats[0].shape[0] or l.numel() != f.shape[1]
                or f.device != feats[0].device):
            raise ValueError("lpips_pair: features [2B, C, H, W] with heads [C] on one device expected")
    nl = len(feats)
    npairs = feats[0].shape[0] // 2
    c = (ctypes.c_int64 * nl)(*[f.shape[1] for f in feats])
    hw = (ctypes.c_int64 * nl)(*[f.shape[2] * f.shape[3] for f in feats])
    fp = (ctypes.c_void_p * nl)(*[f.data_ptr() for f in feats])
    lp = (ctypes.c_void_p * nl)(*[l.data_ptr() for l in lins])
    dev = feats[0].device
    scratch = torch.empty(_lib.lib().sr_lpips_pair_scratch_floats(npairs, nl, hw), dtype=torch.float32, device=dev)
    d = torch.empty(npairs, dtype=torch.float32, device=dev)
    native(feats[0]).sr_lpips_pair(d, fp, lp, c, hw, nl, npairs, float(div), scratch)
    return d
