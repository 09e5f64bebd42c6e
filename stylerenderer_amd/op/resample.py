"""Pillow-exact resampling of uint8 images (C ABI sr_resample_u8, csrc/resample.hip).

    coefficients(in_size, out_size, filter)          -> (int32 [out, ksize] fixed-point taps, int32 [out, 2] (first, count))
    resize_u8(img, size, filter, window, out)        [N, H, W, C] or [H, W, C] uint8 -> the resized image (or a window of it)
    resize_center_crop(img, size, filter, out)       shorter side to `size`, centre crop size x size (torchvision geometry)
    resize_pyramid(img, sizes, filter, out)          {size: resize_center_crop(img, size)}, every size from the one source

Pillow's 8-bit resampler is integer arithmetic on fixed-point coefficients: two separable passes (horizontal into a
uint8 intermediate, then vertical), each output byte clip(0, 255, (2^21 + sum pixel * k) >> 22) in int32.  Integer sums
do not depend on their order, so the host restatement below (numpy; the DEFINITION, compared with Pillow byte for byte
in tests/test_resample_cpu.py) and the kernels give the same bytes.  CPU tensors and arrays take the host path, device
uint8 tensors the kernels; there is no fallback between the two.

The coefficient tables are built on the host in float64 with math.sin / math.cos (the C library's, like Pillow's own)
and cached per (in, out, filter); their device copies are cached per device.  `nearest` is not offered: Pillow's
nearest goes through its affine transform, not through this resampler.
"""
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from ._dispatch import DerivedCache, native

PRECISION_BITS = 32 - 8 - 2
ROUND = 1 << (PRECISION_BITS - 1)
OUT_FORMS = {"u8_hwc": 0, "f32_chw": 1}


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0),
           "lanczos": (_lanczos, 3.0)}


def _filter(name):
    key = str(name).lower()
    if key == "nearest":
        raise ValueError("resample: 'nearest' is not supported: Pillow's nearest is an affine transform, not a pass of "
                         "its resampler, and has no exact restatement here; use one of %s" % ", ".join(sorted(FILTERS)))
    if key not in FILTERS:
        raise ValueError("resample: unknown filter %r; use one of %s" % (name, ", ".join(sorted(FILTERS))))
    return key


_TABLES = {}      # (in, out, filter) -> (coeffs, bounds, fits24)
_DEVICE = DerivedCache(64)      # (in, out, filter, device, transposed) -> (coeffs, bounds) device tensors


def _tables(in_size, out_size, name):
    key = (int(in_size), int(out_size), _filter(name))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    in_size, out_size, name = key
    if in_size < 1 or out_size < 1:
        raise ValueError("resample: sizes must be positive, got %d -> %d" % (in_size, out_size))
    fn, support = FILTERS[name]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = support * fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    coeffs = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * inv) for x in range(n)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        coeffs[xx, :n] = [int((-0.5 if v < 0 else 0.5) + v * (1 << PRECISION_BITS)) for v in w]
        bounds[xx] = (xmin, n)
    # below 2^23 in magnitude, pixel * k is a 24-bit multiply-add at full rate; the kernels take the 32-bit one otherwise
    fits24 = bool(np.abs(coeffs.astype(np.int64)).max() < (1 << 23))
    coeffs.setflags(write=False)
    bounds.setflags(write=False)
    _TABLES[key] = (coeffs, bounds, fits24)
    return _TABLES[key]


def coefficients(in_size, out_size, filter="lanczos"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis: (int32 [out, ksize], int32 [out, 2])."""
    return _tables(in_size, out_size, filter)[:2]


def _device_tables(in_size, out_size, name, device, transposed):
    key = (int(in_size), int(out_size), _filter(name), str(device), bool(transposed))
    hit = _DEVICE.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("resample: the tables of %d -> %d (%s) are not on the device yet; call once outside the "
                               "capture" % key[:3])
        coeffs, bounds, _ = _tables(*key[:3])
        k = torch.from_numpy(np.array(coeffs.T if transposed else coeffs, order="C"))          # a writable copy
        hit = _DEVICE.put(key, (k.to(device), torch.from_numpy(np.array(bounds)).to(device)))
    return hit


def _size2(size):
    if isinstance(size, (tuple, list)):
        oh, ow = size
        return int(oh), int(ow)
    return int(size), int(size)


def _window(window, oh, ow):
    if window is None:
        return 0, 0, oh, ow
    oy0, ox0, wh, ww = (int(v) for v in window)
    if oy0 < 0 or ox0 < 0 or wh < 1 or ww < 1 or oy0 + wh > oh or ox0 + ww > ow:
        raise ValueError("resample: window %s is not inside the %d x %d output" % ((oy0, ox0, wh, ww), oh, ow))
    return oy0, ox0, wh, ww


def _pass_host(a, axis, coeffs, bounds, first, count):
    """One separable pass along `axis` (1 = rows, 2 = columns) of int-valued a [N, H, W, C]: outputs first .. first + count."""
    k = coeffs[first:first + count].astype(np.int32)
    lo = bounds[first:first + count, 0].astype(np.int64)
    acc = np.full(a.shape[:axis] + (count,) + a.shape[axis + 1:], ROUND, np.int32)
    shape = [1, 1, 1, 1]
    shape[axis] = count
    last = a.shape[axis] - 1
    for t in range(k.shape[1]):
        if not k[:, t].any():
            continue
        idx = np.minimum(lo + t, last)           # taps past the count have k = 0
        acc += np.take(a, idx, axis=axis).astype(np.int32) * k[:, t].reshape(shape)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def to_unit_chw(u8_nhwc):
    """dataset.to_unit_tensor over a batch: uint8 [N, H, W, C] array -> float32 [N, C, H, W] tensor in [-1, 1]."""
    t = torch.from_numpy(np.ascontiguousarray(u8_nhwc)).permute(0, 3, 1, 2).to(torch.float32).div_(255.0)
    return t.sub_(0.5).div_(0.5)


def _resize_host(a, oh, ow, name, window):
    n, h, w, c = a.shape
    oy0, ox0, wh, ww = window
    if oh != h:
        kv, bv, _ = _tables(h, oh, name)
        r0 = int(bv[oy0, 0])
        r1 = int(bv[oy0 + wh - 1, 0] + bv[oy0 + wh - 1, 1])
    else:
        r0, r1 = oy0, oy0 + wh
    a = a[:, r0:r1]
    if ow != w:
        kh, bh, _ = _tables(w, ow, name)
        a = _pass_host(a, 2, kh, bh, ox0, ww)
    else:
        a = a[:, :, ox0:ox0 + ww]
    if oh != h:
        shifted = np.array(bv)
        shifted[:, 0] -= r0
        a = _pass_host(a, 1, kv, shifted, oy0, wh)
    return np.ascontiguousarray(a)


def _resize_device(x, oh, ow, name, window, form, force_mul32=False):
    n, h, w, c = x.shape
    oy0, ox0, wh, ww = window
    kh = bh = kv = bv = None
    bh_host = bv_host = None
    ksh = ksv = 0
    fits = True
    if ow != w:
        ck, cb, f24 = _tables(w, ow, name)
        kh, bh = _device_tables(w, ow, name, x.device, True)
        bh_host, ksh, fits = cb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ck.shape[1], fits and f24
    if oh != h:
        ck, cb, f24 = _tables(h, oh, name)
        kv, bv = _device_tables(h, oh, name, x.device, False)
        bv_host, ksv, fits = cb.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ck.shape[1], fits and f24
    need = _lib.lib().sr_resample_u8_scratch_bytes(n, h, w, c, oh, ow, bv_host, oy0, ox0, wh, ww)
    if need < 0:
        raise ValueError("resample: unsupported sizes %s -> %s" % ((n, h, w, c), (oh, ow)))
    scratch = torch.empty(need, dtype=torch.uint8, device=x.device) if need else None
    if form == 0:
        out = torch.empty((n, wh, ww, c), dtype=torch.uint8, device=x.device)
    else:
        out = torch.empty((n, c, wh, ww), dtype=torch.float32, device=x.device)
    native(x).sr_resample_u8(out, x, n, h, w, c, oh, ow, kh, bh, bh_host, ksh, kv, bv, bv_host, ksv, oy0, ox0, wh, ww,
                             form, 1 if fits and not force_mul32 else 0, scratch)
    return out


def resize_u8(img, size, filter="lanczos", window=None, out="u8_hwc", _force_mul32=False):
    """uint8 [N, H, W, C] or [H, W, C] (C in {1, 3, 4}) -> Pillow's resize to size = (oh, ow) (an int: square).
    window = (oy0, ox0, oh', ow') returns that part of the resized image only; neither pass computes a pixel outside
    it.  out = "u8_hwc": uint8 [.., oh', ow', C]; "f32_chw": float32 [.., C, oh', ow'] = dataset.to_unit_tensor of it.
    Arrays come back as arrays (f32_chw: a tensor), tensors as tensors on their device."""
    name = _filter(filter)
    if out not in OUT_FORMS:
        raise ValueError("resample: out must be one of %s" % ", ".join(OUT_FORMS))
    is_tensor = isinstance(img, torch.Tensor)
    if (img.dtype != torch.uint8) if is_tensor else (np.asarray(img).dtype != np.uint8):
        raise ValueError("resample: expected uint8 pixels, got %s" % (img.dtype if is_tensor else np.asarray(img).dtype))
    single = img.ndim == 3
    if img.ndim not in (3, 4) or img.shape[-1] not in (1, 3, 4):
        raise ValueError("resample: expected [N, H, W, C] or [H, W, C] with C in {1, 3, 4}, got %s" % (tuple(img.shape),))
    oh, ow = _size2(size)
    if oh < 1 or ow < 1 or 0 in img.shape:
        raise ValueError("resample: empty image or output (%s -> %s)" % (tuple(img.shape), (oh, ow)))
    win = _window(window, oh, ow)
    if is_tensor and img.device.type == "cuda":
        x = img.contiguous()
        res = _resize_device(x[None] if single else x, oh, ow, name, win, OUT_FORMS[out], _force_mul32)
        return res[0] if single else res
    a = img.numpy() if is_tensor else np.asarray(img)
    res = _resize_host(a[None] if single else a, oh, ow, name, win)
    if out == "f32_chw":
        res = to_unit_chw(res)
    elif is_tensor:
        res = torch.from_numpy(res)
    return res[0] if single else res


def center_crop_geometry(h, w, size):
    """The reference's resize_img (torchvision resize + center_crop): -> ((oh, ow), (top, left, size, size))."""
    size = int(size)
    if w <= h:
        oh, ow = int(size * h / w), size
    else:
        oh, ow = size, int(size * w / h)
    # Python's round is half-to-even, as in torchvision.transforms.functional.center_crop
    return (oh, ow), (int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0)), size, size)


def resize_center_crop(img, size, filter="lanczos", out="u8_hwc"):
    """Shorter side to `size`, longer side to int(size * long / short), then the central size x size window."""
    (oh, ow), window = center_crop_geometry(img.shape[-3], img.shape[-2], size)
    return resize_u8(img, (oh, ow), filter, window, out)


def resize_pyramid(img, sizes, filter="lanczos", out="u8_hwc"):
    """{size: resize_center_crop(img, size)}: every level is resampled from the source itself (no cascade), which a
    device tensor holds once for all of them."""
    return {int(s): resize_center_crop(img, int(s), filter, out) for s in sizes}
