"""Pillow-exact bilinear affine warp of uint8 images (C ABI sr_warp_affine_u8, csrc/warp.hip).

    warp_affine(img, matrix, size, border, fill, out)   [N, H, W, C] or [H, W, C] uint8 -> [.., oh, ow, C]
    from_index_transform(T)                             index-coordinate transform (landmarks, cv2) -> `matrix`

DEFINITION (Pillow's Image.transform(size, Image.AFFINE, a, Image.BILINEAR); float64 throughout, every product and
sum rounded on its own, left to right, no fused multiply-add).  For output pixel (x, y) and matrix a[0..6]:

    xs = x + .5, ys = y + .5;  xin = a0*xs + a1*ys + a2,  yin = a3*xs + a4*ys + a5      (the sample point)
    xf = xin - .5, x0 = floor(xf), dx = xf - x0;  likewise y
    the taps (x0, x0 + 1) x (y0, y0 + 1) are mapped into the image by the border rule
    v1 = p00 + (p01 - p00)*dx,  v2 = p10 + (p11 - p10)*dx,  v = v1 + (v2 - v1)*dy,  byte = (uint8) v, truncated

(x0 and y0 are clamped to [-2^30, 2^30] before they become integers; dx and dy are taken before the clamp.)

Border rules: `replicate` clamps the tap index; `reflect` is cv2's BORDER_REFLECT, fedcba|abcdef|fedcba, periodic (what
the reference's alignment uses); `constant` writes `fill` wherever the sample point (xin, yin) lies outside
[0, W) x [0, H) and clamps elsewhere, which for fill = 0 is Pillow's whole output.  ALL THREE RULES AGREE WHEREVER THE
SAMPLE POINT IS INSIDE THE IMAGE: there the only out-of-range taps are -1 and W (or H), and clamp and reflect send both
to the same pixel (0 and W - 1).  The tests rest on that: Pillow is the yardstick on the inside, for every rule.

The matrix maps output pixel CENTRES to source pixel centres on Pillow's grid, where pixel i covers [i, i + 1).  A
transform T between index coordinates (pixel i sits AT i: landmarks, cv2.warpAffine with WARP_INVERSE_MAP) becomes
from_index_transform(T) = [A | t + .5 - A (.5, .5)].

A numpy array (or a CPU tensor) takes the host path below, which is the definition; a device tensor the kernel: one
launch for the whole batch, nothing allocated but the output, no synchronisation, so it records into a captured graph
when `matrix` is already a device tensor (a host matrix is uploaded first, which a capture does not allow).  There is
no fallback between the two paths.
"""
import numpy as np
import torch

from ._dispatch import native
from .resample import OUT_FORMS, _size2, to_unit_chw

BORDERS = {"replicate": 0, "reflect": 1, "constant": 2}
LIMIT = float(1 << 30)


def from_index_transform(T):
    """2x3 or 3x3 T (last row 0 0 1) taking OUTPUT index coordinates to SOURCE index coordinates -> float64 [6]."""
    T = np.asarray(T, np.float64)
    if T.shape == (3, 3):
        if not np.array_equal(T[2], [0.0, 0.0, 1.0]):
            raise ValueError("warp: the last row of a 3x3 transform must be 0 0 1, got %s" % (T[2],))
        T = T[:2]
    if T.shape != (2, 3):
        raise ValueError("warp: expected a 2x3 or 3x3 transform, got shape %s" % (T.shape,))
    A, t = T[:, :2], T[:, 2]
    shift = t + 0.5 - A.dot(np.array([0.5, 0.5]))
    return np.array([A[0, 0], A[0, 1], shift[0], A[1, 0], A[1, 1], shift[1]], np.float64)


def _border_index(i, size, border):
    if border == 1:
        m = np.mod(i, 2 * size)
        return np.where(m < size, m, 2 * size - 1 - m)
    return np.clip(i, 0, size - 1)


def _warp_one(a, m, oh, ow, border, fill):
    h, w, c = a.shape
    xs = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    ys = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    xf, yf = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xf), np.floor(yf)
    dx, dy = (xf - x0)[:, :, None], (yf - y0)[:, :, None]
    x0 = np.clip(x0, -LIMIT, LIMIT).astype(np.int64)
    y0 = np.clip(y0, -LIMIT, LIMIT).astype(np.int64)
    cx0, cx1 = _border_index(x0, w, border), _border_index(x0 + 1, w, border)
    cy0, cy1 = _border_index(y0, h, border), _border_index(y0 + 1, h, border)
    f = a.astype(np.float64)
    p00, p01, p10, p11 = f[cy0, cx0], f[cy0, cx1], f[cy1, cx0], f[cy1, cx1]
    v1 = p00 + (p01 - p00) * dx
    v2 = p10 + (p11 - p10) * dx
    out = (v1 + (v2 - v1) * dy).astype(np.uint8)
    if border == 2:
        inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
        out[~inside] = fill
    return out


def _warp_host(a, mats, oh, ow, border, fill):
    out = np.empty((a.shape[0], oh, ow, a.shape[3]), np.uint8)
    for i in range(a.shape[0]):
        out[i] = _warp_one(a[i], mats[i if mats.shape[0] > 1 else 0], oh, ow, border, fill)
    return out


def _warp_device(x, mats, oh, ow, border, fill, form):
    n, h, w, c = x.shape
    if form == 0:
        out = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=x.device)
    else:
        out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    native(x).sr_warp_affine_u8(out, x, mats, 6 if mats.shape[0] > 1 else 0, n, h, w, c, oh, ow, border, fill, form)
    return out


def _matrices(matrix, n, device):
    """-> float64 [1, 6] or [n, 6]: an array on the host path (device None), else a tensor on `device`."""
    if isinstance(matrix, torch.Tensor):
        if matrix.dtype != torch.float64:
            raise ValueError("warp: the matrix must be float64, got %s" % matrix.dtype)
        shape = tuple(matrix.shape)
    else:
        matrix = np.asarray(matrix, np.float64)
        shape = matrix.shape
    if shape != (6,) and shape != (n, 6):
        raise ValueError("warp: expected a matrix of shape [6] or [%d, 6], got %s" % (n, shape))
    if device is None:
        m = matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else matrix
        m = m.reshape(-1, 6)
        if not np.isfinite(m).all():
            raise ValueError("warp: the matrix has entries that are not finite")
        return m
    if isinstance(matrix, torch.Tensor):
        if matrix.device != device:
            raise ValueError("warp: the matrix is on %s, the image on %s" % (matrix.device, device))
        return matrix.contiguous().reshape(-1, 6)
    if not np.isfinite(matrix).all():
        raise ValueError("warp: the matrix has entries that are not finite")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("warp: a host matrix cannot be uploaded during a capture; pass a float64 device tensor")
    return torch.from_numpy(np.ascontiguousarray(matrix.reshape(-1, 6))).to(device)


def warp_affine(img, matrix, size, border="reflect", fill=0, out="u8_hwc"):
    """uint8 [N, H, W, C] or [H, W, C] (C in {1, 3, 4}; four channels are plain channels) -> the image of size =
    (oh, ow) (an int: square) whose pixel (x, y) is the bilinear sample of `img` at matrix * (x + .5, y + .5, 1), see the
    module docstring.  matrix: float64 [6], or [N, 6] with one matrix per image (an array, or a tensor on img's device).
    border: "reflect" | "replicate" | "constant" (with `fill`, 0 .. 255, for every channel); the three agree wherever
    the sample point lies inside the image.  out = "u8_hwc": uint8 [.., oh, ow, C]; "f32_chw": float32 [.., C, oh, ow],
    bit-equal to resample.to_unit_chw of the former.  Arrays come back as arrays (f32_chw: a tensor), tensors as tensors
    on their device."""
    if border not in BORDERS:
        raise ValueError("warp: border must be one of %s, got %r" % (", ".join(BORDERS), border))
    if out not in OUT_FORMS:
        raise ValueError("warp: out must be one of %s" % ", ".join(OUT_FORMS))
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("warp: fill must be a byte, got %d" % fill)
    is_tensor = isinstance(img, torch.Tensor)
    if not is_tensor:
        img = np.asarray(img)
    if img.dtype != (torch.uint8 if is_tensor else np.uint8):
        raise ValueError("warp: expected uint8 pixels, got %s" % img.dtype)
    single = img.ndim == 3
    if img.ndim not in (3, 4) or img.shape[-1] not in (1, 3, 4):
        raise ValueError("warp: expected [N, H, W, C] or [H, W, C] with C in {1, 3, 4}, got %s" % (tuple(img.shape),))
    oh, ow = _size2(size)
    if oh < 1 or ow < 1 or 0 in img.shape:
        raise ValueError("warp: empty image or output (%s -> %s)" % (tuple(img.shape), (oh, ow)))
    n = 1 if single else img.shape[0]
    if is_tensor and img.device.type == "cuda":
        x = img.contiguous()
        res = _warp_device(x[None] if single else x, _matrices(matrix, n, x.device), oh, ow, BORDERS[border], fill,
                           OUT_FORMS[out])
        return res[0] if single else res
    a = img.numpy() if is_tensor else img
    res = _warp_host(a[None] if single else a, _matrices(matrix, n, None), oh, ow, BORDERS[border], fill)
    if out == "f32_chw":
        res = to_unit_chw(res)
    elif is_tensor:
        res = torch.from_numpy(res)
    return res[0] if single else res
