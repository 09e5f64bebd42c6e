"""Region-weighted image loss of face reconstruction: fit only the face (csrc/region.hip).

The region is a {0, 1} picture built once per photograph — the filled landmark polygon of the reference's
SkinSegmentationGrabcut.segment without `refine` (reference utils_face.py:250-258: the landmarks' triangulation if one is
given, else their convex hull, after astype(int32)), optionally grown or shrunk by a square window — or any [0, 1] mask of
the caller's; per step it can be gated by the mesh's coverage, (n . n over the normal map's channels) > 1e-3 (reference
train.py:318).  The loss then runs on

    y = target + m_eff * (img - target)

instead of img (`region_blend`): outside the region the loss sees the target itself.

Definitions (the host versions serve CPU tensors and float64 and are what the kernels are tested against):

  hull_triangles(points_int)           convex hull of integer points by a monotone chain (exact), as a triangle fan
  fill_triangles(points, tris, size)   the closed integer polygon: points truncated toward zero; pixel (x, y) is set iff
                                       for some triangle (a, b, c) min <= x <= max and min <= y <= max of its corners and
                                       cross(b - a, p - a), cross(c - b, p - b), cross(a - c, p - c) (int64) are all >= 0
                                       or all <= 0.  Either winding; a degenerate triangle is its segment or point.
                                       This is the project's definition: cv2.fillPoly is not available to compare with and
                                       can differ from it on boundary pixels only (unverified).
  grow(mask_u8, r)                     r > 0: set iff a pixel of the picture within Chebyshev distance r is set; r < 0: set
                                       iff every pixel of the picture within |r| is set (the border does not erode: cv2's
                                       default for a rectangular erode); |r| <= 32
  landmark_region(...)                 hull or triangulation of each sample's landmarks with conf > 0, then grow(margin)
  region_blend(img, target, mask, normal_map, thresh) -> (y, m_eff)

Device tensors: sr_region_fill / sr_region_grow (uint8, byte-equal to the host) and, per step, sr_region_blend_fwd /
sr_region_blend_bwd on float32 (one launch each way, the host composite's bits, capturable).  The gradient reaches img only,
g_img = m_eff * g_y; m_eff is a detached constant.
"""
import numpy as np
import torch
from torch.autograd import Function

from ._dispatch import host_array, is_device_tensor, native

LIMIT = 1 << 20                 # |coordinate| of a point, and H, W
MAX_GROW = 32


def _hw(size):
    if isinstance(size, (tuple, list)):
        return int(size[0]), int(size[1])
    return int(size), int(size)


# ---- convex hull -----------------------------------------------------------------------------------------------------
def hull_triangles(points_int):
    """int32 [T, 3]: the convex hull of integer points [P, 2] as a triangle fan of indices into them (host only; Andrew's
    monotone chain on Python integers: exact).  Fewer than three distinct points, or all points on one line, give one
    degenerate triangle (i, j, j) that covers the segment between the two extreme points (i == j: the point)."""
    raw = host_array(points_int)
    if raw.ndim != 2 or raw.shape[1] != 2 or raw.shape[0] < 1:
        raise ValueError("hull_triangles: points must be [P, 2] with P >= 1, got %s" % (tuple(raw.shape),))
    if not np.all(np.round(raw) == raw):
        raise ValueError("hull_triangles: points hold whole numbers (fill_triangles truncates, this does not)")
    pts = [(int(x), int(y)) for x, y in raw]
    order = sorted(range(len(pts)), key=lambda i: (pts[i], i))
    uniq = [i for k, i in enumerate(order) if k == 0 or pts[i] != pts[order[k - 1]]]      # first index of every point

    def cross(o, a, b):
        return ((pts[a][0] - pts[o][0]) * (pts[b][1] - pts[o][1]) - (pts[a][1] - pts[o][1]) * (pts[b][0] - pts[o][0]))

    def chain(seq):
        out = []
        for i in seq:
            while len(out) >= 2 and cross(out[-2], out[-1], i) <= 0:
                out.pop()
            out.append(i)
        return out

    lower, upper = chain(uniq), chain(uniq[::-1])
    hull = lower[:-1] + upper[:-1]
    if len(hull) < 3:                                                       # one point, or all on a line
        return torch.tensor([[uniq[0], uniq[-1], uniq[-1]]], dtype=torch.int32)
    return torch.tensor([[hull[0], hull[k], hull[k + 1]] for k in range(1, len(hull) - 1)], dtype=torch.int32)


# ---- fill ------------------------------------------------------------------------------------------------------------
def _int_points(points):
    """points [B, P, 2] of any number type, truncated toward zero, as an int32 tensor on their device (or the host)."""
    p = points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
    p = p.detach()
    if p.dim() != 3 or p.shape[2] != 2 or p.shape[1] < 1:
        raise ValueError("fill_triangles: points must be [B, P, 2] with P >= 1, got %s" % (tuple(p.shape),))
    if p.is_floating_point():
        if not bool(torch.isfinite(p).all()):
            raise ValueError("fill_triangles: a point is not finite")
        p = p.trunc()
    if p.numel() and float(p.abs().max()) > LIMIT:
        raise ValueError("fill_triangles: a point lies beyond +-2^20")
    return p.to(torch.int32).contiguous()


def _int_tris(tris, b, n_p):
    t = tris if isinstance(tris, torch.Tensor) else torch.as_tensor(np.asarray(tris))
    t = t.detach()
    if t.is_floating_point():
        raise ValueError("fill_triangles: tris hold indices")
    if t.dim() not in (2, 3) or t.shape[-1] != 3 or (t.dim() == 3 and t.shape[0] != b):
        raise ValueError("fill_triangles: tris must be [T, 3] or [B, T, 3] for B = %d, got %s" % (b, tuple(t.shape)))
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n_p):
        raise ValueError("fill_triangles: a triangle names a point outside [0, %d)" % n_p)
    return t.to(torch.int32).contiguous()


def fill_triangles_host(pi, ti, size):
    """The definition on integer arrays: pi int [B, P, 2], ti int [T, 3] or [B, T, 3] -> uint8 numpy [B, 1, H, W]."""
    h, w = size
    pi, ti = np.asarray(pi, np.int64), np.asarray(ti, np.int64)
    b = pi.shape[0]
    out = np.zeros((b, 1, h, w), np.uint8)
    for s in range(b):
        tri = pi[s][ti if ti.ndim == 2 else ti[s]]                           # [T, 3, 2]
        for (ax, ay), (bx, by), (cx, cy) in tri:
            x0, x1 = max(min(ax, bx, cx), 0), min(max(ax, bx, cx), w - 1)
            y0, y1 = max(min(ay, by, cy), 0), min(max(ay, by, cy), h - 1)
            if x0 > x1 or y0 > y1:
                continue
            x = np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
            y = np.arange(y0, y1 + 1, dtype=np.int64)[:, None]
            e0 = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
            e1 = (cx - bx) * (y - by) - (cy - by) * (x - bx)
            e2 = (ax - cx) * (y - cy) - (ay - cy) * (x - cx)
            inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
            out[s, 0, y0:y1 + 1, x0:x1 + 1] |= inside.astype(np.uint8)
    return out


def fill_triangles(points, tris, size_hw):
    """uint8 [B, 1, H, W]: 1 inside the closed integer triangles `tris` ([T, 3] shared, or [B, T, 3]; indices into each
    sample's points) of points [B, P, 2] (x, y; truncated toward zero), else 0.  Vertices may lie outside the picture.
    Device points run sr_region_fill (one launch), everything else the host definition; the bytes are the same."""
    h, w = _hw(size_hw)
    if not (1 <= h <= LIMIT and 1 <= w <= LIMIT):
        raise ValueError("fill_triangles: size (%d, %d) outside [1, 2^20]" % (h, w))
    pi = _int_points(points)
    b, n_p = int(pi.shape[0]), int(pi.shape[1])
    ti = _int_tris(tris, b, n_p)
    if not is_device_tensor(pi):
        return torch.from_numpy(fill_triangles_host(pi.numpy(), ti.cpu().numpy(), (h, w)))
    ti = ti.to(pi.device)
    n_t = int(ti.shape[-2])
    out = torch.empty((b, 1, h, w), dtype=torch.uint8, device=pi.device)
    native(pi).sr_region_fill(out, pi, ti, 3 * n_t if ti.dim() == 3 else 0, b, n_p, n_t, h, w)
    return out


# ---- grow ------------------------------------------------------------------------------------------------------------
def grow_host(mask, r):
    """The definition on a uint8 numpy array [..., H, W]."""
    m = np.asarray(mask) != 0
    h, w = m.shape[-2:]
    a = abs(int(r))
    want = r > 0
    # dilation looks for a set pixel, erosion for a clear one; what lies outside the picture counts for neither
    hit = np.zeros(m.shape, bool)
    look = m if want else ~m
    for dy in range(-a, a + 1):
        for dx in range(-a, a + 1):
            ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
            xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
            if ys.start < ys.stop and xs.start < xs.stop:
                hit[..., yd, xd] |= look[..., ys, xs]
    return (hit if want else ~hit).astype(np.uint8)


def grow(mask_u8, r):
    """Dilates (r > 0) or erodes (r < 0) a uint8 mask [..., H, W] by the square window of Chebyshev radius |r| <= 32,
    clipped to the picture; r = 0 returns the mask.  A device tensor runs sr_region_grow (one launch, the direct window:
    this happens once per picture)."""
    r = int(r)
    if abs(r) > MAX_GROW:
        raise ValueError("grow: |r| <= %d, got %d" % (MAX_GROW, r))
    m = mask_u8 if isinstance(mask_u8, torch.Tensor) else torch.as_tensor(np.asarray(mask_u8))
    if m.dtype != torch.uint8 or m.dim() < 2:
        raise ValueError("grow: a uint8 mask [..., H, W], got %s %s" % (m.dtype, tuple(m.shape)))
    if r == 0 or m.numel() == 0:
        return m
    if not is_device_tensor(m):
        return torch.from_numpy(grow_host(m.numpy(), r))
    m = (m != 0).to(torch.uint8).contiguous()
    h, w = int(m.shape[-2]), int(m.shape[-1])
    out = torch.empty_like(m)
    native(m).sr_region_grow(out, m, m.numel() // (h * w), h, w, r)
    return out


# ---- the landmark polygon --------------------------------------------------------------------------------------------
def landmark_region(lmk, conf, size_hw, tris=None, margin=0, device=None):
    """float32 [B, 1, H, W] in {0, 1}: for every sample the filled hull of its landmarks lmk [B, L, 2] (pixel index
    coordinates, x then y) with conf [B, L] > 0 (None: all), or the filled triangulation tris [T, 3] over landmark numbers
    without the triangles that touch a missing landmark; then grow(margin).  A sample with no landmark at all gets all
    ones: a picture the landmark file does not list is fitted as without a region.  The hulls are built on the host; the
    fill and the window run on `device` (default: lmk's)."""
    h, w = _hw(size_hw)
    dev = torch.device(device) if device is not None else (lmk.device if isinstance(lmk, torch.Tensor)
                                                            else torch.device("cpu"))
    pts = host_array(lmk).astype(np.float64)
    if pts.ndim != 3 or pts.shape[2] != 2:
        raise ValueError("landmark_region: lmk must be [B, L, 2], got %s" % (tuple(pts.shape),))
    b, n_l = pts.shape[:2]
    on = np.ones((b, n_l), bool) if conf is None else host_array(conf).reshape(b, -1) > 0
    if on.shape != (b, n_l):
        raise ValueError("landmark_region: conf must be [B, L]")
    pts = np.where(on[:, :, None], pts, 0.0)                                # a missing landmark may hold anything
    if not np.isfinite(pts).all() or np.abs(pts).max(initial=0.0) > LIMIT:
        raise ValueError("landmark_region: a landmark is not finite or lies beyond +-2^20")
    pi = np.trunc(pts).astype(np.int64)
    if tris is not None:
        tl = host_array(tris).astype(np.int64).reshape(-1, 3)
        if tl.size and (tl.min() < 0 or tl.max() >= n_l):
            raise ValueError("landmark_region: the triangulation names a landmark outside [0, %d)" % n_l)
    lists, empty = [], np.zeros(b, bool)
    for s in range(b):
        if not on[s].any():
            empty[s] = True
            lists.append(np.zeros((0, 3), np.int64))
        elif tris is None:
            live = np.nonzero(on[s])[0]
            lists.append(live[hull_triangles(pi[s, live]).numpy().astype(np.int64)])
        else:
            lists.append(tl[on[s][tl].all(1)])
    # padded to a common T by repeating the last triangle; a sample without triangles gets the empty triangle list's
    # stand-in (0, 0, 0) and is overwritten below (no landmark) or cleared (a triangulation all of whose triangles drop)
    n_t = max(1, max(len(t) for t in lists))
    none = np.array([len(t) == 0 for t in lists])
    padded = np.stack([np.concatenate((t, np.repeat(t[-1:] if len(t) else np.zeros((1, 3), np.int64), n_t - len(t), 0)))
                       for t in lists])
    mask = fill_triangles(torch.from_numpy(pi).to(dev), torch.from_numpy(padded).to(dev), (h, w))
    if none.any():
        mask[torch.from_numpy(none).to(dev)] = 0
    mask = grow(mask, margin)
    if empty.any():
        mask[torch.from_numpy(empty).to(dev)] = 1
    return mask.to(torch.float32)


# ---- the blend -------------------------------------------------------------------------------------------------------
def effective_mask(mask, normal_map=None, thresh=1e-3):
    """m_eff [B, 1, H, W]: mask, gated by the mesh's coverage (n . n over the 3 channels) > thresh with a normal map
    (logically [B, 3, H, W], any strides)."""
    m = mask.detach()
    if normal_map is None:
        return m
    n = normal_map.detach().to(m.dtype)
    d = n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]
    return m * (d > thresh).to(m.dtype).unsqueeze(1)


def region_blend_composite(img, target, mask, normal_map=None, thresh=1e-3):
    """The defining tensor algebra: (y, m_eff), y = target + m_eff * (img - target).  target and m_eff are constants."""
    m = effective_mask(mask.to(img.dtype), normal_map, thresh)
    t = target.detach()
    return t + m * (img - t), m


def _check_blend(img, target, mask, normal_map):
    if img.dim() != 4 or tuple(target.shape) != tuple(img.shape):
        raise ValueError("region_blend: img and target must both be [B, C, H, W], got %s and %s"
                         % (tuple(img.shape), tuple(target.shape)))
    b, _, h, w = img.shape
    if tuple(mask.shape) != (b, 1, h, w):
        raise ValueError("region_blend: mask must be [B, 1, H, W] = %s, got %s" % ((b, 1, h, w), tuple(mask.shape)))
    if normal_map is not None and tuple(normal_map.shape) != (b, 3, h, w):
        raise ValueError("region_blend: normal_map must be (a view of shape) [B, 3, H, W] = %s, got %s"
                         % ((b, 3, h, w), tuple(normal_map.shape)))


def blend_forward(img, target, mask, normal_map=None, thresh=1e-3):
    """(y, m_eff) by sr_region_blend_fwd (device fp32, no autograd)."""
    x, t, m = img.contiguous(), target.contiguous(), mask.contiguous()
    b, c, h, w = x.shape
    y = torch.empty_like(x)
    m_eff = torch.empty_like(m)
    ns = (0, 0, 0, 0) if normal_map is None else tuple(int(s) for s in normal_map.stride())
    native(x).sr_region_blend_fwd(y, m_eff, x, t, m, normal_map, ns[0], ns[1], ns[2],
                                  ns[3], float(thresh), b, c, h, w)
    return y, m_eff


def blend_backward(g_y, m_eff):
    """g_img = m_eff * g_y by sr_region_blend_bwd (device fp32)."""
    g = g_y.contiguous()
    b, c, h, w = g.shape
    out = torch.empty_like(g)
    native(g).sr_region_blend_bwd(out, g, m_eff, b, c, h, w)
    return out


class _RegionBlend(Function):
    @staticmethod
    def forward(ctx, img, target, mask, normal_map, thresh):
        y, m_eff = blend_forward(img, target, mask, normal_map, thresh)
        ctx.save_for_backward(m_eff)
        ctx.mark_non_differentiable(m_eff)
        ctx.set_materialize_grads(False)
        return y, m_eff

    @staticmethod
    def backward(ctx, g_y, _gm):
        if g_y is None:
            return (None,) * 5
        (m_eff,) = ctx.saved_tensors
        if torch.is_grad_enabled():
            return (m_eff * g_y,) + (None,) * 4           # a recorded backward (create_graph=True): stays differentiable
        return (blend_backward(g_y, m_eff),) + (None,) * 4


def native_ok(img, target, mask, normal_map):
    """The kernels take device fp32 (the normal map through its strides: any view)."""
    ts = (img, target, mask) + (() if normal_map is None else (normal_map,))
    return all(is_device_tensor(t) and t.dtype == torch.float32 for t in ts)


def region_blend(img, target, mask, normal_map=None, thresh=1e-3):
    """(y, m_eff): y [B, C, H, W] = target + m_eff * (img - target) with m_eff [B, 1, H, W] = mask (float in [0, 1], soft
    values allowed), times ((n . n over the 3 channels) > thresh) with a normal map (logically [B, 3, H, W]; read through
    its strides, so the rasterizer's permuted view is not copied).  The gradient reaches img only: g_img = m_eff * g_y;
    m_eff is a detached constant.  Device fp32 tensors take one launch each way; CPU tensors, float64 and second order take
    the composite."""
    _check_blend(img, target, mask, normal_map)
    if native_ok(img, target, mask, normal_map):
        return _RegionBlend.apply(img, target.detach(), mask.detach(),
                                  None if normal_map is None else normal_map.detach(), float(thresh))
    return region_blend_composite(img, target, mask, normal_map, thresh)
