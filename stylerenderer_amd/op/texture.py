"""UV texture baking of face reconstruction: the picture's colours carried onto the fitted surface (csrc/texture.hip), and
the way back: the textured surface drawn into a picture (csrc/texture_sample.hip).

A layout gives the mesh texture coordinates: uv [nt, 2] in [0, 1] with v pointing up and tri_uv [nf, 3], row-parallel to
the mesh's tri (face_model.uv_layout computes one, face_model.load_uv reads one).  Texel (ty, tx) of a (Th, Tw) texture
has its centre at u = (tx + 1/2) / Tw, v = 1 - (ty + 1/2) / Th: row 0 is the top of the image, as OBJ viewers expect.

  texel_map   (face int32 [Th, Tw], coeff float32 [Th, Tw, 3]): the face under every texel centre (-1: none) and its
              barycentric weights, drawn by op.rasterize's forward (no second rasterizer) and cached per layout and size.
  bake        (tex [B, C, Th, Tw], weight [B, 1, Th, Tw]).  For sample b and a texel with f = face >= 0, every step one
              operation of the tensors' float type, in this order:
                  P  = (c0 v[i0] + c1 v[i1]) + c2 v[i2]         i_k = tri[f, k];  N likewise from n
                  m  = N.z / max(|N|, 1e-12)                    |N| = sqrt((N.x^2 + N.y^2) + N.z^2)
                  g  = smoothstep(clamp((m - lo) / (hi - lo), 0, 1))     hi == lo: a step at m > lo (op.landmark's gate)
                  q  = project(P, (Hz, Wz));  ix = floor(q.x + 1/2), iy = floor(q.y + 1/2)
                  vis = 0 <= ix < Wz and 0 <= iy < Hz and P.z >= zbuf[b, iy, ix] - z_bias
                  s  = project(P, (Hs, Ws));  inside = -1/2 <= s.x <= Ws - 1/2 and -1/2 <= s.y <= Hs - 1/2
                  x0 = floor(s.x), fx = s.x - x0, likewise y;  indices clamped to the picture (replicate)
                  colour = ((1 - fx) I[y0, x0] + fx I[y0, x1]) (1 - fy) + ((1 - fx) I[y1, x0] + fx I[y1, x1]) fy
                  weight = g where vis and inside, else 0;   tex = colour where weight > 0, else 0
              project is op.landmark's, the picture's pixel convention.  The rasterizer keeps the greater z; an empty
              z-buffer pixel holds -FLT_MAX and occludes nothing.  An empty texel gives tex = 0 and weight = 0.
  pad         texture padding, so that a renderer's bilinear filter does not bleed black across chart borders.
  fill_mean   what is still unfilled gets the sample's weight-weighted mean colour.
  merge       (tex [1, C, Th, Tw], weight [1, 1, Th, Tw], best uint8 [Th, Tw]) of V bakes of one subject in one layout
              (tex [V, C, Th, Tw], weight [V, 1, Th, Tw]: several views of one head).  Per texel, every step one operation
              of the float type, no fused multiply-add:
                  wmax = max_v w_v;  best = the first v that attains it;  wmax <= 0: colour 0, weight 0, best = 255
                  r_v  = w_v / wmax, correctly rounded; then `sharpness` times r_v = r_v r_v.  After the division and
                         after every squaring a value below 2^-63 becomes 0, so that no operand or result is subnormal
                         whatever the float mode of host or device
                  den  = ((r_0 + r_1) + ...) and num_c = ((r_0 t_0c + r_1 t_1c) + ...) over the views in order, both
                         from 0, the product and the sum rounded separately.  A view with r_v = 0 is skipped, not
                         multiplied: whatever stands in an unweighted texel (NaN included) cannot leak
                  tex_c = num_c / den, correctly rounded;  weight = wmax
              sharpness 0 is the weight-weighted mean; every step up squares the ratios, so the best view takes over
              and a seam between two views narrows; with weights (1, 2^-4) sharpness 4 gives the first view exactly.
              Weights are expected finite and not negative (a negative one counts as 0).

  uv_map      (uvmap [B, H, W, 2], cover bool [B, H, W]): the layout's coordinates of the surface point under every pixel
              of the posed mesh, drawn by the `rasterize` Function over the mesh with its corners exploded (a seam gives a
              vertex two uvs; a face keeps its own), so the gradient to the mesh is the rasterizer's.
  sample      out [B, C, H, W]: the bilinear look-up of a texture T [Bt, C, Th, Tw], Bt = B or 1 (one texture under all
              views), at a uv map.  For a pixel with cover true and finite (u, v), every step one operation of the float
              type, no fused multiply-add:
                  sx = u Tw - 1/2;  sy = (1 - v) Th - 1/2
                  inx = -1 <= sx <= Tw, sxc = clamp(sx, -1, Tw);  likewise iny, syc
                  x0 = floor(sxc), fx = sxc - x0;  xa = clamp(x0, 0, Tw - 1), xb = clamp(x0 + 1, 0, Tw - 1);  likewise y
                  top = (1 - fx) T[ya, xa] + fx T[ya, xb];  bot = (1 - fx) T[yb, xa] + fx T[yb, xb]
                  out_c = top (1 - fy) + bot fy
              Any other pixel gets `background` and contributes to no gradient.  Backward, g the incoming gradient:
                  gx = sum over c from 0 in channel order of g_c ((T[ya, xb] - T[ya, xa]) (1 - fy) + (T[yb, xb] - T[yb, xa]) fy)
                  gy = likewise of g_c (bot - top);  grad_u = inx ? gx Tw : 0;  grad_v = iny ? -(gy Th) : 0
                  grad_T[bt, c, ty, tx] = the sum from 0, in ascending (b, y, x, k) order, over the taps on that texel, of
                         w_k g_c;  k = 0..3: (ya, xa), (ya, xb), (yb, xa), (yb, xb);  w = (1 - fx)(1 - fy), fx (1 - fy),
                         (1 - fx) fy, fx fy, one product each.  Two taps of a pixel that clamp onto one texel are added
                         separately; a texel no tap reaches gets exactly 0; with Bt = 1 the sum runs over all B views.
              The texture's gradient is a gather over a tap list (`tap_plan`), not a scatter: no atomics, one order.
  render      `uv_map` followed by `sample` (or, with mip = a bias, by `sample_mip`).
  TapPlanner  the tap list built by the device in a fixed launch sequence (csrc/tap_plan.hip: a radix sort, the integers
              of `tap_plan`), for a uv map that moves in every step of a captured fit: `sample(..., planner=p)`.
  explode     c[b, 3 f + k] = v[b, tri[f, k]], the corners `uv_map` draws, with an adjoint that is an ordered sum over
              the topology's incidence list (csrc/explode.hip: one launch): `uv_map(..., explode=True)` (DESIGN.md 7k''').

  The mip-mapped look-up (csrc/texture_mip.hip), for a texture drawn smaller than it is (DESIGN.md 7k''):
  mip_layout  ((offset, h, w), ...) of the levels of a (Th, Tw) texture: level 0 is the texture, level l + 1 has half of
              each side and exists while both sides of level l are even, so every level's texel grid is nested exactly in
              the one below (no odd-size filter, no uv shift).  The pyramid is packed [Bt, C, P], P = sum h_l w_l.
  mip_build   pyr from tex: level 0 a copy, p_{l+1}[y, x] = ((p_l[2y, 2x] + p_l[2y, 2x+1]) + (p_l[2y+1, 2x] +
              p_l[2y+1, 2x+1])) 0.25.  Backward per level-0 texel, a gather: t = g_{L-1}[y >> (L-1), x >> (L-1)], then
              t = g_l[y >> l, x >> l] + 0.25 t for l = L-2 .. 0, grad_tex[y, x] = t.
  mip_lod     lod [B, H, W], a constant of the look-up (no gradient).  Along x, over the neighbours n = (y, x + 1) and
              (y, x - 1) that lie inside the picture and are live:  du = (u_n - u) Tw, dv = (v_n - v) Th,
              d = du du + dv dv;  qx = the minimum of d (0 with no usable neighbour), qy likewise along y;
              q = max(qx, qy), rho = sqrt(q) rounded once;  l = the largest integer in [0, L-1] with 2^l <= rho;
              lambda = 0 for rho < 1, L-1 for l = L-1, else l + (rho 2^-l - 1);  lod = clamp(lambda + bias, 0, L-1).
              The minimum over the two sides keeps a chart seam, which runs between two pixels, from forcing the
              coarsest level: one side of a pixel usually lies in its own chart.  No log2: it is not reproducible
              between host and device; the piecewise-linear fraction stays within 0.09 levels of it.
  mip_sample  out [B, C, H, W] from pyr, a uv map and a lod.  lod is clamped to [0, L-1] (NaN counts as 0);
              l0 = floor(lod), l1 = min(l0 + 1, L-1), f = lod - l0;  c_l = `sample`'s definition on level l with
              (Th_l, Tw_l);  out = c_l0 where f == 0 (level l1 is then neither read nor given a gradient), else
              (1 - f) c_l0 + f c_l1.  grad_uv = guv_l0 where f == 0, else (1 - f) guv_l0 + f guv_l1, guv_l `sample`'s
              formula on level l.  grad_pyr is the ordered sum over the 8-tap list of `mip_tap_plan`: k = 0..3 the
              taps of l0 with the weights (1 - f) w_k, k = 4..7 those of l1 with f w_{k-4}.  lod == 0 everywhere is
              `sample` bit for bit, forward and both gradients.
  sample_mip  `mip_build`, `mip_lod` (unless a lod is given) and `mip_sample` in a row.

CPU tensors and float64 take the torch composites `bake_composite`, `pad_host`, `merge_composite` and `sample_composite`,
which are the definition.  Float32 device tensors take sr_texture_bake / sr_texture_pad / sr_texture_merge through the C ABI: one launch
per bake, per padding pass and per merge, nothing allocated by the launch and nothing read back, so the calls can be
captured.  The kernels are compiled without contraction and with correctly rounded division and square root: weight, tex,
the padding and the merge are the host float32 definition's bit for bit.  Under SR_STRICT_NATIVE=1 nothing falls to a
library: a device tensor the kernels do not take (float64) raises.

Non-square sizes.  op.rasterize reproduces the reference's call convention, which swaps the two extents of a non-square
picture: only square pictures come out right.  `texel_map` and `depth_buffer` therefore draw a non-square
(H, W) inside a square of side max(H, W), with the vertices scaled so that pixel (y, x) of the top left H x W block is
the pixel `project(., (H, W))` means, and crop.  For a square size the vertices are the plain (2u - 1, 2v - 1, 0).

z_bias defaults to 4 / max(Hz, Wz); like the command line's facing = (0.1, 0.4) it is a starting value, not tuned on any
trained checkpoint.
"""
import numpy as np
import torch

from ._dispatch import DerivedCache, is_device_tensor, native, strict_native
from .landmark import _hw, project
from .rasterize import forward as _raster_forward, forward_with_depth as _raster_depth

TINY = 1e-12
MAX_PASSES = 64


# ---- the texel map ---------------------------------------------------------------------------------------------------
_MAP_CACHE = DerivedCache(8)


def _square_vertices(x, y, size):
    """Model coordinates (x, y in [-1, 1], y up) of an (H, W) picture -> the same points in the square picture of side
    S = max(H, W) whose top left H x W block is that picture; the identity for a square size."""
    h, w = size
    s = max(h, w)
    if h == w:
        return x, y
    return (1 + x) * (w / s) - 1, 1 - (1 - y) * (h / s)


def texel_map(uv, tri_uv, size, keep=None):
    """(face int32 [Th, Tw], coeff float32 [Th, Tw, 3]) of the layout uv [nt, 2], tri_uv [nf, 3] at size = T or (Th, Tw),
    on uv's device.  face is the face whose uv triangle covers the texel's centre, -1 where there is none (all three
    coefficients 0: the rasterizer's convention for an uncovered pixel); coeff[..., k] belongs to corner k of that face.
    Drawn are the faces with keep[f] true (default: all) and a non-zero uv area; where faces overlap in uv, the one drawn
    first (the lowest face number) wins.  The rasterizer culls one winding, so a face with the culled sign is drawn with
    corners 1 and 2 swapped and its two coefficients are swapped back.  Cached per layout tensors and size."""
    th, tw = _hw(size)
    if th < 1 or tw < 1:
        raise ValueError("texel_map: size must be positive, got (%d, %d)" % (th, tw))
    if uv.dim() != 2 or uv.shape[1] != 2 or tri_uv.dim() != 2 or tri_uv.shape[1] != 3:
        raise ValueError("texel_map: uv [nt, 2] and tri_uv [nf, 3], got %s and %s" % (tuple(uv.shape), tuple(tri_uv.shape)))
    key = (uv.data_ptr(), tri_uv.data_ptr(), tuple(uv.shape), tuple(tri_uv.shape), uv._version, tri_uv._version,
           str(uv.device), str(tri_uv.device), uv.dtype, th, tw,
           None if keep is None else (keep.data_ptr(), keep._version, str(keep.device)))
    hit = _MAP_CACHE.get(key)
    if hit is not None:
        return hit[0], hit[1]
    dev = uv.device
    uvh = uv.detach().cpu().numpy().astype(np.float32)
    th_ = tri_uv.detach().cpu().numpy().astype(np.int64)
    nf, nt = th_.shape[0], uvh.shape[0]
    if th_.size and (th_.min() < 0 or th_.max() >= nt):
        raise ValueError("texel_map: texture coordinate index out of range [0, %d)" % nt)
    if uvh.size and not (np.isfinite(uvh).all() and uvh.min() >= 0 and uvh.max() <= 1):
        raise ValueError("texel_map: uv must lie in [0, 1]")
    kh = np.ones(nf, bool) if keep is None else keep.detach().cpu().numpy().astype(bool).reshape(-1)
    if kh.shape[0] != nf:
        raise ValueError("texel_map: keep must have one entry per face (%d), got %d" % (nf, kh.shape[0]))
    p = uvh.astype(np.float64)[th_]                                             # [nf, 3, 2]
    area = ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1])
            - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1]))            # twice the signed uv area
    drawn = np.nonzero(kh & (area != 0))[0]
    flip = area[drawn] < 0                                                      # the winding the rasterizer culls
    corners = th_[drawn]
    corners[flip] = corners[flip][:, [0, 2, 1]]
    nd = drawn.shape[0]
    face = torch.full((th, tw), -1, dtype=torch.int32, device=dev)
    coeff = torch.zeros((th, tw, 3), dtype=torch.float32, device=dev)
    if nd:
        pts = uvh[corners.reshape(-1)]                                          # [3 nd, 2] float32
        x, y = _square_vertices(2 * pts[:, 0] - 1, 2 * pts[:, 1] - 1, (th, tw))
        verts = np.stack((x, y, np.zeros_like(x)), 1).astype(np.float32)
        s = max(th, tw)
        vt = torch.from_numpy(verts).to(dev)
        tt = torch.arange(3 * nd, dtype=torch.int64, device=dev).view(nd, 3)
        index, c = _raster_forward(vt, tt, s, s)
        index, c = index[:th, :tw], c[:th, :tw]
        covered = (c != 0).any(-1)
        slot = torch.div(index[..., 0], 3, rounding_mode="floor")                # the drawn face: index holds vertex ids
        drawn_t = torch.from_numpy(drawn).to(dev)
        flip_t = torch.from_numpy(flip).to(dev)
        face = torch.where(covered, drawn_t[slot], torch.full_like(slot, -1)).to(torch.int32)
        swapped = flip_t[slot] & covered
        coeff = torch.where(swapped.unsqueeze(-1), c[..., [0, 2, 1]], c)
        coeff = torch.where(covered.unsqueeze(-1), coeff, torch.zeros_like(coeff)).contiguous()
        face = face.contiguous()
    _MAP_CACHE.put(key, (face, coeff, uv, tri_uv, keep))                         # (the key holds their addresses)
    return face, coeff


def texel_centres(size, dtype=torch.float64):
    """uv [Th, Tw, 2] of the texel centres."""
    th, tw = _hw(size)
    u = (torch.arange(tw, dtype=dtype) + 0.5) / tw
    v = 1 - (torch.arange(th, dtype=dtype) + 0.5) / th
    return torch.stack((u.view(1, tw).expand(th, tw), v.view(th, 1).expand(th, tw)), -1)


def depth_buffer(v, tri, size):
    """zbuf [B, Hz, Wz] of the posed mesh v [B, nv, 3], tri [nf, 3] in the pixels `project(., (Hz, Wz))` means: the
    rasterizer's z-buffer (`forward_with_depth`; greater z is nearer, -FLT_MAX is empty).  A non-square size is drawn
    in a square and cropped (see the module's note)."""
    hz, wz = _hw(size)
    if hz != wz:
        x, y = _square_vertices(v[..., 0], v[..., 1], (hz, wz))
        v = torch.stack((x, y, v[..., 2]), -1)
    s = max(hz, wz)
    zbuf = _raster_depth(v.contiguous(), tri.contiguous(), s, s)[2]
    return zbuf[:, :hz, :wz].contiguous()


# ---- bake ------------------------------------------------------------------------------------------------------------
def _facing(facing, dtype):
    """(lo, hi, hi - lo) as Python floats that hold the values of the tensors' float type: float32 takes the difference of
    the rounded ends, as the kernel does."""
    lo, hi = float(facing[0]), float(facing[1])
    if not lo <= hi:
        raise ValueError("bake: facing = (lo, hi) needs lo <= hi, got (%g, %g)" % (lo, hi))
    if dtype == torch.float32:
        lo32, hi32 = np.float32(lo), np.float32(hi)
        return float(lo32), float(hi32), float(np.float32(hi32 - lo32))
    return lo, hi, hi - lo


def _check_bake(v, n, tri, face, coeff, image, zbuf):
    if v.dim() != 3 or v.shape[2] != 3 or tuple(n.shape) != tuple(v.shape):
        raise ValueError("bake: v and n must both be [B, nv, 3], got %s and %s" % (tuple(v.shape), tuple(n.shape)))
    if tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64:
        raise ValueError("bake: tri must be int64 [nf, 3]")
    if face.dim() != 2 or face.dtype != torch.int32 or tuple(coeff.shape) != tuple(face.shape) + (3,):
        raise ValueError("bake: face int32 [Th, Tw] and coeff [Th, Tw, 3] of texel_map, got %s and %s"
                         % (tuple(face.shape), tuple(coeff.shape)))
    b = v.shape[0]
    if image.dim() != 4 or image.shape[0] != b or zbuf.dim() != 3 or zbuf.shape[0] != b:
        raise ValueError("bake: %d samples need image [B, C, Hs, Ws] and zbuf [B, Hz, Wz], got %s and %s"
                         % (b, tuple(image.shape), tuple(zbuf.shape)))
    if min(image.shape[1:]) < 1 or min(zbuf.shape[1:]) < 1 or v.shape[1] < 1 or tri.shape[0] < 1:
        raise ValueError("bake: empty mesh, picture or z-buffer")


def _div(a, b):
    """a / b rounded once to the tensors' float type.  For float32 the quotient is taken in float64 and rounded: with 53
    bits against 24 that is the correctly rounded float32 quotient, whatever the host's vector library does."""
    if a.dtype == torch.float32:
        return (a.double() / (b.double() if isinstance(b, torch.Tensor) else float(b))).float()
    return a / b


def _sqrt(a):
    """sqrt rounded once to the tensor's float type (float32: through float64, as `_div`; torch's vectorised float32
    sqrt on the host is not correctly rounded on every CPU)."""
    return torch.sqrt(a.double()).float() if a.dtype == torch.float32 else torch.sqrt(a)


def bake_composite(v, n, tri, face, coeff, image, zbuf, facing, z_bias, parts=False):
    """The defining tensor algebra, in v's float type: (tex [B, C, Th, Tw], weight [B, 1, Th, Tw]); with parts=True also
    (vis, inside) bool [B, Th, Tw], the two decisions (False on empty texels)."""
    dt, dev = v.dtype, v.device
    lo, hi, span = _facing(facing, dt)
    b, c_n, hs, ws = image.shape
    hz, wz = int(zbuf.shape[1]), int(zbuf.shape[2])
    th, tw = face.shape
    live = face >= 0
    f = face.long().clamp_min(0).reshape(-1)
    corner = tri.to(dev)[f]                                                      # [T, 3]
    cf = coeff.to(dt).reshape(-1, 3)

    def mix(a):                                                                  # [B, nv, 3] -> [B, T, 3]
        return (cf[:, 0:1] * a[:, corner[:, 0]] + cf[:, 1:2] * a[:, corner[:, 1]]) + cf[:, 2:3] * a[:, corner[:, 2]]

    p, nn = mix(v), mix(n.to(dt))
    length = _sqrt((nn[..., 0] * nn[..., 0] + nn[..., 1] * nn[..., 1]) + nn[..., 2] * nn[..., 2])
    m = _div(nn[..., 2], length.clamp_min(TINY))
    if hi > lo:
        t = _div(m - lo, span).clamp(0.0, 1.0)
        g = t * t * (3.0 - 2.0 * t)
    else:
        g = (m > lo).to(dt)
    q = project(p, (hz, wz))
    qx, qy = torch.floor(q[..., 0] + 0.5), torch.floor(q[..., 1] + 0.5)
    on = (qx >= 0) & (qx < wz) & (qy >= 0) & (qy < hz)
    zero = torch.zeros_like(qx)
    at = torch.where(on, qy, zero).long() * wz + torch.where(on, qx, zero).long()
    depth = torch.gather(zbuf.to(dt).reshape(b, -1), 1, at)
    vis = on & (p[..., 2] >= depth - float(z_bias))
    s = project(p, (hs, ws))
    sx, sy = s[..., 0], s[..., 1]
    inside = (sx >= -0.5) & (sx <= ws - 0.5) & (sy >= -0.5) & (sy <= hs - 0.5)
    lv = live.reshape(1, -1)
    vis, inside = vis & lv, inside & lv
    weight = torch.where(vis & inside, g, torch.zeros_like(g))
    take = weight > 0
    x0f, y0f = torch.floor(torch.where(take, sx, zero)), torch.floor(torch.where(take, sy, zero))
    fx, fy = torch.where(take, sx, zero) - x0f, torch.where(take, sy, zero) - y0f
    x0, y0 = x0f.long(), y0f.long()
    xa, xb = x0.clamp(0, ws - 1), (x0 + 1).clamp(0, ws - 1)
    ya, yb = y0.clamp(0, hs - 1), (y0 + 1).clamp(0, hs - 1)
    flat = image.to(dt).reshape(b, c_n, hs * ws)

    def tap(yy, xx):
        return torch.gather(flat, 2, (yy * ws + xx).unsqueeze(1).expand(-1, c_n, -1))

    fx, fy = fx.unsqueeze(1), fy.unsqueeze(1)
    top = (1.0 - fx) * tap(ya, xa) + fx * tap(ya, xb)
    bot = (1.0 - fx) * tap(yb, xa) + fx * tap(yb, xb)
    colour = top * (1.0 - fy) + bot * fy
    tex = torch.where(take.unsqueeze(1), colour, torch.zeros_like(colour))
    out = tex.view(b, c_n, th, tw), weight.view(b, 1, th, tw)
    if parts:
        return out + (vis.view(b, th, tw), inside.view(b, th, tw))
    return out


def native_ok(*tensors):
    return all(is_device_tensor(t) and t.dtype == torch.float32 for t in tensors)


def bake(v, n, tri, face, coeff, image, zbuf, facing=(0.1, 0.4), z_bias=None):
    """(tex [B, C, Th, Tw], weight [B, 1, Th, Tw]): the picture image [B, C, Hs, Ws] (any resolution) carried onto the
    texels of the map (face, coeff) of `texel_map` through the posed mesh v, n [B, nv, 3], tri [nf, 3] and its z-buffer
    zbuf [B, Hz, Wz] (`depth_buffer`, or `forward_with_depth` at a square size).  weight in [0, 1] fades a texel out as
    its normal turns away from the camera (facing = (lo, hi) on the normal's z) and is 0 where the surface is hidden,
    outside the picture or the texel is empty; z_bias (default 4 / max(Hz, Wz)) is the slack of the depth test.  Both
    defaults are starting values, not tuned on any trained checkpoint.  Device float32 runs sr_texture_bake, one launch;
    everything else `bake_composite`.  tri, face and coeff must be valid for the mesh (texel_map's are for its layout)."""
    _check_bake(v, n, tri, face, coeff, image, zbuf)
    hz, wz = int(zbuf.shape[1]), int(zbuf.shape[2])
    if z_bias is None:
        z_bias = 4.0 / max(hz, wz)
    z_bias = float(np.float32(z_bias)) if v.dtype == torch.float32 else float(z_bias)
    if not z_bias >= 0:
        raise ValueError("bake: z_bias must not be negative")
    if not native_ok(v, n, coeff, image, zbuf):
        if is_device_tensor(v) and strict_native():
            raise RuntimeError("bake: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
        return bake_composite(v, n, tri, face, coeff, image, zbuf, facing, z_bias)
    lo, hi, _ = _facing(facing, v.dtype)
    vc, nc, tc, fc, cc, ic, zc = (t.contiguous() for t in (v, n, tri.to(v.device), face.to(v.device), coeff, image, zbuf))
    b, nv = int(vc.shape[0]), int(vc.shape[1])
    c_n, hs, ws = (int(x) for x in ic.shape[1:])
    th, tw = (int(x) for x in fc.shape)
    tex = torch.empty((b, c_n, th, tw), dtype=vc.dtype, device=vc.device)
    weight = torch.empty((b, 1, th, tw), dtype=vc.dtype, device=vc.device)
    native(vc).sr_texture_bake(tex, weight, vc, nc, tc, fc, cc, ic, zc, b, c_n, nv, int(tc.shape[0]), th, tw, hs, ws,
                               hz, wz, lo, hi, z_bias)
    return tex, weight


# ---- padding ---------------------------------------------------------------------------------------------------------
def _shift(a, dy, dx):
    """a [..., H, W] moved so that out[y, x] = a[y + dy, x + dx], zeros from outside."""
    h, w = a.shape[-2:]
    out = torch.zeros_like(a)
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[..., yd, xd] = a[..., ys, xs]
    return out


def pad_host(tex, filled):
    """One padding pass, the definition: (tex', filled') of tex [B, C, Th, Tw] and filled bool [B, 1, Th, Tw]."""
    acc = torch.zeros_like(tex)
    count = torch.zeros(filled.shape, dtype=tex.dtype, device=tex.device)
    for dy in (-1, 0, 1):                                                        # rows top to bottom, left to right
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            nf = _shift(filled, dy, dx)
            acc = acc + torch.where(nf, _shift(tex, dy, dx), torch.zeros_like(tex))
            count = count + nf.to(tex.dtype)
    grow = ~filled & (count > 0)
    return torch.where(grow, acc / count.clamp_min(1), tex), filled | grow


def pad(tex, weight, passes=8):
    """Texture padding: (tex_padded, filled uint8 [B, 1, Th, Tw]).  Initially filled = weight > 0; in each of `passes`
    passes (0..64) every unfilled texel with at least one filled 8-neighbour becomes filled with the sum of its filled
    neighbours' colours (added rows top to bottom, left to right) divided by their count.  All of a pass reads the
    previous pass's state; weight is not changed.  Device float32 runs sr_texture_pad once per pass."""
    passes = int(passes)
    if not 0 <= passes <= MAX_PASSES:
        raise ValueError("pad: 0 <= passes <= %d, got %d" % (MAX_PASSES, passes))
    if tex.dim() != 4 or weight.dim() != 4 or weight.shape[1] != 1 or weight.shape[0] != tex.shape[0] or (
            tuple(weight.shape[2:]) != tuple(tex.shape[2:])):
        raise ValueError("pad: tex [B, C, Th, Tw] and weight [B, 1, Th, Tw], got %s and %s"
                         % (tuple(tex.shape), tuple(weight.shape)))
    filled = weight > 0
    if not native_ok(tex, weight):
        if is_device_tensor(tex) and strict_native():
            raise RuntimeError("pad: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
        out = tex
        for _ in range(passes):
            out, filled = pad_host(out, filled)
        return (out.clone() if out is tex else out), filled.to(torch.uint8)
    b, c_n, th, tw = (int(x) for x in tex.shape)
    cur, cur_f = tex.contiguous(), filled.to(torch.uint8)
    if passes == 0:
        return cur.clone(), cur_f
    bufs = [(torch.empty_like(cur), torch.empty_like(cur_f)) for _ in range(min(passes, 2))]
    for k in range(passes):
        nxt, nxt_f = bufs[k % 2]
        native(cur).sr_texture_pad(nxt, nxt_f, cur, cur_f, b, c_n, th, tw)
        cur, cur_f = nxt, nxt_f
    return cur, cur_f


def fill_mean(tex, weight, filled):
    """tex with every texel that is still unfilled (filled == 0) set to its sample's weight-weighted mean colour
    sum(weight tex) / sum(weight) per channel; a sample with total weight 0 stays as it is (0).  Plain tensor ops: this
    runs once per picture."""
    total = weight.sum((2, 3), keepdim=True)
    mean = (tex * weight).sum((2, 3), keepdim=True) / total.clamp_min(TINY)
    mean = torch.where(total > 0, mean, torch.zeros_like(mean))
    return torch.where(filled.bool(), tex, mean.expand_as(tex))


# ---- merging several views --------------------------------------------------------------------------------------------
MAX_VIEWS = 64
MAX_SHARPNESS = 4
FLUSH = 2.0 ** -63


def _check_merge(tex, weight, sharpness):
    if tex.dim() != 4 or weight.dim() != 4 or weight.shape[1] != 1 or weight.shape[0] != tex.shape[0] or (
            tuple(weight.shape[2:]) != tuple(tex.shape[2:])) or weight.dtype != tex.dtype or weight.device != tex.device:
        raise ValueError("merge: tex [V, C, Th, Tw] and weight [V, 1, Th, Tw] of one float type on one device, got %s "
                         "and %s" % (tuple(tex.shape), tuple(weight.shape)))
    if not tex.is_floating_point() or tex.shape[1] < 1:
        raise ValueError("merge: tex must be floating point with at least one channel")
    if not 1 <= tex.shape[0] <= MAX_VIEWS:
        raise ValueError("merge: 1 <= V <= %d views, got %d" % (MAX_VIEWS, tex.shape[0]))
    if isinstance(sharpness, bool) or int(sharpness) != sharpness or not 0 <= int(sharpness) <= MAX_SHARPNESS:
        raise ValueError("merge: sharpness is an int in 0..%d, got %r" % (MAX_SHARPNESS, sharpness))
    return int(sharpness)


def merge_composite(tex, weight, sharpness=2):
    """The defining tensor algebra of `merge`, in tex's float type."""
    n_v = int(tex.shape[0])
    w = weight[:, 0]                                                             # [V, Th, Tw]
    wmax, best = w[0], torch.zeros(w.shape[1:], dtype=torch.int64, device=w.device)
    for v in range(1, n_v):
        more = w[v] > wmax
        wmax = torch.where(more, w[v], wmax)
        best = torch.where(more, torch.full_like(best, v), best)
    live = wmax > 0
    safe = torch.where(live, wmax, torch.ones_like(wmax))
    zero = torch.zeros_like(wmax)
    den = zero
    num = torch.zeros_like(tex[0])                                               # [C, Th, Tw]
    for v in range(n_v):
        r = _div(w[v], safe)
        r = torch.where(r < FLUSH, zero, r)
        for _ in range(sharpness):
            r = r * r
            r = torch.where(r < FLUSH, zero, r)
        take = live & (r > 0)
        den = torch.where(take, den + r, den)
        num = torch.where(take.unsqueeze(0), num + r.unsqueeze(0) * tex[v], num)
    out = torch.where(live.unsqueeze(0), _div(num, torch.where(live, den, torch.ones_like(den)).unsqueeze(0)),
                      torch.zeros_like(num))
    best = torch.where(live, best, torch.full_like(best, 255)).to(torch.uint8)
    return out.unsqueeze(0), torch.where(live, wmax, zero).view(1, 1, *wmax.shape), best


def merge(tex, weight, sharpness=2):
    """(tex [1, C, Th, Tw], weight [1, 1, Th, Tw], best uint8 [Th, Tw]): the V bakes tex [V, C, Th, Tw] with their weights
    [V, 1, Th, Tw] (one subject, one layout, 1 <= V <= 64) blended per texel with the weights (w_v / max_v w_v)^(2^sharpness),
    sharpness an int in 0..4; the merged weight is the largest of the views', best the first view that has it (255 where
    no view saw the texel; colour and weight are 0 there).  The module's note has the definition step by step.  Device
    float32 runs sr_texture_merge, one launch; everything else `merge_composite`.  The inputs are not changed."""
    sharpness = _check_merge(tex, weight, sharpness)
    if not native_ok(tex, weight):
        if is_device_tensor(tex) and strict_native():
            raise RuntimeError("merge: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
        return merge_composite(tex, weight, sharpness)
    tc, wc = tex.contiguous(), weight.contiguous()
    n_v, c_n, th, tw = (int(x) for x in tc.shape)
    out = torch.empty((1, c_n, th, tw), dtype=tc.dtype, device=tc.device)
    wout = torch.empty((1, 1, th, tw), dtype=tc.dtype, device=tc.device)
    best = torch.empty((th, tw), dtype=torch.uint8, device=tc.device)
    native(tc).sr_texture_merge(out, wout, best, tc, wc, n_v, c_n, th, tw, sharpness)
    return out, wout, best


def coverage(face, weight):
    """The share of the non-empty texels with weight > 0, per sample: [B] float64."""
    live = (face >= 0).view(1, 1, *face.shape)
    n = live.sum().clamp_min(1).double()
    return ((weight > 0) & live).sum((1, 2, 3)).double() / n


# ---- the uv map of a posed mesh ----------------------------------------------------------------------------------------
_TOPO_CACHE = DerivedCache(8)                                                # the exploded meshes' topologies


class _Explode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, tri):
        ctx.save_for_backward(tri)
        ctx.nv = int(v.shape[1])
        return v[:, tri.reshape(-1)].contiguous()

    @staticmethod
    def backward(ctx, g):
        from .rasterize import incidence

        tri, = ctx.saved_tensors
        nv, nf = ctx.nv, int(tri.shape[0])
        b = int(g.shape[0])
        off, adj = incidence(tri, nv)[:2]
        if native_ok(g):
            gc = g.contiguous()
            gv = torch.empty((b, nv, 3), dtype=g.dtype, device=g.device)
            native(gc).sr_explode_bwd(gv, gc, off, adj, b, nv, nf)
            return gv, None
        if is_device_tensor(g) and strict_native():
            raise RuntimeError("explode: SR_STRICT_NATIVE=1 and the kernel takes float32 device tensors only")
        # the definition: corner k nf + f of the incidence list is row 3 f + k of the exploded mesh
        terms = g.reshape(b, nf, 3, 3).permute(0, 3, 2, 1).reshape(b * 3, 3 * nf)
        acc = _ordered_sum(terms, off, adj, nv)                                  # [B 3, nv]
        return acc.view(b, 3, nv).permute(0, 2, 1).contiguous(), None


def explode(v, tri):
    """c [B, 3 nf, 3] with c[b, 3 f + k] = v[b, tri[f, k]]: the mesh v [B, nv, 3] with the corners of tri int64 [nf, 3]
    exploded, the same values as v[:, tri.reshape(-1)].  The gradient of a vertex is the sum of its corners' gradients,
    each coordinate from 0 in the fixed order of op.rasterize.incidence(tri, nv) (built once per topology and cached; its
    entries k nf + f ascend): on float32 device tensors one launch of sr_explode_bwd, everywhere else the same ordered sum
    in torch operations, so host and device agree bit for bit and reruns are bit-identical.  A vertex no face uses gets
    exactly 0.  tri must hold valid vertex numbers and live on v's device."""
    if v.dim() != 3 or v.shape[2] != 3 or tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64:
        raise ValueError("explode: v [B, nv, 3] and tri int64 [nf, 3], got %s and %s" % (tuple(v.shape), tuple(tri.shape)))
    if tri.device != v.device:
        raise ValueError("explode: tri must be on v's device (the incidence list is cached per topology tensor)")
    return _Explode.apply(v, tri)


_explode_corners = explode                                                   # (uv_map has an argument of that name)


def uv_map(v, tri, uv, tri_uv, size, keep=None, explode=False):
    """(uvmap [B, H, W, 2], cover bool [B, H, W]) of the posed mesh v [B, nv, 3], tri [nf, 3] with the layout uv [nt, 2],
    tri_uv [nf, 3] in the pixels `project(., (H, W))` means: the texture coordinates of the surface point under every
    pixel and whether there is one.  A layout has seams, so a vertex has no single uv: the mesh is drawn with its corners
    exploded to 3 nf vertices (v[:, tri.reshape(-1)] with the attributes uv[tri_uv.reshape(-1)], topology
    arange(3 nf).view(nf, 3)) through the `rasterize` Function, so every face interpolates its own chart's coordinates
    and the gradient to v comes from the rasterizer's.  cover is the rasterizer's "some coefficient is non-zero", read
    from a third attribute that is 1 on every corner.  With keep (bool [nf], the faces face_model.uv_layout maps) the
    other faces still occlude, but their pixels are not covered (their three attributes are 0).  A non-square size is
    drawn in a square of side max(H, W) and cropped, as `depth_buffer` does.  Host and device results are equal bit for
    bit (the rasterizer's parity).  explode=True takes the corners through `explode` instead of the indexing: the same
    values, and a gradient to v that is an ordered sum (one launch on the device) instead of a library's
    index_put(accumulate=True); tri must then be on v's device."""
    from .rasterize import rasterize

    h, w = _hw(size)
    if h < 1 or w < 1:
        raise ValueError("uv_map: size must be positive, got (%d, %d)" % (h, w))
    if v.dim() != 3 or v.shape[2] != 3 or tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64:
        raise ValueError("uv_map: v [B, nv, 3] and tri int64 [nf, 3], got %s and %s" % (tuple(v.shape), tuple(tri.shape)))
    if uv.dim() != 2 or uv.shape[1] != 2 or tuple(tri_uv.shape) != tuple(tri.shape):
        raise ValueError("uv_map: uv [nt, 2] and tri_uv [nf, 3] row-parallel to tri, got %s and %s"
                         % (tuple(uv.shape), tuple(tri_uv.shape)))
    dev, dt = v.device, v.dtype
    b, nf = int(v.shape[0]), int(tri.shape[0])
    if keep is not None and int(keep.numel()) != nf:
        raise ValueError("uv_map: keep must have one entry per face (%d), got %d" % (nf, int(keep.numel())))
    if h != w:
        x, y = _square_vertices(v[..., 0], v[..., 1], (h, w))
        v = torch.stack((x, y, v[..., 2]), -1)
    if explode:
        corners = _explode_corners(v, tri)                                     # [B, 3 nf, 3]
    else:
        corners = v[:, tri.to(dev).reshape(-1)].contiguous()
    attr = torch.cat((uv.detach().to(device=dev, dtype=dt)[tri_uv.to(dev).reshape(-1)],
                      torch.ones(3 * nf, 1, dtype=dt, device=dev)), 1)
    if keep is not None:
        attr = attr * keep.to(dev).reshape(-1, 1).expand(-1, 3).reshape(-1, 1).to(dt)
    attr = attr.unsqueeze(0).expand(b, -1, -1).contiguous()
    if explode:
        # one topology tensor per size and device: the rasterizer's backward keys its incidence list by the tensor, and a
        # captured iteration must find it built
        topo = _TOPO_CACHE.get((nf, str(dev)))
        if topo is None:
            topo = _TOPO_CACHE.put((nf, str(dev)), torch.arange(3 * nf, dtype=torch.int64, device=dev).view(nf, 3))
    else:
        topo = torch.arange(3 * nf, dtype=torch.int64, device=dev).view(nf, 3)
    s = max(h, w)
    out = rasterize(corners, attr, topo, s, s, False, 1e-9)[:, :h, :w]
    return out[..., :2].contiguous(), (out[..., 2].detach() != 0).contiguous()


# ---- the sampler -------------------------------------------------------------------------------------------------------
_PLAN_CACHE = DerivedCache(8)


def _check_sample(tex, uvmap, cover):
    if tex.dim() != 4 or not tex.is_floating_point() or min(tex.shape[1:]) < 1:
        raise ValueError("sample: tex must be a floating-point [Bt, C, Th, Tw], got %s %s" % (tex.dtype, tuple(tex.shape)))
    if uvmap.dim() != 4 or uvmap.shape[3] != 2 or uvmap.dtype != tex.dtype or uvmap.device != tex.device:
        raise ValueError("sample: uvmap must be [B, H, W, 2] of tex's float type and device, got %s %s"
                         % (uvmap.dtype, tuple(uvmap.shape)))
    if cover.dtype != torch.bool or tuple(cover.shape) != tuple(uvmap.shape[:3]) or cover.device != tex.device:
        raise ValueError("sample: cover must be bool [B, H, W] on tex's device, got %s %s" % (cover.dtype, tuple(cover.shape)))
    if tex.shape[0] != uvmap.shape[0] and tex.shape[0] != 1:
        raise ValueError("sample: %d views need B textures or one, got %d" % (uvmap.shape[0], tex.shape[0]))


def _footprint(uvmap, cover, th, tw):
    """The definition's per-pixel quantities, each [B, H W]: (live, inx, iny, fx, fy, xa, xb, ya, yb)."""
    b = uvmap.shape[0]
    u, v = uvmap[..., 0].reshape(b, -1), uvmap[..., 1].reshape(b, -1)
    live = cover.reshape(b, -1) & torch.isfinite(u) & torch.isfinite(v)
    zero = torch.zeros_like(u)
    u, v = torch.where(live, u, zero), torch.where(live, v, zero)
    sx, sy = u * tw - 0.5, (1.0 - v) * th - 0.5
    inx, iny = (sx >= -1) & (sx <= tw), (sy >= -1) & (sy <= th)
    sxc, syc = sx.clamp(-1.0, float(tw)), sy.clamp(-1.0, float(th))
    x0f, y0f = torch.floor(sxc.detach()), torch.floor(syc.detach())
    fx, fy = sxc - x0f, syc - y0f
    x0, y0 = x0f.long(), y0f.long()
    return (live, inx, iny, fx, fy, x0.clamp(0, tw - 1), (x0 + 1).clamp(0, tw - 1), y0.clamp(0, th - 1),
            (y0 + 1).clamp(0, th - 1))


def _taps(tex, foot, b):
    """(t00, t01, t10, t11), each [B, C, H W]: the four texels of every pixel."""
    bt, c_n, th, tw = tex.shape
    flat = tex.reshape(bt, c_n, th * tw)
    if bt != b:
        flat = flat.expand(b, -1, -1)
    xa, xb, ya, yb = foot[5:]

    def tap(yy, xx):
        return torch.gather(flat, 2, (yy * tw + xx).unsqueeze(1).expand(-1, c_n, -1))

    return tap(ya, xa), tap(ya, xb), tap(yb, xa), tap(yb, xb)


def _sample_forward(tex, uvmap, cover, background):
    b, h, w = (int(x) for x in uvmap.shape[:3])
    foot = _footprint(uvmap, cover, int(tex.shape[2]), int(tex.shape[3]))
    live, fx, fy = foot[0].unsqueeze(1), foot[3].unsqueeze(1), foot[4].unsqueeze(1)
    t00, t01, t10, t11 = _taps(tex, foot, b)
    top = (1.0 - fx) * t00 + fx * t01
    bot = (1.0 - fx) * t10 + fx * t11
    colour = top * (1.0 - fy) + bot * fy
    out = torch.where(live, colour, torch.full_like(colour, float(background)))
    return out.view(b, int(tex.shape[1]), h, w)


def tap_plan(uvmap, cover, size, bt):
    """(off int32 [Bt Th Tw + 2], entries int32 [4 B H W]): the tap list of the uv map on a (Th, Tw) texture, a CSR over
    the texel keys bt Th Tw + ty Tw + tx (bt = b with Bt = B textures, 0 with one shared texture).  The entries of a key
    are the taps ((b H + y) W + x) 4 + k that fall on it, ascending; k = 0..3 names (ya, xa), (ya, xb), (yb, xa),
    (yb, xb).  The bucket after the last key holds the entries of the uncovered pixels, so the sizes do not depend on the
    data and nothing is read back.  Built with tensor ops on uvmap's device (a stable sort, bincount, cumsum: as
    op.rasterize.incidence builds its list) and cached per uv map (its address and version, cover's, the texture's size
    and Bt): with a fixed pose (texture refinement, a turntable frame) it is built once, while a uv map that changes from
    call to call rebuilds it in every call."""
    th, tw = _hw(size)
    b, h, w = (int(x) for x in uvmap.shape[:3])
    bt = int(bt)
    if bt not in (1, b):
        raise ValueError("tap_plan: Bt is B (%d) or 1, got %d" % (b, bt))
    if 4 * b * h * w >= 2 ** 31 or bt * th * tw >= 2 ** 31 - 1:
        raise ValueError("tap_plan: 4 B H W and Bt Th Tw must be below 2^31")
    key = (uvmap.data_ptr(), uvmap._version, tuple(uvmap.shape), uvmap.dtype, str(uvmap.device), cover.data_ptr(),
           cover._version, th, tw, bt)
    hit = _PLAN_CACHE.get(key)
    if hit is not None:
        return hit[0], hit[1]
    with torch.no_grad():
        foot = _footprint(uvmap.detach(), cover, th, tw)
        live, (xa, xb, ya, yb) = foot[0], foot[5:]
        n_keys = bt * th * tw
        base = torch.arange(b, device=uvmap.device).view(b, 1) * (th * tw) if bt == b else torch.zeros_like(xa)
        keys = torch.stack((ya * tw + xa, ya * tw + xb, yb * tw + xa, yb * tw + xb), -1) + base.unsqueeze(-1)
        keys = torch.where(live.unsqueeze(-1), keys, torch.full_like(keys, n_keys)).reshape(-1)
        entries = torch.sort(keys, stable=True)[1].to(torch.int32).contiguous()
        off = torch.zeros(n_keys + 2, dtype=torch.int32, device=uvmap.device)
        off[1:] = torch.cumsum(torch.bincount(keys, minlength=n_keys + 1), 0).to(torch.int32)
    _PLAN_CACHE.put(key, (off, entries, uvmap, cover))                       # (holds both: the key is their addresses)
    return off, entries


def _ordered_sum(terms, off, entries, n_keys):
    """[C, n_keys]: per key the sum from 0, in list order, of terms [C, 4 B H W] at the key's entries.  Pass r adds every
    list's r-th entry, one addition per texel, so the order inside a list is the list's."""
    acc = terms.new_zeros((terms.shape[0], n_keys))
    start = off[:n_keys].long()
    counts = off[1:n_keys + 1].long() - start
    longest = int(counts.max()) if n_keys else 0
    if longest == 0:
        return acc
    by = torch.sort(counts, descending=True, stable=True)[1]
    more = (n_keys - torch.cumsum(torch.bincount(counts, minlength=longest + 1), 0)).tolist()      # lists longer than r
    for r in range(longest):
        ks = by[:more[r]]
        acc.index_add_(1, ks, terms[:, entries[start[ks] + r].long()])
    return acc


def _sample_backward(tex, uvmap, cover, g, need_uv=True, need_tex=True):
    """(grad_uv [B, H, W, 2], grad_tex [Bt, C, Th, Tw]) of the gradient g [B, C, H, W] of `sample`'s output: the
    definition, the ordered sum of grad_tex included.  Torch operations throughout, so a recorded backward
    (create_graph=True) differentiates again."""
    bt, c_n, th, tw = (int(x) for x in tex.shape)
    b, h, w = (int(x) for x in uvmap.shape[:3])
    foot = _footprint(uvmap, cover, th, tw)
    live, inx, iny, fx, fy = foot[:5]
    gf = g.reshape(b, c_n, h * w)
    guv = gtex = None
    if need_uv:
        t00, t01, t10, t11 = _taps(tex, foot, b)
        fxe, fye = fx.unsqueeze(1), fy.unsqueeze(1)
        top = (1.0 - fxe) * t00 + fxe * t01
        bot = (1.0 - fxe) * t10 + fxe * t11
        dx = (t01 - t00) * (1.0 - fye) + (t11 - t10) * fye
        dy = bot - top
        gx, gy = torch.zeros_like(fx), torch.zeros_like(fy)
        for c in range(c_n):
            gx = gx + gf[:, c] * dx[:, c]
            gy = gy + gf[:, c] * dy[:, c]
        zero = torch.zeros_like(gx)
        guv = torch.stack((torch.where(live & inx, gx * tw, zero), torch.where(live & iny, -(gy * th), zero)), -1)
        guv = guv.view(b, h, w, 2)
    if need_tex:
        off, entries = tap_plan(uvmap, cover, (th, tw), bt)
        wgt = torch.stack(((1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy), -1)      # [B, H W, 4]
        safe = torch.where(live.unsqueeze(1), gf, torch.zeros_like(gf))        # (what stands under no tap cannot leak)
        terms = wgt.unsqueeze(1) * safe.unsqueeze(-1)                          # [B, C, H W, 4]
        terms = terms.permute(1, 0, 2, 3).reshape(c_n, -1)
        acc = _ordered_sum(terms, off, entries, bt * th * tw)
        gtex = acc.view(c_n, bt, th, tw).permute(1, 0, 2, 3).contiguous()
    return guv, gtex


class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uvmap, cover, background, kernels, planner=None):
        ctx.kernels, ctx.background, ctx.planner = kernels, background, planner
        tc, uc, cc = tex.contiguous(), uvmap.contiguous(), cover.contiguous()
        ctx.save_for_backward(tc, uc, cc)
        if not kernels:
            return _sample_forward(tc, uc, cc, background)
        bt, c_n, th, tw = (int(x) for x in tc.shape)
        b, h, w = (int(x) for x in uc.shape[:3])
        out = torch.empty((b, c_n, h, w), dtype=tc.dtype, device=tc.device)
        native(tc).sr_texture_sample_fwd(out, tc, uc, cc, b, bt, c_n, h, w, th, tw, background)
        return out

    @staticmethod
    def backward(ctx, g):
        tc, uc, cc = ctx.saved_tensors
        need_tex, need_uv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_tex or need_uv):
            return None, None, None, None, None, None
        if torch.is_grad_enabled() or not ctx.kernels:
            # the definition in torch operations; under create_graph=True it is recorded and differentiates again
            guv, gtex = _sample_backward(tc, uc, cc, g, need_uv, need_tex)
            return gtex, guv, None, None, None, None
        g = g.contiguous()
        bt, c_n, th, tw = (int(x) for x in tc.shape)
        b, h, w = (int(x) for x in uc.shape[:3])
        guv = gtex = None
        if need_uv:
            guv = torch.empty_like(uc)
            native(tc).sr_texture_sample_bwd_uv(guv, g, tc, uc, cc, b, bt, c_n, h, w, th, tw)
        if need_tex:
            # the tap list: the planner's fixed launch sequence (capturable with a moving uv map), or the cached one
            off, entries = ctx.planner.build(uc, cc) if ctx.planner is not None else tap_plan(uc, cc, (th, tw), bt)
            gtex = torch.empty_like(tc)
            native(tc).sr_texture_sample_bwd_tex(gtex, g, uc, cc, off, entries, b, bt, c_n, h, w, th, tw)
        return gtex, guv, None, None, None, None


def _background(background, dtype):
    return float(np.float32(background)) if dtype == torch.float32 else float(background)


def sample_composite(tex, uvmap, cover, background=0.0):
    """The defining tensor algebra of `sample`, in tex's float type, as an autograd node whose backward is the stated
    formulas (`_sample_backward`: the ordered sum of the texture's gradient included)."""
    _check_sample(tex, uvmap, cover)
    return _Sample.apply(tex.contiguous(), uvmap.contiguous(), cover, _background(background, tex.dtype), False, None)


TAP_RADIX_BITS = 8                                                           # the digit width d of csrc/tap_plan.hip


class TapPlanner:
    """The tap list of `tap_plan` built by the device in a fixed launch sequence (csrc/tap_plan.hip), for a uv map that
    changes from call to call: a fit with the pose among its variables rebuilds the list in every step, inside its
    captured iteration.  A planner is made for one shape: B views of (H, W) pixels on a (Th, Tw) texture, Bt = B or 1.  It
    owns off int32 [Bt Th Tw + 2], entries int32 [4 B H W] and the scratch, all sized from the shapes alone;
    `build(uvmap, cover)` writes every element of off and entries (and every element of the scratch it later reads) on the
    current stream and returns (off, entries), the integers `tap_plan` returns: nothing is allocated, nothing read back,
    no memset, so the sequence can be captured.  The arrays are the planner's own: the next build overwrites them.
    `passes` is the number of digit passes, ceil(bits(Bt Th Tw) / TAP_RADIX_BITS); `launches` the kernels of one build.
    The host definition remains `tap_plan`: a planner takes device tensors only."""

    def __init__(self, b, h, w, size, bt, device):
        th, tw = _hw(size)
        b, h, w, bt = int(b), int(h), int(w), int(bt)
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("TapPlanner: a planner builds its list on the device; on the host `tap_plan` is the list")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())       # (tensors name their device with its index)
        if b < 1 or h < 1 or w < 1 or th < 1 or tw < 1:
            raise ValueError("TapPlanner: sizes must be positive, got B = %d, (%d, %d), (%d, %d)" % (b, h, w, th, tw))
        if bt not in (1, b):
            raise ValueError("TapPlanner: Bt is B (%d) or 1, got %d" % (b, bt))
        if 4 * b * h * w >= 2 ** 31 or bt * th * tw >= 2 ** 31 - 1:
            raise ValueError("TapPlanner: 4 B H W and Bt Th Tw must be below 2^31")
        from .. import _lib

        lib = _lib.lib()
        if int(lib.sr_tap_plan_digit_bits()) != TAP_RADIX_BITS:
            raise RuntimeError("TapPlanner: the library sorts %d-bit digits, this module expects %d"
                               % (int(lib.sr_tap_plan_digit_bits()), TAP_RADIX_BITS))
        self.shape, self.size, self.bt, self.device = (b, h, w), (th, tw), bt, device
        self.passes = int(lib.sr_tap_plan_passes(bt, th, tw))
        self.scratch_ints = int(lib.sr_tap_plan_scratch_ints(b, h, w))
        if self.passes < 1 or self.scratch_ints < 0:
            raise ValueError("TapPlanner: sizes out of the kernels' range")
        self.launches = 2 + 3 * self.passes
        self.off = torch.empty(bt * th * tw + 2, dtype=torch.int32, device=device)
        self.entries = torch.empty(4 * b * h * w, dtype=torch.int32, device=device)
        self.scratch = torch.empty(self.scratch_ints, dtype=torch.int32, device=device)

    def buffers(self):
        """(off, entries, scratch): everything a build writes."""
        return self.off, self.entries, self.scratch

    def build(self, uvmap, cover):
        """(off, entries) of uvmap float32 [B, H, W, 2] and cover bool [B, H, W], contiguous, on the planner's device."""
        b, h, w = self.shape
        if tuple(uvmap.shape) != (b, h, w, 2) or uvmap.dtype != torch.float32 or tuple(cover.shape) != (b, h, w) or (
                cover.dtype != torch.bool):
            raise ValueError("TapPlanner.build: this planner takes uvmap float32 %s and cover bool %s, got %s %s and %s %s"
                             % ((b, h, w, 2), (b, h, w), uvmap.dtype, tuple(uvmap.shape), cover.dtype, tuple(cover.shape)))
        if uvmap.device != self.device or cover.device != self.device:
            raise ValueError("TapPlanner.build: uvmap and cover must be on the planner's device %s" % self.device)
        uc, cc = uvmap.detach().contiguous(), cover.contiguous()
        native(uc).sr_tap_plan_build(self.off, self.entries, self.scratch, self.scratch_ints, uc, cc, b, self.bt, h, w,
                                     self.size[0], self.size[1])
        return self.off, self.entries


def sample(tex, uvmap, cover, background=0.0, planner=None):
    """out [B, C, H, W]: the texture tex [Bt, C, Th, Tw] (Bt = B, or 1: one texture shared by all views) looked up
    bilinearly at the uv map [B, H, W, 2] of `uv_map`; a pixel with cover false or a non-finite coordinate gets
    `background` and contributes to no gradient.  Differentiable in tex and uvmap (the module's note has both gradients).
    Device float32 runs sr_texture_sample_fwd / _bwd_uv / _bwd_tex, one launch each, nothing allocated by a launch and
    nothing read back; everything else `sample_composite`.  The texture's gradient walks the tap list of `tap_plan`, which
    is cached per uv map: with a fixed uv map (refinement, a turntable frame) it is built once and forward and backward can
    be captured after one call of `tap_plan`; a uv map that changes from call to call rebuilds the list in every
    backward.  With planner = a `TapPlanner` of these shapes the device backward takes its list from `planner.build`
    instead: the same integers from a fixed launch sequence, so forward and backward can be captured with a uv map that
    moves between replays (a planner with host tensors is refused).  The results are the host float32 composite's bit
    for bit, and reruns are bit-identical (no atomics)."""
    _check_sample(tex, uvmap, cover)
    kernels = native_ok(tex, uvmap) and is_device_tensor(cover)
    if planner is not None:
        if not kernels:
            raise ValueError("sample: a planner serves the device kernels (float32 device tensors); the host definition's "
                             "list is tap_plan")
        b, h, w = (int(x) for x in uvmap.shape[:3])
        if planner.shape != (b, h, w) or planner.size != (int(tex.shape[2]), int(tex.shape[3])) or (
                planner.bt != int(tex.shape[0])) or planner.device != tex.device:
            raise ValueError("sample: the planner was made for B, H, W = %s, a texture %s and Bt = %d on %s"
                             % (planner.shape, planner.size, planner.bt, planner.device))
    if not kernels and is_device_tensor(tex) and strict_native():
        raise RuntimeError("sample: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
    return _Sample.apply(tex.contiguous(), uvmap.contiguous(), cover, _background(background, tex.dtype), kernels, planner)


def render(v, tri, uv, tri_uv, tex, size, background=0.0, keep=None, mip=None, antialias=False):
    """(image [B, C, H, W], cover bool [B, H, W]): the posed mesh v [B, nv, 3], tri [nf, 3] with the layout uv, tri_uv
    drawn with the texture tex [B or 1, C, Th, Tw] over `background`: `uv_map` followed by `sample`.  Differentiable in tex
    and, through the uv map and the rasterizer, in v.  mip: None, or the lod bias of the mip-mapped look-up
    (`sample_mip` in `sample`'s place).  antialias=True: the image is blended along the mesh's silhouette edges
    (op.edge.antialias; one more rasterizer pass for the face map), which also gives v a gradient from the outline; the
    cover stays the hard one."""
    uvmap, cover = uv_map(v, tri, uv, tri_uv, size, keep)
    if mip is not None:
        image = sample_mip(tex, uvmap, cover, bias=float(mip), background=background)
    else:
        image = sample(tex, uvmap, cover, background)
    if antialias:
        from .edge import antialias as edge_antialias

        image = edge_antialias(image, v.contiguous(), tri.to(v.device))
    return image, cover


# ---- the mip-mapped look-up --------------------------------------------------------------------------------------------
_MIP_PLAN_CACHE = DerivedCache(8)
MIP_MAX_LEVELS = 21                                                          # (sides up to 2^20, as the kernels take)


def mip_layout(size, levels=None):
    """((offset, h, w), ...) of the pyramid of a (Th, Tw) texture: level 0 is (Th, Tw) at offset 0; level l + 1 has half
    of each side and exists while both sides of level l are even and, with `levels` given, while l + 1 < levels.  512^2
    has 10 levels, (12, 20) 3, (33, 65) 1, (128, 64) 7 (the last is 2 x 1).  Level l starts at offset_l of the packed
    [Bt, C, P] pyramid, P = offset + h w of the last level."""
    th, tw = _hw(size)
    if th < 1 or tw < 1:
        raise ValueError("mip_layout: size must be positive, got (%d, %d)" % (th, tw))
    if levels is not None and int(levels) < 1:
        raise ValueError("mip_layout: levels must be at least 1, got %r" % (levels,))
    out, off, h, w = [], 0, th, tw
    while True:
        out.append((off, h, w))
        off += h * w
        if h % 2 or w % 2 or len(out) >= MIP_MAX_LEVELS or (levels is not None and len(out) >= int(levels)):
            break
        h, w = h // 2, w // 2
    return tuple(out)


def _mip_total(layout):
    return layout[-1][0] + layout[-1][1] * layout[-1][2]


def _layout_of(size, p):
    """The layout of a packed pyramid of P elements per plane over a (Th, Tw) texture."""
    full = mip_layout(size)
    for n in range(1, len(full) + 1):
        if _mip_total(full[:n]) == int(p):
            return full[:n]
    raise ValueError("mip: a pyramid of %d elements per plane is none of a %s texture" % (int(p), tuple(_hw(size))))


def _mip_build_forward(tex, layout):
    bt, c_n = int(tex.shape[0]), int(tex.shape[1])
    parts, cur = [tex.reshape(bt, c_n, -1)], tex
    for _ in layout[1:]:
        cur = ((cur[..., 0::2, 0::2] + cur[..., 0::2, 1::2]) + (cur[..., 1::2, 0::2] + cur[..., 1::2, 1::2])) * 0.25
        parts.append(cur.reshape(bt, c_n, -1))
    return torch.cat(parts, 2)


def _mip_build_backward(g, layout):
    """grad_tex [Bt, C, Th, Tw] of the gradient g [Bt, C, P] of the pyramid: the stated chain from the top level down.
    t_l is held per texel of level l: all level-0 texels under one of them share its value."""
    bt, c_n = int(g.shape[0]), int(g.shape[1])
    t = None
    for off, h, w in reversed(layout):
        gl = g[..., off:off + h * w].reshape(bt, c_n, h, w)
        t = gl if t is None else gl + 0.25 * t.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return t if len(layout) > 1 else t.clone()


class _MipBuild(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, n_levels, kernels):
        tc = tex.contiguous()
        bt, c_n, th, tw = (int(x) for x in tc.shape)
        ctx.kernels, ctx.size, ctx.n_levels = kernels, (th, tw), n_levels
        layout = mip_layout((th, tw), n_levels)
        if not kernels:
            return _mip_build_forward(tc, layout)
        pyr = torch.empty((bt, c_n, _mip_total(layout)), dtype=tc.dtype, device=tc.device)
        native(tc).sr_mip_build_fwd(pyr, tc, bt * c_n, th, tw, len(layout))
        return pyr

    @staticmethod
    def backward(ctx, g):
        layout = mip_layout(ctx.size, ctx.n_levels)
        if torch.is_grad_enabled() or not ctx.kernels:
            return _mip_build_backward(g, layout), None, None
        g = g.contiguous()
        bt, c_n = int(g.shape[0]), int(g.shape[1])
        gtex = torch.empty((bt, c_n) + ctx.size, dtype=g.dtype, device=g.device)
        native(g).sr_mip_build_bwd(gtex, g, bt, c_n, ctx.size[0], ctx.size[1], len(layout))
        return gtex, None, None


def _check_mip_tex(tex, name):
    if tex.dim() != 4 or not tex.is_floating_point() or min(tex.shape[1:]) < 1:
        raise ValueError("%s: tex must be a floating-point [Bt, C, Th, Tw], got %s %s" % (name, tex.dtype, tuple(tex.shape)))


def mip_build_composite(tex, levels=None):
    """The defining tensor algebra of `mip_build`, in tex's float type, as an autograd node with the stated backward."""
    _check_mip_tex(tex, "mip_build")
    return _MipBuild.apply(tex, None if levels is None else int(levels), False)


def mip_build(tex, levels=None):
    """pyr [Bt, C, P]: the mip pyramid of tex [Bt, C, Th, Tw] in `mip_layout`'s packing: level 0 a copy of tex, every
    further level the 2 x 2 mean of the one below in the order ((a + b) + (c + d)) 0.25.  Differentiable in tex; the
    backward is a gather per level-0 texel over its ancestors, one order and no scatter.  Device float32 runs
    sr_mip_build_fwd (a launch per five levels) and sr_mip_build_bwd (one launch), nothing allocated by a launch and
    nothing read back; everything else the composite.  The results are the host float32 composite's bit for bit."""
    _check_mip_tex(tex, "mip_build")
    kernels = native_ok(tex)
    if not kernels and is_device_tensor(tex) and strict_native():
        raise RuntimeError("mip_build: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
    return _MipBuild.apply(tex, None if levels is None else int(levels), kernels)


def _check_mip_map(uvmap, cover, name):
    if uvmap.dim() != 4 or uvmap.shape[3] != 2 or not uvmap.is_floating_point():
        raise ValueError("%s: uvmap must be a floating-point [B, H, W, 2], got %s %s" % (name, uvmap.dtype, tuple(uvmap.shape)))
    if cover.dtype != torch.bool or tuple(cover.shape) != tuple(uvmap.shape[:3]) or cover.device != uvmap.device:
        raise ValueError("%s: cover must be bool [B, H, W] on uvmap's device, got %s %s"
                         % (name, cover.dtype, tuple(cover.shape)))


def mip_lod_composite(uvmap, cover, size, levels=None, bias=0.0):
    """The defining tensor algebra of `mip_lod`, in uvmap's float type."""
    _check_mip_map(uvmap, cover, "mip_lod")
    th, tw = _hw(size)
    n_l = len(mip_layout((th, tw), levels))
    dt = uvmap.dtype
    bias = _background(bias, dt)
    with torch.no_grad():
        u, v = uvmap[..., 0], uvmap[..., 1]
        live = cover & torch.isfinite(u) & torch.isfinite(v)
        zero = torch.zeros_like(u)
        u, v = torch.where(live, u, zero), torch.where(live, v, zero)

        def axis(dim):
            """The minimum of d over the usable neighbours along `dim` (1: y, 2: x); 0 with none."""
            n = u.shape[dim]
            a, b = [slice(None)] * 3, [slice(None)] * 3
            a[dim], b[dim] = slice(0, n - 1), slice(1, n)
            a, b = tuple(a), tuple(b)
            du, dv = (u[b] - u[a]) * float(tw), (v[b] - v[a]) * float(th)     # from a to its neighbour b = a + 1
            d_next = du * du + dv * dv
            du, dv = (u[a] - u[b]) * float(tw), (v[a] - v[b]) * float(th)     # from b to its neighbour a = b - 1
            d_prev = du * du + dv * dv
            nxt, prv = torch.zeros_like(u), torch.zeros_like(u)
            has_n, has_p = torch.zeros_like(live), torch.zeros_like(live)
            nxt[a], has_n[a] = d_next, live[b]
            prv[b], has_p[b] = d_prev, live[a]
            both = torch.minimum(nxt, prv)
            return torch.where(has_n & has_p, both, torch.where(has_n, nxt, torch.where(has_p, prv, zero)))

        # a difference of two finite numbers is finite or an infinity, never NaN; its square is not negative, so the sum
        # of two squares is no NaN either: an overflow gives d = inf, rho = inf and the top level
        q = torch.maximum(axis(2), axis(1))
        rho = _sqrt(q)
        lvl = torch.zeros(rho.shape, dtype=torch.int64, device=rho.device)
        for k in range(1, n_l):
            lvl = lvl + (rho >= float(2 ** k)).long()                        # the exact constants 2^k
        scale = torch.tensor([2.0 ** -k for k in range(n_l)], dtype=dt, device=rho.device)[lvl]
        lam = lvl.to(dt) + (rho * scale - 1.0)
        top = float(n_l - 1)
        lam = torch.where(lvl == n_l - 1, torch.full_like(lam, top), lam)
        lam = torch.where(rho < 1, zero, lam)
        lod = (lam + bias).clamp(0.0, top)
        return torch.where(live, lod, zero).contiguous()


def mip_lod(uvmap, cover, size, levels=None, bias=0.0):
    """lod [B, H, W] of uvmap's float type: the level of detail at which a (Th, Tw) = size texture with `mip_layout`'s
    levels is looked up under the uv map [B, H, W, 2] with cover bool [B, H, W]; 0 for a pixel that is not live (cover
    false or a non-finite coordinate).  rho is the texel distance to the nearer of the two live neighbours along each
    axis, the larger of the two axes (the module's note has every step and the seam rule); lod is piecewise linear in rho
    between the powers of two (rho 2^-l - 1 for 2^l <= rho < 2^(l+1)), which stays within 0.09 levels of log2(rho), plus
    `bias`, clamped to [0, L - 1].  A pixel with no usable neighbour at all gets 0 + bias.  Coordinates so large that a
    difference overflows give L - 1; no NaN arises from live pixels.  It carries no gradient: the level is a constant of
    the look-up.  Device float32 runs sr_mip_lod, one launch; everything else `mip_lod_composite`; bit for bit equal."""
    _check_mip_map(uvmap, cover, "mip_lod")
    if not (native_ok(uvmap) and is_device_tensor(cover)):
        if is_device_tensor(uvmap) and strict_native():
            raise RuntimeError("mip_lod: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
        return mip_lod_composite(uvmap, cover, size, levels, bias)
    th, tw = _hw(size)
    n_l = len(mip_layout((th, tw), levels))
    uc, cc = uvmap.detach().contiguous(), cover.contiguous()
    b, h, w = (int(x) for x in uc.shape[:3])
    lod = torch.empty((b, h, w), dtype=uc.dtype, device=uc.device)
    native(uc).sr_mip_lod(lod, uc, cc, b, h, w, th, tw, n_l, _background(bias, uc.dtype))
    return lod


def _mip_foot(uvmap, cover, lod, layout):
    """The per-pixel quantities of the look-up, each [B, H W]: (live, f, (foot0, foot1)) with foot_s = (inx, iny, fx, fy,
    i00, i01, i10, i11, th_l, tw_l) of level l0 + s, s = 0, 1 (l1 = min(l0 + 1, L - 1)); i.. index one packed plane."""
    b = uvmap.shape[0]
    dt, dev = uvmap.dtype, uvmap.device
    n_l = len(layout)
    u, v = uvmap[..., 0].reshape(b, -1), uvmap[..., 1].reshape(b, -1)
    live = cover.reshape(b, -1) & torch.isfinite(u) & torch.isfinite(v)
    zero = torch.zeros_like(u)
    u, v = torch.where(live, u, zero), torch.where(live, v, zero)
    lod = lod.detach().reshape(b, -1).to(dt)
    lodc = torch.where(lod >= 0, lod.clamp_max(float(n_l - 1)), torch.zeros_like(lod))      # (a NaN compares false)
    l0f = torch.floor(lodc)
    f = lodc - l0f
    l0 = l0f.long()
    offs = torch.tensor([o for o, _, _ in layout], dtype=torch.int64, device=dev)
    hs = torch.tensor([h for _, h, _ in layout], dtype=torch.int64, device=dev)
    ws = torch.tensor([w for _, _, w in layout], dtype=torch.int64, device=dev)
    feet = []
    for s in (0, 1):
        lv = (l0 + s).clamp_max(n_l - 1)
        off, hi, wi = offs[lv], hs[lv], ws[lv]
        th, tw = hi.to(dt), wi.to(dt)
        sx, sy = u * tw - 0.5, (1.0 - v) * th - 0.5
        inx, iny = (sx >= -1) & (sx <= tw), (sy >= -1) & (sy <= th)
        sxc = torch.minimum(torch.maximum(sx, torch.full_like(sx, -1.0)), tw)
        syc = torch.minimum(torch.maximum(sy, torch.full_like(sy, -1.0)), th)
        x0f, y0f = torch.floor(sxc.detach()), torch.floor(syc.detach())
        fx, fy = sxc - x0f, syc - y0f
        x0, y0 = x0f.long(), y0f.long()
        lo = torch.zeros_like(x0)
        xa, xb = torch.minimum(torch.maximum(x0, lo), wi - 1), torch.minimum(torch.maximum(x0 + 1, lo), wi - 1)
        ya, yb = torch.minimum(torch.maximum(y0, lo), hi - 1), torch.minimum(torch.maximum(y0 + 1, lo), hi - 1)
        feet.append((inx, iny, fx, fy, off + ya * wi + xa, off + ya * wi + xb, off + yb * wi + xa, off + yb * wi + xb,
                     th, tw))
    return live, f, feet


def _mip_taps(pyr, foot, b):
    bt, c_n, p = pyr.shape
    flat = pyr if bt == b else pyr.expand(b, -1, -1)
    return tuple(torch.gather(flat, 2, i.unsqueeze(1).expand(-1, c_n, -1)) for i in foot[4:8])


def _mip_sample_forward(pyr, layout, uvmap, cover, lod, background):
    b, h, w = (int(x) for x in uvmap.shape[:3])
    live, f, feet = _mip_foot(uvmap, cover, lod, layout)
    cols = []
    for foot in feet:
        fx, fy = foot[2].unsqueeze(1), foot[3].unsqueeze(1)
        t00, t01, t10, t11 = _mip_taps(pyr, foot, b)
        top = (1.0 - fx) * t00 + fx * t01
        bot = (1.0 - fx) * t10 + fx * t11
        cols.append(top * (1.0 - fy) + bot * fy)
    fe = f.unsqueeze(1)
    colour = torch.where(fe == 0, cols[0], (1.0 - fe) * cols[0] + fe * cols[1])
    out = torch.where(live.unsqueeze(1), colour, torch.full_like(colour, float(background)))
    return out.view(b, int(pyr.shape[1]), h, w)


def mip_tap_plan(uvmap, cover, lod, size, levels, bt):
    """(off int32 [Bt P + 2], entries int32 [8 B H W]): the tap list of the mip-mapped look-up, a CSR over the keys
    bt P + offset_l + ty Tw_l + tx of the packed pyramid (`mip_layout(size, levels)`).  The entries of a key are the taps
    ((b H + y) W + x) 8 + k that fall on it, ascending; k = 0..3 are the four taps of level l0 in `tap_plan`'s order,
    k = 4..7 those of l1.  Taps 4..7 of a pixel with f == 0 and all taps of a pixel that is not live lie in the one
    bucket after the last key.  Built with tensor ops on uvmap's device, nothing read back, the sizes depend on shapes
    only; cached per uv map, cover and lod (address and version), size, levels and Bt."""
    th, tw = _hw(size)
    layout = mip_layout((th, tw), levels)
    p = _mip_total(layout)
    b, h, w = (int(x) for x in uvmap.shape[:3])
    bt = int(bt)
    if bt not in (1, b):
        raise ValueError("mip_tap_plan: Bt is B (%d) or 1, got %d" % (b, bt))
    if 8 * b * h * w >= 2 ** 31 or bt * p >= 2 ** 31 - 1:
        raise ValueError("mip_tap_plan: 8 B H W and Bt P must be below 2^31")
    if tuple(lod.shape) != (b, h, w):
        raise ValueError("mip_tap_plan: lod must be [B, H, W], got %s" % (tuple(lod.shape),))
    key = (uvmap.data_ptr(), uvmap._version, tuple(uvmap.shape), uvmap.dtype, str(uvmap.device), cover.data_ptr(),
           cover._version, lod.data_ptr(), lod._version, lod.dtype, th, tw, len(layout), bt)
    hit = _MIP_PLAN_CACHE.get(key)
    if hit is not None:
        return hit[0], hit[1]
    with torch.no_grad():
        live, f, feet = _mip_foot(uvmap.detach(), cover, lod, layout)
        n_keys = bt * p
        keys = torch.stack(feet[0][4:8] + feet[1][4:8], -1)                  # [B, H W, 8]
        if bt == b:
            keys = keys + (torch.arange(b, device=uvmap.device).view(b, 1, 1) * p)
        used = live.unsqueeze(-1) & torch.stack([torch.ones_like(live)] * 4 + [f != 0] * 4, -1)
        keys = torch.where(used, keys, torch.full_like(keys, n_keys)).reshape(-1)
        entries = torch.sort(keys, stable=True)[1].to(torch.int32).contiguous()
        off = torch.zeros(n_keys + 2, dtype=torch.int32, device=uvmap.device)
        off[1:] = torch.cumsum(torch.bincount(keys, minlength=n_keys + 1), 0).to(torch.int32)
    _MIP_PLAN_CACHE.put(key, (off, entries, uvmap, cover, lod))              # (holds all three: the key is their addresses)
    return off, entries


def _mip_sample_backward(pyr, layout, size, uvmap, cover, lod, g, need_uv=True, need_pyr=True):
    """(grad_uv [B, H, W, 2], grad_pyr [Bt, C, P]) of the gradient g [B, C, H, W] of `mip_sample`'s output: the
    definition in torch operations, the ordered sum included; a recorded backward differentiates again."""
    bt, c_n, p = (int(x) for x in pyr.shape)
    b, h, w = (int(x) for x in uvmap.shape[:3])
    live, f, feet = _mip_foot(uvmap, cover, lod, layout)
    gf = g.reshape(b, c_n, h * w)
    guv = gpyr = None
    if need_uv:
        per = []
        for foot in feet:
            inx, iny, fx, fy, th, tw = foot[:4] + foot[8:]
            t00, t01, t10, t11 = _mip_taps(pyr, foot, b)
            fxe, fye = fx.unsqueeze(1), fy.unsqueeze(1)
            top = (1.0 - fxe) * t00 + fxe * t01
            bot = (1.0 - fxe) * t10 + fxe * t11
            dx = (t01 - t00) * (1.0 - fye) + (t11 - t10) * fye
            dy = bot - top
            gx, gy = torch.zeros_like(fx), torch.zeros_like(fy)
            for c in range(c_n):
                gx = gx + gf[:, c] * dx[:, c]
                gy = gy + gf[:, c] * dy[:, c]
            zero = torch.zeros_like(gx)
            per.append(torch.stack((torch.where(live & inx, gx * tw, zero), torch.where(live & iny, -(gy * th), zero)), -1))
        fe = f.unsqueeze(-1)
        guv = torch.where(fe == 0, per[0], (1.0 - fe) * per[0] + fe * per[1])
        guv = torch.where(live.unsqueeze(-1), guv, torch.zeros_like(guv)).view(b, h, w, 2)
    if need_pyr:
        off, entries = mip_tap_plan(uvmap, cover, lod, size, len(layout), bt)
        blend = (1.0 - f, f)
        wgt = []
        for s, foot in enumerate(feet):
            fx, fy = foot[2], foot[3]
            for wk in ((1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy):
                wgt.append(blend[s] * wk)
        wgt = torch.stack(wgt, -1)                                             # [B, H W, 8]
        safe = torch.where(live.unsqueeze(1), gf, torch.zeros_like(gf))        # (what stands under no tap cannot leak)
        terms = wgt.unsqueeze(1) * safe.unsqueeze(-1)                          # [B, C, H W, 8]
        terms = terms.permute(1, 0, 2, 3).reshape(c_n, -1)
        acc = _ordered_sum(terms, off, entries, bt * p)
        gpyr = acc.view(c_n, bt, p).permute(1, 0, 2).contiguous()
    return guv, gpyr


class _MipSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pyr, uvmap, cover, lod, size, background, kernels):
        ctx.kernels, ctx.size = kernels, size
        pc, uc, cc, lc = pyr.contiguous(), uvmap.contiguous(), cover.contiguous(), lod.detach().contiguous()
        ctx.save_for_backward(pc, uc, cc, lc)
        layout = _layout_of(size, pc.shape[2])
        if not kernels:
            return _mip_sample_forward(pc, layout, uc, cc, lc, background)
        bt, c_n = int(pc.shape[0]), int(pc.shape[1])
        b, h, w = (int(x) for x in uc.shape[:3])
        out = torch.empty((b, c_n, h, w), dtype=pc.dtype, device=pc.device)
        native(pc).sr_mip_sample_fwd(out, pc, uc, cc, lc, b, bt, c_n, h, w, size[0], size[1], len(layout), background)
        return out

    @staticmethod
    def backward(ctx, g):
        pc, uc, cc, lc = ctx.saved_tensors
        need_pyr, need_uv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        none = (None,) * 5
        if not (need_pyr or need_uv):
            return (None, None) + none
        size = ctx.size
        layout = _layout_of(size, pc.shape[2])
        if torch.is_grad_enabled() or not ctx.kernels:
            # the definition in torch operations; under create_graph=True it is recorded and differentiates again
            guv, gpyr = _mip_sample_backward(pc, layout, size, uc, cc, lc, g, need_uv, need_pyr)
            return (gpyr, guv) + none
        g = g.contiguous()
        bt, c_n = int(pc.shape[0]), int(pc.shape[1])
        b, h, w = (int(x) for x in uc.shape[:3])
        dims = (b, bt, c_n, h, w, size[0], size[1], len(layout))
        guv = gpyr = None
        if need_uv:
            guv = torch.empty_like(uc)
            native(pc).sr_mip_sample_bwd_uv(guv, g, pc, uc, cc, lc, *dims)
        if need_pyr:
            off, entries = mip_tap_plan(uc, cc, lc, size, len(layout), bt)
            gpyr = torch.empty_like(pc)
            native(pc).sr_mip_sample_bwd_pyr(gpyr, g, uc, cc, lc, off, entries, *dims)
        return (gpyr, guv) + none


def _check_mip_sample(pyr, size, uvmap, cover, lod):
    if pyr.dim() != 3 or not pyr.is_floating_point() or min(pyr.shape[1:]) < 1:
        raise ValueError("mip_sample: pyr must be a floating-point [Bt, C, P], got %s %s" % (pyr.dtype, tuple(pyr.shape)))
    _check_mip_map(uvmap, cover, "mip_sample")
    if uvmap.dtype != pyr.dtype or uvmap.device != pyr.device:
        raise ValueError("mip_sample: uvmap must be of pyr's float type and device")
    if tuple(lod.shape) != tuple(uvmap.shape[:3]) or lod.dtype != pyr.dtype or lod.device != pyr.device:
        raise ValueError("mip_sample: lod must be [B, H, W] of pyr's float type and device, got %s %s"
                         % (lod.dtype, tuple(lod.shape)))
    if pyr.shape[0] != uvmap.shape[0] and pyr.shape[0] != 1:
        raise ValueError("mip_sample: %d views need B pyramids or one, got %d" % (uvmap.shape[0], pyr.shape[0]))
    th, tw = _hw(size)
    _layout_of((th, tw), pyr.shape[2])
    return th, tw


def mip_sample_composite(pyr, size, uvmap, cover, lod, background=0.0):
    """The defining tensor algebra of `mip_sample`, in pyr's float type, as an autograd node with the stated backward."""
    size = _check_mip_sample(pyr, size, uvmap, cover, lod)
    return _MipSample.apply(pyr, uvmap, cover, lod, size, _background(background, pyr.dtype), False)


def mip_sample(pyr, size, uvmap, cover, lod, background=0.0):
    """out [B, C, H, W]: the pyramid pyr [Bt, C, P] (`mip_build` of a (Th, Tw) = size texture; Bt = B or 1) looked up at
    the uv map [B, H, W, 2] at the level of detail lod [B, H, W] (`mip_lod`): bilinear on the two levels around lod,
    blended by its fraction; a whole lod reads one level.  A pixel that is not live gets `background` and contributes to
    no gradient.  Differentiable in pyr and uvmap; lod gets none.  The pyramid's gradient walks the 8-tap list of
    `mip_tap_plan`, cached per (uv map, cover, lod): with all three fixed it is built once and forward and backward can be
    captured after one call of `mip_tap_plan`.  Device float32 runs sr_mip_sample_fwd / _bwd_uv / _bwd_pyr, one launch
    each; everything else the composite; bit for bit equal, reruns bit-identical (no atomics)."""
    size = _check_mip_sample(pyr, size, uvmap, cover, lod)
    kernels = native_ok(pyr, uvmap, lod) and is_device_tensor(cover)
    if not kernels and is_device_tensor(pyr) and strict_native():
        raise RuntimeError("mip_sample: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
    return _MipSample.apply(pyr, uvmap, cover, lod, size, _background(background, pyr.dtype), kernels)


def sample_mip(tex, uvmap, cover, lod=None, bias=0.0, levels=None, background=0.0):
    """out [B, C, H, W]: tex [Bt, C, Th, Tw] looked up at the uv map through its mip pyramid: `mip_build`, `mip_lod`
    (with `bias`; skipped when a lod [B, H, W] is given) and `mip_sample`.  Differentiable in tex and uvmap.  levels=1 is
    `sample`."""
    _check_sample(tex, uvmap, cover)
    size = (int(tex.shape[2]), int(tex.shape[3]))
    if lod is None:
        lod = mip_lod(uvmap, cover, size, levels, bias)
    return mip_sample(mip_build(tex, levels), size, uvmap, cover, lod, background)
