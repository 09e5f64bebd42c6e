"""Albedo and lighting of the textured head: Lambertian shading under second-order spherical harmonics (csrc/light.hip).

A baked texture holds the picture's colours, lighting included.  This module states a shading model, applies and
differentiates it per pixel, estimates the light of one picture in closed form and removes it from a bake.  Every formula
below is one operation of the tensors' float type per step, in the written order, no fused multiply-add; quotients and
roots are correctly rounded (`texture._div`, `texture._sqrt` on the host).

  basis      For a normal n = (nx, ny, nz):
                 r = sqrt((nx nx + ny ny) + nz nz);  len = r > TINY ? r : TINY;  TINY = 1e-12
                 (x, y, z) = (nx / len, ny / len, nz / len)
                 Y = [1, x, y, z, x y, x z, y z, x x - y y, 3 (z z) - 1]
             the Ramamoorthi-Hanrahan polynomial form: nine polynomials that span the same space as the real spherical
             harmonics up to order two, with the orthonormal constants and the Lambert kernel's band factors absorbed in
             the coefficients.  A light in the Deep3DFaceRecon convention, gamma_d . (a_0 c_0, -a_1 c_1 y, a_1 c_1 z,
             -a_1 c_1 x, a_2 c_2 x y, -a_2 c_2 y z, a_2 c_2 / (2 sqrt 3) (3 z z - 1), -a_2 c_2 x z,
             a_2 c_2 / 2 (x x - y y)) with a = (pi, 2 pi / sqrt 3, 2 pi / sqrt 8) and c = (1 / sqrt(4 pi),
             sqrt 3 / sqrt(4 pi), 3 sqrt 5 / sqrt(12 pi)), is this module's gamma with the nine factors `D3DFR` applied to
             gamma_d reordered by `D3DFR_ORDER`:  gamma[k] = D3DFR[k] gamma_d[D3DFR_ORDER[k]].
  light      gamma [B, Cl, 9], Cl = 1 (one white light for every colour channel) or Cl = C (channel c reads light c).
                 s_l = (((g0 + g1 Y1) + g2 Y2) + ...) + g8 Y8           in index order
  range      intensities live in an affine range whose black level is the Python float `black`: -1 for this project's
             [-1, 1] images, 0 for [0, 1].
  shade      out [B, C, H, W] of a [B, C, H, W], normals [B, 3, H, W], on bool [B, H, W].  A pixel is live when `on`
             holds and its three normal components are finite.  With l = c (Cl = C) or 0 (Cl = 1):
                 live:      sp = s_l > 0 ? s_l : 0;   out_c = (a_c - black) sp + black
                 not live:  out_c = background, and no contribution to any gradient
             backward, g the incoming gradient, pos_l = s_l > 0:
                 ga_c  = g_c sp                                           (0 where not live)
                 e_l   = the sum from 0, in channel order, of g_c (a_c - black) over the channels that read light l;
                         0 where not pos_l
                 ggamma[b, l, k] = the sum over the live pixels of e_l Y_k          (Y_0 = 1: the term is e_l)
                 gY_k  = the sum from 0, in l order, of e_l gamma[l, k]             k = 1..8
                 gx = ((gY1 + gY4 y) + gY5 z) + (2 gY7) x
                 gy = ((gY2 + gY4 x) + gY6 z) - (2 gY7) y
                 gz = ((gY3 + gY5 x) + gY6 y) + (6 gY8) z
                 d  = (x gx + y gy) + z gz
                 gn = ((gx - x d) / len, (gy - y d) / len, (gz - z d) / len);   0 where r < TINY or not live
  unshade    the inverse, forward only (no gradient on either path):
                 live:      m = s_l > floor ? s_l : floor;   out_c = (a_c - black) / m + black
                 not live:  out_c = a_c, bit for bit
             `floor` keeps a grazing texel from blowing up.
  texel_attribute   a per-vertex attribute attr [B, nv, A], 1 <= A <= 4, carried into texture space by the texel map
             (face, coeff) of texture.texel_map with the bake's own expression and order,
                 out[b, :, ty, tx] = (c0 attr[b, i0] + c1 attr[b, i1]) + c2 attr[b, i2],   i_k = tri[face, k]
             0 on empty texels; a face or vertex index outside the mesh counts as empty and is never read.  With the posed
             normals this gives the bake's normals per texel.
  normal_map the posed vertex normals drawn over the posed mesh by the `rasterize` Function (channel_major=True): the
             camera-space normals, not camera.project's n_view: shading depends on the surface, not on the ray.
  moments    float64 [B, 45 + 9 C]: the upper triangle (i <= j, row-major) of M = sum w Y Y^T and then R_c = sum w Y
             (a_c - black) for c = 0..C-1, over the pixels with w > 0 and finite normals.  Y and a_c - black are formed in
             the tensors' float type as above; the products (w Y_i) Y_j and (w Y_k)(a_c - black) and the sums are float64.
  fit        the closed-form light under a constant-albedo assumption.  `moments` is read back once (45 + 9 C doubles per
             sample), the rest is float64 on the host: it solves
                 (M + ridge M_00 diag(0, 1, ..., 1)) L_c = R_c,    gamma_c = L_c / abar_c,   abar_c = R_c[0] / M_00
             abar_c is the weighted mean intensity above black.  The ridge leaves the constant's equation alone, so the
             weighted mean of s_c over the fitted pixels is 1:  row 0 of the system is  sum w (Y . L_c) = R_c[0]
             = abar_c M_00  (Y_0 = 1 and the ridge's row 0 is zero);  divide by abar_c M_00:  sum w s_c / sum w = 1.
             The albedo therefore keeps the picture's exposure and the light carries only the variation.  Where M_00 = 0
             or abar_c <= TINY the light is the identity (1, 0, ..., 0); a singular system (a patch of equal normals)
             takes the least-squares solution of least norm.

CPU tensors and float64 take the torch composites below, which are the definition; `shade_composite` is an autograd node
whose backward is the stated formulas in torch operations, so it differentiates again.  Float32 device tensors take
sr_light_shade_fwd / sr_light_shade_bwd / sr_light_reduce / sr_light_moments / sr_light_texel_attr through the C ABI:
shade, ga, gn, unshade and texel_attribute are the host float32 composite's bit for bit.  The light's gradient and the
moments are fixed-order sums (no atomics; reruns are bit-identical): a lane owns `ITEMS` items of four consecutive pixels
of a row, item j of the sample's H ceil(W / 4) items belonging to workgroup j // (BLOCK ITEMS), and adds its terms in
index order; a wave tree of depth 6 and a tree of depth 2 over the workgroup's four waves follow (`TREE_DEPTH` = 8); the
workgroup writes one partial row and sr_light_reduce adds the `partial_rows` rows in ascending order.  Against the exact
sum of the terms the result is within (`terms_per_lane` + TREE_DEPTH + partial_rows) u sum |term| to first order, u =
2^-24 for the light's gradient and 2^-53 for the moments.  The backward's scratch is allocated in forward, sized from the
shapes alone: no launch allocates or reads back, so forward and backward can be captured.  Under SR_STRICT_NATIVE=1
nothing falls to a library: a device tensor the kernels do not take (float64, more than four lights) raises.

Not built: specular terms, cast shadows or ambient occlusion, sRGB linearisation, an albedo prior or symmetry, choosing
the ridge or the floor from data.
"""
import math

import numpy as np
import torch

from ._dispatch import is_device_tensor, mark_inputs, native, strict_native, wanted
from .landmark import _hw
from .texture import _div, _square_vertices, _sqrt

TINY = 1e-12
NB = 9                                # basis functions
NM = 45                               # entries of M's upper triangle
# the layout of the two reductions: lanes per workgroup, items (of four pixels) per lane, pixels per item, the depth of
# the tree that adds a workgroup's lanes, and the most lights / channels the kernels carry in registers
BLOCK = 256
ITEMS = 4
GROUP = 4
TREE_DEPTH = 8
MAX_LIGHTS = 4
MAX_ATTR = 4

# this module's gamma from a Deep3DFaceRecon light gamma_d: gamma[k] = D3DFR[k] * gamma_d[D3DFR_ORDER[k]]
_A = (math.pi, 2 * math.pi / math.sqrt(3.0), 2 * math.pi / math.sqrt(8.0))
_C = (1 / math.sqrt(4 * math.pi), math.sqrt(3.0) / math.sqrt(4 * math.pi), 3 * math.sqrt(5.0) / math.sqrt(12 * math.pi))
D3DFR_ORDER = (0, 3, 1, 2, 4, 7, 5, 8, 6)
D3DFR = (_A[0] * _C[0], -_A[1] * _C[1], -_A[1] * _C[1], _A[1] * _C[1],
         _A[2] * _C[2], -_A[2] * _C[2], -_A[2] * _C[2], _A[2] * _C[2] / 2, _A[2] * _C[2] / (2 * math.sqrt(3.0)))


def partial_rows(h, w):
    """How many partial rows per sample the two reductions write for an [.., H, W] picture."""
    items = int(h) * (-(-int(w) // GROUP))
    return max(1, -(-items // (BLOCK * ITEMS)))


def terms_per_lane(h, w):
    """How many terms the busiest lane adds before the tree: its items' pixels, in index order."""
    h, w = int(h), int(w)
    items = h * (-(-w // GROUP))
    per_lane = min(ITEMS, -(-items // BLOCK))
    return per_lane * min(GROUP, w)


def scratch_floats(b, cl, h, w):
    """The float32 elements of sr_light_shade_bwd's scratch."""
    return int(b) * partial_rows(h, w) * int(cl) * NB


def _value(x, dtype):
    return float(np.float32(x)) if dtype == torch.float32 else float(x)


def _check(name, a, normals, on, gamma=None):
    if a.dim() != 4 or not a.is_floating_point() or a.shape[1] < 1:
        raise ValueError("%s: a must be a floating-point [B, C, H, W], got %s %s" % (name, a.dtype, tuple(a.shape)))
    b, c, h, w = a.shape
    if tuple(normals.shape) != (b, 3, h, w) or normals.dtype != a.dtype or normals.device != a.device:
        raise ValueError("%s: normals must be [%d, 3, %d, %d] of a's float type and device, got %s %s"
                         % (name, b, h, w, normals.dtype, tuple(normals.shape)))
    if on is not None and (on.dtype != torch.bool or tuple(on.shape) != (b, h, w) or on.device != a.device):
        raise ValueError("%s: on must be bool [%d, %d, %d] on a's device, got %s %s"
                         % (name, b, h, w, on.dtype, tuple(on.shape)))
    if gamma is not None and (gamma.dim() != 3 or gamma.shape[0] != b or gamma.shape[1] not in (1, c)
                              or gamma.shape[2] != NB or gamma.dtype != a.dtype or gamma.device != a.device):
        raise ValueError("%s: gamma must be [%d, 1 or %d, 9] of a's float type and device, got %s %s"
                         % (name, b, c, gamma.dtype, tuple(gamma.shape)))


# ---- the definition ----------------------------------------------------------------------------------------------------
def basis(normals):
    """(Y: a list of nine [B, H, W] tensors, (x, y, z), r, len) of normals [B, 3, H, W]: the definition."""
    nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
    r = _sqrt((nx * nx + ny * ny) + nz * nz)
    length = torch.where(r > TINY, r, torch.full_like(r, TINY))
    x, y, z = _div(nx, length), _div(ny, length), _div(nz, length)
    ys = [torch.ones_like(x), x, y, z, x * y, x * z, y * z, x * x - y * y, 3.0 * (z * z) - 1.0]
    return ys, (x, y, z), r, length


def _live(normals, on):
    return on & torch.isfinite(normals).all(1)


def _shading(ys, gamma):
    """s [B, Cl, H, W]."""
    g = gamma.unsqueeze(-1).unsqueeze(-1)                                        # [B, Cl, 9, 1, 1]
    s = g[:, :, 0] + g[:, :, 1] * ys[1].unsqueeze(1)
    for k in range(2, NB):
        s = s + g[:, :, k] * ys[k].unsqueeze(1)
    return s


def _clean(normals, live):
    """normals with the pixels that are not live replaced by +z, so that nothing non-finite enters the algebra."""
    fill = torch.zeros_like(normals)
    fill[:, 2] = 1.0
    return torch.where(live.unsqueeze(1), normals, fill)


def _shade_forward(a, normals, on, gamma, black, background):
    live = _live(normals, on)
    ys = basis(_clean(normals, live))[0]
    s = _shading(ys, gamma)
    sp = torch.where(s > 0, s, torch.zeros_like(s))
    out = (a - black) * sp + black
    return torch.where(live.unsqueeze(1), out, torch.full_like(out, background))


def light_terms(a, normals, on, gamma, g, black=-1.0):
    """The terms e_l Y_k [B, Cl, 9, H, W] that ggamma sums (0 on the pixels that are not live), in a's float type."""
    black = _value(black, a.dtype)
    live = _live(normals, on)
    ys = basis(_clean(normals, live))[0]
    e = _light_e(a, ys, gamma, g, black, live)
    return torch.stack([e] + [e * ys[k].unsqueeze(1) for k in range(1, NB)], 2)


def _light_e(a, ys, gamma, g, black, live):
    """e [B, Cl, H, W]."""
    c, cl = a.shape[1], gamma.shape[1]
    s = _shading(ys, gamma)
    prod = g * (a - black)
    if cl == c:
        e = torch.zeros_like(prod) + prod
    else:
        e = torch.zeros_like(prod[:, :1])
        for ch in range(c):
            e = e + prod[:, ch:ch + 1]
    return torch.where((s > 0) & live.unsqueeze(1), e, torch.zeros_like(e))


def _shade_backward(a, normals, on, gamma, g, black, need_n=True, need_gamma=True):
    """(ga, gn, ggamma) of the gradient g of `shade`'s output: the definition, in torch operations."""
    live = _live(normals, on)
    ys, (x, y, z), r, length = basis(_clean(normals, live))
    s = _shading(ys, gamma)
    sp = torch.where(s > 0, s, torch.zeros_like(s))
    lv = live.unsqueeze(1)
    ga = torch.where(lv, g * sp, torch.zeros_like(g))
    gn = ggamma = None
    if not (need_n or need_gamma):
        return ga, gn, ggamma
    e = _light_e(a, ys, gamma, g, black, live)
    if need_gamma:
        terms = torch.stack([e] + [e * ys[k].unsqueeze(1) for k in range(1, NB)], 2)
        ggamma = terms.sum((3, 4))
    if need_n:
        gy_ = [None]
        for k in range(1, NB):
            acc = torch.zeros_like(x)
            for l in range(gamma.shape[1]):
                acc = acc + e[:, l] * gamma[:, l, k].view(-1, 1, 1)
            gy_.append(acc)
        gx = ((gy_[1] + gy_[4] * y) + gy_[5] * z) + (2.0 * gy_[7]) * x
        gy = ((gy_[2] + gy_[4] * x) + gy_[6] * z) - (2.0 * gy_[7]) * y
        gz = ((gy_[3] + gy_[5] * x) + gy_[6] * y) + (6.0 * gy_[8]) * z
        d = (x * gx + y * gy) + z * gz
        gn = torch.stack((_div(gx - x * d, length), _div(gy - y * d, length), _div(gz - z * d, length)), 1)
        gn = torch.where((live & ~(r < TINY)).unsqueeze(1), gn, torch.zeros_like(gn))
    return ga, gn, ggamma


class _ShadeComposite(torch.autograd.Function):
    """The definition as an autograd node: its backward is the stated formulas in torch operations (not what autograd
    would derive from the forward, which rounds differently), so it can be differentiated again."""

    @staticmethod
    def forward(ctx, a, normals, on, gamma, black, background):
        ctx.black = black
        ctx.save_for_backward(a, normals, on, gamma)
        return _shade_forward(a, normals, on, gamma, black, background)

    @staticmethod
    def backward(ctx, g):
        a, normals, on, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        ga, gn, ggamma = _shade_backward(a, normals, on, gamma, g, ctx.black, need[1], need[3])
        return (ga if need[0] else None), gn, None, ggamma, None, None


def shade_composite(a, normals, on, gamma, black=-1.0, background=-1.0):
    """The defining tensor algebra of `shade`, in a's float type."""
    _check("shade", a, normals, on, gamma)
    return _ShadeComposite.apply(a, normals, on, gamma, _value(black, a.dtype), _value(background, a.dtype))


def unshade_composite(a, normals, on, gamma, black=-1.0, floor=0.05):
    """The defining tensor algebra of `unshade`, in a's float type."""
    _check("unshade", a, normals, on, gamma)
    black, floor = _value(black, a.dtype), _value(floor, a.dtype)
    with torch.no_grad():
        live = _live(normals, on)
        s = _shading(basis(_clean(normals, live))[0], gamma)
        m = torch.where(s > floor, s, torch.full_like(s, floor))
        return torch.where(live.unsqueeze(1), _div(a - black, m) + black, a)


def _check_attr(attr, tri, face, coeff):
    if attr.dim() != 3 or not attr.is_floating_point() or not 1 <= attr.shape[2] <= MAX_ATTR or attr.shape[1] < 1:
        raise ValueError("texel_attribute: attr must be a floating-point [B, nv, A] with 1 <= A <= %d, got %s %s"
                         % (MAX_ATTR, attr.dtype, tuple(attr.shape)))
    if tri.dim() != 2 or tri.shape[1] != 3 or tri.dtype != torch.int64:
        raise ValueError("texel_attribute: tri must be int64 [nf, 3]")
    if face.dim() != 2 or face.dtype != torch.int32 or tuple(coeff.shape) != tuple(face.shape) + (3,):
        raise ValueError("texel_attribute: face int32 [Th, Tw] and coeff [Th, Tw, 3] of texel_map, got %s and %s"
                         % (tuple(face.shape), tuple(coeff.shape)))


def texel_attribute_composite(attr, tri, face, coeff):
    """The defining tensor algebra of `texel_attribute`, in attr's float type."""
    _check_attr(attr, tri, face, coeff)
    with torch.no_grad():
        dt, dev = attr.dtype, attr.device
        b, nv, n_a = attr.shape
        th, tw = face.shape
        tri, nf = tri.to(dev), int(tri.shape[0])
        f = face.to(dev).long().reshape(-1)
        live = (f >= 0) & (f < nf)
        if nf == 0:
            return torch.zeros((b, n_a, th, tw), dtype=dt, device=dev)
        corner = tri[torch.where(live, f, torch.zeros_like(f))]                  # [T, 3]
        live = live & ((corner >= 0) & (corner < nv)).all(1)
        corner = torch.where(live.unsqueeze(1), corner, torch.zeros_like(corner))
        cf = coeff.to(device=dev, dtype=dt).reshape(-1, 3)
        mix = (cf[:, 0:1] * attr[:, corner[:, 0]] + cf[:, 1:2] * attr[:, corner[:, 1]]) + cf[:, 2:3] * attr[:, corner[:, 2]]
        mix = torch.where(live.view(1, -1, 1), mix, torch.zeros_like(mix))
        return mix.permute(0, 2, 1).reshape(b, n_a, th, tw).contiguous()


def _check_moments(a, normals, weight):
    _check("moments", a, normals, None)
    b, _, h, w = a.shape
    if tuple(weight.shape) != (b, 1, h, w) or weight.dtype != a.dtype or weight.device != a.device:
        raise ValueError("moments: weight must be [%d, 1, %d, %d] of a's float type and device, got %s %s"
                         % (b, h, w, weight.dtype, tuple(weight.shape)))


def moment_terms(a, normals, weight, black=-1.0):
    """The float64 terms [B, 45 + 9 C, H, W] that `moments` sums (0 on the pixels it skips): the definition."""
    _check_moments(a, normals, weight)
    black = _value(black, a.dtype)
    with torch.no_grad():
        w = weight[:, 0]
        live = (w > 0) & torch.isfinite(normals).all(1)
        ys = [t.double() for t in basis(_clean(normals, live))[0]]
        wd = torch.where(live, w, torch.zeros_like(w)).double()
        wy = [wd * t for t in ys]
        rows = [wy[i] * ys[j] for i in range(NB) for j in range(i, NB)]
        d = (a - black).double()
        rows += [wy[k] * d[:, c] for c in range(a.shape[1]) for k in range(NB)]
        out = torch.stack(rows, 1)
        return torch.where(live.unsqueeze(1), out, torch.zeros_like(out))


def moments_composite(a, normals, weight, black=-1.0):
    """The defining tensor algebra of `moments`."""
    return moment_terms(a, normals, weight, black).sum((2, 3))


# ---- the kernels -------------------------------------------------------------------------------------------------------
def native_ok(*tensors):
    return all(is_device_tensor(t) and t.dtype == torch.float32 for t in tensors if t is not None)


def _strict(name, like):
    if is_device_tensor(like) and strict_native():
        raise RuntimeError("%s: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors (at most %d lights) only"
                           % (name, MAX_LIGHTS))


def _kernels(a, normals, gamma, on=None):
    return (native_ok(a, normals, gamma) and (on is None or is_device_tensor(on))
            and (gamma is None or gamma.shape[1] <= MAX_LIGHTS))


class _ShadeNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, normals, on, gamma, black, background, ggamma_out):
        mark_inputs(ctx, a, normals, on, gamma, black, background, ggamma_out)
        ac, nc, oc, gc = a.contiguous(), normals.contiguous(), on.contiguous(), gamma.contiguous()
        b, c, h, w = (int(x) for x in ac.shape)
        cl = int(gc.shape[1])
        out = torch.empty_like(ac)
        native(ac).sr_light_shade_fwd(out, ac, nc, oc, gc, b, c, cl, h, w, black, 0.0, background, 0)
        ctx.black, ctx.ggamma_out = black, ggamma_out
        # the backward's scratch, sized from the shapes alone: its launches allocate nothing
        ctx.scratch = None
        if ctx.needs_input_grad[3] or ggamma_out is not None:
            ctx.scratch = torch.empty(scratch_floats(b, cl, h, w), dtype=torch.float32, device=ac.device)
        ctx.save_for_backward(ac, nc, oc, gc)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        ac, nc, oc, gc = ctx.saved_tensors
        need = wanted(ctx)
        g = g.contiguous()
        b, c, h, w = (int(x) for x in ac.shape)
        cl = int(gc.shape[1])
        to_buffer = ctx.ggamma_out is not None
        need_gamma = to_buffer or need[3]
        ga = torch.empty_like(ac)
        gn = torch.empty_like(nc) if need[1] else None
        scratch = ctx.scratch if need_gamma else None
        run = native(ac)
        run.sr_light_shade_bwd(ga, gn, scratch, g, ac, nc, oc, gc, b, c, cl, h, w, ctx.black)
        ggamma = None
        if need_gamma:
            ggamma = ctx.ggamma_out if to_buffer else torch.empty_like(gc)
            run.sr_light_reduce(ggamma, scratch, b, partial_rows(h, w), cl * NB, 0)
        return (ga if need[0] else None), gn, None, (None if to_buffer else ggamma), None, None, None


def shade(a, normals, on, gamma, black=-1.0, background=-1.0, ggamma_out=None):
    """out [B, C, H, W]: the albedo a [B, C, H, W] lit by the light gamma [B, 1 or C, 9] on the surface with the normals
    [B, 3, H, W], where `on` (bool [B, H, W]) holds and the normal is finite; `background` elsewhere.  Differentiable in a,
    normals and gamma (the module's note has the formulas).  Device float32 runs sr_light_shade_fwd and, backward,
    sr_light_shade_bwd and sr_light_reduce; everything else `shade_composite`.
    ggamma_out (kernels only): a contiguous float32 device buffer of at least B Cl 9 elements; the backward writes the
    light's gradient into its first B Cl 9 elements and gamma receives no gradient through autograd."""
    _check("shade", a, normals, on, gamma)
    kernels = _kernels(a, normals, gamma, on)
    if ggamma_out is not None and not (kernels and native_ok(ggamma_out) and ggamma_out.is_contiguous()
                                       and ggamma_out.numel() >= gamma.numel() and ggamma_out.device == a.device):
        raise ValueError("shade: ggamma_out is for the kernels: float32 device tensors and a contiguous float32 buffer of "
                         "at least B Cl 9 elements on their device")
    if not kernels or a.numel() == 0:
        if not kernels:
            _strict("shade", a)
        return shade_composite(a, normals, on, gamma, black, background)
    return _ShadeNative.apply(a, normals, on, gamma, _value(black, a.dtype), _value(background, a.dtype), ggamma_out)


def unshade(a, normals, on, gamma, black=-1.0, floor=0.05):
    """out [B, C, H, W]: the light gamma removed from the lit intensities a, out_c = (a_c - black) / max(s, floor) + black
    on the live pixels and a_c itself elsewhere.  Forward only: the result carries no gradient.  floor = 0.05 is a
    starting value, not tuned on any picture.  Device float32 runs sr_light_shade_fwd in its dividing form."""
    _check("unshade", a, normals, on, gamma)
    if not float(floor) > 0:
        raise ValueError("unshade: floor must be positive, got %r" % (floor,))
    if a.numel() == 0:
        return a.detach().clone()
    if not _kernels(a, normals, gamma, on):
        _strict("unshade", a)
        return unshade_composite(a, normals, on, gamma, black, floor)
    ac, nc, oc, gc = (t.detach().contiguous() for t in (a, normals, on, gamma))
    b, c, h, w = (int(x) for x in ac.shape)
    out = torch.empty_like(ac)
    native(ac).sr_light_shade_fwd(out, ac, nc, oc, gc, b, c, int(gc.shape[1]), h, w, _value(black, a.dtype),
                                  _value(floor, a.dtype), 0.0, 1)
    return out


def texel_attribute(attr, tri, face, coeff):
    """out [B, A, Th, Tw]: the per-vertex attribute attr [B, nv, A] (1 <= A <= 4) of a mesh with the faces tri [nf, 3] at
    the texels of the map (face, coeff) of texture.texel_map, 0 on empty texels.  No gradient.  Device float32 runs
    sr_light_texel_attr, one launch; everything else `texel_attribute_composite`."""
    _check_attr(attr, tri, face, coeff)
    if attr.shape[0] == 0 or face.numel() == 0 or tri.shape[0] == 0:
        return texel_attribute_composite(attr, tri, face, coeff)
    if not native_ok(attr, coeff):
        _strict("texel_attribute", attr)
        return texel_attribute_composite(attr, tri, face, coeff)
    dev = attr.device
    ac, tc, fc, cc = (t.detach().contiguous() for t in (attr, tri.to(dev), face.to(dev), coeff.to(dev)))
    b, nv, n_a = (int(x) for x in ac.shape)
    th, tw = (int(x) for x in fc.shape)
    out = torch.empty((b, n_a, th, tw), dtype=ac.dtype, device=dev)
    native(ac).sr_light_texel_attr(out, ac, tc, fc, cc, b, n_a, nv, int(tc.shape[0]), th, tw)
    return out


def normal_map(v, n, tri, size):
    """normals [B, 3, H, W] of the posed mesh v, n [B, nv, 3], tri [nf, 3] in the pixels `landmark.project(., (H, W))`
    means: the vertex normals interpolated by the `rasterize` Function (0 where nothing is drawn; not normalised: the
    basis does that).  A non-square size is drawn in a square of side max(H, W) and cropped, as texture.uv_map does."""
    from .rasterize import rasterize

    h, w = _hw(size)
    if h < 1 or w < 1:
        raise ValueError("normal_map: size must be positive, got (%d, %d)" % (h, w))
    if v.dim() != 3 or v.shape[2] != 3 or tuple(n.shape) != tuple(v.shape) or tri.dim() != 2 or tri.shape[1] != 3:
        raise ValueError("normal_map: v and n [B, nv, 3] and tri [nf, 3], got %s, %s and %s"
                         % (tuple(v.shape), tuple(n.shape), tuple(tri.shape)))
    if h != w:
        x, y = _square_vertices(v[..., 0], v[..., 1], (h, w))
        v = torch.stack((x, y, v[..., 2]), -1)
    s = max(h, w)
    out = rasterize(v.contiguous(), n.to(v.dtype).contiguous(), tri.to(v.device).contiguous(), s, s, False, 1e-9, True)
    return out[:, :, :h, :w].contiguous()


def moments(a, normals, weight, black=-1.0):
    """float64 [B, 45 + 9 C]: the upper triangle of M = sum w Y Y^T and R_c = sum w Y (a_c - black) over the pixels with
    weight [B, 1, H, W] > 0 and finite normals.  Device float32 with C <= 4 runs sr_light_moments and sr_light_reduce
    (fixed-order float64 sums on the device); everything else `moments_composite`."""
    _check_moments(a, normals, weight)
    if a.numel() == 0:
        return torch.zeros((a.shape[0], NM + NB * a.shape[1]), dtype=torch.float64, device=a.device)
    if not (native_ok(a, normals, weight) and a.shape[1] <= MAX_LIGHTS):
        _strict("moments", a)
        return moments_composite(a, normals, weight, black)
    ac, nc, wc = (t.detach().contiguous() for t in (a, normals, weight))
    b, c, h, w = (int(x) for x in ac.shape)
    n_m, rows = NM + NB * c, partial_rows(h, w)
    scratch = torch.empty(b * rows * n_m, dtype=torch.float64, device=ac.device)
    out = torch.empty((b, n_m), dtype=torch.float64, device=ac.device)
    run = native(ac)
    run.sr_light_moments(scratch, ac, nc, wc, b, c, h, w, _value(black, a.dtype))
    run.sr_light_reduce(out, scratch, b, rows, n_m, 1)
    return out


def solve_light(mom, c, mono=False, ridge=1e-3):
    """gamma float64 [B, Cl, 9] (numpy) of the moments mom [B, 45 + 9 C]: the host half of `fit`."""
    mom = np.asarray(mom, np.float64).reshape(-1, NM + NB * int(c))
    iu = np.triu_indices(NB)
    lights = 1 if mono else int(c)
    out = np.zeros((mom.shape[0], lights, NB))
    out[:, :, 0] = 1.0
    for b in range(mom.shape[0]):
        m = np.zeros((NB, NB))
        m[iu] = mom[b, :NM]
        m = m + np.triu(m, 1).T
        rhs = mom[b, NM:].reshape(int(c), NB)
        if mono:
            rhs = rhs.sum(0, keepdims=True) / int(c)
        if not (np.isfinite(m).all() and np.isfinite(rhs).all() and m[0, 0] > 0):
            continue
        sys = m + float(ridge) * m[0, 0] * np.diag([0.0] + [1.0] * (NB - 1))
        for l in range(lights):
            mean = rhs[l, 0] / m[0, 0]
            if not mean > TINY:
                continue
            try:
                sol = np.linalg.solve(sys, rhs[l])
                if not np.isfinite(sol).all():
                    raise np.linalg.LinAlgError
            except np.linalg.LinAlgError:
                sol = np.linalg.lstsq(sys, rhs[l], rcond=None)[0]
            if np.isfinite(sol).all():
                out[b, l] = sol / mean
    return out


def fit(a, normals, weight, black=-1.0, mono=False, ridge=1e-3):
    """gamma [B, Cl, 9] (Cl = 1 with mono, else C) on a's device and in its dtype: the light that explains the
    intensities a [B, C, H, W] on the surface with the normals [B, 3, H, W] best, in the least squares weighted by weight
    [B, 1, H, W], if the albedo were constant (the module's note: the system, the ridge and why the weighted mean shading
    is 1).  `moments` is read back once; the solve is float64 on the host.  Once per picture, never inside a captured
    step.  ridge = 1e-3 is a starting value, not tuned on any picture."""
    if not float(ridge) >= 0:
        raise ValueError("fit: ridge must not be negative, got %r" % (ridge,))
    mom = moments(a, normals, weight, black).cpu().numpy()
    gamma = solve_light(mom, int(a.shape[1]), mono, ridge)
    return torch.from_numpy(gamma).to(device=a.device, dtype=a.dtype)
