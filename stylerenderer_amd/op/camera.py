"""The perspective camera of face reconstruction: one node between the posed mesh and everything that consumes it
(csrc/camera.hip).

Every consumer of a posed mesh here is orthographic: op.rasterize inside the generator, op.landmark, op.texture's
depth_buffer and bake, the mesh gate of op.region.  `project` bends the mesh so that their orthographic view of the result
is the perspective view of the input; they stay as they are.

  project(v [B, nv, 3], kappa [B], normals=None) -> v' [B, nv, 3], or (v', n_view) with normals [B, nv, 3].
      kappa = 1 / D, D the camera's distance from the plane z = 0 of pose space in half-picture-widths.  That is the focal
      length in the same unit, so kappa = tan(hfov / 2).  Per vertex (x, y, z) of row b with k = kappa[b], every step one
      operation of the tensors' float type, in this order, no fused multiply-add:
          q0 = 1 - k z
          clamped = q0 < QMIN                  QMIN = 1/16: at or behind the camera
          q  = QMIN if clamped else q0
          v' = (x / q, y / q, z / q)           each quotient correctly rounded
      k = 0 is the identity bit for bit.  Points on z = 0 never move, so the pose's scale and translation keep their
      meaning and the orthographic closed-form pose start stays a start.  z' is monotone in z: "greater z is nearer"
      survives for the z-buffers.
  n_view  what the facing gates (the landmark term's visibility, the bake's facing weight) read instead of the normal: the
      normal N turned by the smallest rotation that takes the ray to the camera, d, onto +z.
          a = (k x', k y');  len = sqrt(1 + (a.x a.x + a.y a.y));  d = (-a.x / len, -a.y / len, 1 / len)
          c = (N.x d.x + N.y d.y) + N.z d.z
          e = (c + N.z) / (1 + d.z)
          n_view = (N.x - e d.x, N.y - e d.y, (N.z - e (d.z + 1)) + 2 c)
      It keeps |N|, its z is N . d, it varies smoothly over the surface (both gates interpolate normals) and for k = 0 it is
      N itself (taken as such, so that not even the sign of a zero changes).  n_view is a constant of the backward pass, as
      the gates' inputs already are; the generator still receives the camera-space normals.
  backward, with g' the gradient of v':
          u = (x' gx' + y' gy') + z' gz';  t = u / q
          g = (gx' / q, gy' / q, gz' / q + k t)     without k t where clamped
          gkappa[b] = sum_i z_i t_i                  a clamped vertex adds 0

CPU tensors and float64 take the torch composite below, which is the definition and is differentiable twice
(create_graph=True).  Float32 device tensors take sr_camera_fwd / sr_camera_bwd through the C ABI: one launch each way for
the batch, nothing allocated by the launch and nothing read back, so both can be captured.  v', n_view and gv are the host
float32 composite's bit for bit.  gkappa is a fixed-order sum (no atomics; reruns are bit-identical): a lane of the row's
1024-lane workgroup adds the float32 terms z_i t_i of its items in index order, then a tree of depth 10; against the exact
sum of those terms it is within (`bwd_terms_per_lane(nv)` + 10) 2^-24 sum_i |z_i t_i| to first order.  Under
SR_STRICT_NATIVE=1 nothing falls to a library: a device tensor the kernels do not take (float64) raises.

Not built: a principal-point offset (the crop is assumed centred on the optical axis), lens distortion, and
perspective-correct interpolation inside a triangle: the consumers interpolate attributes linearly in the projected
triangle, where a true perspective rasterizer's weights are b_i = (a_i / q_i) / sum_j a_j / q_j; the two differ by at most
(q_max - q_min) / q_min over the triangle's corners.
"""
import torch

from ._dispatch import is_device_tensor, native, strict_native
from .texture import _div, _sqrt

QMIN = 1.0 / 16.0
# the layout of sr_camera_bwd's sum: lanes per row, vertices per aligned group, the tree's depth
BWD_BLOCK = 1024
GROUP = 4
TREE_DEPTH = 10


def bwd_terms_per_lane(nv, row=0, aligned=True):
    """How many terms the busiest lane of sr_camera_bwd adds for row `row` of a [B, nv, 3] tensor (aligned: the tensors'
    base addresses are 16-byte aligned, as torch's allocations are).  The row's first (-nv row) mod 4 and last vertices
    outside an aligned group of four are items of one vertex, a group is one item of four; lane l takes items l,
    l + 1024, ..., the groups first."""
    nv = int(nv)
    if not aligned:
        return -(-nv // BWD_BLOCK)
    head = min((GROUP - (nv * int(row)) % GROUP) % GROUP, nv)
    groups = (nv - head) // GROUP
    singles = nv - GROUP * groups
    terms = [0] * BWD_BLOCK
    full, rest = divmod(groups, BWD_BLOCK)
    for lane in range(BWD_BLOCK):
        terms[lane] = GROUP * (full + (1 if lane < rest else 0))
    for j in range(groups, groups + singles):
        terms[j % BWD_BLOCK] += 1
    return max(terms)


def _check(v, kappa, normals):
    if v.dim() != 3 or v.shape[2] != 3 or not v.is_floating_point():
        raise ValueError("project: v must be a floating-point [B, nv, 3], got %s %s" % (v.dtype, tuple(v.shape)))
    if not isinstance(kappa, torch.Tensor) or tuple(kappa.shape) != (v.shape[0],) or kappa.dtype != v.dtype or (
            kappa.device != v.device):
        raise ValueError("project: kappa must be a [%d] tensor of v's float type and device, got %s"
                         % (v.shape[0], "%s %s on %s" % (kappa.dtype, tuple(kappa.shape), kappa.device)
                            if isinstance(kappa, torch.Tensor) else type(kappa).__name__))
    if normals is not None and (tuple(normals.shape) != tuple(v.shape) or normals.dtype != v.dtype
                                or normals.device != v.device):
        raise ValueError("project: normals must be v's shape, float type and device, got %s %s"
                         % (normals.dtype, tuple(normals.shape)))


# ---- the definition ----------------------------------------------------------------------------------------------------
def _depth(v, kappa):
    """(q [B, nv], clamped bool [B, nv])."""
    q0 = 1.0 - kappa.view(-1, 1) * v[..., 2]
    clamped = q0 < QMIN
    return torch.where(clamped, torch.full_like(q0, QMIN), q0), clamped


def _forward(v, kappa):
    q, _ = _depth(v, kappa)
    return _div(v, q.unsqueeze(-1))


def view_normals(vp, kappa, normals):
    """n_view of the projected vertices vp = v', the definition."""
    k = kappa.view(-1, 1)
    nx, ny, nz = normals[..., 0], normals[..., 1], normals[..., 2]
    ax, ay = k * vp[..., 0], k * vp[..., 1]
    length = _sqrt(1.0 + (ax * ax + ay * ay))
    dx, dy, dz = _div(-ax, length), _div(-ay, length), _div(torch.ones_like(length), length)
    c = (nx * dx + ny * dy) + nz * dz
    e = _div(c + nz, 1.0 + dz)
    out = torch.stack((nx - e * dx, ny - e * dy, (nz - e * (dz + 1.0)) + 2.0 * c), -1)
    return torch.where((k == 0).unsqueeze(-1), normals, out)


def _backward(v, kappa, g):
    """(gv [B, nv, 3], terms [B, nv]): the gradient of v and the terms z_i t_i of gkappa, of the gradient g of v'."""
    q, clamped = _depth(v, kappa)
    qe = q.unsqueeze(-1)
    vp = _div(v, qe)
    u = (vp[..., 0] * g[..., 0] + vp[..., 1] * g[..., 1]) + vp[..., 2] * g[..., 2]
    t = _div(u, q)
    gv = _div(g, qe)
    gz = torch.where(clamped, gv[..., 2], gv[..., 2] + kappa.view(-1, 1) * t)
    terms = torch.where(clamped, torch.zeros_like(t), v[..., 2] * t)
    return torch.stack((gv[..., 0], gv[..., 1], gz), -1), terms


class _ProjectComposite(torch.autograd.Function):
    """The definition as an autograd node: its backward is the stated formula in torch operations (not what autograd would
    derive from the forward, which rounds differently), so it can be differentiated again."""

    @staticmethod
    def forward(ctx, v, kappa, normals):
        ctx.set_materialize_grads(False)                 # (no zeros made for n_view's absent gradient)
        ctx.save_for_backward(v, kappa)
        vp = _forward(v, kappa)
        if normals is None:
            return vp
        n_view = view_normals(vp, kappa, normals)
        ctx.mark_non_differentiable(n_view)
        return vp, n_view

    @staticmethod
    def backward(ctx, g, *_):
        if g is None:
            return None, None, None
        v, kappa = ctx.saved_tensors
        gv, terms = _backward(v, kappa, g)
        return gv, terms.sum(1), None


def project_composite(v, kappa, normals=None):
    """The defining tensor algebra, in v's float type."""
    _check(v, kappa, normals)
    return _ProjectComposite.apply(v, kappa, None if normals is None else normals.detach())


def kappa_terms(v, kappa, g):
    """The terms z_i t_i [B, nv] that gkappa sums, in v's float type (tests: the bound on the kernel's sum)."""
    with torch.no_grad():
        return _backward(v, kappa, g)[1]


# ---- the kernels -------------------------------------------------------------------------------------------------------
def native_ok(*tensors):
    return all(is_device_tensor(t) and t.dtype == torch.float32 for t in tensors if t is not None)


class _ProjectNative(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, kappa, normals, gkappa_out):
        ctx.gkappa_out = gkappa_out
        ctx.set_materialize_grads(False)                 # (no zeros made, and no launch, for n_view's absent gradient)
        vc, kc = v.contiguous(), kappa.contiguous()
        nc = None if normals is None else normals.contiguous()
        b, nv = int(vc.shape[0]), int(vc.shape[1])
        vp = torch.empty_like(vc)
        n_view = None if nc is None else torch.empty_like(nc)
        native(vc).sr_camera_fwd(vp, n_view, vc, nc, kc, b, nv)
        ctx.save_for_backward(vc, kc, vp)
        if n_view is None:
            return vp
        ctx.mark_non_differentiable(n_view)
        return vp, n_view

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, *_):
        if g is None:
            return None, None, None, None
        vc, kc, vp = ctx.saved_tensors
        g = g.contiguous()
        b, nv = int(vc.shape[0]), int(vc.shape[1])
        gv = torch.empty_like(vc)
        gk = ctx.gkappa_out
        if gk is None and ctx.needs_input_grad[1]:
            gk = torch.empty_like(kc)
        native(vc).sr_camera_bwd(gv, gk, vc, vp, g, kc, b, nv)
        return gv, (None if ctx.gkappa_out is not None else gk), None, None


def project(v, kappa, normals=None, gkappa_out=None):
    """v' [B, nv, 3] of the posed mesh v [B, nv, 3] seen by a camera with kappa [B] = 1 / distance (the module's note), or
    (v', n_view) when normals [B, nv, 3] are given.  Differentiable in v and kappa; n_view carries no gradient.  Device
    float32 runs sr_camera_fwd / sr_camera_bwd, one launch each way; everything else `project_composite`.
    gkappa_out (kernels only): a contiguous float32 device buffer of at least B elements; the backward launch writes gkappa
    into its first B elements and kappa receives no gradient through autograd (an optimiser that reads its gradients from a
    buffer of its own, inversion.LatentInverter's, then needs no copy)."""
    _check(v, kappa, normals)
    kernels = native_ok(v, kappa, normals) and v.shape[0] > 0 and v.shape[1] > 0
    if gkappa_out is not None and not (kernels and native_ok(gkappa_out) and gkappa_out.is_contiguous()
                                       and gkappa_out.numel() >= v.shape[0] and gkappa_out.device == v.device):
        raise ValueError("project: gkappa_out is for the kernels: float32 device tensors and a contiguous float32 buffer of "
                         "at least B elements on their device")
    if not kernels:
        if is_device_tensor(v) and strict_native():
            raise RuntimeError("project: SR_STRICT_NATIVE=1 and the kernels take float32 device tensors only")
        return project_composite(v, kappa, normals)
    return _ProjectNative.apply(v, kappa, None if normals is None else normals.detach(), gkappa_out)
