"""Morphable-mesh node of face reconstruction: 3DMM coefficients and a rigid pose -> posed vertices, normals and the
coefficient prior, in one autograd node (csrc/morph.hip).

    v   = (fc.bias + fc.weight @ coeff[b]).view(nv, 3) @ (exp(s) R(yaw, pitch, roll)) + (tx, ty, tz)
    n   = mesh_point_normal(v, tri)
    reg = reg_weight * model.regulation(coeff)

with the reference's definitions (face_model.py:71-74 LinearMorphableModel.forward / regulation, utils_3d.py euler_mat
"yxz", mesh_point_normal) and the inverter's pose convention pose [B, 7] = (yaw, pitch, roll, tx, ty, tz, log-scale).

Device fp32 with a frozen model: four launches forward (pose matrices, one streaming pass over fc.weight for all B,
the vertex-normal gather of the unposed shape, its rotation — the scale is uniform and positive, so the normals of the
posed mesh are the rotated normals up to rounding) and six backward (the vertex-normal adjoint gather, the split-K
coefficient gradient in two passes, the pose sums and the pose gradient).  No library GEMM, no atomics: reruns are
bit-identical.  First order only.  Anything else (CPU tensors, float64, a trainable basis) is the composite tensor
algebra, which is also the definition the kernels are tested against.
"""
import torch
from torch.autograd import Function

from .. import _lib, utils_3d
from ._dispatch import on_device_of, stream_of

EPS = 1e-8


def _sigma(model, like):
    return model.sigma.detach().to(device=like.device, dtype=like.dtype)


def morph_composite(coeff, pose, weight, bias, sigma, tri, reg_weight=0.0):
    """The defining tensor algebra (coeff [B, d], pose [B, 7])."""
    b = coeff.shape[0]
    vs = torch.nn.functional.linear(coeff, weight, bias).view(b, -1, 3)
    lin = torch.exp(pose[:, 6]).view(-1, 1, 1) * utils_3d.euler_mat(pose[:, :3], "yxz")
    v = torch.matmul(vs, lin) + pose[:, 3:6].view(-1, 1, 3)
    n = utils_3d.mesh_point_normal(v, tri)
    reg = reg_weight * ((coeff / sigma.view(1, -1)) ** 2).sum()
    return v, n, reg


class _Morph(Function):
    @staticmethod
    def forward(ctx, coeff, pose, weight, bias, sigma, tri, reg_weight):
        c, p = coeff.contiguous(), pose.contiguous()
        w, bs, sg = weight.contiguous(), bias.contiguous(), sigma.contiguous()
        b, d = c.shape
        nv = bs.numel() // 3
        off, adj, _ = utils_3d.incidence_lists(tri, nv)
        tric = tri.contiguous()
        nf = tric.size(0)
        dev, f32 = c.device, c.dtype
        lin = torch.empty((b, 3, 3), dtype=f32, device=dev)
        rot = torch.empty_like(lin)
        vs = torch.empty((b, nv, 3), dtype=f32, device=dev)
        v = torch.empty_like(vs)
        ns = torch.empty_like(vs)
        n = torch.empty_like(vs)
        normc = torch.empty((b, nv), dtype=f32, device=dev)
        reg = torch.empty((), dtype=f32, device=dev)
        L = _lib.lib()
        st = stream_of(c)
        ptr = _lib.ptr
        with on_device_of(c):
            _lib.check(L.sr_pose_batch_fwd(ptr(lin), ptr(rot), ptr(p), b, st), "sr_pose_batch_fwd")
            _lib.check(L.sr_morph_fwd(ptr(v), ptr(vs), ptr(reg), ptr(w), ptr(bs), ptr(c), ptr(lin), ptr(p), ptr(sg),
                                      float(reg_weight), b, nv, d, st), "sr_morph_fwd")
            _lib.check(L.sr_vertex_normals_f32(ptr(ns), ptr(normc), ptr(vs), ptr(tric), ptr(off), ptr(adj), b, nv, nf,
                                               EPS, st), "sr_vertex_normals_f32")
            _lib.check(L.sr_affine3_fwd(ptr(n), ptr(ns), ptr(rot), None, b, nv, nv * 3, st), "sr_affine3_fwd")
        ctx.save_for_backward(c, p, w, sg, tric, off, adj, lin, rot, vs, ns, normc)
        ctx.reg_weight = float(reg_weight)
        return v, n, reg

    @staticmethod
    def backward(ctx, gv, gn, greg):
        c, p, w, sg, tric, off, adj, lin, rot, vs, ns, normc = ctx.saved_tensors
        b, d = c.shape
        nv = vs.shape[1]
        gv, gn, greg = gv.contiguous(), gn.contiguous(), greg.contiguous()
        L = _lib.lib()
        st = stream_of(c)
        ptr = _lib.ptr
        gcoeff = gpose = None
        with on_device_of(c):
            if ctx.needs_input_grad[0]:
                gvs = torch.empty_like(vs)
                _lib.check(L.sr_vertex_normals_bwd_f32(ptr(gvs), ptr(gv), ptr(gn), ptr(lin), ptr(rot), ptr(vs), ptr(ns),
                                                       ptr(normc), ptr(tric), ptr(off), ptr(adj), b, nv, tric.size(0),
                                                       EPS, st), "sr_vertex_normals_bwd_f32")
                scratch = torch.empty(max(1, int(L.sr_morph_gcoeff_scratch_floats(3 * nv, b, d))), dtype=c.dtype,
                                      device=c.device)
                gcoeff = torch.empty_like(c)
                _lib.check(L.sr_morph_gcoeff(ptr(gcoeff), ptr(scratch), ptr(w), ptr(gvs), ptr(c), ptr(sg),
                                             ctx.reg_weight, ptr(greg), b, 3 * nv, d, st), "sr_morph_gcoeff")
            if ctx.needs_input_grad[1]:
                glin = torch.empty_like(lin)
                grot = torch.empty_like(rot)
                gt = torch.empty((b, 3), dtype=c.dtype, device=c.device)
                gpose = torch.empty_like(p)
                _lib.check(L.sr_affine3_bwd(ptr(glin), ptr(gt), ptr(vs), ptr(gv), b, nv, nv * 3, st), "sr_affine3_bwd")
                _lib.check(L.sr_affine3_bwd(ptr(grot), None, ptr(ns), ptr(gn), b, nv, nv * 3, st), "sr_affine3_bwd")
                _lib.check(L.sr_morph_pose_bwd(ptr(gpose), ptr(glin), ptr(grot), ptr(gt), ptr(p), b, st),
                           "sr_morph_pose_bwd")
        return gcoeff, gpose, None, None, None, None, None


def _native_ok(coeff, pose, weight, bias):
    ts = (coeff, pose, weight, bias)
    return (all(t.device.type == "cuda" and t.dtype == torch.float32 for t in ts)
            and not weight.requires_grad and not bias.requires_grad)


def morph_mesh(model, coeff, pose, tri, reg_weight=0.0):
    """(v [B, nv, 3], n [B, nv, 3], reg []) of a LinearMorphableModel at coefficients coeff [B, d] (or [d]) and poses
    pose [B, 7] (or [7]); reg = reg_weight * model.regulation(coeff)."""
    if coeff.dim() == 1:
        coeff = coeff.view(1, -1)
    if pose.dim() == 1:
        pose = pose.view(1, 7)
    if pose.shape[0] != coeff.shape[0]:
        raise ValueError("morph_mesh: %d coefficient vectors but %d poses" % (coeff.shape[0], pose.shape[0]))
    weight, bias = model.fc.weight, model.fc.bias
    sigma = _sigma(model, coeff)
    if _native_ok(coeff, pose, weight, bias):
        return _Morph.apply(coeff, pose, weight.detach(), bias.detach(), sigma, tri, float(reg_weight))
    return morph_composite(coeff, pose, weight, bias, sigma, tri, reg_weight)


def vertex_normals_backward(v, tri, g):
    """Gradient w.r.t. v [B, nv, 3] of <g, mesh_point_normal(v, tri)> by the device gather (k_vertex_normals_bwd),
    no pose: the kernel behind the node's backward, exposed for tests and measurements."""
    vc, gc = v.contiguous(), g.contiguous()
    b, nv, _ = vc.shape
    off, adj, _ = utils_3d.incidence_lists(tri, nv)
    tric = tri.contiguous()
    ns = torch.empty_like(vc)
    normc = torch.empty((b, nv), dtype=vc.dtype, device=vc.device)
    out = torch.empty_like(vc)
    L = _lib.lib()
    st = stream_of(vc)
    ptr = _lib.ptr
    with on_device_of(vc):
        _lib.check(L.sr_vertex_normals_f32(ptr(ns), ptr(normc), ptr(vc), ptr(tric), ptr(off), ptr(adj), b, nv,
                                           tric.size(0), EPS, st), "sr_vertex_normals_f32")
        _lib.check(L.sr_vertex_normals_bwd_f32(ptr(out), None, ptr(gc), None, None, ptr(vc), ptr(ns), ptr(normc),
                                               ptr(tric), ptr(off), ptr(adj), b, nv, tric.size(0), EPS, st),
                   "sr_vertex_normals_bwd_f32")
    return out
