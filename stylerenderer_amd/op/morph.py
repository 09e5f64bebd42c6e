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
from . import _mesh_node
from ._dispatch import native
from ._mesh_node import EPS


def _sigma(model, like):
    return model.sigma.detach().to(device=like.device, dtype=like.dtype)


def morph_composite(coeff, pose, weight, bias, sigma, tri, reg_weight=0.0):
    """The defining tensor algebra (coeff [B, d], pose [B, 7])."""
    vs = torch.nn.functional.linear(coeff, weight, bias).view(coeff.shape[0], -1, 3)
    v, n = _mesh_node.pose_composite(vs, pose, tri)
    reg = reg_weight * ((coeff / sigma.view(1, -1)) ** 2).sum()
    return v, n, reg


class _Morph(Function):
    @staticmethod
    def forward(ctx, coeff, pose, weight, bias, sigma, tri, reg_weight):
        c, p = coeff.contiguous(), pose.contiguous()
        w, bs, sg = weight.contiguous(), bias.contiguous(), sigma.contiguous()
        b, d = c.shape
        nv = bs.numel() // 3

        def model_fwd(run, v, vs, reg, lin):
            run.sr_morph_fwd(v, vs, reg, w, bs, c, lin, p, sg, float(reg_weight), b, nv, d)

        v, n, reg, mesh, _ = _mesh_node.forward(c, p, tri, nv, model_fwd)
        ctx.save_for_backward(c, w, sg, *mesh)
        ctx.reg_weight, ctx.rows = float(reg_weight), 3 * nv
        return v, n, reg

    @staticmethod
    def backward(ctx, gv, gn, greg):
        c, w, sg, *mesh = ctx.saved_tensors
        (b, d), rows = c.shape, ctx.rows
        greg = greg.contiguous()

        def model_bwd(run, gvs):
            scratch = torch.empty(max(1, int(_lib.lib().sr_morph_gcoeff_scratch_floats(rows, b, d))), dtype=c.dtype,
                                  device=c.device)
            gcoeff = torch.empty_like(c)
            run.sr_morph_gcoeff(gcoeff, scratch, w, gvs, c, sg, ctx.reg_weight, greg, b, rows, d)
            return gcoeff

        return _mesh_node.backward(ctx.needs_input_grad, mesh, gv, gn, model_bwd) + (None,) * 5


def morph_mesh(model, coeff, pose, tri, reg_weight=0.0):
    """(v [B, nv, 3], n [B, nv, 3], reg []) of a LinearMorphableModel at coefficients coeff [B, d] (or [d]) and poses
    pose [B, 7] (or [7]); reg = reg_weight * model.regulation(coeff)."""
    coeff, pose = _mesh_node.as_batch(coeff, pose, "morph_mesh")
    weight, bias = model.fc.weight, model.fc.bias
    sigma = _sigma(model, coeff)
    if _mesh_node.native_ok((coeff, pose), (weight, bias)):
        return _Morph.apply(coeff, pose, weight.detach(), bias.detach(), sigma, tri, float(reg_weight))
    # (no strict-native guard here, unlike skin_mesh and blend_mesh: see _mesh_node.refuse_composite)
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
    run = native(vc)
    run.sr_vertex_normals_f32(ns, normc, vc, tric, off, adj, b, nv, tric.size(0), EPS)
    run.sr_vertex_normals_bwd_f32(out, None, gc, None, None, vc, ns, normc, tric, off, adj, b, nv, tric.size(0), EPS)
    return out
