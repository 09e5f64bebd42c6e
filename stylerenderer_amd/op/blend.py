"""Blendshape node of face reconstruction: identity and expression coefficients and a rigid pose -> posed vertices,
normals and the coefficient prior of a BlendShapeModel (FaceWarehouse), in one autograd node (csrc/blend.hip).

With coeff [B, ds + de], pose [B, 7] = (yaw, pitch, roll, tx, ty, tz, log-scale), W = model.weight [ds + 1, de + 1, 3 nv]
(reference face_model.py:128-146):

    xs  = softmax(cat(coeff[:, :ds], -sum coeff[:, :ds]))          xe = cat(1 - sum s, s), s = sigmoid(coeff[:, ds:])
    vs  = sum_ij xs[:, i] xe[:, j] W[i, j].view(nv, 3)
    v   = vs (exp(s) R(yaw, pitch, roll)) + (tx, ty, tz)
    n   = mesh_point_normal(v, tri)
    reg = reg_weight * model.regulation(coeff)

Device fp32 with a frozen model: five launches forward (pose matrices; the head kernel: xs, xe, every sample's prior and
the products z = xs (x) xe for all B; one streaming pass over W for all B with the pose as its epilogue; the vertex-normal
gather of the unposed shape; its rotation) and six backward (the vertex-normal adjoint gather, one streaming pass over W
for gz = W gvs, the tail kernel through the softmax / sigmoid Jacobians with the prior's gradient, the two pose sums and
the pose gradient).  W is used as stored: no transposed copy.  No library GEMM, no atomics: reruns are bit-identical.  First
order only.  The per-sample priors reg_weight * regulation(coeff[b]) of the last native call are the node's fourth,
non-differentiable output (`blend_mesh(..., per_sample=True)`): the batched inverter's per-sample losses take them.
Anything else (CPU tensors, float64, learnable=True) is the composite tensor algebra, which is also what the kernels are
tested against.
"""
import torch
from torch.autograd import Function

from .. import _lib
from . import _mesh_node
from ._dispatch import native


def mixing_weights(x, ds):
    """(xs [B, ds + 1], xe [B, de + 1]): the identity and expression weights of coefficients x [B, ds + de]."""
    xs = torch.softmax(torch.cat((x[:, :ds], -x[:, :ds].sum(1, keepdim=True)), 1), dim=1)
    s = torch.sigmoid(x[:, ds:])
    return xs, torch.cat((1 - s.sum(1, keepdim=True), s), 1)


def blend_vertices_composite(x, weight, ds):
    """vs [B, nv, 3] of the definition above (no pose)."""
    ns, ne, c = weight.shape
    xs, xe = mixing_weights(x, ds)
    z = (xs.unsqueeze(2) * xe.unsqueeze(1)).reshape(-1, ns * ne)
    return torch.matmul(z, weight.reshape(ns * ne, c)).view(-1, c // 3, 3)


def blend_composite(model, coeff, pose, tri, reg_weight=0.0):
    """The defining tensor algebra of the node (coeff [B, ds + de], pose [B, 7])."""
    vs = blend_vertices_composite(coeff, model.weight.to(coeff.dtype), model.dim[0])
    v, n = _mesh_node.pose_composite(vs, pose, tri)
    return v, n, reg_weight * model.regulation(coeff)


def _head(run, c, beta, reg_weight, ds, de):
    b = c.shape[0]
    dev, f32 = c.device, c.dtype
    xs = torch.empty((b, ds + 1), dtype=f32, device=dev)
    xe = torch.empty((b, de + 1), dtype=f32, device=dev)
    prior = torch.empty((b,), dtype=f32, device=dev)
    z = torch.empty((int(_lib.lib().sr_blend_z_floats(b, ds, de)),), dtype=f32, device=dev)
    run.sr_blend_head(xs, xe, prior, z, c, beta, float(reg_weight), b, ds, de)
    return xs, xe, prior, z


class _Blend(Function):
    @staticmethod
    def forward(ctx, coeff, pose, weight, beta, tri, reg_weight):
        c, p = coeff.contiguous(), pose.contiguous()
        w, bt = weight.contiguous(), beta.contiguous()
        b = c.shape[0]
        ds, de, nv = w.shape[0] - 1, w.shape[1] - 1, w.shape[2] // 3

        def model_fwd(run, v, vs, reg, lin):
            xs, xe, prior, z = _head(run, c, bt, reg_weight, ds, de)
            run.sr_blend_fwd(v, vs, reg, w, z, prior, lin, p, b, nv, ds, de)
            return xs, xe, prior

        v, n, reg, mesh, (xs, xe, prior) = _mesh_node.forward(c, p, tri, nv, model_fwd)
        ctx.save_for_backward(w, bt, xs, xe, *mesh)
        ctx.reg_weight = float(reg_weight)
        ctx.dims = (b, ds, de, nv)
        ctx.mark_non_differentiable(prior)
        return v, n, reg, prior

    @staticmethod
    def backward(ctx, gv, gn, greg, _gprior):
        w, bt, xs, xe, *mesh = ctx.saved_tensors
        b, ds, de, nv = ctx.dims
        greg = greg.contiguous()

        def model_bwd(run, gvs):
            gz = torch.empty((b, (ds + 1) * (de + 1)), dtype=gvs.dtype, device=gvs.device)
            run.sr_blend_gz(gz, w, gvs, b, nv, ds, de)
            gcoeff = torch.empty((b, ds + de), dtype=gvs.dtype, device=gvs.device)
            run.sr_blend_tail(gcoeff, gz, xs, xe, bt, ctx.reg_weight, greg, b, ds, de)
            return gcoeff

        return _mesh_node.backward(ctx.needs_input_grad, mesh, gv, gn, model_bwd) + (None,) * 4


class _BlendVertices(Function):
    """The unposed forward alone (two launches) and its coefficient gradient (two)."""

    @staticmethod
    def forward(ctx, coeff, weight, beta):
        c, w, bt = coeff.contiguous(), weight.contiguous(), beta.contiguous()
        b = c.shape[0]
        ds, de, nv = w.shape[0] - 1, w.shape[1] - 1, w.shape[2] // 3
        vs = torch.empty((b, nv, 3), dtype=c.dtype, device=c.device)
        run = native(c)
        xs, xe, _, z = _head(run, c, bt, 0.0, ds, de)
        run.sr_blend_fwd(None, vs, None, w, z, None, None, None, b, nv, ds, de)
        ctx.save_for_backward(w, bt, xs, xe)
        ctx.dims = (b, ds, de, nv)
        return vs

    @staticmethod
    def backward(ctx, gvs):
        w, bt, xs, xe = ctx.saved_tensors
        b, ds, de, nv = ctx.dims
        gvs = gvs.contiguous()
        run = native(gvs)
        gz = torch.empty((b, (ds + 1) * (de + 1)), dtype=gvs.dtype, device=gvs.device)
        gcoeff = torch.empty((b, ds + de), dtype=gvs.dtype, device=gvs.device)
        run.sr_blend_gz(gz, w, gvs, b, nv, ds, de)
        run.sr_blend_tail(gcoeff, gz, xs, xe, bt, 0.0, None, b, ds, de)
        return gcoeff, None, None


def _check(model, coeff):
    if coeff.dim() != 2 or coeff.shape[1] != model.dim[0] + model.dim[1]:
        raise ValueError("blend: coefficients %s, the model takes [B, %d + %d]"
                         % (tuple(coeff.shape), model.dim[0], model.dim[1]))


def blend_vertices(model, x):
    """model.forward: vs [B, nv, 3] (no pose, no normals); the native forward on device fp32 with a frozen model."""
    _check(model, x)
    if _mesh_node.native_ok((x, model.beta), (model.weight,)):
        return _BlendVertices.apply(x, model.weight.detach(), model.beta.detach())
    _mesh_node.refuse_composite("blendshape", (x,), (model.weight,))
    return blend_vertices_composite(x, model.weight.to(x.dtype), model.dim[0])


def prior_rows(model, coeff, reg_weight):
    """[B]: reg_weight * regulation(coeff[b]) of every sample by the defining algebra (regulation is a sum over the batch)."""
    ds, de = model.dim[0], model.dim[1]
    beta = model.beta.to(coeff.dtype)
    ls = torch.cat((coeff[:, :ds], -coeff[:, :ds].sum(1, keepdim=True)), 1)
    xe = coeff[:, ds:]
    bs, be = beta[:ds + 1], beta[ds + 1:].reshape(de, 2)
    return -reg_weight * ((ls * bs).sum(1) - torch.logsumexp(ls, 1) * (bs.sum() - ds - 1) + (xe * be[:, 0] - 1).sum(1)
                          - (torch.nn.functional.softplus(xe) * (be.sum(1) - 2)).sum(1))


def blend_mesh(model, coeff, pose, tri, reg_weight=0.0, per_sample=False):
    """(v [B, nv, 3], n [B, nv, 3], reg []) of a BlendShapeModel at coefficients coeff [B, ds + de] (or 1-D) and poses
    pose [B, 7] (or [7]); reg = reg_weight * model.regulation(coeff).  With per_sample=True a fourth, detached output
    [B] holds reg_weight * regulation(coeff[b]) of every sample (their sum is reg)."""
    coeff, pose = _mesh_node.as_batch(coeff, pose, "blend_mesh")
    _check(model, coeff)
    if _mesh_node.native_ok((coeff, pose, model.beta), (model.weight,)):
        out = _Blend.apply(coeff, pose, model.weight.detach(), model.beta.detach(), tri, float(reg_weight))
        return out if per_sample else out[:3]
    _mesh_node.refuse_composite("blendshape", (coeff, pose), (model.weight,))
    out = blend_composite(model, coeff, pose, tri, reg_weight)
    return out + (prior_rows(model, coeff.detach(), reg_weight),) if per_sample else out
