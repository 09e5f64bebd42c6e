"""Shared skeleton of the posed-mesh nodes of face reconstruction (op/morph.py, op/skin.py, op/blend.py): the argument
handling and native / composite dispatch all three repeat, the composite pose, and the forward and backward halves that
the morphable and the blendshape node have in common — everything around the one model-specific contraction each way."""
import torch

from .. import utils_3d
from ._dispatch import native, strict_native

EPS = 1e-8


def as_batch(coeff, pose, name):
    """coeff [d] -> [1, d], pose [7] -> [1, 7]; one pose per coefficient vector."""
    if coeff.dim() == 1:
        coeff = coeff.view(1, -1)
    if pose.dim() == 1:
        pose = pose.view(1, 7)
    if pose.shape[0] != coeff.shape[0]:
        raise ValueError("%s: %d coefficient vectors but %d poses" % (name, coeff.shape[0], pose.shape[0]))
    return coeff, pose


def native_ok(tensors, model_tensors):
    """The kernels take device fp32 throughout and a frozen model."""
    return (all(t.device.type == "cuda" and t.dtype == torch.float32 for t in tuple(tensors) + tuple(model_tensors))
            and not any(t.requires_grad for t in model_tensors))


def refuse_composite(kind, tensors, model_tensors):
    """Under SR_STRICT_NATIVE=1 a device tensor never falls to the composite (library matmul) silently.  (morph_mesh has
    never had this guard and does not call it: giving it one is a change of behaviour.)"""
    if strict_native() and any(t.device.type == "cuda" for t in tuple(tensors) + tuple(model_tensors)):
        raise RuntimeError("SR_STRICT_NATIVE: the %s node takes device fp32 tensors and a frozen model on the "
                           "device; this call (%s, learnable=%s) would run the composite on library GEMMs"
                           % (kind, ", ".join(str(t.dtype) + "@" + t.device.type for t in tensors),
                              any(t.requires_grad for t in model_tensors)))


def pose_composite(vs, pose, tri):
    """(v, n): the unposed vertices vs [B, nv, 3] under pose [B, 7], and their normals, as tensor algebra."""
    lin = torch.exp(pose[:, 6]).view(-1, 1, 1) * utils_3d.euler_mat(pose[:, :3], "yxz")
    v = torch.matmul(vs, lin) + pose[:, 3:6].view(-1, 1, 3)
    return v, utils_3d.mesh_point_normal(v, tri)


def forward(c, p, tri, nv, model_fwd):
    """The forward of a node whose model is a contraction with the pose as its epilogue: pose matrices, then
    `model_fwd(run, v, vs, reg, lin)` (its launches write the posed vertices v, the unposed vs and the prior reg), the
    vertex-normal gather of the unposed shape and its rotation.  Returns (v, n, reg, mesh, what model_fwd returned): mesh
    is the tensors `backward` takes, to be saved by the node."""
    b = c.shape[0]
    off, adj, _ = utils_3d.incidence_lists(tri, nv)
    tric = tri.contiguous()
    dev, f32 = c.device, c.dtype
    lin = torch.empty((b, 3, 3), dtype=f32, device=dev)
    rot = torch.empty_like(lin)
    vs = torch.empty((b, nv, 3), dtype=f32, device=dev)
    v = torch.empty_like(vs)
    ns = torch.empty_like(vs)
    n = torch.empty_like(vs)
    normc = torch.empty((b, nv), dtype=f32, device=dev)
    reg = torch.empty((), dtype=f32, device=dev)
    run = native(c)
    run.sr_pose_batch_fwd(lin, rot, p, b)
    kept = model_fwd(run, v, vs, reg, lin)
    run.sr_vertex_normals_f32(ns, normc, vs, tric, off, adj, b, nv, tric.size(0), EPS)
    run.sr_affine3_fwd(n, ns, rot, None, b, nv, nv * 3)
    return v, n, reg, (p, tric, off, adj, lin, rot, vs, ns, normc), kept


def backward(needs, mesh, gv, gn, model_bwd):
    """(gcoeff, gpose) of that node, each None unless `needs` (ctx.needs_input_grad) asks for it: the vertex-normal
    adjoint gather into gvs and `model_bwd(run, gvs)` -> gcoeff; the two pose sums and the pose gradient."""
    p, tric, off, adj, lin, rot, vs, ns, normc = mesh
    b, nv = vs.shape[:2]
    gv, gn = gv.contiguous(), gn.contiguous()
    run = native(p)
    gcoeff = gpose = None
    if needs[0]:
        gvs = torch.empty_like(vs)
        run.sr_vertex_normals_bwd_f32(gvs, gv, gn, lin, rot, vs, ns, normc, tric, off, adj, b, nv, tric.size(0), EPS)
        gcoeff = model_bwd(run, gvs)
    if needs[1]:
        glin = torch.empty_like(lin)
        grot = torch.empty_like(rot)
        gt = torch.empty((b, 3), dtype=p.dtype, device=p.device)
        gpose = torch.empty_like(p)
        run.sr_affine3_bwd(glin, gt, vs, gv, b, nv, nv * 3)
        run.sr_affine3_bwd(grot, None, ns, gn, b, nv, nv * 3)
        run.sr_morph_pose_bwd(gpose, glin, grot, gt, p, b)
    return gcoeff, gpose
