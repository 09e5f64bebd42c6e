"""Skinning node of face reconstruction: shape coefficients, joint rotations and a rigid pose -> posed vertices, normals
and the coefficient prior of a LinearBlendSkinningModel (FLAME), in one autograd node (csrc/skin.hip).

With coeff [B, ds + 3 (nj-1)] = (beta, one axis-angle theta_i per non-root joint), pose [B, 7] = (yaw, pitch, roll, tx,
ty, tz, log-scale), S the stacked basis [ds + 9 (nj-1), 3 nv], row vectors throughout (reference face_model.py:313-341):

    v_shaped = v_template + S[:ds]^T beta               J = Jreg v_shaped               R_i = rodrigues(theta_i)
    v_posed  = v_shaped + S[ds:]^T vec(R - I)
    chain    root: T = [I; J_root]     child c of p: T_c = [R_c^T A_p ; (J_c - J_p) A_p + t_p]
    v_skin[k] = sum_i W[k, i] ((v_posed[k] - J_i) A_i + t_i)
    v   = v_skin (exp(s) R(yaw, pitch, roll)) + (tx, ty, tz)
    n   = mesh_point_normal(v, tri)
    reg = reg_weight * model.regulation(coeff)

Device fp32 with a frozen model: three launches forward (the joint kernel: Rodrigues, regressed joints, chain, the global
pose folded into the joints' transforms and the prior, for all B; one streaming pass over S with the blend as its
epilogue; the vertex-normal gather) and five backward (the vertex-normal adjoint gather, the blend's backward with stage
one of the per-joint sums, the split-K coefficient gradient of op.morph over S in two passes, the joint adjoint).  No
library GEMM, no scatter, no atomics: reruns are bit-identical.  First order only.  `Jreg v_template`, `Jreg S[:ds]^T`
and the transposed basis are prepared once per frozen model and cached like the incidence lists.  Anything else (CPU
tensors, float64, learnable=True) is the composite tensor algebra, which is also what the kernels are tested against.
"""
import torch
from torch.autograd import Function

from .. import _lib, utils_3d
from . import _mesh_node
from ._dispatch import DerivedCache, native
from ._mesh_node import EPS
_PREP_CACHE = DerivedCache(4)


def lbs_composite(x, basis, template, weights, regressor, parent, ds):
    """v_skin [B, nv, 3] of the definition above (no global pose)."""
    b = x.shape[0]
    nv = template.numel() // 3
    nj = regressor.shape[0]
    npose = len(parent)
    v_shaped = torch.matmul(x[:, :ds], basis[:ds]) + template.view(1, -1)
    rot = utils_3d.rodrigues(x[:, ds:].reshape(-1, 3)).view(b, npose, 3, 3)
    joints = torch.matmul(regressor.unsqueeze(0), v_shaped.view(b, nv, 3))
    eye = torch.eye(3, dtype=x.dtype, device=x.device)
    v_posed = (torch.matmul((rot - eye).reshape(b, npose * 9), basis[ds:]) + v_shaped).view(b, nv, 3)
    lin = [eye.expand(b, 3, 3) for _ in range(nj - npose)]
    off = [joints[:, i:i + 1] for i in range(nj - npose)]
    for i, p in enumerate(parent):
        p, c = int(p), len(lin)
        off.append(torch.matmul(joints[:, c:c + 1] - joints[:, p:p + 1], lin[p]) + off[p])
        lin.append(torch.matmul(rot[:, i].transpose(1, 2), lin[p]))
    v = None
    for i in range(nj):
        term = weights[:, i].view(1, -1, 1) * (torch.matmul(v_posed - joints[:, i:i + 1], lin[i]) + off[i])
        v = term if v is None else v + term
    return v


def skin_composite(model, coeff, pose, tri, reg_weight=0.0):
    """The defining tensor algebra of the node (coeff [B, dc], pose [B, 7])."""
    dt = coeff.dtype
    basis, template = (t.to(dt) for t in model.fc)
    weights, regressor = (t.to(dt) for t in model.weight)
    vs = lbs_composite(coeff, basis, template, weights, regressor, model.parent, model.dim[0])
    v, n = _mesh_node.pose_composite(vs, pose, tri)
    return v, n, reg_weight * model.regulation(coeff)


def prepared(model):
    """(S^T [3 nv, D], Jreg v_template [nj, 3], Jreg S[:ds]^T [3 nj, ds]) of a frozen model, built once (plain tensor
    algebra accumulated in float64, outside the per-step path) and cached on the arrays' addresses and versions.
    The transposed basis is a second copy of the model's largest array (53.5 MB at nv = 24 770, D = 180; about 90 MB for
    FLAME itself) that lives as long as the cache entry.  sigma and pose_inv are not part of the key: they are passed to
    the kernels live on every call."""
    basis, template = model.fc
    weights, regressor = model.weight
    key = tuple((t.data_ptr(), tuple(t.shape), t._version, str(t.device)) for t in (basis, template, regressor))
    hit = _PREP_CACHE.get(key)
    if hit is not None:
        return hit[:3]
    with torch.no_grad():
        ds, nv, nj = model.dim[0], model.dim[2] // 3, regressor.shape[0]
        st = basis.t().contiguous()
        jr = regressor.double()
        j0 = torch.matmul(jr, template.double().view(nv, 3)).float().contiguous()
        # js[3 j + axis, k] = sum_v Jreg[j, v] S[k, 3 v + axis]
        js = torch.einsum("jv,kva->jak", jr, basis[:ds].double().view(ds, nv, 3)).reshape(3 * nj, ds).float().contiguous()
    # the sources are held so that their addresses cannot be reused
    return _PREP_CACHE.put(key, (st, j0, js, basis, template, regressor))[:3]


class _Skin(Function):
    @staticmethod
    def forward(ctx, coeff, pose, st, template, weights, j0, js, parent, sigma, pose_inv, tri, reg_weight):
        c = coeff.contiguous()
        p = pose.contiguous() if pose is not None else None
        b = c.shape[0]
        nv = template.numel() // 3
        nj = j0.shape[0]
        npose = parent.numel()
        ds = c.shape[1] - 3 * npose
        dfull = ds + 9 * npose
        dev, f32 = c.device, c.dtype
        cx = torch.empty((b, dfull), dtype=f32, device=dev)
        tg = torch.empty((b, nj, 12), dtype=f32, device=dev)
        chain = torch.empty((b, nj, 15), dtype=f32, device=dev)
        reg = torch.empty((), dtype=f32, device=dev)
        vp = torch.empty((b, nv, 3), dtype=f32, device=dev)
        v = torch.empty_like(vp)
        run = native(c)
        run.sr_skin_joints_fwd(cx, tg, chain, reg, c, p, j0, js, parent, sigma, pose_inv, float(reg_weight), b, nj,
                               nj - npose, ds)
        run.sr_skin_fwd(v, vp, st, template, cx, weights, tg, b, nv, dfull, nj)
        if tri is not None:
            off, adj, _ = utils_3d.incidence_lists(tri, nv)
            tric = tri.contiguous()
            n = torch.empty_like(v)
            normc = torch.empty((b, nv), dtype=f32, device=dev)
            run.sr_vertex_normals_f32(n, normc, v, tric, off, adj, b, nv, tric.size(0), EPS)
        else:
            tric = off = adj = n = normc = None
        ctx.with_normals = tri is not None
        ctx.with_pose = p is not None
        ctx.reg_weight = float(reg_weight)
        ctx.sizes = (b, nv, nj, npose, ds, dfull)
        saved = [c, st, weights, js, parent, sigma, pose_inv, cx, tg, chain, vp]
        if ctx.with_pose:
            saved.append(p)
        if ctx.with_normals:
            saved += [tric, off, adj, v, n, normc]
        ctx.save_for_backward(*saved)
        if tri is None:
            ctx.mark_non_differentiable(reg)
            return v, reg
        return v, n, reg

    @staticmethod
    def backward(ctx, gv, *rest):
        saved = list(ctx.saved_tensors)
        c, st, weights, js, parent, sigma, pose_inv, cx, tg, chain, vp = saved[:11]
        k = 11
        p = None
        if ctx.with_pose:
            p = saved[k]
            k += 1
        b, nv, nj, npose, ds, dfull = ctx.sizes
        L = _lib.lib()
        run = native(c)
        gv = gv.contiguous()
        greg = None
        gvn = None
        if ctx.with_normals:
            tric, off, adj, v, n, normc = saved[k:k + 6]
            gn, greg = rest[0].contiguous(), rest[1].contiguous()
            gvn = torch.empty_like(vp)
            run.sr_vertex_normals_bwd_f32(gvn, None, gn, None, None, v, n, normc, tric, off, adj, b, nv, tric.size(0), EPS)
        gvp = torch.empty_like(vp)
        nblk = (nv + 255) // 256
        part = torch.empty(max(1, int(L.sr_skin_bwd_scratch_floats(nv, b, nj))), dtype=c.dtype, device=c.device)
        run.sr_skin_bwd(gvp, part, gv, gvn, vp, weights, tg, b, nv, nj)
        scratch = torch.empty(max(1, int(L.sr_morph_gcoeff_scratch_floats(3 * nv, b, dfull))), dtype=c.dtype,
                              device=c.device)
        gcx = torch.empty_like(cx)
        run.sr_morph_gcoeff(gcx, scratch, st, gvp, cx, None, 0.0, None, b, 3 * nv, dfull)
        gcoeff = torch.empty_like(c)
        gpose = torch.empty_like(p) if (p is not None and ctx.needs_input_grad[1]) else None
        run.sr_skin_joints_bwd(gcoeff, gpose, gcx, part, c, p, chain, js, parent, sigma, pose_inv, ctx.reg_weight, greg, b,
                               nblk, nj, nj - npose, ds)
        return (gcoeff, gpose) + (None,) * 10


def _check(model, coeff):
    if coeff.shape[1] != model.dim[0] + model.dim[1]:
        raise ValueError("skin: %d coefficients, the model takes %d + %d" % (coeff.shape[1], model.dim[0], model.dim[1]))


def skin_vertices(model, x):
    """model.forward: v_skin [B, nv, 3] (no global pose, no normals); the native forward on device fp32 with a frozen
    model."""
    _check(model, x)
    if _mesh_node.native_ok((x,), model.fc + model.weight):
        return _Skin.apply(x, None, *_native_args(model), None, 0.0)[0]
    _mesh_node.refuse_composite("skinning", (x,), model.fc + model.weight)
    dt = x.dtype
    return lbs_composite(x, model.fc[0].to(dt), model.fc[1].to(dt), model.weight[0].to(dt), model.weight[1].to(dt),
                         model.parent, model.dim[0])


def _native_args(model):
    st, j0, js = prepared(model)
    return (st, model.fc[1].detach(), model.weight[0].detach(), j0, js, model._parent,
            model.sigma.detach()[:model.dim[0]].contiguous(), model.pose_inv.detach().contiguous())


def skin_mesh(model, coeff, pose, tri, reg_weight=0.0):
    """(v [B, nv, 3], n [B, nv, 3], reg []) of a LinearBlendSkinningModel at coefficients coeff [B, ds + 3 (nj-1)] (or
    1-D) and poses pose [B, 7] (or [7]); reg = reg_weight * model.regulation(coeff)."""
    coeff, pose = _mesh_node.as_batch(coeff, pose, "skin_mesh")
    _check(model, coeff)
    if _mesh_node.native_ok((coeff, pose), model.fc + model.weight):
        return _Skin.apply(coeff, pose, *_native_args(model), tri, float(reg_weight))
    _mesh_node.refuse_composite("skinning", (coeff, pose), model.fc + model.weight)
    return skin_composite(model, coeff, pose, tri, reg_weight)
