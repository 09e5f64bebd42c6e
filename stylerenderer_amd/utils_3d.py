"""Mesh front-end of the rasterizer: the three helpers the reference's training loop calls between the
3DMM and GeneratorWithMap (reference train.py:229-230, 250-251, 305-306) — same names and argument
meaning as reference utils_3d.py / layers.py:

    normalize(vec, axis=-1, _type='L2', eps=1e-8)          layers.py:13-53 (Normalize)
    euler_mat(angle, _type='yxz')                          utils_3d.py:43-80
    random_apply_pose3D(p=[...], v=None)                   utils_3d.py:360-378
    mesh_point_normal(v, tri)                              utils_3d.py:379-404
    save_obj(file_name, v, tri, vt, trit, vn, trin)        utils_3d.py:405-444
`save_textured_obj` adds what a textured mesh needs on top of save_obj's records: a material file and its two lines.

`mesh_point_normal` on device tensors runs ONE gather kernel (csrc/mesh.hip, C ABI
sr_vertex_normals_f32) over a per-topology incidence list built once and cached, instead of three
sparse.mm scatters over index tensors rebuilt in Python on every call; it is deterministic and
differentiable (first and higher order through the defining tensor algebra).
"""
import torch
from torch.autograd import Function

from .op._dispatch import DerivedCache, native


def normalize(vec, axis=-1, _type="L2", eps=1e-8):
    eps = abs(eps)
    kind = _type.upper()
    if "L2" in kind:
        norm = torch.sqrt(torch.sum(vec * vec, axis, keepdim=True))
    elif "L1" in kind:
        norm = torch.sum(vec, axis, keepdim=True)              # (sic) the reference sums signed entries
    elif "LINF" in kind:
        norm = torch.max(torch.abs(vec), axis, keepdim=True)[0]
    else:
        raise ValueError("normalize: unknown type %r" % (_type,))
    # the reference's hand-written backward treats the clamp as pass-through: same here
    norm = norm + (torch.clamp(norm, min=eps) - norm).detach()
    return vec / norm


def euler_mat(angle, _type="yxz"):
    """Rotation matrices from Euler angles; axis i of `_type` uses angle[:, i]; later axes multiply
    from the left (T = R_i @ T)."""
    single = angle.dim() == 1
    a = angle.view(1, -1) if single else angle
    c, s = torch.cos(a), torch.sin(a)
    one = torch.ones(len(c), 1, dtype=c.dtype, device=c.device)
    zero = torch.zeros(len(c), 1, dtype=c.dtype, device=c.device)
    T = None
    for i in range(3):
        ci, si = c[:, i:i + 1], s[:, i:i + 1]
        ax = _type[i].lower()
        if ax == "x":
            rows = (one, zero, zero, zero, ci, -si, zero, si, ci)
        elif ax == "y":
            rows = (ci, zero, si, zero, one, zero, -si, zero, ci)
        elif ax == "z":
            rows = (ci, -si, zero, si, ci, zero, zero, zero, one)
        else:
            continue
        R = torch.cat(rows, -1).view(-1, 3, 3)
        T = R if T is None else torch.matmul(R, T)
    return T.view(3, 3) if single else T


def random_apply_pose3D(p=[.5, .1, .05, .1, .1, .1, .15], v=None):
    """p = sigmas of [yaw, pitch, roll, tx, ty, tz, log-scale]; returns the posed vertices
    v @ (scale * R) + t (row-vector convention of the reference), or one 3x4 transform when v is None."""
    batch = len(v) if v is not None and v.dim() >= 3 else 1
    if not isinstance(p, torch.Tensor):
        # sigmas created where the vertices live: the draw below then runs on that device (no host round trip)
        p = torch.tensor([float(x) for x in p], dtype=torch.float32, device=v.device if v is not None else None)
    p = torch.abs(p.reshape(-1)[:7])
    if len(p) < 7:
        p = torch.cat((p, torch.zeros(7 - len(p), dtype=p.dtype, device=p.device)))
    # ~ N(0, diag(p^2)) like the reference's torch.normal(mean=0, std=p[None].expand(batch, -1)) (utils_3d.py:368); drawn as
    # randn * p because torch.normal checks `std >= 0` on the host — a device read hipGraph capture refuses
    z = torch.randn(batch, 7, dtype=p.dtype, device=p.device) * p
    if v is not None and v.device.type == "cuda" and v.dtype == torch.float32 and z.device == v.device:
        # device path: the B scaled rotations in one launch (_pose_batch) and the vertices in one streaming pass
        # (sr_affine3_fwd) instead of ~30 element-wise launches and a 3-wide batched GEMM — this runs twice per training
        # iteration, inside the captured D and G phases
        zc = z.contiguous()
        lin, _ = _pose_batch(zc, with_rot=False)
        return affine3(v[..., :3].reshape(batch, -1, 3), lin, zc[:, 3:6])
    T = torch.cat((torch.exp(z[:, -1]).view(-1, 1, 1) * euler_mat(z[:, :3], "yxz"), z[:, 3:6].view(-1, 3, 1)), -1)
    if v is None:
        return T[0]
    T = T.to(v.device)
    return torch.matmul(v[..., :3].reshape(batch, -1, 3), T[:, :3, :3]) + T[:, :3, 3:].view(-1, 1, 3)


def _pose_batch(pc, with_rot=True):
    """(lin, rot or None), each [B, 3, 3], of contiguous device poses pc [B, 7]: one launch."""
    lin = torch.empty((pc.shape[0], 3, 3), dtype=pc.dtype, device=pc.device)
    rot = torch.empty_like(lin) if with_rot else None
    native(pc).sr_pose_batch_fwd(lin, rot, pc, pc.shape[0])
    return lin, rot


class _Affine3(Function):
    """out[b] = v[b | 0] @ M[b] (+ t[b]) on the device path (csrc/mesh.hip sr_affine3_fwd / _bwd): one streaming pass
    instead of a 3-wide library GEMM; gradients of M and t by fixed-order sums (deterministic), of v by the same pass
    with M^T.  First order only (poses are leaves of the loops that use it)."""

    @staticmethod
    def forward(ctx, v, m, t):
        vc, mc = v.contiguous(), m.contiguous()
        tc = t.contiguous() if t is not None else None
        b, nv = mc.shape[0], vc.shape[-2]
        out = torch.empty((b, nv, 3), dtype=vc.dtype, device=vc.device)
        share = vc.dim() == 2 or vc.shape[0] == 1
        native(vc).sr_affine3_fwd(out, vc, mc, tc, b, nv, 0 if share else nv * 3)
        ctx.save_for_backward(vc, mc)
        ctx.share, ctx.has_t, ctx.v_shape = share, t is not None, tuple(v.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        vc, mc = ctx.saved_tensors
        g = g.contiguous()
        b, nv = mc.shape[0], vc.shape[-2]
        need_v, need_m, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_t and ctx.needs_input_grad[2]
        gm = torch.empty_like(mc) if need_m else None
        gt = torch.empty((b, 3), dtype=g.dtype, device=g.device) if need_t else None
        gv = None
        if need_m or need_t:
            native(g).sr_affine3_bwd(gm, gt, vc, g, b, nv, 0 if ctx.share else nv * 3)
        if need_v:
            gv = torch.empty_like(g)
            mt = mc.transpose(1, 2).contiguous()
            native(g).sr_affine3_fwd(gv, g, mt, None, b, nv, nv * 3)
            if ctx.share:
                gv = gv.sum(0, keepdim=True)
            gv = gv.reshape(ctx.v_shape)
        return gv, gm, gt


class _PoseMatrices(Function):
    """(lin, rot) [1, 3, 3] from pose [7] on the device path (csrc/mesh.hip sr_pose_fwd / _bwd), see `pose_matrices`."""

    @staticmethod
    def forward(ctx, pose):
        pc = pose.contiguous()
        lin = torch.empty((1, 3, 3), dtype=pc.dtype, device=pc.device)
        rot = torch.empty_like(lin)
        native(pc).sr_pose_fwd(lin, rot, pc)
        ctx.save_for_backward(pc)
        return lin, rot

    @staticmethod
    def backward(ctx, glin, grot):
        (pc,) = ctx.saved_tensors
        gp = torch.empty_like(pc)
        gl = glin.contiguous() if glin is not None else None
        gr = grot.contiguous() if grot is not None else None
        native(pc).sr_pose_bwd(gp, gl, gr, pc)
        return gp


class _PoseBatchMatrices(Function):
    """(lin, rot) [B, 3, 3] from pose [B, 7] on the device path: sr_pose_batch_fwd forward, sr_morph_pose_bwd (without
    the translation's gradient, which is affine3's: entries 3..5 are 0) backward, one launch each."""

    @staticmethod
    def forward(ctx, pose):
        pc = pose.contiguous()
        ctx.save_for_backward(pc)
        return _pose_batch(pc)

    @staticmethod
    def backward(ctx, glin, grot):
        (pc,) = ctx.saved_tensors
        gp = torch.empty_like(pc)
        gl = glin.contiguous() if glin is not None else None
        gr = grot.contiguous() if grot is not None else None
        native(pc).sr_morph_pose_bwd(gp, gl, gr, None, pc, pc.shape[0])
        return gp


def pose_matrices(pose):
    """pose [7] = (yaw, pitch, roll, tx, ty, tz, log-scale) -> (lin, rot), each [1, 3, 3]: rot = euler_mat(pose[:3],
    "yxz"), lin = exp(pose[6]) * rot; pose [B, 7] -> [B, 3, 3] each.  Device fp32: one launch forward, one backward
    (first order); otherwise the tensor algebra it stands for."""
    if pose.device.type == "cuda" and pose.dtype == torch.float32:
        if pose.numel() == 7:
            return _PoseMatrices.apply(pose)
        if pose.dim() == 2 and pose.shape[1] == 7:
            return _PoseBatchMatrices.apply(pose)
    if pose.dim() == 2:
        rot = euler_mat(pose[:, :3], "yxz")
        return torch.exp(pose[:, 6]).view(-1, 1, 1) * rot, rot
    rot = euler_mat(pose[:3].view(1, 3), "yxz")
    return torch.exp(pose[6]) * rot, rot


def affine3(v, m, t=None):
    """v [B or 1, nv, 3] @ m [B, 3, 3] + t [B, 3] (row-vector convention of the reference's pose functions)."""
    if v.device.type == "cuda" and v.dtype == torch.float32 and m.dim() == 3:
        return _Affine3.apply(v, m, t)
    out = torch.matmul(v, m)
    return out + t.view(-1, 1, 3) if t is not None else out


# ---- vertex normals -------------------------------------------------------------------------------
_ADJ_CACHE = DerivedCache(16)


def incidence_lists(tri, nv):
    """CSR incidence of a [nf, 3] triangle list: (adj_off [nv+1] int32, adj [3 nf] int32) with the entries
    of vertex i = ascending corner-major indices k*nf + f such that tri[f, k] == i.  Cached per tensor."""
    key = (tri.data_ptr(), tuple(tri.shape), tri._version, str(tri.device), int(nv))
    hit = _ADJ_CACHE.get(key)
    if hit is not None:
        return hit
    flat = tri.t().reshape(-1)                                   # corner-major: index = k*nf + f
    if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= nv):
        raise RuntimeError("mesh_point_normal: triangle index out of range [0, %d)" % nv)
    order = torch.sort(flat, stable=True)[1].to(torch.int32)
    counts = torch.bincount(flat, minlength=nv)
    off = torch.zeros(nv + 1, dtype=torch.int32, device=tri.device)
    off[1:] = torch.cumsum(counts, 0).to(torch.int32)
    # keep `tri` alive: the key holds its address
    return _ADJ_CACHE.put(key, (off, order.contiguous(), tri))


def _normals_composite(v, tri):
    """The defining tensor algebra (reference utils_3d.py:380-404 with index_add in place of sparse.mm)."""
    va, vb, vc = v[:, tri[:, 0]], v[:, tri[:, 1]], v[:, tri[:, 2]]
    fn = torch.cross(vb - va, vc - va, dim=2)
    vn = torch.zeros_like(v[:, :, :3])
    for j in range(3):
        vn = vn + torch.zeros_like(vn).index_add_(1, tri[:, j], fn)
    return normalize(vn)


class _VertexNormals(Function):
    @staticmethod
    def forward(ctx, v, tri):
        vc = v.contiguous()
        b, nv, _ = vc.shape
        off, adj, _ = incidence_lists(tri, nv)
        tric = tri.contiguous()
        out = torch.empty_like(vc)
        native(vc).sr_vertex_normals_f32(out, None, vc, tric, off, adj, b, nv, tric.size(0), 1e-8)
        ctx.save_for_backward(v, tri)
        return out

    @staticmethod
    def backward(ctx, g):
        v, tri = ctx.saved_tensors
        higher = torch.is_grad_enabled()                         # create_graph=True upstream
        with torch.enable_grad():
            vv = v if (higher and v.requires_grad) else v.detach().requires_grad_(True)
            out = _normals_composite(vv, tri)
            (gv,) = torch.autograd.grad(out, vv, g, create_graph=higher)
        return gv, None


def mesh_point_normal(v, tri):
    """Area-weighted, normalised vertex normals [B, nv, 3] of vertices v [B, nv, >=3] and triangles
    tri [nf, 3] (int64)."""
    if v.dim() != 3 or tri.dim() != 2 or tri.size(1) != 3:
        raise ValueError("mesh_point_normal: expected v [B, nv, 3+] and tri [nf, 3]")
    if v.dtype not in (torch.float32, torch.float64):
        raise ValueError("Not supported type")
    if v.device.type == "cuda" and v.dtype == torch.float32:
        return _VertexNormals.apply(v[:, :, :3], tri)
    return _normals_composite(v[:, :, :3], tri)


def save_obj(file_name, v, tri=[], vt=[], trit=[], vn=[], trin=[]):
    """Wavefront OBJ with the reference's output contract: `v` lines (every coordinate given), `vt` (first two) and
    `vn` (first three) lines with %f, then one `f` record per face with 1-based indices in the richest form the
    attributes allow — `a/t/n`, `a/t`, `a//n` or `a`.  Texture (normal) indices default to `tri` when vt (vn) has one
    entry per vertex; a texture (normal) index list whose length differs from `tri` drops that attribute.  Tensors
    or arrays are accepted.  Returns whether the file exists."""
    import os

    with open(file_name, "w") as f:
        f.write("".join(line + "\n" for line in _obj_records(v, tri, vt, trit, vn, trin)))
    return os.path.exists(file_name)


def _obj_records(v, tri=[], vt=[], trit=[], vn=[], trin=[]):
    """The lines of `save_obj`'s file."""
    def rows(a):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu()
        return [list(r) for r in (a.tolist() if hasattr(a, "tolist") else a)]

    v, tri, vt, trit, vn, trin = (rows(a) for a in (v, tri, vt, trit, vn, trin))
    if not trit and len(vt) == len(v):
        trit = tri
    elif len(trit) != len(tri):
        vt, trit = [], []
    if not trin and len(vn) == len(v):
        trin = tri
    elif len(trin) != len(tri):
        vn, trin = [], []
    out = []
    out += ["v" + "".join(" %f" % x for x in p) for p in v]
    out += ["vt" + "".join(" %f" % x for x in p[:2]) for p in vt]
    out += ["vn" + "".join(" %f" % x for x in p[:3]) for p in vn]
    for i, face in enumerate(tri):
        has_t = len(trit) > i and len(trit[i]) >= len(face)
        has_n = len(trin) > i and len(trin[i]) >= len(face)
        if has_t and has_n:
            corners = ["%d/%d/%d" % (face[j] + 1, trit[i][j] + 1, trin[i][j] + 1) for j in range(len(face))]
        elif has_t:
            corners = ["%d/%d" % (face[j] + 1, trit[i][j] + 1) for j in range(len(face))]
        elif has_n:
            corners = ["%d//%d" % (face[j] + 1, trin[i][j] + 1) for j in range(len(face))]
        else:
            corners = ["%d" % (face[j] + 1) for j in range(len(face))]
        out.append("f " + " ".join(corners) if corners else "f")
    return out


def save_textured_obj(file_name, v, tri, vt, trit, vn, texture_file):
    """`save_obj`'s records (v, vt, vn, f a/t/n) behind `mtllib <stem>.mtl` and `usemtl face`, and beside the file the
    material <stem>.mtl: `newmtl face`, `Kd 1 1 1`, `map_Kd <texture_file>` (a file name relative to the .obj).  Returns
    whether both files exist."""
    import os

    stem = os.path.splitext(file_name)[0]
    head = ["mtllib %s.mtl" % os.path.basename(stem), "usemtl face"]
    with open(file_name, "w") as f:
        f.write("".join(line + "\n" for line in head + _obj_records(v, tri, vt, trit, vn)))
    with open(stem + ".mtl", "w") as f:
        f.write("newmtl face\nKd 1 1 1\nmap_Kd %s\n" % texture_file)
    return os.path.exists(file_name) and os.path.exists(stem + ".mtl")


# ---- ADA augmentation (reference utils_3d.py:155-188, 189-349 cam=None branch, 350-359) ------------
def _axis_angle_matrix(axis_angle):
    """[B, 3] rotation vectors -> [B, 3, 3] (Rodrigues' formula in closed form)."""
    theta = torch.sqrt((axis_angle * axis_angle).sum(1, keepdim=True)).clamp_min(1e-12)
    k = axis_angle / theta
    kx, ky, kz = k[:, 0], k[:, 1], k[:, 2]
    zero = torch.zeros_like(kx)
    K = torch.stack([zero, -kz, ky, kz, zero, -kx, -ky, kx, zero], 1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=k.dtype, device=k.device).unsqueeze(0)
    s, c = torch.sin(theta).view(-1, 1, 1), torch.cos(theta).view(-1, 1, 1)
    return eye + s * K + (1 - c) * torch.matmul(K, K)


def _color_sigmas(p):
    p = torch.abs(torch.as_tensor(p, dtype=torch.float32).reshape(-1)[:5])
    return torch.cat((p, torch.zeros(5 - len(p))))


def _color_draws(batch, p):
    """z [B, 5] = brightness, log-contrast ~ N(0, p[:2]^2); luma-flip uniform; hue, log-saturation ~ N(0, p[3:]^2)."""
    return torch.cat([torch.normal(mean=0, std=p[:2].unsqueeze(0).expand(batch, -1)), torch.rand(batch, 1),
                      torch.normal(mean=0, std=p[3:].unsqueeze(0).expand(batch, -1))], 1)


def _color_matrix(z, p):
    """[B, 3, 4] colour matrices of the draws z (dtype of z)."""
    batch = z.shape[0]
    bright, contrast = z[:, 0], torch.exp(z[:, 1])
    luma = (z[:, 2] < p[2]).to(z.dtype)
    hue, sat = z[:, 3:4], torch.exp(z[:, 4]).view(-1, 1, 1)
    eye = torch.eye(3, dtype=z.dtype).unsqueeze(0)
    ones = torch.ones(3, 3, dtype=z.dtype).unsqueeze(0)
    C = torch.cat([contrast.view(-1, 1, 1) * eye.expand(batch, -1, -1),
                   (contrast * bright).view(-1, 1, 1).expand(-1, 3, 1)], 2)               # [B, 3, 4]
    C = torch.matmul(eye - luma.view(-1, 1, 1) * 2. / 3, C)
    C = torch.matmul(_axis_angle_matrix(hue.expand(-1, 3) / (3 ** 0.5)), C)
    return torch.matmul(eye * sat + ones * (1 - sat) / 3., C)


def _color_from_draws(img, z, p):
    """The apply half of random_apply_color: img [B, C, H, W] (or [C, H, W]) coloured by the draws z [B, 5]."""
    C = _color_matrix(z, p)
    batch = z.shape[0]
    shape = img.shape
    x = img.reshape(batch, -1, shape[-1] * shape[-2])
    C = C.to(dtype=img.dtype, device=img.device)
    return (torch.matmul(C[:, :, :3], x) + C[:, :, 3:4]).view(shape)


def random_apply_color(p=[.2, .3, 0, .15, .5], img=None):
    """Random brightness / contrast / luma flip / hue rotation / saturation as one 3x4 colour matrix per sample
    (p = sigmas of [brightness, log-contrast], luma-flip probability, sigmas of [hue, log-saturation])."""
    batch = len(img) if img is not None and img.dim() >= 4 else 1
    p = _color_sigmas(p)
    z = _color_draws(batch, p)
    if img is None:
        return _color_matrix(z, p)[0]
    return _color_from_draws(img, z, p)


def _pose2d_sigmas(p):
    p = torch.abs(torch.as_tensor(p, dtype=torch.float32).reshape(-1)[:6])
    return torch.cat((p, torch.zeros(6 - len(p))))


def _pose2d_draws(batch, p):
    """z [B, 5] = tx, ty, rotation ~ N(0, p[:3]^2); log-zoom ~ N(p[4], p[3]^2); flip uniform."""
    return torch.cat([torch.normal(mean=0, std=p[:3].unsqueeze(0).expand(batch, -1)),
                      torch.normal(mean=p[4:5].unsqueeze(0).expand(batch, 1), std=p[3:4].unsqueeze(0).expand(batch, -1)),
                      torch.rand(batch, 1)], 1)


def _pose2d_grid(z, p, hi, wi, pad=None):
    """The sampling grid [B, H, W, 2] (grid_sample, align_corners=True) of the draws z, in z's dtype, and the padding
    mode.  pad=None: the zoom is raised per sample until the rotated, shifted frame stays inside the source."""
    batch = z.shape[0]
    ho, wo = hi, wi
    flip = z[:, 4:5] < p[-1]
    f = torch.exp(z[:, 3:4])
    s, c = torch.sin(z[:, 2:3]), torch.cos(z[:, 2:3])
    tx, ty = z[:, 0:1], z[:, 1:2]
    yy, xx = torch.meshgrid(torch.linspace(0, ho, ho, dtype=z.dtype), torch.linspace(0, wo, wo, dtype=z.dtype),
                            indexing="ij")
    half = max(wo, ho) / 2.
    x = ((xx.reshape(1, -1) - wo / 2.) / half).expand(batch, -1)
    y = ((ho / 2. - yy.reshape(1, -1)) / half).expand(batch, -1)
    x = torch.where(flip.expand(-1, ho * wo), -x, x) - tx
    y = y - ty
    mode = "zeros"
    if pad is None:
        corner = [0, wo - 1, wo * (ho - 1), ho * wo - 1]
        cx, cy = x[:, corner], y[:, corner]
        rx = (c * cx + s * cy) * max(wo, ho) / float(wi)
        ry = (-s * cx + c * cy) * max(wo, ho) / float(hi)
        fmax = torch.max(torch.abs(torch.cat((rx, ry), 1)), 1, keepdim=True)[0]
        f = torch.where(f < fmax, fmax, f)
    else:
        mode = {"z": "zeros", "b": "border", "r": "reflection"}[str(pad).lower()[0]]
    x, y = x / f, y / f
    x, y = c * x + s * y, -s * x + c * y
    gx = (x * max(wo, ho) / float(wi)).view(-1, ho, wo, 1)
    gy = (-y * max(wo, ho) / float(hi)).view(-1, ho, wo, 1)
    return torch.cat((gx, gy), -1), mode


def _pose2d_from_draws(img, z, p, pad=None):
    """The apply half of random_apply_pose2D_img: img [B, C, H, W] resampled by the draws z [B, 5]."""
    grid, mode = _pose2d_grid(z, p, int(img.shape[-2]), int(img.shape[-1]), pad)
    grid = grid.to(dtype=img.dtype, device=img.device)
    # the reference's grid runs linspace(-1, 1) over pixel CENTRES, i.e. it was written for grid_sample's
    # pre-1.3 default (align_corners=True); with today's default the identity transform would blur the image
    return torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode=mode, align_corners=True)


def random_apply_pose2D_img(p=[.1, .1, .05, .15, 0, .5], img=None, pad=None):
    """Random translation / in-plane rotation / zoom / horizontal flip of a batch of images by bilinear resampling.
    pad=None: the zoom is raised per sample until the rotated, shifted frame stays inside the source (no border
    shows), the behaviour `augment` relies on; 'zeros' / 'border' / 'reflection' skip that and pad instead."""
    if img is None or img.dim() < 4:
        raise ValueError("random_apply_pose2D_img: a batch of images [B, C, H, W] is required")
    p = _pose2d_sigmas(p)
    return _pose2d_from_draws(img, _pose2d_draws(img.shape[0], p), p, pad)


def _augment_from_draws(img, z_pose, z_color, pick, augment_ratio, pose_p=(.1, .1, .05, .15, 0, .5),
                        color_p=(.2, .3, 0, .15, .5)):
    """The composite `augment` of a 4-D batch given its draws: pose, then colour, then the per-sample choice."""
    aug = _color_from_draws(_pose2d_from_draws(img, z_pose, _pose2d_sigmas(pose_p), None), z_color,
                            _color_sigmas(color_p))
    return torch.where(pick.expand_as(img) < augment_ratio, aug, img)


def augment(img, augment_ratio=.5):
    """Per sample, with probability `augment_ratio` (a float or a 0-d tensor): random 2-D pose then random colour
    (reference utils_3d.py:350-359).  Float32 3-channel images on the GPU take the native kernels (op.augment: three
    launches, nothing read back, capturable); everything else the composite form below."""
    shape = img.shape
    while img.dim() < 4:
        img = img.unsqueeze(0)
    if img.is_cuda and img.dtype == torch.float32 and img.shape[1] == 3:
        from .op import augment as native

        return native.augment(img, augment_ratio).view(shape)
    batch = img.shape[0]
    pose_p, color_p = _pose2d_sigmas([.1, .1, .05, .15, 0, .5]), _color_sigmas([.2, .3, 0, .15, .5])
    z_pose = _pose2d_draws(batch, pose_p)
    z_color = _color_draws(batch, color_p)
    pick = torch.rand(batch, 1, 1, 1, dtype=img.dtype, device=img.device)
    return _augment_from_draws(img, z_pose, z_color, pick, augment_ratio).view(shape)


# ---- axis-angle rotations ----------------------------------------------------------------------------
def rodrigues(rvec, eps=1e-8):
    """Rotation matrices [N, 3, 3] ([3, 3]) of axis-angle vectors rvec [N, 3] ([3]): R = cos(r) I + cc r r^T + sc [r]_x
    with r = |rvec|, sc = sin(r) / r, cc = (1 - cos(r)) / r^2 (reference utils_3d.py:81-154).  For r <= eps the series
    sc = 1 - r^2/6, cc = 1/2 - r^2/24 take over, whose derivatives are the reference's backward coefficients
    -1/3 + r^2/30 and -1/12 + r^2/180 up to O(r^4).  Plain tensor algebra: differentiable to any order, finite at 0.
    The device kernels of the skinning node use the same function as a __device__ helper (csrc/rodrigues.h)."""
    eps = abs(eps)
    single = rvec.dim() == 1
    a = rvec.view(1, 3) if single else rvec
    r2 = (a * a).sum(1)
    small = torch.sqrt(r2.detach()) <= eps
    r2s = torch.where(small, torch.ones_like(r2), r2)           # the unused branch stays finite (and its gradient)
    r = torch.sqrt(r2s)
    c = torch.where(small, 1 - r2 / 2, torch.cos(r))
    sc = torch.where(small, 1 - r2 / 6, torch.sin(r) / r)
    cc = torch.where(small, .5 - r2 / 24, (1 - torch.cos(r)) / r2s)
    zero = torch.zeros_like(r2)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    rx = torch.stack((zero, -z, y, z, zero, -x, -y, x, zero), 1).view(-1, 3, 3)
    rr = a.unsqueeze(2) * a.unsqueeze(1)
    eye = torch.eye(3, dtype=a.dtype, device=a.device).view(1, 3, 3)
    out = c.view(-1, 1, 1) * eye + cc.view(-1, 1, 1) * rr + sc.view(-1, 1, 1) * rx
    return out.view(3, 3) if single else out
