"""Face models in front of the rasterizer.

LinearMorphableModel — same class name, constructor arguments, parameter names (`fc.weight`, `fc.bias`, `sigma`) and
methods as reference face_model.py:4-74, so its checkpoints load unchanged.  Vertices = fc(coefficients).view(B, nv, 3):
one [B, d] x [d, 3 nv] GEMM (d = shape + expression dims), a library call on the device.

LinearBlendSkinningModel / load_flame — the skinned, articulated model (FLAME: neck, jaw, eyeballs) of reference
face_model.py:146-341 and 378-408; on the device its forward is the skinning node's kernels (op/skin.py).

BlendShapeModel / load_facewarehouse — the bilinear identity x expression model (FaceWarehouse) of reference
face_model.py:75-146 and 363-377; on the device its forward is the blendshape node's kernels (op/blend.py).

What the fitting loop (inversion.LatentInverter, reconstruct) asks of a model, the same for all three:
    kind                           "linear" | "skinned" | "blended"
    n_coeff                        length of a coefficient vector
    n_identity                     how many leading coefficients describe the person rather than the moment: what the views
                                   of a multi-view fit share (LatentInverter's shared_identity).  dim[0] for all three
                                   (shape before expression, identity logits before expression logits, shape before the
                                   joints' rotations); load_flame lowers it where the file's shape basis carries
                                   expression columns behind the identity columns
    mesh(coeff, pose, tri, reg_weight=0.0)
                                   (v, n, reg, prior_rows) of the model's node (op.morph / op.skin / op.blend); prior_rows
                                   [B] is every sample's share of reg, or None where the prior is a diagonal Gaussian
                                   (lpips_layer.fit_loss_rows then evaluates it from prior_sigma itself)
    prior_sigma(batch, shape_reg)  that Gaussian's sigma [n_coeff] for a fit of `batch` images, or None
    fit_extras(coeff)              the model's own entries of a fit's .npz, from coeff [1, n_coeff]
    landmarks                      (idx int32 [L, 3], bary float32 [L, 3]) of `landmark_embedding`, or None: the model's own
                                   landmarks (load_bfm: the file's `landmarks68`), for the landmark term of the fit
`contour_lines` builds, from any model's mean shape, the candidate lines along which the jaw landmarks of that term slide
with the pose (op.landmark); `load_contour_lines` reads hand-made ones.  `uv_layout` computes a texture layout from a mean
shape and `load_uv` reads one from a file, for op.texture."""
import numpy as np
import torch
from torch import nn

from .op._dispatch import host_array


def _as_basis(w, rows, dim):
    """Accepts [dim, 3 nv] or [3 nv, dim] (or anything reshapeable to [-1, last]) and returns [dim', 3 nv']."""
    w = np.array(w, np.float32)
    w = w.reshape((-1, w.shape[-1]))
    if w.shape[0] == rows and w.shape[1] >= dim:
        w = w.T
    return w


def _load_array(path):
    """The array(s) of a landmark file: .npy, .txt (numbers), or .npz with `idx` or with `faces` and `bary`."""
    path = str(path)
    if path.lower().endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            if "faces" in z.files and "bary" in z.files:
                return z["faces"], z["bary"]
            if "idx" in z.files:
                return z["idx"]
            raise ValueError("landmark_embedding: %s holds neither `idx` nor `faces` and `bary`" % path)
    if path.lower().endswith(".npy"):
        return np.load(path, allow_pickle=False)
    return np.loadtxt(path)


def landmark_embedding(source, tri=None):
    """(idx int32 [L, 3], bary float32 [L, 3]): every landmark as a barycentric combination of three vertices, the form
    op.landmark takes.  `source` is
      * an integer array [L] of vertex indices: idx = (i, i, i), bary = (1, 0, 0);
      * a pair (faces [L], bary [L, 3]): triangle indices into `tri` [nf, 3] and weights on their corners (FLAME's static
        embedding);
      * the path of a .npy / .txt holding vertex indices (a .txt with four columns: face, three weights), or of a .npz
        with `idx`, or with `faces` and `bary`.
    Negative indices, faces outside `tri` and non-finite weights are refused; the upper bound of a vertex index is the
    mesh's, checked where the embedding meets one (op.landmark.vertex_lists)."""
    import os

    if isinstance(source, (str, os.PathLike)):
        source = _load_array(source)
        if isinstance(source, np.ndarray) and source.ndim == 2 and source.shape[1] == 4:
            source = (source[:, 0], source[:, 1:])
    if isinstance(source, (tuple, list)) and len(source) == 2 and np.ndim(source[1]) == 2:
        faces, bary = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in source)
        if tri is None:
            raise ValueError("landmark_embedding: (faces, bary) needs the mesh's tri")
        t = tri.detach().cpu().numpy() if isinstance(tri, torch.Tensor) else np.asarray(tri)
        faces = faces.reshape(-1)
        if not np.all(np.round(faces) == faces):
            raise ValueError("landmark_embedding: face indices must be whole numbers")
        faces = faces.astype(np.int64)
        bary = np.asarray(bary, np.float32)
        if bary.shape != (len(faces), 3) or not np.isfinite(bary).all():
            raise ValueError("landmark_embedding: bary must be finite [L, 3] for %d faces, got %s"
                             % (len(faces), bary.shape))
        if len(faces) and (faces.min() < 0 or faces.max() >= len(t)):
            raise ValueError("landmark_embedding: face index out of range [0, %d)" % len(t))
        idx = t[faces].astype(np.int64)
    else:
        idx = source.detach().cpu().numpy() if isinstance(source, torch.Tensor) else np.asarray(source)
        idx = idx.reshape(-1)
        if not np.all(np.round(idx) == idx):
            raise ValueError("landmark_embedding: vertex indices must be whole numbers")
        idx = np.repeat(idx.astype(np.int64).reshape(-1, 1), 3, 1)
        bary = np.tile(np.array([[1.0, 0.0, 0.0]], np.float32), (len(idx), 1))
    if idx.size and (idx.min() < 0 or idx.max() >= 2 ** 31):
        raise ValueError("landmark_embedding: vertex index out of range")
    return torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(bary, np.float32))


def contour_lines(v_mean, embedding, contour=range(17), max_candidates=64, inner=0.5, normals=None, tri=None):
    """Contour lines of a model's mean shape for op.landmark's pose-aware term: (line_lmk int32 [C], side int32 [C],
    cand_off int32 [C + 1], cand int32 [E]) on the host.  v_mean [nv, 3] (or [1, nv, 3]) is the mean shape, centred in x
    and seen from +z; `embedding` = (idx, bary) of `landmark_embedding`; `contour` names the landmarks of the jaw line in
    their order along it (0-16 of a 68-point set).  For contour landmark l at mean position P: side = sign of P.x; a
    landmark with |P.x| below 2 % of the face's half width (max |x|; the chin) gets no line.  Its candidates are the
    vertices
      * whose y lies within half the spacing to the neighbouring contour landmarks (an end of the jaw line mirrors its one
        neighbour),
      * whose side x lies between inner side P.x and side P.x,
      * whose mean-shape normal has z > 0 (`normals` [nv, 3], or computed from `tri`; without either this test is left
        out),
    ordered by descending side x after the static vertex (the vertex of the landmark's largest weight, always
    candidate 0) and cut at max_candidates."""
    v = host_array(v_mean).astype(np.float64).reshape(-1, 3)
    idx, bary = (host_array(t) for t in embedding)
    idx, bary = idx.astype(np.int64), bary.astype(np.float64)
    nv = len(v)
    if idx.size and (idx.min() < 0 or idx.max() >= nv):
        raise ValueError("contour_lines: landmark vertex index out of range [0, %d)" % nv)
    contour = [int(l) for l in contour]
    if len(set(contour)) != len(contour):
        raise ValueError("contour_lines: a landmark is named twice in `contour`")
    if contour and (min(contour) < 0 or max(contour) >= len(idx)):
        raise ValueError("contour_lines: `contour` names a landmark outside [0, %d)" % len(idx))
    if int(max_candidates) < 1 or not 0.0 <= float(inner) <= 1.0:
        raise ValueError("contour_lines: max_candidates >= 1 and 0 <= inner <= 1")
    if normals is None and tri is not None:
        from .utils_3d import mesh_point_normal

        normals = mesh_point_normal(torch.from_numpy(v)[None], torch.as_tensor(host_array(tri)).long())[0]
    facing = np.ones(nv, bool) if normals is None else host_array(normals).reshape(-1, 3)[:, 2] > 0
    pts = (bary[:, :, None] * v[idx]).sum(1)                                           # [L, 3]
    half_width = np.abs(v[:, 0]).max()
    line_lmk, sides, cand, off = [], [], [], [0]
    for k, l in enumerate(contour):
        px, py = pts[l, 0], pts[l, 1]
        if abs(px) < 0.02 * half_width:
            continue
        side = 1.0 if px > 0 else -1.0
        near = [pts[contour[j], 1] for j in (k - 1, k + 1) if 0 <= j < len(contour)]
        half = [0.5 * abs(y - py) for y in near]
        if len(near) == 2 and (near[0] - py) * (near[1] - py) < 0:
            lo, hi = py - half[0 if near[0] < py else 1], py + half[0 if near[0] > py else 1]
        else:                                   # an end of the line, or a turning point of it: the wider half both ways
            lo, hi = py - max(half, default=0.0), py + max(half, default=0.0)
        sx = side * v[:, 0]
        ok = facing & (v[:, 1] >= lo) & (v[:, 1] <= hi) & (sx >= inner * side * px) & (sx <= side * px)
        static = int(idx[l, int(np.argmax(bary[l]))])
        ok[static] = False
        rest = np.nonzero(ok)[0]
        rest = rest[np.argsort(-sx[rest], kind="stable")][:int(max_candidates) - 1]
        line_lmk.append(l)
        sides.append(int(side))
        cand.extend([static] + rest.tolist())
        off.append(len(cand))
    as_t = lambda a: torch.from_numpy(np.asarray(a, np.int32).reshape(-1))                       # noqa: E731
    return as_t(line_lmk), as_t(sides), as_t(off), as_t(cand)


def save_contour_lines(path, lines):
    """Writes lines = (line_lmk, side, cand_off, cand) to an .npz under those four names."""
    a = [host_array(x).astype(np.int32).reshape(-1) for x in lines]
    np.savez(str(path), line_lmk=a[0], side=a[1], cand_off=a[2], cand=a[3])


def load_contour_lines(path, n_landmarks=None, nv=None):
    """Reads hand-made contour lines from an .npz with `line_lmk` [C], `side` [C], `cand_off` [C + 1] and `cand` [E]
    (candidate 0 of a line: its landmark's static vertex); checked like op.landmark does (a landmark in two lines, an
    empty line, a side other than -1 / +1, and, where n_landmarks / nv are given, indices out of range)."""
    from .op.landmark import check_lines

    with np.load(str(path), allow_pickle=False) as z:
        missing = [k for k in ("line_lmk", "side", "cand_off", "cand") if k not in z.files]
        if missing:
            raise ValueError("load_contour_lines: %s lacks %s" % (path, ", ".join(missing)))
        raw = tuple(z[k] for k in ("line_lmk", "side", "cand_off", "cand"))
    n_l = int(n_landmarks) if n_landmarks is not None else (int(np.max(raw[0])) + 1 if np.size(raw[0]) else 0)
    return tuple(torch.from_numpy(a.astype(np.int32)) for a in check_lines(raw, n_l, nv))


def landmark_vertices(embedding):
    """The main vertex [L] (int64, host) of every landmark of an embedding: the one of its largest weight."""
    idx, bary = (host_array(t) for t in embedding)
    return idx.astype(np.int64)[np.arange(len(idx)), np.argmax(bary, 1)]


# ---- texture layouts (op.texture) ------------------------------------------------------------------------------------
def uv_layout(v_mean, tri, margin=1.0 / 64):
    """(uv float32 [nv, 2], tri_uv int64 [nf, 3], keep bool [nf]): a cylindrical unwrap of the mean shape v_mean [nv, 3]
    about the vertical axis through its centroid (cx, ., cz), for op.texture.texel_map:
        theta = atan2(x - cx, z - cz)      u = theta / 2 pi + 1/2      v = (y - y_min) / (y_max - y_min)
    both then mapped affinely from [0, 1] into [margin, 1 - margin]; one texture coordinate per vertex, so tri_uv = tri.
    keep[f] is false for the faces that straddle the seam at the back (max u - min u > 1/2 before the margin map): they
    would smear across the whole texture and are left out of it.  No file of the supported models carries a layout (a
    Basel file has none); this one is meant for face patches and convex heads, where a ray from the axis meets the
    surface once; a vertex on the axis itself (the pole of a closed head) has no angle of its own and lands wherever the
    centroid's rounding puts it.  A template's own layout (FLAME's) comes in through `load_uv`."""
    raw = host_array(v_mean).reshape(-1, 3)
    v = raw.astype(np.float64)
    t = host_array(tri).astype(np.int64).reshape(-1, 3)
    if not 0 <= float(margin) < 0.5:
        raise ValueError("uv_layout: margin lies in [0, 1/2)")
    if t.size and (t.min() < 0 or t.max() >= len(v)):
        raise ValueError("uv_layout: triangle index out of range [0, %d)" % len(v))
    c = raw.mean(0).astype(np.float64)                      # (the centroid in the mean shape's own float type)
    u = np.arctan2(v[:, 0] - c[0], v[:, 2] - c[2]) / (2 * np.pi) + 0.5
    span = v[:, 1].max() - v[:, 1].min()
    w = (v[:, 1] - v[:, 1].min()) / (span if span > 0 else 1.0)
    ut = u[t]
    keep = (ut.max(1) - ut.min(1)) <= 0.5
    uv = float(margin) + np.stack((u, w), 1) * (1 - 2 * float(margin))
    return (torch.from_numpy(uv.astype(np.float32)), torch.from_numpy(t.copy()), torch.from_numpy(keep))


def load_uv(path, tri):
    """(uv float32 [nt, 2], tri_uv int64 [nf, 3]) of a layout file for the mesh `tri` [nf, 3]: a Wavefront .obj with `vt`
    lines and `f a/t[/n]` records (1-based; the `a` columns must equal tri row by row), or an .npz with `vt` [nt, 2] and
    `ft` [nf, 3] (0-based).  This is how a template's own layout (FLAME's head_template.obj) comes in."""
    path = str(path)
    t = host_array(tri).astype(np.int64).reshape(-1, 3)
    if path.lower().endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("vt", "ft") if k not in z.files]
            if missing:
                raise ValueError("load_uv: %s lacks %s" % (path, ", ".join(missing)))
            vt, ft = np.asarray(z["vt"], np.float64), np.asarray(z["ft"])
        if not np.all(np.round(ft) == ft):
            raise ValueError("load_uv: %s: ft holds whole numbers" % path)
        ft = ft.astype(np.int64)
    else:
        vt, fa, ft = [], [], []
        with open(path) as f:
            for line in f:
                tok = line.split()
                if not tok:
                    continue
                if tok[0] == "vt":
                    vt.append([float(x) for x in tok[1:3]])
                elif tok[0] == "f":
                    parts = [c.split("/") for c in tok[1:]]
                    if len(parts) != 3 or any(len(p) < 2 or not p[1] for p in parts):
                        raise ValueError("load_uv: %s: every face must be a triangle of a/t[/n] records, got %r"
                                         % (path, line.strip()))
                    fa.append([int(p[0]) - 1 for p in parts])
                    ft.append([int(p[1]) - 1 for p in parts])
        vt = np.asarray(vt, np.float64).reshape(-1, 2)
        fa, ft = np.asarray(fa, np.int64).reshape(-1, 3), np.asarray(ft, np.int64).reshape(-1, 3)
        if fa.shape != t.shape or not np.array_equal(fa, t):
            raise ValueError("load_uv: the faces of %s differ from the mesh's tri (%d faces against %d, or other vertices): "
                             "the layout must list the model's triangles row by row" % (path, len(fa), len(t)))
    if vt.ndim != 2 or vt.shape[1] != 2 or ft.shape != t.shape:
        raise ValueError("load_uv: %s: vt [nt, 2] and one texture triangle per face (%d) are needed, got %s and %s"
                         % (path, len(t), vt.shape, ft.shape))
    if ft.size and (ft.min() < 0 or ft.max() >= len(vt)):
        raise ValueError("load_uv: %s: texture coordinate index out of range [0, %d)" % (path, len(vt)))
    if vt.size and not (np.isfinite(vt).all() and vt.min() >= 0 and vt.max() <= 1):
        raise ValueError("load_uv: %s: texture coordinates must lie in [0, 1]" % path)
    return torch.from_numpy(vt.astype(np.float32)), torch.from_numpy(np.ascontiguousarray(ft))


class LinearMorphableModel(nn.Module):
    kind = "linear"
    landmarks = None

    def __init__(self, vertices_num, shape_dim=0, expression_dim=0, vertices_mean=None, w_shape_numpy=None,
                 w_expression_numpy=None, sigma_shape=1, sigma_expression=.01, learnable=False):
        super().__init__()
        vertices_num = max(int(vertices_num), 1)
        shape_dim = max(int(shape_dim), 0)
        expression_dim = max(int(expression_dim), 0)
        d = shape_dim + expression_dim
        # random model when no data is given (reference face_model.py:16-19)
        v = (np.random.rand(vertices_num * 3).astype(np.float32) * 2 - 1) * np.sqrt(d)
        w = (np.random.rand(d, v.shape[0]).astype(np.float32) * 2 - 1) * np.sqrt(d)
        if vertices_mean is not None:
            m = np.array(vertices_mean, np.float32)
            if m.shape[0] == 3:
                m = m.reshape(3, -1).T
            elif m.ndim > 1:
                m = m.reshape(-1, m.shape[-1])
            else:
                m = m.reshape(-1, 3)
            n = min(vertices_num, m.shape[0])
            v[:3 * n] = m[:n, :3].reshape(-1)
        if w_shape_numpy is not None:
            ws = _as_basis(w_shape_numpy, w.shape[1], shape_dim)
            k, n = min(shape_dim, ws.shape[0]), min(vertices_num, ws.shape[1] // 3)
            w[:k, :3 * n] = ws[:k, :3 * n]
        if w_expression_numpy is not None and expression_dim > 0:
            we = _as_basis(w_expression_numpy, w.shape[1], expression_dim)
            k, n = min(expression_dim, we.shape[0]), min(vertices_num, we.shape[1] // 3)
            w[shape_dim:shape_dim + k, :3 * n] = we[:k, :3 * n]

        def sigmas(src, count):
            src = [] if src is None else list(np.reshape(src, -1))
            return [abs(src[i]) if len(src) > i else (abs(src[-1]) if src else 1) for i in range(count)]

        self.dim = [shape_dim, expression_dim, vertices_num * 3]
        self.fc = nn.Linear(d, vertices_num * 3, bias=True)
        self.sigma = nn.Parameter(torch.Tensor(sigmas(sigma_shape, shape_dim) + sigmas(sigma_expression, expression_dim)),
                                  requires_grad=False)
        with torch.no_grad():
            self.fc.weight.copy_(torch.from_numpy(w.T).float())
            self.fc.bias.copy_(torch.from_numpy(v).float())
        if not learnable:
            self.fc.weight.requires_grad = False
            self.fc.bias.requires_grad = False

    def random_input(self, batch_size=1):
        # = torch.normal(mean=0, std=sigma[None].expand(batch, -1)) (reference face_model.py:69-70: same distribution, another draw) without its host-side
        # check of `std >= 0`, which reads the device and is refused inside a hipGraph capture (graph_train samples the
        # meshes inside the captured D / G phases)
        return torch.randn(batch_size, self.sigma.shape[0], device=self.sigma.device, dtype=self.sigma.dtype) * self.sigma

    def forward(self, x):
        return torch.reshape(self.fc(x), (-1, self.dim[2] // 3, 3))

    def regulation(self, x):
        return ((x / self.sigma[np.newaxis, :]) ** 2).sum()

    @property
    def n_coeff(self):
        return self.sigma.numel()

    @property
    def n_identity(self):
        return self.dim[0]

    def mesh(self, coeff, pose, tri, reg_weight=0.0):
        from .op.morph import morph_mesh

        return morph_mesh(self, coeff, pose, tri, reg_weight) + (None,)

    def prior_sigma(self, batch, shape_reg):
        return self.sigma

    def fit_extras(self, coeff):
        return {}


def load_bfm(file_name="/data/BaselFaceModel.mat"):
    """Basel Face Model -> (LinearMorphableModel, tri int64 [nf, 3]) with the reference's `.mat` contract
    (reference face_model.py:342-362): keys `v` [3, nv] (mean shape), `w_shape` [3 nv, ds], `w_exp` [3 nv, de],
    optional `sigma_shape` / `sigma_exp` (folded into the bases), `tri` as a 1x1 MATLAB cell of 1-based indices.
    Coordinates are centred and scaled by 1e-5 like the reference.  `file_name` may be the path of the (licensed,
    not distributed) file or an already loaded dict."""
    if isinstance(file_name, str):
        import scipy.io as sio

        data = sio.loadmat(file_name)
    else:
        data = file_name
    v = (data["v"] - data["v"].mean(1).reshape(-1, 1)).T * 1e-5
    w_shape = data["w_shape"] * 1e-5
    w_exp = data["w_exp"] * 1e-5
    if "sigma_shape" in data.keys():
        w_shape = w_shape.dot(np.diag(np.reshape(data["sigma_shape"], -1)))
    if "sigma_exp" in data.keys():
        w_exp = w_exp.dot(np.diag(np.reshape(data["sigma_exp"], -1)))
    tri = np.asarray(data["tri"][0, 0]).astype(np.int64)
    tri = tri - tri.min()
    if tri.shape[0] == 3 and tri.shape[1] != 3:
        tri = tri.T
    model = LinearMorphableModel(len(v), w_shape.shape[1], w_exp.shape[1], v, w_shape, w_exp)
    if "landmarks68" in data.keys():
        # based like `tri` (align.template_from_bfm)
        base = np.asarray(data["tri"][0, 0]).astype(np.int64).min()
        model.landmarks = landmark_embedding(np.asarray(data["landmarks68"]).reshape(-1).astype(np.int64) - base, tri)
    return model, torch.from_numpy(np.ascontiguousarray(tri))


class BlendShapeModel(nn.Module):
    """Bilinear identity x expression blendshape model (FaceWarehouse; reference face_model.py:75-146): same constructor
    arguments, `dim` = [shape_dim, expression_dim, 3 nv], methods and state-dict keys (`beta` [ds + 1 + 2 de], `weight`
    [ds + 1, de + 1, 3 nv], in that order), so its checkpoints load.  With x [B, ds + de]:

        xs = softmax(cat(x[:, :ds], -sum x[:, :ds]))        identity weights, on the simplex
        xe = cat(1 - sum s, s),  s = sigmoid(x[:, ds:])     expression weights in [0, 1], xe[0] the neutral face
        forward(x)[b] = sum_ij xs[b, i] xe[b, j] weight[i, j].view(nv, 3)

    `regulation` is the reference's negative Dirichlet / Beta log-likelihood in the logits, written with log-sum-exp and
    softplus (equal to its log(sum(exp)) and log(exp + 1) wherever those are finite).  With concentrations below 1
    (`load_facewarehouse`'s beta_shape = .01) its identity part is unbounded below: it falls without limit as one logit
    grows, so a positive weight on it pushes the identity away from the mean.

    One defect of the reference is not reproduced: its `random_input` centres the identity log-ratios log(p_i / p_last) by
    their sum over ds (line 126), which is not the inverse of forward's softmax (with beta = (2, 3, 5) the weights it
    yields average (.27, .42, .30), not (.2, .3, .5)); here they are centred over all ds + 1 parts, so that
    softmax(cat(x, -sum x)) is the Dirichlet draw itself.  It also runs with expression_dim = 0, where the reference's
    raises."""
    kind = "blended"
    landmarks = None

    def __init__(self, vertices_num, shape_dim=0, expression_dim=0, bs=None, beta_shape=1, beta_expression=[1, 10],
                 learnable=False):
        super().__init__()
        vertices_num = max(int(vertices_num), 1)
        shape_dim = max(int(shape_dim), 0)
        expression_dim = max(int(expression_dim), 0)
        # random model when no data is given (reference face_model.py:85-86)
        w = (np.random.rand(shape_dim + 1, expression_dim + 1, vertices_num * 3).astype(np.float32) * 2 - 1) \
            * np.sqrt(shape_dim + expression_dim)
        if bs is not None:
            bs = np.array(bs, np.float32)
            if bs.ndim >= 3:
                bs = bs.reshape(bs.shape[0], bs.shape[1], -1)
                if bs.shape[0] == w.shape[-1]:                      # [3 nv, ., .] -> [., ., 3 nv]
                    bs = np.transpose(bs, [1, 2, 0])
                d = [min(bs.shape[0], w.shape[0]), min(bs.shape[1], w.shape[1]), min((bs.shape[2] // 3) * 3, w.shape[2])]
                w[:d[0], :d[1], :d[2]] = bs[:d[0], :d[1], :d[2]]
        bsh = [] if beta_shape is None else [float(v) for v in np.reshape(beta_shape, -1)]
        bex = [] if beta_expression is None else [float(v) for v in np.reshape(beta_expression, -1)]
        self.dim = [shape_dim, expression_dim, vertices_num * 3]
        # the reference's padding rule (lines 104-110): a short identity list repeats its last value; an expression list
        # that does not reach pair i repeats its last pair (a single value or none: 1)
        beta = [abs(bsh[i]) if len(bsh) > i else (abs(bsh[-1]) if bsh else 1) for i in range(shape_dim + 1)]
        beta += [abs(bex[2 * i + j]) if len(bex) > 2 * i + 1 else (abs(bex[j - 2]) if len(bex) > 1 else 1)
                 for i in range(expression_dim) for j in range(2)]
        self.beta = nn.Parameter(torch.tensor(beta, dtype=torch.float32), requires_grad=False)
        self.weight = nn.Parameter(torch.from_numpy(w).float(), requires_grad=bool(learnable))

    def random_input(self, batch_size=1):
        # Dirichlet(beta_s) identity weights and Beta(a_j, b_j) expression weights from unit-scale gamma draws on the
        # model's device, mapped to centred log-ratios and logits in log space: finite (the gamma sampler never returns
        # 0) and with no host-side check, so that it runs under graph capture like the other models' samplers.
        ds, de = self.dim[0], self.dim[1]
        lg = torch.log(torch._standard_gamma(self.beta.detach().unsqueeze(0).expand(batch_size, -1).contiguous()))
        ls = lg[:, :ds + 1]
        xs = ls[:, :ds] - ls.mean(1, keepdim=True)
        le = lg[:, ds + 1:].reshape(batch_size, de, 2)
        return torch.cat((xs, le[:, :, 0] - le[:, :, 1]), 1)

    def mixing_weights(self, x):
        """(xs [B, ds + 1], xe [B, de + 1]): the identity and expression weights of coefficients x."""
        from .op import blend

        return blend.mixing_weights(x, self.dim[0])

    def forward(self, x):
        from .op import blend

        return blend.blend_vertices(self, x)

    def regulation(self, x):
        ds = self.dim[0]
        beta = self.beta.to(x.dtype)
        ls = torch.cat((x[:, :ds], -x[:, :ds].sum(1, keepdim=True)), 1)
        xe = x[:, ds:]
        bs, be = beta[:ds + 1], beta[ds + 1:].reshape(self.dim[1], 2)
        return -((ls * bs.unsqueeze(0)).sum() - torch.logsumexp(ls, 1).sum() * (bs.sum() - ds - 1)
                 + (xe * be[:, 0].unsqueeze(0) - 1).sum()
                 - (torch.nn.functional.softplus(xe) * (be.sum(1) - 2).unsqueeze(0)).sum())

    @property
    def n_coeff(self):
        return self.dim[0] + self.dim[1]

    @property
    def n_identity(self):
        return self.dim[0]

    def mesh(self, coeff, pose, tri, reg_weight=0.0):
        from .op.blend import blend_mesh

        return blend_mesh(self, coeff, pose, tri, reg_weight, per_sample=True)

    def prior_sigma(self, batch, shape_reg):
        return None                                  # a Dirichlet / Beta prior: the node's prior_rows

    def fit_extras(self, coeff):
        xs, xe = self.mixing_weights(coeff)
        return {"identity": xs[0].cpu().numpy(), "expression": xe[0].cpu().numpy()}


def load_facewarehouse(file_name="/data/FaceWareHouse.mat", beta_shape=.01):
    """FaceWarehouse -> (BlendShapeModel, tri int64 [nf, 3]) with the reference's contract (face_model.py:363-377):
    keys `v` [3, nv] (a mean shape: only its per-axis mean is used, to centre), `p` [3 nv, de + 1, ds + 1] (every
    identity's every expression, vertex coordinate first) and `tri` (any base, [nf, 3] or [3, nf]).  `file_name` is the
    path of the (licensed, not distributed) `.mat` or an already loaded dict.  `beta_shape` is the Dirichlet concentration
    of the identity prior; the default is the reference's .01, with which `regulation` is unbounded below (see
    BlendShapeModel) — give a value >= 1 for a prior that pulls towards the mean identity."""
    if isinstance(file_name, str):
        import scipy.io as sio

        data = sio.loadmat(file_name)
    else:
        data = file_name
    v, p = np.asarray(data["v"]), np.asarray(data["p"])
    v_mean = np.tile(v.mean(1).reshape(-1, 1, 1), (v.shape[1], 1, 1))
    bs = np.transpose(p - v_mean, [2, 1, 0])
    t = np.asarray(data["tri"])
    tri = (t - t.min()).astype(np.int64)
    if tri.shape[0] == 3 and tri.shape[1] != 3:
        tri = tri.T
    model = BlendShapeModel(v.shape[1], bs.shape[0] - 1, bs.shape[1] - 1, bs, beta_shape)
    return model, torch.from_numpy(np.ascontiguousarray(tri))


def _is_diagonal(cov):
    return bool((cov - torch.diag_embed(torch.diagonal(cov, dim1=-2, dim2=-1))).abs().max() == 0) if cov.numel() else True


class LinearBlendSkinningModel(nn.Module):
    """Linear blend skinning over a shape basis with pose-corrective blendshapes (reference face_model.py:146-341): same
    constructor arguments, attributes (`dim` = [shape_dim, 3 (nj - 1), 3 nv], `parent`, `fc` = [S, v], `weight` =
    [W, Jreg], `sigma`, `pose_mean`, `pose_cov`, `pose_inv`), methods and state-dict keys (`sigma`, `pose_mean`,
    `pose_cov`: the four arrays are outside it, as in the reference, so its checkpoints load).  Unlike the reference's
    Python lists the arrays are non-persistent buffers, so `.to()` moves them; `learnable=True` makes them require
    gradients (leaves for as long as the model is not moved).

    Three defects of the reference's constructor are not reproduced:
    * its re-ordering of a `kintree_table` that is not parent-before-child reads `j`, `w`, `s` before they exist (lines
      180-188) and cannot run.  Tables in parent-before-child order (FLAME's) are supported, others raise ValueError.
      The root's parent may be any value outside [0, nj): -1, or 2^32 - 1 in FLAME's uint32 table.
    * the number of `posedirs` rows copied is taken from `shapedirs` (line 222); here from `posedirs`.
    * without `weights` it needs scikit-learn for the nearest joint (lines 247-252); here the same weight
      exp(-d^2 / d_max^2) on the nearest joint comes from a brute-force argmin (nj is tiny)."""
    kind = "skinned"
    landmarks = None

    def __init__(self, vertices_num, pose_nodes=1, shape_dim=0, v_template=None, J_regressor=None, kintree_table=None,
                 weights=None, posedirs=None, shapedirs=None, sigma_shape=1, sigma_pose=1, mean_pose=0, learnable=False):
        super().__init__()
        nv = max(int(vertices_num), 1)
        ds = max(int(shape_dim), 0)
        nj = max(int(pose_nodes), 1)
        if kintree_table is not None:
            kt = np.asarray(kintree_table).astype(np.int64)
            if kt.ndim == 1:
                if len(kt) == nj - 1:
                    kt = np.concatenate(([-1], kt))
                kt = np.vstack((kt, np.arange(nj)))
            elif kt.shape[1] == 2 and kt.shape[0] == nj:
                kt = kt.T
            par = kt[0]
            root = np.logical_or(par < 0, par >= nj)
            k = int(root.sum())
            ok = (kt.shape[1] == nj and np.array_equal(kt[1], np.arange(nj)) and k >= 1 and root[:k].all()
                  and all(par[c] < c for c in range(k, nj)))
            if not ok:
                raise ValueError("LinearBlendSkinningModel: kintree_table must list the joints 0..%d in order, roots "
                                 "first and every parent before its children" % (nj - 1))
            self.parent = par[k:].copy()
        else:
            self.parent = np.zeros(nj - 1, np.int64)
        npose = len(self.parent)
        scale = np.sqrt(ds + npose * 9)
        # random model when no data is given (reference face_model.py:191-196)
        v = (np.random.rand(nv * 3).astype(np.float32) * 2 - 1) * scale
        s = (np.random.rand(ds + (nj - 1) * 9, v.shape[0]).astype(np.float32) * 2 - 1) * scale
        j = (np.random.rand(nj, nv).astype(np.float32) * 2 - 1) * np.sqrt(nj)
        if v_template is not None:
            m = np.array(v_template, np.float32)
            if m.shape[0] == 3:
                m = m.reshape(3, -1).T
            elif m.ndim > 1:
                m = m.reshape(-1, m.shape[-1])
            else:
                m = m.reshape(-1, 3)
            n = min(nv, m.shape[0])
            v[:3 * n] = m[:n, :3].reshape(-1)
        if shapedirs is not None:
            b = _as_basis(shapedirs, s.shape[1], ds)
            d, n = min(ds, b.shape[0]), min(nv, b.shape[1] // 3)
            s[:d, :3 * n] = b[:d, :3 * n]
        if posedirs is not None:
            b = _as_basis(posedirs, s.shape[1], npose * 9)
            d, n = min(npose * 9, b.shape[0]), min(nv, b.shape[1] // 3)
            s[ds:ds + d, :3 * n] = b[:d, :3 * n]
        if J_regressor is not None:
            if hasattr(J_regressor, "todense"):
                jr = np.asarray(J_regressor.astype(np.float32).todense())
            else:
                jr = np.array(J_regressor, np.float32)
            if jr.shape[1] == nj and jr.shape[0] >= nv:
                jr = jr.T
            m, n = min(nj, jr.shape[0]), min(nv, jr.shape[1])
            j[:m, :n] = jr[:m, :n]
        w = np.zeros((nv, nj), np.float32)
        if weights is not None:
            ws = np.array(weights, np.float32)
            if ws.shape[0] == nj and ws.shape[1] >= nv:
                ws = ws.T
            m, n = min(nj, ws.shape[1]), min(nv, ws.shape[0])
            w[:n, :m] = ws[:n, :m]
        else:
            joints = j.dot(v.reshape(-1, 3))
            d2 = ((v.reshape(-1, 1, 3) - joints.reshape(1, -1, 3)) ** 2).sum(2)
            idx = d2.argmin(1)
            dis = np.sqrt(d2[np.arange(nv), idx])
            w[np.arange(nv), idx] = np.exp(-dis * dis / (dis.max() * dis.max()))
        w = abs(w)
        w = w / np.maximum(w.sum(1).reshape(-1, 1), 1e-5)

        def flat(src):
            return [] if src is None else [float(x) for x in np.reshape(src, -1)]

        def padded(src, count, default, f=lambda x: x):
            return [f(src[i]) if len(src) > i else (f(src[-1]) if src else default) for i in range(count)]

        sigma_shape, sigma_pose, mean_pose = flat(sigma_shape), flat(sigma_pose), flat(mean_pose)
        self.dim = [ds, npose * 3, nv * 3]
        self.register_buffer("_basis", torch.from_numpy(s).float(), persistent=False)
        self.register_buffer("_template", torch.from_numpy(v).float(), persistent=False)
        self.register_buffer("_skin_weights", torch.from_numpy(w).float(), persistent=False)
        self.register_buffer("_joint_regressor", torch.from_numpy(j).float(), persistent=False)
        self.register_buffer("_parent", torch.from_numpy(np.asarray(self.parent, np.int32)), persistent=False)
        self.sigma = nn.Parameter(torch.tensor(padded(sigma_shape, ds, 1, abs) + [1.0] * (npose * 3), dtype=torch.float32),
                                  requires_grad=False)
        if len(mean_pose) <= npose:
            mean = np.repeat(np.array(padded(mean_pose, npose, 0), np.float32), 3)
        else:
            mean = np.array(padded(mean_pose, npose * 3, 0), np.float32)
        self.pose_mean = nn.Parameter(torch.from_numpy(mean).float().reshape(-1), requires_grad=False)
        if len(sigma_pose) <= npose:
            cov = torch.stack([x * torch.eye(3) for x in padded(sigma_pose, npose, 1)]) if npose else torch.zeros(0, 3, 3)
        elif len(sigma_pose) <= npose * 3:
            cov = torch.diag_embed(torch.tensor(padded(sigma_pose, npose * 3, 1), dtype=torch.float32).view(-1, 3))
        else:
            full = [sigma_pose[i] if len(sigma_pose) > i else float((i % 9) % 4 == 0) for i in range(npose * 9)]
            cov = torch.tensor(full, dtype=torch.float32).view(-1, 3, 3)
        self.pose_cov = nn.Parameter(cov.float(), requires_grad=False)
        self.register_buffer("pose_inv", torch.inverse(self.pose_cov.detach()) if npose else cov.clone(), persistent=False)
        self.learnable = bool(learnable)
        if learnable:
            for t in self.fc + self.weight:
                t.requires_grad_(True)

    # the reference's list attributes
    @property
    def fc(self):
        return [self._basis, self._template]

    @property
    def weight(self):
        return [self._skin_weights, self._joint_regressor]

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if self.pose_cov.numel():
            self.pose_inv = torch.inverse(self.pose_cov.detach())

    def effective_sigma(self):
        """[sigma_shape, diag(pose_cov)]: regulation(x) == sum (x / effective_sigma)^2 when pose_cov is diagonal."""
        return torch.cat([self.sigma.detach()[:self.dim[0]], torch.diagonal(self.pose_cov.detach(), dim1=1, dim2=2).reshape(-1)])

    def pose_cov_is_diagonal(self):
        return _is_diagonal(self.pose_cov.detach())

    def random_input(self, batch_size=1):
        # randn * sigma like LinearMorphableModel.random_input (no host-side check: usable under graph capture), then the
        # reference's per-joint x_i @ pose_cov[i] + pose_mean[i] (face_model.py:306-312)
        x = torch.randn(batch_size, self.sigma.shape[0], device=self.sigma.device, dtype=self.sigma.dtype) * self.sigma
        ds = self.dim[0]
        if self.dim[1] == 0:
            return x
        th = (x[:, ds:].reshape(batch_size, -1, 1, 3) * self.pose_cov.permute(0, 2, 1).unsqueeze(0)).sum(3)
        return torch.cat([x[:, :ds], th.reshape(batch_size, -1) + self.pose_mean.view(1, -1)], 1)

    def forward(self, x):
        from .op import skin

        return skin.skin_vertices(self, x)

    def regulation(self, x):
        ds = self.dim[0]
        l_shape = ((x[:, :ds] / self.sigma[np.newaxis, :ds]) ** 2).sum()
        if self.dim[1] == 0:
            return l_shape
        y = (x[:, ds:].reshape(x.shape[0], -1, 3, 1) * self.pose_inv.to(x.dtype).unsqueeze(0)).sum(2)
        return l_shape + (y ** 2).sum()

    @property
    def n_coeff(self):
        return self.sigma.numel()

    @property
    def n_identity(self):
        """dim[0], unless a loader set `identity_dim` (load_flame: the shape basis' identity columns)."""
        k = getattr(self, "identity_dim", None)
        return self.dim[0] if k is None else min(int(k), self.dim[0])

    def mesh(self, coeff, pose, tri, reg_weight=0.0):
        from .op.skin import skin_mesh

        return skin_mesh(self, coeff, pose, tri, reg_weight) + (None,)

    def prior_sigma(self, batch, shape_reg):
        # fit_loss_rows takes a diagonal prior: exact for a diagonal pose_cov (load_flame's)
        if batch > 1 and shape_reg != 0.0 and not self.pose_cov_is_diagonal():
            raise ValueError("LatentInverter: a batched fit with shape_reg != 0 needs a diagonal pose_cov")
        return self.effective_sigma()

    def fit_extras(self, coeff):
        return {"joints": coeff[0, self.dim[0]:].view(-1, 3).cpu().numpy()}


FLAME_IDENTITY_DIMS = 300                         # of the 400 columns of a published FLAME file's shapedirs


def load_flame(file_name="/data/flame/generic_model.mat"):
    """FLAME -> (LinearBlendSkinningModel, tri int64 [nf, 3]) with the reference's contract (face_model.py:378-408):
    `file_name` is a `.pkl` (pickle, latin1), a `.mat`, or an already loaded dict with the keys `v_template` [nv, 3],
    `shapedirs` [nv, 3, ds], `posedirs` [nv, 3, 9 (nj - 1)], `J_regressor` [nj, nv] (dense or scipy sparse),
    `kintree_table` [2, nj], `weights` [nv, nj] and `f` [nf, 3].  The pose prior's sigmas are the reference's neck / jaw /
    eye values in degrees (pitch, yaw, roll).  The licensed file is not distributed.

    `n_identity` of the model (what the views of a multi-view fit share).  FLAME's files keep identity and expression in one
    `shapedirs`: the published models have 400 columns, 300 of identity followed by 100 of expression, and nothing in the
    file marks the border.  The rule here is that layout's: a shape basis of more than FLAME_IDENTITY_DIMS = 300 columns has
    its first 300 as identity and the rest as expression; a basis of up to 300 columns (a truncated or synthetic file) is
    identity throughout, n_identity = dim[0]."""
    if isinstance(file_name, str):
        if file_name.endswith(".pkl"):
            import pickle

            with open(file_name, "rb") as f:
                data = pickle.load(f, encoding="latin1")
        elif file_name.endswith(".mat"):
            import scipy.io as sio

            data = sio.loadmat(file_name)
        else:
            raise ValueError("load_flame: %r is neither .pkl nor .mat" % (file_name,))
    else:
        data = file_name
    neck, jaw, eye = [10, 30, 5], [10, 1, 1], [10, 10, 1e-5]
    sigma_pose = [a * np.pi / 180 for a in neck + jaw + eye * 2]
    v_template = np.asarray(data["v_template"])
    model = LinearBlendSkinningModel(v_template.shape[0], np.asarray(data["posedirs"]).shape[-1] // 9 + 1,
                                     np.asarray(data["shapedirs"]).shape[-1], v_template, data["J_regressor"],
                                     data["kintree_table"], data["weights"], data["posedirs"], data["shapedirs"], 1,
                                     sigma_pose)
    if model.dim[0] > FLAME_IDENTITY_DIMS:
        model.identity_dim = FLAME_IDENTITY_DIMS
    f = np.asarray(data["f"])
    tri = (f - f.min()).astype(np.int64)
    if tri.shape[0] == 3 and tri.shape[1] != 3:
        tri = tri.T
    return model, torch.from_numpy(np.ascontiguousarray(tri))
