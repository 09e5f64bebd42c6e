"""The optional parts of the latent fit (inversion.LatentInverter): the landmark term, the region of the image loss, the
perspective camera and the photometric term.  Each is a plain object that owns its settings, the buffers the captured iteration reads and the
outputs of the last forward; the inverter holds one of each, or None when the part is off, and calls it at one place of
the iteration.  Nothing here draws random numbers.
"""
import math

import torch


class LandmarkTerm:
    """+ landmark_weight * op.landmark.landmark_loss(vertices, embedding, landmarks, landmark_conf): the fit's landmarks
    against the picture's.  The pose then starts at align.pose_from_landmarks of the mean shape instead of 0
    (`pose_start`).  With lines (and axis) the jaw landmarks slide along the posed mesh's silhouette, with vis landmarks
    turned away from the camera are faded out: op.landmark's pose-aware term, the pose start in two closed-form passes.

    index, bary: the embedding; lines, axis, vis: the pose-aware settings (None: off), dynamic: any of them is on.
    Outputs of the last forward: rows [B] (weighted), landmarks_fit [B, L, 2] (pixel index coordinates of the target),
    and of the pose-aware term contour_fit [B, C] (the vertices the lines selected) and landmark_visibility [B, L] (the
    gate on every landmark's confidence)."""

    def __init__(self, face, pose, size, landmarks, conf, weight, beta, embedding, lines, axis, vis):
        """face: (model, tri) or None; pose: the inverter's pose (its shape and device); size: (H, W) of the target."""
        if landmarks is None:
            raise ValueError("LatentInverter: landmark_conf without landmarks")
        if face is None:
            raise ValueError("LatentInverter: landmarks need fit_shape=True and face=(model, tri): the landmarks of the "
                             "fit are read off the model's mesh")
        model, tri = face
        emb = embedding if embedding is not None else getattr(model, "landmarks", None)
        if emb is None:
            raise ValueError("LatentInverter: landmarks need a landmark embedding and the face model has none "
                             "(model.landmarks is None): pass landmark_embedding=face_model.landmark_embedding(...)")
        device = pose.device
        self.batch, self.size = int(pose.numel()) // 7, tuple(int(x) for x in size)
        self.index, self.bary = (t.detach().to(device).contiguous() for t in emb)
        self.weight, self.beta = float(weight), float(beta)
        n_l = int(self.index.shape[0])
        # the pose-aware term (op.landmark.landmark_loss_ex): contour lines that slide along the silhouette (on the host:
        # the kernels' lists are built from them once), the two anchor vertices of the face's up direction, the gate
        self.dynamic = lines is not None or vis is not None
        if lines is not None and axis is None:
            raise ValueError("LatentInverter: landmark_lines need landmark_axis=(i_up, i_down), the vertices that span "
                             "the face's up direction")
        if vis is not None and not float(vis[0]) <= float(vis[1]):
            raise ValueError("LatentInverter: landmark_vis = (lo, hi) needs lo <= hi")
        self.lines = None if lines is None else tuple(
            (t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)).to(torch.int32).reshape(-1)
            for t in lines)
        self.axis = None if lines is None else (int(axis[0]), int(axis[1]))
        self.vis = None if vis is None else (float(vis[0]), float(vis[1]))
        # the buffers the iteration (and its captured graph) reads; set() rewrites them
        self.target = torch.zeros(self.batch, n_l, 2, device=device)
        self.conf = torch.zeros(self.batch, n_l, device=device)
        self.pose_start = torch.zeros_like(pose)
        self.rows = self.landmarks_fit = self.contour_fit = self.landmark_visibility = None
        # the model's landmark points on its mean shape (host, float64): what the closed-form pose start is fitted to
        with torch.no_grad():
            v_mean = model.mesh(torch.zeros(1, model.n_coeff, device=device), torch.zeros(1, 7, device=device), tri)[0]
            from .op.landmark import landmark_points

            self.points = landmark_points(v_mean.double().cpu(), self.index.cpu(), self.bary.double().cpu())[0].numpy()
            self.mean = v_mean[0].double().cpu().numpy() if self.lines is not None else None
        self.set(landmarks, conf)

    @torch.no_grad()
    def set(self, landmarks, conf):
        """Target landmarks [B, L, 2] (or [L, 2]) and confidences [B, L] (None: 1; landmarks None: all missing) into the
        buffers, and every sample's closed-form starting pose into pose_start (0 for a sample without landmarks)."""
        import numpy as np

        from .align import pose_from_landmarks, pose_from_landmarks_contour
        from .op._dispatch import host_array

        n_l = int(self.index.shape[0])
        if landmarks is None:
            lm, c = np.zeros((self.batch, n_l, 2)), np.zeros((self.batch, n_l))
        else:
            lm = host_array(landmarks).astype(np.float64)
            lm = lm[None] if lm.ndim == 2 else lm
            c = np.ones(lm.shape[:2]) if conf is None else host_array(conf).astype(np.float64).reshape(lm.shape[0], -1)
        if lm.shape != (self.batch, n_l, 2) or c.shape != (self.batch, n_l):
            raise ValueError("LatentInverter: %d images and %d landmarks need landmarks [B, L, 2] and landmark_conf "
                             "[B, L], got %s and %s" % (self.batch, n_l, lm.shape, c.shape))
        if (c < 0).any() or not np.isfinite(c).all():
            raise ValueError("LatentInverter: landmark_conf must be finite and not negative")
        lm = np.where(c[:, :, None] > 0, lm, 0.0)                       # a missing landmark may hold anything
        if not np.isfinite(lm).all():
            raise ValueError("LatentInverter: a landmark with a positive confidence is not finite")
        start = np.zeros((self.batch, 7))
        for b in range(self.batch):
            if c[b].sum() > 0 and self.lines is not None:
                # the jaw landmarks follow the silhouette: a second closed-form pass on the vertices the lines select
                start[b] = pose_from_landmarks_contour(self.mean, (self.index.cpu(), self.bary.cpu()), self.lines,
                                                       self.axis, lm[b], self.size, c[b])[0]
            elif c[b].sum() > 0:
                start[b] = pose_from_landmarks(self.points, lm[b], self.size, c[b])
        self.target.copy_(torch.from_numpy(lm).float())
        self.conf.copy_(torch.from_numpy(c).float())
        self.pose_start.copy_(torch.from_numpy(start).float().view(self.pose_start.shape))

    def __call__(self, v, n_gate):
        """weight * rows [B] of the vertices the consumers see (one launch each way on the device), kept as `rows`;
        keeps landmarks_fit: those of this forward pass, that is of the mesh before the iteration's update (reconstruct
        projects fitted_mesh() for what it writes).  With lines / vis the pose-aware term runs (the same two launches;
        n_gate: the normals a facing gate reads, taken detached) and contour_fit / landmark_visibility keep its
        selection and gate."""
        from .op.landmark import landmark_loss, landmark_loss_ex

        if self.dynamic:
            self.rows, p, sel, gate = landmark_loss_ex(
                v, self.index, self.bary, self.target, self.conf, self.size, self.beta, self.weight,
                normals=n_gate.detach() if self.vis is not None else None, lines=self.lines, axis=self.axis, vis=self.vis)
            self.landmarks_fit, self.contour_fit, self.landmark_visibility = p.detach(), sel.detach(), gate.detach()
        else:
            self.rows, p = landmark_loss(v, self.index, self.bary, self.target, self.conf, self.size, self.beta,
                                         self.weight)
            self.landmarks_fit = p.detach()
        return self.rows


class Region:
    """The region of the image loss: with mask ([B, 1, H, W] in [0, 1]) and / or mask_mesh=True the image terms run on
    y = target + m_eff (image - target) instead of image (op.region.region_blend; m_eff = mask, times the mesh's coverage
    (n . n of the rendered normal map > 1e-3) with mask_mesh): outside the region the loss sees the target itself.  The
    pixel term is then mean((m_eff (image - target))^2) over ALL pixels, not renormalised by the region's area.  An
    all-zero region gives loss 0 and gradient 0.

    mask: the buffer the iteration (and its captured graph) reads; normal_map: the generator's last normal map of this
    forward (mask_mesh only); mask_fit: m_eff [B, 1, H, W] of the last forward."""

    def __init__(self, target, mask, mask_mesh, with_map):
        self.mask_mesh = bool(mask_mesh)
        if self.mask_mesh and not with_map:
            raise ValueError("LatentInverter: mask_mesh=True needs a GeneratorWithMap: the mesh's coverage is read off "
                             "the normal map it renders")
        self.batch = int(target.shape[0])
        self.mask = torch.ones((self.batch, 1) + tuple(target.shape[-2:]), device=target.device)
        self.normal_map = self.mask_fit = None
        self.set(mask)

    @torch.no_grad()
    def set(self, mask):
        """mask [B, 1, H, W] ([1, H, W] / [H, W] at B = 1; None: all ones), finite and in [0, 1], into the buffer."""
        if mask is None:
            self.mask.fill_(1.0)
            return
        m = mask.detach() if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
        if self.batch == 1 and tuple(m.shape) in (tuple(self.mask.shape[1:]), tuple(self.mask.shape[2:])):
            m = m.reshape(self.mask.shape)
        if tuple(m.shape) != tuple(self.mask.shape):
            raise ValueError("LatentInverter: mask %s, the inverter fits %s (a mask is [B, 1, H, W], or [1, H, W] / "
                             "[H, W] for one image)" % (tuple(m.shape), tuple(self.mask.shape)))
        m = m.to(torch.float32)
        if not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0 or float(m.max()) > 1.0:
            raise ValueError("LatentInverter: a mask is finite and in [0, 1]")
        self.mask.copy_(m)

    @staticmethod
    def target_features(perceptual, target):
        """The target's LPIPS features under a region: a render that equals the target inside it must have distance
        exactly 0, so they are normalised the way the loss normalises the render's (lpips.PNetLin.target_features), not
        by `features` as without a region."""
        return [x.detach() for x in perceptual.target_features(target)]

    def see(self, maps, img):
        """Keeps the normal map at the image's resolution, which gates the region in this step (the same nodes: the
        generator rasterises it either way)."""
        self.normal_map = maps[-1].detach()
        if tuple(self.normal_map.shape[-2:]) != tuple(img.shape[-2:]):
            raise RuntimeError("LatentInverter: mask_mesh needs the generator's last normal map at the image's "
                               "resolution, got %s for %s" % (tuple(self.normal_map.shape), tuple(img.shape)))

    def __call__(self, img, target):
        """y = target + m_eff (img - target): outside the region the loss sees the target itself (the target composites
        to itself, so its features stay valid)."""
        from .op.region import region_blend

        img, m_eff = region_blend(img, target, self.mask, self.normal_map)
        self.mask_fit = m_eff.detach()
        return img


class Photometric:
    """+ weight * sum_{c,y,x} on (render - target)^2 / (C H W) per row: the textured mesh against the picture.  render is
    op.texture.sample of a texture variable at the uv map of the mesh the consumers see (op.texture.uv_map with its corners
    through op.texture.explode); on is the uv map's cover, times the region's mask where the inverter has a region.  The
    normaliser is fixed (like the pixel term's, it is not the covered area), so nothing is read back.  The gradient
    reaches the texture and, through the uv map and the rasterizer's backward, the mesh: pose, coefficients and camera.
    It does not reach the latent.  On the device the texture's gradient walks a tap list that a TapPlanner rebuilds in
    every step (the uv map moves with the pose), in a fixed launch sequence, so the iteration can be captured.

    layout: (uv [nt, 2], tri_uv [nf, 3]) or (uv, tri_uv, keep), row-parallel to the mesh's tri (face_model.uv_layout /
    load_uv).  texture: the variable [Bt, C, T, T], Bt = 1 (one texture under all rows: the rows are views of one
    subject) or B; rows [B]: the weighted rows of the last forward; render_fit [B, C, H, W], cover_fit [B, H, W],
    uvmap_fit [B, H, W, 2]: the textured render of the last forward, its coverage and its uv map."""

    def __init__(self, layout, tri, target, size, weight, shared, device, edges=False):
        from .op.landmark import _hw

        if len(layout) not in (2, 3):
            raise ValueError("LatentInverter: photometric = (uv, tri_uv) or (uv, tri_uv, keep), the texture layout")
        uv, tri_uv = layout[0], layout[1]
        keep = layout[2] if len(layout) == 3 else None
        if tuple(tri_uv.shape) != tuple(tri.shape):
            raise ValueError("LatentInverter: the layout's tri_uv %s must be row-parallel to the mesh's tri %s"
                             % (tuple(tri_uv.shape), tuple(tri.shape)))
        self.batch, self.channels = int(target.shape[0]), int(target.shape[1])
        self.hw = tuple(int(x) for x in target.shape[-2:])
        self.size = _hw(size)
        self.weight = float(weight)
        self.bt = 1 if shared or self.batch == 1 else self.batch
        self.tri = tri.detach().to(device).contiguous()
        self.uv = uv.detach().to(device).contiguous()                   # (uv_map takes it in the mesh's float type)
        self.tri_uv = tri_uv.detach().to(device).contiguous()
        self.keep = None if keep is None else keep.detach().to(device).contiguous()
        self.texture = torch.zeros((self.bt, self.channels) + self.size, device=device, requires_grad=True)
        self.planner = None
        if torch.device(device).type == "cuda":
            from .op.texture import TapPlanner

            self.planner = TapPlanner(self.batch, self.hw[0], self.hw[1], self.size, self.bt, device)
        self.scale = self.weight / float(self.channels * self.hw[0] * self.hw[1])
        self.rows = self.render_fit = self.cover_fit = self.uvmap_fit = None
        self.edges = bool(edges)

    def __call__(self, v, target, mask=None):
        """weight * rows [B] of the mesh v [B, nv, 3] the consumers see, kept as `rows`."""
        from .op.texture import sample, uv_map

        uvmap, cover = uv_map(v, self.tri, self.uv, self.tri_uv, self.hw, self.keep, explode=True)
        out = sample(self.texture, uvmap, cover, 0.0, planner=self.planner)
        if self.edges:
            return self._with_edges(v, target, mask, out, cover, uvmap)
        on = cover.unsqueeze(1).to(out.dtype)
        if mask is not None:
            on = on * mask
        d = out - target
        self.rows = (on * (d * d)).sum((1, 2, 3)) * self.scale
        self.render_fit, self.cover_fit, self.uvmap_fit = out.detach(), cover, uvmap.detach()
        return self.rows

    def _with_edges(self, v, target, mask, out, cover, uvmap):
        """photo_edges: the render composited over the picture (c = render where covered, the picture elsewhere) and
        antialiased along the mesh's silhouette edges; rows = scale sum m (aa - target)^2, m the region's mask or 1.  At
        an untouched uncovered pixel the difference is exactly 0; along the outline it depends on where the outline is.
        The face map is a second rasterizer pass on the same v."""
        from .op.edge import antialias, face_map

        face, zbuf = face_map(v, self.tri, self.hw)
        c = torch.where(cover.unsqueeze(1), out, target)
        aa = antialias(c, v, self.tri, face, zbuf)
        d = aa - target
        sq = d * d
        if mask is not None:
            sq = mask * sq
        self.rows = sq.sum((1, 2, 3)) * self.scale
        self.render_fit, self.cover_fit, self.uvmap_fit = aa.detach(), cover, uvmap.detach()
        return self.rows


class Silhouette:
    """+ weight * sum_{y,x} (coverage(v) - mask)^2 / (H W) per row: the outline of the mesh the consumers see against the
    picture's.  coverage is op.edge.coverage, the hard cover antialiased along the mesh's silhouette edges, so the term
    moves the vertices that form the outline; the face map is one rasterizer pass per step.  The normaliser
    is fixed, so nothing is read back.  weight = 1.0 is an untuned starting value.

    mask: the buffer [B, H, W] the iteration (and its captured graph) reads; rows [B]: the weighted rows of the last
    forward; coverage_fit [B, H, W]: the coverage of the last forward."""

    def __init__(self, tri, target, mask, weight, device):
        self.batch = int(target.shape[0])
        self.hw = tuple(int(x) for x in target.shape[-2:])
        self.weight = float(weight)
        self.tri = tri.detach().to(device).contiguous()
        self.mask = torch.zeros((self.batch,) + self.hw, device=device)
        self.scale = self.weight / float(self.hw[0] * self.hw[1])
        self.rows = self.coverage_fit = None
        self.set(mask)

    @torch.no_grad()
    def set(self, mask):
        """mask [B, H, W] or [B, 1, H, W] ([H, W] at B = 1), finite and in [0, 1], into the buffer."""
        m = mask.detach() if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
        if m.dim() == 4 and m.shape[1] == 1:
            m = m[:, 0]
        if self.batch == 1 and tuple(m.shape) == self.hw:
            m = m.reshape(self.mask.shape)
        if tuple(m.shape) != tuple(self.mask.shape):
            raise ValueError("LatentInverter: silhouette %s, the inverter fits %s (a silhouette is [B, H, W] or "
                             "[B, 1, H, W], or [H, W] for one image)" % (tuple(m.shape), tuple(self.mask.shape)))
        m = m.to(torch.float32)
        if not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0 or float(m.max()) > 1.0:
            raise ValueError("LatentInverter: a silhouette is finite and in [0, 1]")
        self.mask.copy_(m)

    def __call__(self, v):
        """weight * rows [B] of the mesh v [B, nv, 3] the consumers see, kept as `rows`."""
        from .op.edge import coverage

        alpha = coverage(v, self.tri, self.hw)
        d = alpha - self.mask
        self.rows = (d * d).sum((1, 2)) * self.scale
        self.coverage_fit = alpha.detach()
        return self.rows


class Camera:
    """The perspective camera: kappa [B] = 1 / distance, the camera's distance from the plane z = 0 of pose space in
    half-picture-widths.  The posed mesh passes through op.camera.project before the landmark term and the generator see
    it: one node, one launch each way, after the model's node (or the fixed mesh's pose).  The consumers stay
    orthographic; for a facing gate the same launch writes n_view, the normals as the gate must read them under a camera,
    while the generator keeps the camera-space normals.  fit=True makes kappa a variable with its own Adam group: one
    value per row, per view under a shared identity, unconstrained (a negative fit is reported as it is).
    Known degeneracy: for image-plane positions, (e^s, t_xy, t_z, kappa) and (e^s / (1 - kappa t_z), t_xy / (1 - kappa t_z),
    0, kappa) project identically, so t_z and the scale trade off along a flat direction; compare projections, kappa and
    angles between fits, never raw t_z or s.  kappa is only weakly determined by the image terms alone: it wants landmarks.

    kappa: the value (requires_grad with fit); start: what reset() puts back; grad: on the device the buffer of kappa's
    Adam, which the projection's backward writes itself (None: autograd's kappa.grad)."""

    def __init__(self, camera, fit, batch, device):
        """camera: a float or [B] of kappa, the start values."""
        self.fit = bool(fit)
        if camera is None:
            raise ValueError("LatentInverter: fit_camera=True needs camera=, the start value of kappa = 1 / distance")
        if isinstance(camera, torch.Tensor):
            k = camera.detach().to(device="cpu", dtype=torch.float64).reshape(-1)
        elif isinstance(camera, (int, float)) and not isinstance(camera, bool):
            k = torch.full((batch,), float(camera), dtype=torch.float64)
        else:
            try:
                k = torch.as_tensor([float(x) for x in camera], dtype=torch.float64)
            except (TypeError, ValueError):
                raise ValueError("LatentInverter: camera is a float or %d floats, got %r" % (batch, camera))
        if k.numel() == 1 and batch > 1 and not isinstance(camera, (int, float)):
            k = k.expand(batch).clone()
        if k.numel() != batch:
            raise ValueError("LatentInverter: %d images need camera [%d] (or one float), got %d values"
                             % (batch, batch, k.numel()))
        if not all(math.isfinite(x) for x in k.tolist()):
            raise ValueError("LatentInverter: camera (kappa = 1 / distance) must be finite")
        self.start = k.to(device=device, dtype=torch.float32)
        self.kappa = self.start.clone().requires_grad_(self.fit)
        self.grad = None

    def project(self, v, n, gate=False):
        """The mesh the consumers see, of the camera-space mesh (op.camera.project: one launch each way on the device):
        (v', the normals a facing gate reads).  gate: a facing gate will read them, so the same launch writes n_view;
        without one they are n itself."""
        from .op.camera import project

        # (on the device a fitted kappa's gradient goes straight into its Adam's buffer)
        out = self.grad if torch.is_grad_enabled() else None
        if gate:
            return project(v, self.kappa, normals=n, gkappa_out=out)
        return project(v, self.kappa, gkappa_out=out), n

    @torch.no_grad()
    def reset(self):
        self.kappa.copy_(self.start)
