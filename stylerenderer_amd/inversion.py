"""Latent inversion of a face image (BASELINE config[4]).

The reference has no fitting script; its pieces are the generator's `input_is_latent` entry
(reference model.py:224-295), the differentiable rasterizer (op/rasterize.py:17-82) and the LPIPS metric
(lpips/networks_basic.py:27-92).  This module defines the loop BASELINE.json names:

    variables   w [B, n_latent, style_dim]  (W+ latent, initialised at the mean latent)
                pose [7] = yaw, pitch, roll (rad), tx, ty, tz, log-scale of the 3DMM mesh ([B, 7] when B > 1)
                coeff [B, d] = 3DMM shape + expression coefficients (fit_shape=True only; from 0, the mean face)
    forward     vertices = v0 @ (exp(s) * R(yaw, pitch, roll)) + t ; normals = n0 @ R
                image = GeneratorWithMap([w], (vertices, normals, tri), input_is_latent=True, noise=fixed)
                with fit_shape=True: vertices, normals = op.morph.morph_mesh(face model, coeff, pose, tri), or
                op.skin.skin_mesh for a LinearBlendSkinningModel (coeff = shape, then one axis-angle per joint),
                op.blend.blend_mesh for a BlendShapeModel (coeff = identity logits, then expression logits; 0 is the
                mean identity with every expression at sigmoid(0))
    loss        LPIPS-shaped distance(image, target) + pixel_weight * mean((image - target)^2)
                (+ shape_reg * face_model.regulation(coeff), reference face_model.py:73-74, with fit_shape=True)
                (+ landmark_weight * op.landmark.landmark_loss(vertices, embedding, landmarks, landmark_conf), with
                 landmarks=: the fit's landmarks against the picture's; the pose then starts at
                 align.pose_from_landmarks of the mean shape instead of 0; with landmark_lines= (and landmark_axis=) the
                 jaw landmarks slide along the posed mesh's silhouette, with landmark_vis= landmarks turned away from the
                 camera are faded out: op.landmark's pose-aware term, the pose start in two closed-form passes)
                with mask= ([B, 1, H, W] in [0, 1]) and / or mask_mesh=True the image terms run on
                y = target + m_eff (image - target) instead of image (op.region.region_blend; m_eff = mask, times the
                mesh's coverage (n . n of the rendered normal map > 1e-3) with mask_mesh): outside the region the loss
                sees the target itself.  The pixel term is then mean((m_eff (image - target))^2) over ALL pixels, not
                renormalised by the region's area.  An all-zero region gives loss 0 and gradient 0.
    update      Adam, `steps` iterations (default 400)

A target [B, 3, H, W] with B > 1 fits B independent images in one iteration (one captured graph): every variable
carries the batch, the noise is one fixed set broadcast over it, and the objective is sum_b L_b, so each sample's
gradient is the one it would have alone and the element-wise Adam moves every sample along its own single-image
trajectory.  Per-sample losses come from op.lpips_layer.mse_rows and fit_loss_rows (one launch each way for the sum of
the LPIPS layers, the pixel term and the prior); `loss_value` is [B] and `run` returns [steps, B].  B = 1 keeps the
shapes and launches above.  `reset(target)` re-targets an inverter whose graph is captured: the next `run` computes
exactly what a fresh inverter on that target would, with no new warm-up or capture.

With shared_identity=K (fit_shape=True, 1 <= K <= the model's n_coeff; the models name their own K as `n_identity`) the B
rows are B views of ONE subject: the leading K columns of coeff are one variable shared by all rows, and everything else
(w, pose, the remaining columns: expression, FLAME's joints, the landmarks and masks) stays per view.  coeff keeps its
shape [B, d]; between backward and the optimiser's step the leading K columns of every row of coeff.grad are replaced by
their sum over the rows (op.share.share_rows_, one launch inside the captured step), which is the gradient of sum_b L_b
with respect to the shared variable.  All rows start equal (zero, also after `reset`), see the same gradient and pass
through the same element-wise Adam, so coeff[:, :K] stays equal across the rows bit for bit, with no copy and no second
parameter.  Every row keeps its own prior term, as in the batched fit: the objective is the sum of the V single-view
objectives under the constraint, so the shared columns' prior enters V times; it is not rescaled.

With camera= (a float or [B] of kappa = 1 / distance, the camera's distance from the plane z = 0 of pose space in
half-picture-widths) the posed mesh passes through op.camera.project before the landmark term and the generator see it: one
node, one launch each way, after the model's node (or the fixed mesh's pose).  The consumers stay orthographic; with
landmark_vis the same launch writes n_view, the normals as a facing gate must read them under a camera, while the generator
keeps the camera-space normals.  fit_camera=True makes kappa a variable [B] with its own Adam group (camera_lr, a starting
value, not tuned): one value per row, per view under shared_identity, unconstrained (a negative fit is reported as it is).
`fitted_mesh()` returns what the consumers saw, `fitted_mesh(projected=False)` the camera-space mesh; `reset` puts kappa
back at its start.  With camera=None there is no node and no parameter: the iteration and its captured graph are unchanged.
Known degeneracy: for image-plane positions, (e^s, t_xy, t_z, kappa) and (e^s / (1 - kappa t_z), t_xy / (1 - kappa t_z), 0,
kappa) project identically, so t_z and the scale trade off along a flat direction; compare projections, kappa and angles
between fits, never raw t_z or s.  kappa is only weakly determined by the image terms alone: it wants landmarks.

The pose gradient reaches the vertices only through the rasterizer's backward (deterministic gather, so two
runs from the same state produce bit-identical trajectories).  On a GPU the whole iteration — forward, backward,
Adam — is one hipGraph (batch 1 is launch-latency bound: ~2 000 kernels per step), replayed `steps` times; the
loss history stays on the device until the end.
"""
import torch
from torch import optim

from . import graphs, utils_3d


class _FlatAdamSet:
    """The per-variable optim.FlatAdam instances of the device path behind torch.optim's two calls (scripts and callers
    written against `inverter.optim.step()` keep working: ADVICE r4)."""

    def __init__(self, adams, direct=()):
        self.adams = adams
        # variables whose backward node writes the gradient into the optimiser's buffer itself (op.camera's gkappa_out):
        # no p.grad, no copy
        self.direct = tuple(direct)

    @torch.no_grad()
    def step(self):
        for p, adam in self.adams:
            if any(p is q for q in self.direct):
                adam.step()
            elif p.grad is not None:
                adam.flat_g[:p.numel()].copy_(p.grad.reshape(-1))
                adam.step()

    def zero_grad(self, set_to_none=True):
        for p, _ in self.adams:
            p.grad = None


class LatentInverter:
    def __init__(self, generator, perceptual, target, mesh, lr=0.05, pose_lr=0.01, pixel_weight=1.0, noise=None,
                 n_mean_latent=4096, use_graph=None, optimise_pose=True, *, face=None, fit_shape=False, coeff_lr=0.01,
                 shape_reg=0.0, landmarks=None, landmark_conf=None, landmark_weight=1.0, landmark_beta=1.0,
                 landmark_embedding=None, landmark_lines=None, landmark_axis=None, landmark_vis=None, mask=None,
                 mask_mesh=False, shared_identity=None, camera=None, fit_camera=False, camera_lr=0.01):
        self.g = generator.eval()
        self.perceptual = perceptual.eval()
        for p in list(self.g.parameters()) + list(self.perceptual.parameters()):
            p.requires_grad_(False)
        # frozen networks: tap-major weights, demodulation matrices and adjoints are prepared once, not per step
        from .op.weight_prep import freeze_prepared_weights

        freeze_prepared_weights(self.g)
        self.device = target.device
        # (a copy: reset() writes new targets into it under the captured graph)
        self.target = target.detach().clone()
        self.batch = int(self.target.shape[0])
        self.fit_shape = bool(fit_shape)
        self.shape_reg = float(shape_reg)
        if self.fit_shape:
            if face is None:
                raise ValueError("LatentInverter: fit_shape=True needs face=(LinearMorphableModel, tri)")
            self.face_model, self.tri = face[0], face[1].detach()
            self.face_model.requires_grad_(False)
            # the sigma of a diagonal Gaussian prior for fit_loss_rows, or None (the blendshape model's Dirichlet / Beta
            # prior): the per-sample losses then take each sample's prior from the node
            self._prior_sigma = self.face_model.prior_sigma(self.batch, self.shape_reg)
            # the fitted mesh comes from the morphable-mesh node; `mesh` is not used
            self.v0 = self.n0 = None
        else:
            self.v0, self.n0, self.tri = (t.detach() for t in mesh)
        # the rows are views of one subject: the leading columns of coeff are tied in every step (None: off)
        self.shared_identity = None
        if shared_identity is not None:
            if not self.fit_shape:
                raise ValueError("LatentInverter: shared_identity needs fit_shape=True and face=(model, tri)")
            if isinstance(shared_identity, bool) or not isinstance(shared_identity, int) or not (
                    1 <= shared_identity <= self.face_model.n_coeff):
                raise ValueError("LatentInverter: shared_identity is an int in [1, %d] (the model's coefficients), got %r"
                                 % (self.face_model.n_coeff, shared_identity))
            self.shared_identity = int(shared_identity)
        self.pixel_weight = float(pixel_weight)
        self.with_map = hasattr(self.g, "norm_to_style")
        with torch.no_grad():
            mean_w = self.g.mean_latent(n_mean_latent)                                  # [1, D]
            self.target_feats = [f.detach() for f in self.perceptual.features(self.target)]
        self._mean_w = mean_w
        self.w = mean_w.unsqueeze(1).repeat(self.batch, self.g.n_latent, 1).clone().requires_grad_(True)
        pose_shape = (7,) if self.batch == 1 else (self.batch, 7)
        self.pose = torch.zeros(pose_shape, device=self.device, requires_grad=optimise_pose)
        # the landmark term: not part of the iteration at all without landmarks
        self.with_landmarks = landmarks is not None
        self.landmarks_fit = None
        # of the pose-aware term (landmark_lines / landmark_vis): the vertices the contour lines selected [B, C] and the
        # gate on every landmark's confidence [B, L] in the last forward
        self.contour_fit = self.landmark_visibility = None
        if self.with_landmarks:
            self._init_landmarks(landmarks, landmark_conf, landmark_weight, landmark_beta, landmark_embedding,
                                 landmark_lines, landmark_axis, landmark_vis)
        elif landmark_conf is not None:
            raise ValueError("LatentInverter: landmark_conf without landmarks")
        # the region of the image loss (op.region): not part of the iteration at all without mask / mask_mesh
        self.mask_mesh = bool(mask_mesh)
        self.with_mask = mask is not None or self.mask_mesh
        self.mask_fit = None                             # m_eff [B, 1, H, W] of the last forward
        self._normal_map = None
        if self.mask_mesh and not self.with_map:
            raise ValueError("LatentInverter: mask_mesh=True needs a GeneratorWithMap: the mesh's coverage is read off "
                             "the normal map it renders")
        if self.with_mask:
            # the buffer the iteration (and its captured graph) reads; reset() rewrites it
            self._mask = torch.ones((self.batch, 1) + tuple(self.target.shape[-2:]), device=self.device)
            self._set_mask(mask)
            with torch.no_grad():
                self.target_feats = self._features_of_target()
        # 3DMM coefficients [B, d], from the mean face
        self.coeff = (torch.zeros(self.batch, self.face_model.n_coeff, device=self.device, requires_grad=True)
                      if self.fit_shape else None)
        self.noise = noise if noise is not None else [n.detach() for n in self.g.make_noise()]
        # the perspective camera (op.camera): not part of the iteration at all with camera=None
        self.camera = self._camera_start = self._camera_grad = None
        self.fit_camera = bool(fit_camera)
        if camera is not None:
            self._init_camera(camera)
        elif self.fit_camera:
            raise ValueError("LatentInverter: fit_camera=True needs camera=, the start value of kappa = 1 / distance")
        on_gpu = self.device.type == "cuda"
        groups = [{"params": [self.w], "lr": lr}]
        if optimise_pose:
            groups.append({"params": [self.pose], "lr": pose_lr})
        if self.fit_shape:
            groups.append({"params": [self.coeff], "lr": coeff_lr})
        if self.fit_camera:
            groups.append({"params": [self.camera], "lr": camera_lr})
        if on_gpu:
            # one sr_adam_flat launch per variable (optim.FlatAdam, the training loop's optimiser) instead of the ~30
            # multi-tensor passes of torch's capturable foreach Adam: at batch 1 every launch is ~5 us of an 8 ms step
            from .optim import ALIGN, FlatAdam

            self._adams = []
            for g_ in groups:
                p = g_["params"][0]
                flat_g = torch.zeros((p.numel() + ALIGN - 1) // ALIGN * ALIGN, device=self.device)
                # kappa's Adam counts its steps on the latent's counter (they step together, the latent first): with the
                # gradient written into flat_g by the camera's backward, the variable costs one launch per step
                own = p is self.camera
                self._adams.append((p, FlatAdam([p], flat_g, lr=g_["lr"], betas=(0.9, 0.999),
                                                step_from=self._adams[0][1] if own else None)))
                if own:
                    self._camera_grad = flat_g
            self.optim = _FlatAdamSet(self._adams, [self.camera] if self.fit_camera else [])
        else:
            self._adams = None
            self.optim = optim.Adam(groups, betas=(0.9, 0.999))
        self.use_graph = on_gpu if use_graph is None else bool(use_graph)
        self.graph = None
        self.loss_value = torch.zeros(() if self.batch == 1 else (self.batch,), device=self.device)
        self.image = None

    # ---- model ----------------------------------------------------------------------------------------
    skinned = property(lambda self: self.fit_shape and self.face_model.kind == "skinned")       # FLAME: op.skin
    blended = property(lambda self: self.fit_shape and self.face_model.kind == "blended")       # FaceWarehouse: op.blend

    # ---- camera --------------------------------------------------------------------------------------
    def _init_camera(self, camera):
        """camera: a float or [B] of kappa = 1 / distance, the start values (kept for reset)."""
        import math

        if isinstance(camera, torch.Tensor):
            k = camera.detach().to(device="cpu", dtype=torch.float64).reshape(-1)
        elif isinstance(camera, (int, float)) and not isinstance(camera, bool):
            k = torch.full((self.batch,), float(camera), dtype=torch.float64)
        else:
            try:
                k = torch.as_tensor([float(x) for x in camera], dtype=torch.float64)
            except (TypeError, ValueError):
                raise ValueError("LatentInverter: camera is a float or %d floats, got %r" % (self.batch, camera))
        if k.numel() == 1 and self.batch > 1 and not isinstance(camera, (int, float)):
            k = k.expand(self.batch).clone()
        if k.numel() != self.batch:
            raise ValueError("LatentInverter: %d images need camera [%d] (or one float), got %d values"
                             % (self.batch, self.batch, k.numel()))
        if not all(math.isfinite(x) for x in k.tolist()):
            raise ValueError("LatentInverter: camera (kappa = 1 / distance) must be finite")
        self._camera_start = k.to(device=self.device, dtype=torch.float32)
        self.camera = self._camera_start.clone().requires_grad_(self.fit_camera)

    def _project(self, v, n, gate=False):
        """The mesh the consumers see: (v', n_view or None) of the camera-space mesh (op.camera.project: one launch each
        way on the device).  gate: a facing gate will read the normals, so the same launch writes n_view."""
        from .op.camera import project

        # (on the device a fitted kappa's gradient goes straight into its Adam's buffer)
        out = self._camera_grad if torch.is_grad_enabled() else None
        if gate:
            return project(v, self.camera, normals=n, gkappa_out=out)
        return project(v, self.camera, gkappa_out=out), None

    # ---- landmarks -----------------------------------------------------------------------------------
    def _init_landmarks(self, landmarks, conf, weight, beta, embedding, lines=None, axis=None, vis=None):
        if not self.fit_shape:
            raise ValueError("LatentInverter: landmarks need fit_shape=True and face=(model, tri): the landmarks of the "
                             "fit are read off the model's mesh")
        emb = embedding if embedding is not None else getattr(self.face_model, "landmarks", None)
        if emb is None:
            raise ValueError("LatentInverter: landmarks need a landmark embedding and the face model has none "
                             "(model.landmarks is None): pass landmark_embedding=face_model.landmark_embedding(...)")
        self._lmk_idx, self._lmk_bary = (t.detach().to(self.device).contiguous() for t in emb)
        self.landmark_weight, self.landmark_beta = float(weight), float(beta)
        n_l = int(self._lmk_idx.shape[0])
        # the pose-aware term (op.landmark.landmark_loss_ex): contour lines that slide along the silhouette (on the host:
        # the kernels' lists are built from them once), the two anchor vertices of the face's up direction, the gate
        self._lmk_dynamic = lines is not None or vis is not None
        if lines is not None and axis is None:
            raise ValueError("LatentInverter: landmark_lines need landmark_axis=(i_up, i_down), the vertices that span "
                             "the face's up direction")
        if vis is not None and not float(vis[0]) <= float(vis[1]):
            raise ValueError("LatentInverter: landmark_vis = (lo, hi) needs lo <= hi")
        self._lmk_lines = None if lines is None else tuple(
            (t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)).to(torch.int32).reshape(-1)
            for t in lines)
        self._lmk_axis = None if lines is None else (int(axis[0]), int(axis[1]))
        self._lmk_vis = None if vis is None else (float(vis[0]), float(vis[1]))
        # the buffers the iteration (and its captured graph) reads; reset() rewrites them
        self._lmk_target = torch.zeros(self.batch, n_l, 2, device=self.device)
        self._lmk_conf = torch.zeros(self.batch, n_l, device=self.device)
        self._pose_start = torch.zeros_like(self.pose)
        # the model's landmark points on its mean shape (host, float64): what the closed-form pose start is fitted to
        with torch.no_grad():
            v_mean = self.face_model.mesh(torch.zeros(1, self.face_model.n_coeff, device=self.device),
                                          torch.zeros(1, 7, device=self.device), self.tri)[0]
            from .op.landmark import landmark_points

            self._lmk_points = landmark_points(v_mean.double().cpu(), self._lmk_idx.cpu(),
                                               self._lmk_bary.double().cpu())[0].numpy()
            self._lmk_mean = v_mean[0].double().cpu().numpy() if self._lmk_lines is not None else None
        self._set_landmarks(landmarks, conf)
        with torch.no_grad():
            self.pose.copy_(self._pose_start)

    @torch.no_grad()
    def _set_landmarks(self, landmarks, conf):
        """Target landmarks [B, L, 2] (or [L, 2]) and confidences [B, L] (None: 1; landmarks None: all missing) into the
        buffers, and every sample's closed-form starting pose into _pose_start (0 for a sample without landmarks)."""
        import numpy as np

        from .align import pose_from_landmarks, pose_from_landmarks_contour
        from .op._dispatch import host_array

        n_l = int(self._lmk_idx.shape[0])
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
        size = tuple(int(x) for x in self.target.shape[-2:])
        start = np.zeros((self.batch, 7))
        for b in range(self.batch):
            if c[b].sum() > 0 and self._lmk_lines is not None:
                # the jaw landmarks follow the silhouette: a second closed-form pass on the vertices the lines select
                start[b] = pose_from_landmarks_contour(self._lmk_mean, (self._lmk_idx.cpu(), self._lmk_bary.cpu()),
                                                       self._lmk_lines, self._lmk_axis, lm[b], size, c[b])[0]
            elif c[b].sum() > 0:
                start[b] = pose_from_landmarks(self._lmk_points, lm[b], size, c[b])
        self._lmk_target.copy_(torch.from_numpy(lm).float())
        self._lmk_conf.copy_(torch.from_numpy(c).float())
        self._pose_start.copy_(torch.from_numpy(start).float().view(self._pose_start.shape))

    # ---- region ---------------------------------------------------------------------------------------
    def _features_of_target(self):
        """The target's LPIPS features.  With a region a render that equals the target inside it must have distance
        exactly 0, so they are normalised the way the loss normalises the render's (lpips.PNetLin.target_features);
        without one they are `features`, as ever."""
        f = self.perceptual.target_features if self.with_mask else self.perceptual.features
        return [x.detach() for x in f(self.target)]

    @torch.no_grad()
    def _set_mask(self, mask):
        """mask [B, 1, H, W] ([1, H, W] / [H, W] at B = 1; None: all ones), finite and in [0, 1], into the buffer."""
        if mask is None:
            self._mask.fill_(1.0)
            return
        m = mask.detach() if isinstance(mask, torch.Tensor) else torch.as_tensor(mask)
        if self.batch == 1 and tuple(m.shape) in (tuple(self._mask.shape[1:]), tuple(self._mask.shape[2:])):
            m = m.reshape(self._mask.shape)
        if tuple(m.shape) != tuple(self._mask.shape):
            raise ValueError("LatentInverter: mask %s, the inverter fits %s (a mask is [B, 1, H, W], or [1, H, W] / "
                             "[H, W] for one image)" % (tuple(m.shape), tuple(self._mask.shape)))
        m = m.to(torch.float32)
        if not bool(torch.isfinite(m).all()) or float(m.min()) < 0.0 or float(m.max()) > 1.0:
            raise ValueError("LatentInverter: a mask is finite and in [0, 1]")
        self._mask.copy_(m)

    def _landmark_term(self, v, n=None):
        """landmark_weight * rows [B] of the posed vertices (one launch each way on the device); keeps the fitted
        landmarks [B, L, 2] (pixel index coordinates of the target) as landmarks_fit: those of this forward pass, that is
        of the mesh before the iteration's update (reconstruct projects fitted_mesh() for what it writes).  With
        landmark_lines / landmark_vis the pose-aware term runs (the same two launches; n: the posed normals, read
        detached) and contour_fit / landmark_visibility keep its selection and gate."""
        from .op.landmark import landmark_loss, landmark_loss_ex

        if self._lmk_dynamic:
            self._lmk_rows, p, sel, gate = landmark_loss_ex(
                v, self._lmk_idx, self._lmk_bary, self._lmk_target, self._lmk_conf, tuple(self.target.shape[-2:]),
                self.landmark_beta, self.landmark_weight, normals=n.detach() if self._lmk_vis is not None else None,
                lines=self._lmk_lines, axis=self._lmk_axis, vis=self._lmk_vis)
            self.landmarks_fit, self.contour_fit, self.landmark_visibility = p.detach(), sel.detach(), gate.detach()
            return
        self._lmk_rows, p = landmark_loss(v, self._lmk_idx, self._lmk_bary, self._lmk_target, self._lmk_conf,
                                          tuple(self.target.shape[-2:]), self.landmark_beta, self.landmark_weight)
        self.landmarks_fit = p.detach()

    def _shape_mesh(self):
        """(v, n, tri, reg) of the fitted coefficients and pose (the model's node — op.morph / op.skin / op.blend: no
        library GEMM on the device)."""
        v, n, reg, self._prior_rows = self.face_model.mesh(self.coeff, self.pose.view(-1, 7), self.tri, self.shape_reg)
        return v, n, self.tri, reg

    def posed_mesh(self, projected=True):
        """(v, n, tri) of the current variables.  With a camera and projected=True, v is what the consumers see (v' of
        op.camera.project) and n stays the camera-space normal; projected=False gives the camera-space mesh."""
        v, n, tri = self._camera_space_mesh()
        if self.camera is not None and projected:
            v = self._project(v, n)[0]
        return v, n, tri

    def _camera_space_mesh(self):
        if self.fit_shape:
            return self._shape_mesh()[:3]
        lin, rot = utils_3d.pose_matrices(self.pose)                                    # [B, 3, 3] each
        # [nv, 3] x [3, 3]: one streaming kernel each (utils_3d.affine3), not a 3-wide library GEMM
        t = self.pose[3:6].view(1, 3) if self.batch == 1 else self.pose[:, 3:6]
        v = utils_3d.affine3(self.v0, lin, t)
        n = utils_3d.affine3(self.n0, rot)
        return v.contiguous(), n.contiguous(), self.tri

    def fitted_mesh(self, projected=True):
        """(v, n, tri) of the current fit, posed and detached.  With a camera this is what the consumers saw: the
        projected vertices v' and n_view, the normals as the facing gates read them (op.camera); projected=False returns
        the camera-space mesh.  Without a camera the two are the same."""
        with torch.no_grad():
            v, n, tri = self._camera_space_mesh()
            if self.camera is not None and projected:
                v, n = self._project(v.contiguous(), n.contiguous(), gate=True)
        return v.detach(), n.detach(), tri

    def render(self):
        self._reg = None
        if self.with_map:
            if self.fit_shape:
                v, n, tri, self._reg = self._shape_mesh()
                n_gate = n
                if self.camera is not None:
                    gate = self.with_landmarks and self._lmk_vis is not None
                    v, n_view = self._project(v, n, gate)
                    n_gate = n_view if gate else n
                mesh = (v, n, tri)                       # (the generator keeps the camera-space normals)
                if self.with_landmarks:
                    self._landmark_term(v, n_gate)
            else:
                mesh = self.posed_mesh()
            if self.mask_mesh:
                # the normal map at the image's resolution gates the region per step (the same nodes: the generator
                # rasterises it either way)
                img, _, maps = self.g([self.w], mesh, input_is_latent=True, noise=self.noise, return_normals=True)
                self._normal_map = maps[-1].detach()
                if tuple(self._normal_map.shape[-2:]) != tuple(img.shape[-2:]):
                    raise RuntimeError("LatentInverter: mask_mesh needs the generator's last normal map at the image's "
                                       "resolution, got %s for %s" % (tuple(self._normal_map.shape), tuple(img.shape)))
            else:
                img, _, _ = self.g([self.w], mesh, input_is_latent=True, noise=self.noise)
        else:
            if self.with_landmarks:
                v, n = self._shape_mesh()[:2]
                if self.camera is not None:
                    gate = self._lmk_vis is not None
                    v, n_view = self._project(v, n, gate)
                    n = n_view if gate else n
                self._landmark_term(v, n)
            img, _ = self.g([self.w], input_is_latent=True, noise=self.noise)
        return img

    def loss(self, img):
        if self.with_mask:
            # the loss below runs on y = target + m_eff (img - target): outside the region it sees the target itself
            # (target composites to itself, so target_feats stay valid)
            from .op.region import region_blend

            img, m_eff = region_blend(img, self.target, self._mask, self._normal_map)
            self.mask_fit = m_eff.detach()
        if self.batch > 1:
            return self._loss_rows(img)
        from .op.lpips_layer import mse

        d = self.perceptual.distance_to(self.target_feats, img).mean()
        value = d + self.pixel_weight * mse(img, self.target)
        if self.fit_shape and self.shape_reg != 0.0 and getattr(self, "_reg", None) is not None:
            value = value + self._reg                    # shape_reg * regulation(coeff), from the node's forward
        if self.with_landmarks:
            value = value + self._lmk_rows.view(())
        return value

    def _loss_rows(self, img):
        """sum_b L_b; the per-sample L_b go to self._rows (one fit_loss_rows node: no per-sample launches)."""
        from .op.lpips_layer import fit_loss_rows, mse_rows

        layers = self.perceptual.layer_distances(self.target_feats, img)
        prior = self.fit_shape and self.shape_reg != 0.0 and getattr(self, "_reg", None) is not None
        if prior and self._prior_rows is not None:
            self._rows, total = fit_loss_rows(layers, mse_rows(img, self.target), self.pixel_weight, reg=self._reg,
                                              prior_rows=self._prior_rows)
        else:
            self._rows, total = fit_loss_rows(layers, mse_rows(img, self.target), self.pixel_weight,
                                              coeff=self.coeff if prior else None,
                                              sigma=self._prior_sigma if prior else None, shape_reg=self.shape_reg,
                                              reg=self._reg if prior else None)
        if self.with_landmarks:
            self._rows = self._rows + self._lmk_rows.detach()
            total = total + self._lmk_rows.sum()
        return total

    def _iteration(self):
        self.w.grad = None
        self.pose.grad = None
        if self.coeff is not None:
            self.coeff.grad = None
        if self.camera is not None:
            self.camera.grad = None
        img = self.render()
        value = self.loss(img)
        value.backward()
        if self.shared_identity is not None:
            # the gradient of the shared variable: the rows' sum, written into every row
            from .op.share import share_rows_

            if not self.coeff.grad.is_contiguous():
                self.coeff.grad = self.coeff.grad.contiguous()
            share_rows_(self.coeff.grad, self.shared_identity)
        self.optim.step()
        self.loss_value.copy_(value.detach() if self.batch == 1 else self._rows)
        self.image = img.detach()

    # ---- driver ---------------------------------------------------------------------------------------
    def _warm_and_capture(self, history, warmup=3):
        """`warmup` real iterations on a side stream (lazy initialisation, Adam state), then one capture.
        Returns the number of optimisation steps already taken (capture itself executes nothing)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for k in range(warmup):
                self._iteration()
                history[k] = self.loss_value
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = graphs.capture(self._iteration)      # memset nodes of torch's reductions repaired: graphs.py
        return warmup

    @torch.no_grad()
    def reset(self, target, landmarks=None, landmark_conf=None, mask=None):
        """Re-targets the inverter to `target` (the shape of the first): copies it and its LPIPS features into the
        buffers the captured graph reads, puts w back at the mean latent, pose and coeff at zero, and zeroes the Adam
        moments and step counts.  An inverter built with landmarks also takes the new picture's `landmarks` and
        `landmark_conf` into its buffers and puts the pose at their closed-form start (landmarks None: every landmark
        missing, pose 0).  `run(steps)` then gives what a fresh inverter on `target` (and these landmarks) gives (same
        mean latent, same noise), bit for bit, without a new warm-up or capture.  landmarks_fit, contour_fit and
        landmark_visibility are outputs of the (possibly captured) iteration: they keep the previous picture's values
        until the next step writes them.  An inverter built with a region (mask= or mask_mesh=) takes the new picture's
        `mask` into its buffer (None: all ones); mask_fit is an output of the iteration like landmarks_fit."""
        target = target.detach()
        if not self.with_mask and mask is not None:
            raise ValueError("LatentInverter.reset: this inverter was built without a mask; the region blend is part of "
                             "the captured iteration or it is not")
        if not self.with_landmarks and (landmarks is not None or landmark_conf is not None):
            raise ValueError("LatentInverter.reset: this inverter was built without landmarks; the landmark term is "
                             "part of the captured iteration or it is not")
        if tuple(target.shape) != tuple(self.target.shape):
            raise ValueError("LatentInverter.reset: target %s, the inverter fits %s"
                             % (tuple(target.shape), tuple(self.target.shape)))
        if self.with_mask:
            self._set_mask(mask)
        self.target.copy_(target)
        for buf, f in zip(self.target_feats, self._features_of_target()):
            buf.copy_(f)
        self.w.copy_(self._mean_w.unsqueeze(1).expand_as(self.w))
        if self.with_landmarks:
            self._set_landmarks(landmarks, landmark_conf)
            self.pose.copy_(self._pose_start)
        else:
            self.pose.zero_()
        if self.coeff is not None:
            self.coeff.zero_()
        if self.camera is not None:
            self.camera.copy_(self._camera_start)
        if self._adams is not None:
            for _, adam in self._adams:
                for t in (adam.m, adam.v, adam.step_t, adam.flat_g):
                    t.zero_()
        else:
            self.optim.state.clear()                     # torch's Adam initialises its state at the next step
        self.loss_value.zero_()

    def run(self, steps=400):
        """Runs `steps` Adam iterations; returns the loss history [steps] ([steps, B] for B > 1; device tensor: no host
        read here)."""
        history = torch.zeros((steps,) if self.batch == 1 else (steps, self.batch), device=self.device)
        done = 0
        if self.use_graph and self.graph is None and steps > 4:
            done = self._warm_and_capture(history)
        for i in range(done, steps):
            if self.graph is not None:
                self.graph.replay()
            else:
                self._iteration()
            history[i] = self.loss_value
        return history
