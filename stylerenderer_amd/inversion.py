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
                (the optional parts below: + a landmark term; the image terms on a region; a camera before the consumers)
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

The optional parts are objects of fit_parts, each None when it is off, and each called at one place of the iteration:
    landmark    fit_parts.LandmarkTerm (landmarks=): the fit's landmarks against the picture's, and the pose's start
    region      fit_parts.Region (mask=, mask_mesh=): the image terms see the target itself outside a region
    cam         fit_parts.Camera (camera=, fit_camera=): the consumers see the mesh through a perspective projection
    photo       fit_parts.Photometric (photometric=): a texture variable and the textured mesh against the picture.  Unlike
                the others it has an iteration of its own: `run(steps)` stays the iteration without it, bit for bit, and
                `run(steps, photometric=True)` runs the iteration with the term (a second captured graph over the same
                variable buffers).  `set_texture` puts a starting texture (a bake) into the variable
    silhouette  fit_parts.Silhouette (silhouette=): the antialiased coverage of the mesh (op.edge.coverage) against the
                picture's silhouette, in the one captured step; photo_edges=True takes the same node into the photometric
                term.  Not part of anything without the arguments
`_mesh` is the one place that builds the mesh (and applies the camera) for `render`, `posed_mesh` and `fitted_mesh`:
`fitted_mesh()` returns what the consumers saw, `fitted_mesh(projected=False)` the camera-space mesh; `reset` puts kappa
back at its start.  With a part off there is no node and no parameter for it: the iteration and its captured graph are
those without it.

The pose gradient reaches the vertices only through the rasterizer's backward (deterministic gather, so two
runs from the same state produce bit-identical trajectories).  On a GPU the whole iteration — forward, backward,
Adam — is one hipGraph (batch 1 is launch-latency bound: ~2 000 kernels per step), replayed `steps` times; the
loss history stays on the device until the end.
"""
import torch
from torch import optim

from . import graphs, utils_3d
from .fit_parts import Camera, LandmarkTerm, Photometric, Region, Silhouette


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
                 mask_mesh=False, shared_identity=None, camera=None, fit_camera=False, camera_lr=0.01, photometric=None,
                 photo_size=64, photo_weight=1.0, photo_lr=0.01, silhouette=None, silhouette_weight=1.0,
                 photo_edges=False):
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
        # the region of the image loss (op.region): not part of the iteration at all without mask / mask_mesh
        self.region = Region(self.target, mask, mask_mesh, self.with_map) if mask is not None or mask_mesh else None
        with torch.no_grad():
            mean_w = self.g.mean_latent(n_mean_latent)                                  # [1, D]
            self.target_feats = self._features_of_target()
        self._mean_w = mean_w
        self.w = mean_w.unsqueeze(1).repeat(self.batch, self.g.n_latent, 1).clone().requires_grad_(True)
        pose_shape = (7,) if self.batch == 1 else (self.batch, 7)
        self.pose = torch.zeros(pose_shape, device=self.device, requires_grad=optimise_pose)
        # the landmark term: not part of the iteration at all without landmarks
        self.landmark = None
        if landmarks is not None or landmark_conf is not None:
            self.landmark = LandmarkTerm((self.face_model, self.tri) if self.fit_shape else None, self.pose,
                                         self.target.shape[-2:], landmarks, landmark_conf, landmark_weight,
                                         landmark_beta, landmark_embedding, landmark_lines, landmark_axis, landmark_vis)
            with torch.no_grad():
                self.pose.copy_(self.landmark.pose_start)
        # 3DMM coefficients [B, d], from the mean face
        self.coeff = (torch.zeros(self.batch, self.face_model.n_coeff, device=self.device, requires_grad=True)
                      if self.fit_shape else None)
        self.noise = noise if noise is not None else [n.detach() for n in self.g.make_noise()]
        # the perspective camera (op.camera): not part of the iteration at all with camera=None
        self.cam = Camera(camera, fit_camera, self.batch, self.device) if camera is not None or fit_camera else None
        # what render leaves for loss: the prior of this forward (None: not added), and the per-sample losses
        self._reg = self._prior_rows = self._rows = None
        on_gpu = self.device.type == "cuda"
        from .optim import ALIGN, FlatAdam

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
                    self.cam.grad = flat_g
            self.optim = _FlatAdamSet(self._adams, [self.camera] if self.fit_camera else [])
        else:
            self._adams = None
            self.optim = optim.Adam(groups, betas=(0.9, 0.999))
        # the photometric term (fit_parts.Photometric): a texture variable with its own Adam and step count, stepped by
        # the iteration with the term only; not part of anything without photometric=
        self.photo = self._photo_optim = self.graph_photo = None
        self._photo_on = False
        if photometric is not None:
            self.photo = Photometric(photometric, self.tri, self.target, photo_size, photo_weight,
                                     self.shared_identity is not None, self.device, edges=photo_edges)
            tex = self.photo.texture
            if on_gpu:
                flat_g = torch.zeros((tex.numel() + ALIGN - 1) // ALIGN * ALIGN, device=self.device)
                self._photo_adam = FlatAdam([tex], flat_g, lr=photo_lr, betas=(0.9, 0.999))
                self._photo_optim = _FlatAdamSet([(tex, self._photo_adam)])
            else:
                self._photo_adam = None
                self._photo_optim = optim.Adam([{"params": [tex], "lr": photo_lr}], betas=(0.9, 0.999))
        elif photo_edges:
            raise ValueError("LatentInverter: photo_edges=True needs photometric=")
        # the silhouette term (fit_parts.Silhouette): not part of the iteration at all without silhouette=
        self.sil = None
        if silhouette is not None:
            self.sil = Silhouette(self.tri, self.target, silhouette, silhouette_weight, self.device)
        self.use_graph = on_gpu if use_graph is None else bool(use_graph)
        self.graph = None
        self.loss_value = torch.zeros(() if self.batch == 1 else (self.batch,), device=self.device)
        self.image = None

    # ---- model ----------------------------------------------------------------------------------------
    skinned = property(lambda self: self.fit_shape and self.face_model.kind == "skinned")       # FLAME: op.skin
    blended = property(lambda self: self.fit_shape and self.face_model.kind == "blended")       # FaceWarehouse: op.blend

    # ---- the optional parts (fit_parts) ---------------------------------------------------------------
    with_landmarks = property(lambda self: self.landmark is not None)
    with_mask = property(lambda self: self.region is not None)
    camera = property(lambda self: None if self.cam is None else self.cam.kappa)                # kappa [B], or None
    fit_camera = property(lambda self: self.cam is not None and self.cam.fit)
    # outputs of the last forward (they keep the previous picture's values after reset, until the next step)
    landmarks_fit = property(lambda self: None if self.landmark is None else self.landmark.landmarks_fit)
    contour_fit = property(lambda self: None if self.landmark is None else self.landmark.contour_fit)
    landmark_visibility = property(lambda self: None if self.landmark is None else self.landmark.landmark_visibility)
    mask_fit = property(lambda self: None if self.region is None else self.region.mask_fit)
    with_photometric = property(lambda self: self.photo is not None)
    with_silhouette = property(lambda self: self.sil is not None)
    coverage_fit = property(lambda self: None if self.sil is None else self.sil.coverage_fit)    # [B, H, W]
    texture = property(lambda self: None if self.photo is None else self.photo.texture.detach())   # [Bt, C, T, T]

    def _features_of_target(self):
        """The target's LPIPS features: `features`, or with a region the region's choice."""
        if self.region is not None:
            return self.region.target_features(self.perceptual, self.target)
        return [x.detach() for x in self.perceptual.features(self.target)]

    def _mesh(self, projected=True, gate=False):
        """The one mesh path: (v, n, n_gate, reg, prior_rows) of the current variables.  v is what the consumers see: the
        camera-space vertices of the model's node (op.morph / op.skin / op.blend: no library GEMM on the device) or of the
        posed fixed mesh, through the camera's projection if there is one (projected=False: left in camera space); the
        projection is applied here and nowhere else.  n stays the camera-space normal, which the generator keeps; n_gate
        is what a facing gate reads: with gate=True under a camera n_view, written by the projection's launch, else n.
        reg, prior_rows: the prior of the model's node (None for the fixed mesh)."""
        reg = prior_rows = None
        if self.fit_shape:
            v, n, reg, prior_rows = self.face_model.mesh(self.coeff, self.pose.view(-1, 7), self.tri, self.shape_reg)
        else:
            lin, rot = utils_3d.pose_matrices(self.pose)                                # [B, 3, 3] each
            # [nv, 3] x [3, 3]: one streaming kernel each (utils_3d.affine3), not a 3-wide library GEMM
            t = self.pose[3:6].view(1, 3) if self.batch == 1 else self.pose[:, 3:6]
            v, n = utils_3d.affine3(self.v0, lin, t).contiguous(), utils_3d.affine3(self.n0, rot).contiguous()
        n_gate = n
        if self.cam is not None and projected:
            v, n_gate = self.cam.project(v, n, gate)
        return v, n, n_gate, reg, prior_rows

    def posed_mesh(self, projected=True):
        """(v, n, tri) of the current variables.  With a camera and projected=True, v is what the consumers see (v' of
        op.camera.project) and n stays the camera-space normal; projected=False gives the camera-space mesh."""
        v, n = self._mesh(projected)[:2]
        return v, n, self.tri

    def fitted_mesh(self, projected=True):
        """(v, n, tri) of the current fit, posed and detached.  With a camera this is what the consumers saw: the
        projected vertices v' and n_view, the normals as the facing gates read them (op.camera); projected=False returns
        the camera-space mesh.  Without a camera the two are the same."""
        with torch.no_grad():
            v, _, n = self._mesh(projected, gate=True)[:3]
        return v.detach(), n.detach(), self.tri

    def render(self):
        self._reg = self._prior_rows = None
        lmk = self.landmark
        if self.with_map or lmk is not None or self._photo_on or self.sil is not None:
            v, n, n_gate, reg, prior_rows = self._mesh(gate=lmk is not None and lmk.vis is not None)
            if lmk is not None:
                lmk(v, n_gate)
            if self.sil is not None:
                self.sil(v)
            if self._photo_on:
                # the textured mesh against the picture, on the mesh every consumer sees
                self.photo(v, self.target, None if self.region is None else self.region.mask)
        if not self.with_map:
            # a plain Generator takes no mesh: the model's mesh serves the landmark term only, and the prior is not added
            # (_reg stays None), as it never was on this path
            return self.g([self.w], input_is_latent=True, noise=self.noise)[0]
        self._reg, self._prior_rows = reg, prior_rows
        # with mask_mesh the normal map at the image's resolution gates the region in this step
        want = self.region is not None and self.region.mask_mesh
        img, _, maps = self.g([self.w], (v, n, self.tri), input_is_latent=True, noise=self.noise, return_normals=want)
        if want:
            self.region.see(maps, img)
        return img

    def loss(self, img):
        if self.region is not None:
            img = self.region(img, self.target)
        if self.batch > 1:
            return self._loss_rows(img)
        from .op.lpips_layer import mse

        d = self.perceptual.distance_to(self.target_feats, img).mean()
        value = d + self.pixel_weight * mse(img, self.target)
        if self.fit_shape and self.shape_reg != 0.0 and self._reg is not None:
            value = value + self._reg                    # shape_reg * regulation(coeff), from the node's forward
        if self.landmark is not None:
            value = value + self.landmark.rows.view(())
        if self.sil is not None:
            value = value + self.sil.rows.view(())
        if self._photo_on:
            value = value + self.photo.rows.view(())
        return value

    def _loss_rows(self, img):
        """sum_b L_b; the per-sample L_b go to self._rows (one fit_loss_rows node: no per-sample launches)."""
        from .op.lpips_layer import fit_loss_rows, mse_rows

        layers = self.perceptual.layer_distances(self.target_feats, img)
        prior = self.fit_shape and self.shape_reg != 0.0 and self._reg is not None
        if prior and self._prior_rows is not None:
            self._rows, total = fit_loss_rows(layers, mse_rows(img, self.target), self.pixel_weight, reg=self._reg,
                                              prior_rows=self._prior_rows)
        else:
            self._rows, total = fit_loss_rows(layers, mse_rows(img, self.target), self.pixel_weight,
                                              coeff=self.coeff if prior else None,
                                              sigma=self._prior_sigma if prior else None, shape_reg=self.shape_reg,
                                              reg=self._reg if prior else None)
        if self.landmark is not None:
            self._rows = self._rows + self.landmark.rows.detach()
            total = total + self.landmark.rows.sum()
        if self.sil is not None:
            self._rows = self._rows + self.sil.rows.detach()
            total = total + self.sil.rows.sum()
        if self._photo_on:
            self._rows = self._rows + self.photo.rows.detach()
            total = total + self.photo.rows.sum()
        return total

    def _iteration_photo(self):
        """The iteration with the photometric term: the same steps, the term in the forward, the texture's Adam after
        the others'."""
        self._photo_on = True
        try:
            self._iteration()
        finally:
            self._photo_on = False

    def _iteration(self):
        self.w.grad = None
        self.pose.grad = None
        if self.coeff is not None:
            self.coeff.grad = None
        if self.camera is not None:
            self.camera.grad = None
        if self._photo_on:
            self.photo.texture.grad = None
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
        if self._photo_on:
            self._photo_optim.step()
        self.loss_value.copy_(value.detach() if self.batch == 1 else self._rows)
        self.image = img.detach()

    # ---- driver ---------------------------------------------------------------------------------------
    def _warm_and_capture(self, history, warmup=3, photometric=False):
        """`warmup` real iterations on a side stream (lazy initialisation, Adam state), then one capture.
        Returns the number of optimisation steps already taken (capture itself executes nothing).  photometric: of the
        iteration with the term, into a graph of its own."""
        body = self._iteration_photo if photometric else self._iteration
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for k in range(warmup):
                body()
                history[k] = self.loss_value
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = graphs.capture(body)                      # memset nodes of torch's reductions repaired: graphs.py
        if photometric:
            self.graph_photo = graph
        else:
            self.graph = graph
        return warmup

    @torch.no_grad()
    def reset(self, target, landmarks=None, landmark_conf=None, mask=None, silhouette=None):
        """Re-targets the inverter to `target` (the shape of the first): copies it and its LPIPS features into the
        buffers the captured graph reads, puts w back at the mean latent, pose and coeff at zero, and zeroes the Adam
        moments and step counts.  An inverter built with landmarks also takes the new picture's `landmarks` and
        `landmark_conf` into its buffers and puts the pose at their closed-form start (landmarks None: every landmark
        missing, pose 0).  `run(steps)` then gives what a fresh inverter on `target` (and these landmarks) gives (same
        mean latent, same noise), bit for bit, without a new warm-up or capture.  landmarks_fit, contour_fit and
        landmark_visibility are outputs of the (possibly captured) iteration: they keep the previous picture's values
        until the next step writes them.  An inverter built with a region (mask= or mask_mesh=) takes the new picture's
        `mask` into its buffer (None: all ones); mask_fit is an output of the iteration like landmarks_fit.  An inverter
        built with silhouette= takes the new picture's `silhouette` into its buffer in the same way (it has no default:
        None raises)."""
        target = target.detach()
        if (self.sil is None) != (silhouette is None):
            raise ValueError("LatentInverter.reset: silhouette= goes with an inverter built with silhouette=, and such an "
                             "inverter needs the new picture's; the term is part of the captured iteration or it is not")
        if not self.with_mask and mask is not None:
            raise ValueError("LatentInverter.reset: this inverter was built without a mask; the region blend is part of "
                             "the captured iteration or it is not")
        if not self.with_landmarks and (landmarks is not None or landmark_conf is not None):
            raise ValueError("LatentInverter.reset: this inverter was built without landmarks; the landmark term is "
                             "part of the captured iteration or it is not")
        if tuple(target.shape) != tuple(self.target.shape):
            raise ValueError("LatentInverter.reset: target %s, the inverter fits %s"
                             % (tuple(target.shape), tuple(self.target.shape)))
        if self.region is not None:
            self.region.set(mask)
        if self.sil is not None:
            self.sil.set(silhouette)
        self.target.copy_(target)
        for buf, f in zip(self.target_feats, self._features_of_target()):
            buf.copy_(f)
        self.w.copy_(self._mean_w.unsqueeze(1).expand_as(self.w))
        if self.landmark is not None:
            self.landmark.set(landmarks, landmark_conf)
            self.pose.copy_(self.landmark.pose_start)
        else:
            self.pose.zero_()
        if self.coeff is not None:
            self.coeff.zero_()
        if self.cam is not None:
            self.cam.reset()
        if self.photo is not None:
            self._zero_texture()
        if self._adams is not None:
            for _, adam in self._adams:
                for t in (adam.m, adam.v, adam.step_t, adam.flat_g):
                    t.zero_()
        else:
            self.optim.state.clear()                     # torch's Adam initialises its state at the next step
        self.loss_value.zero_()

    @torch.no_grad()
    def _zero_texture(self):
        """The texture at 0, its Adam's moments and step count at 0."""
        self.photo.texture.zero_()
        if self._photo_adam is not None:
            for t in (self._photo_adam.m, self._photo_adam.v, self._photo_adam.step_t, self._photo_adam.flat_g):
                t.zero_()
        else:
            self._photo_optim.state.clear()

    @torch.no_grad()
    def set_texture(self, tex):
        """A starting texture [Bt, C, T, T] (a bake; [C, T, T] at Bt = 1) into the variable, in place (the captured
        iteration reads that buffer), with the moments and the step count of the texture's Adam back at 0."""
        if self.photo is None:
            raise ValueError("LatentInverter.set_texture: this inverter was built without photometric=")
        var = self.photo.texture
        t = tex.detach()
        if t.dim() == 3 and var.shape[0] == 1:
            t = t.unsqueeze(0)
        if tuple(t.shape) != tuple(var.shape):
            raise ValueError("LatentInverter.set_texture: texture %s, the inverter's variable is %s"
                             % (tuple(t.shape), tuple(var.shape)))
        self._zero_texture()
        var.copy_(t)

    def run(self, steps=400, photometric=False):
        """Runs `steps` Adam iterations; returns the loss history [steps] ([steps, B] for B > 1; device tensor: no host
        read here).  photometric=True (an inverter built with photometric=): the iteration with the photometric term,
        whose texture takes Adam steps too; it is warmed and captured on first use into a graph of its own, and the
        history then includes the term."""
        if photometric and self.photo is None:
            raise ValueError("LatentInverter.run: photometric=True needs an inverter built with photometric=")
        history = torch.zeros((steps,) if self.batch == 1 else (steps, self.batch), device=self.device)
        done = 0
        if photometric:
            if self.use_graph and self.graph_photo is None and steps > 4:
                done = self._warm_and_capture(history, photometric=True)
            graph, body = self.graph_photo, self._iteration_photo
        else:
            if self.use_graph and self.graph is None and steps > 4:
                done = self._warm_and_capture(history)
            graph, body = self.graph, self._iteration
        for i in range(done, steps):
            if graph is not None:
                graph.replay()
            else:
                body()
            history[i] = self.loss_value
        return history
