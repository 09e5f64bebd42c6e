"""Face reconstruction by inverting the generative renderer (the paper's use of the model; the reference ships no script
for it):

    python -m stylerenderer_amd.reconstruct [--size 256] [--steps 400] [--lr] [--pose_lr] [--coeff_lr] [--shape_reg]
        [--bfm BFM.mat | --flame FLAME.{pkl,mat} | --facewarehouse FW.mat [--beta_shape X]] [--lpips-trunk VGG16.pth] [--batch N] [--gpu 0] [--seed S] [--out DIR]
        [--multiview V [--identity_dims K] [--subject NAME] [--merge_sharpness S]]
        [--lmk LANDMARKS.txt [--lmk_index FILE] [--lmk_weight 1.0] [--lmk_beta 1.0] [--lmk_contour 1.0]
         [--lmk_dynamic | --lmk_lines FILE] [--lmk_axis I,J] [--lmk_vis LO,HI]]
        [--mask_lmk [--mask_tri FILE] [--mask_margin R]] [--mask_dir DIR] [--mask_mesh]
        [--texture [T] [--uv FILE] [--texture_from picture|render] [--texture_facing LO,HI] [--texture_pad N]
         [--texture_fill mean|none] [--texture_check] [--turntable N [--turntable_yaw DEG]]
         [--texture_refine STEPS [--texture_lr LR]] [--texture_mip [BIAS]]
         [--light [--light_mono] [--light_floor S] [--light_ridge L] [--light_lr LR] [--relight FILE]]]
        [--silhouette_dir DIR [--silhouette_weight 1.0]] [--photo_edges] [--render_aa]
        [--camera_distance D | --camera_fov DEG] [--fit_camera] [--camera_lr 0.01] CHECKPOINT IMAGE [IMAGE ...]

For every image: the checkpoint's GeneratorWithMap (`g_ema`) is inverted with inversion.LatentInverter(fit_shape=True)
— the W+ latent, a rigid pose and the 3DMM shape / expression coefficients are fitted together (op.morph on the device)
— and DIR receives

    <stem>.obj            the posed mesh with vertex normals
    <stem>_canonical.obj  the fitted shape without the pose (with --flame: with the fitted articulation)
    <stem>_render.png     the generator's image of the fit
    <stem>_normal.png     the rasterised normal map of the posed mesh
    <stem>.npz            w, coeff, pose and the loss history (with --flame also joints [nj-1, 3], the axis-angles; with
                          --facewarehouse also identity [ds+1] and expression [de+1], the fitted mixing weights, each
                          summing to 1: expression[0] is the neutral face's share)

With --batch N the images are fitted N at a time, each group as one batched LatentInverter (one captured graph; every
image still follows its own single-image optimisation): the first group builds the inverter, the following ones
re-target it with `reset`, and a short last group is padded with copies of its last image whose results are dropped.
The files and their shapes are those of --batch 1, the default, which fits one image per inverter.

With --lmk the fit is guided by 2-D landmarks (a text file in align.LandmarksReader's format, pixel indices of each input
picture): the pose starts at the closed-form scaled-orthographic fit of the model's landmarks to the picture's
(align.pose_from_landmarks) and --lmk_weight times the reprojection term of op.landmark joins the loss.  The model's
landmarks are its own (a Basel file's `landmarks68`) or those of --lmk_index (face_model.landmark_embedding: vertex indices,
or faces and barycentric weights).  --lmk_contour weighs landmarks 0-16 of a 68-point set, the jaw line, which detectors
slide along the silhouette.  A picture the file does not list is fitted without the term's pull (every confidence 0) and
counted in the last line of the output.  <stem>.npz then also holds `landmarks` [L, 2] (the fit's, in pixel indices of the
input picture), `landmarks_target` (the file's; NaN when not listed) and `lmk_error` (their mean distance in those
pixels over the weighted landmarks).  --lmk_weight's default is a starting value, not tuned on a trained checkpoint.

A detector puts the jaw landmarks on the visible silhouette and guesses landmarks that are turned out of sight.  With
--lmk_dynamic (contour lines built from the model's mean shape, face_model.contour_lines) or --lmk_lines FILE (hand-made
ones, an .npz of face_model.load_contour_lines) every jaw landmark slides along its line of candidate vertices to the one
furthest out in the picture; --lmk_axis I,J names the two landmarks (27 and 8 of a 68-point set: nose bridge and chin)
whose vertices span the face's up direction.  --lmk_vis LO,HI fades a landmark out as its normal turns away from the camera
(normal z from HI down to LO; 0,0.2 is a starting value, untuned like --lmk_weight).  The pose start then takes two
closed-form passes, and <stem>.npz also holds `contour_vertices` [C] (the vertex every line selected) and `lmk_visibility`
[L] (the gate; 1 without --lmk_vis).  Without these options nothing changes.

With --mask_lmk, --mask_dir or --mask_mesh the image terms of the loss see only a region of the picture (op.region: the
loss runs on target + m (render - target), so hair, a hand, a microphone or the background no longer pull the fit).
--mask_lmk fills the polygon of --lmk's landmarks, scaled to the generator's size as they are for the landmark term: their
convex hull, or with --mask_tri FILE the triangles of a landmark triangulation (an .obj whose `f` lines name landmarks
1-based, or an .npy / .txt of [T, 3] 0-based); --mask_margin R grows (R > 0) or shrinks (R < 0) it by R pixels of that size.
--mask_dir DIR reads <stem>.png or <stem>.npy (grey, scaled to [0, 1], soft values allowed), resized as the picture is; a
picture without a file gets all ones and is counted in the last line of the output; with --mask_lmk the two are
multiplied.  --mask_mesh gates the region in every step by the fitted mesh's coverage of the picture.  A picture the
landmark file does not list gets all ones from --mask_lmk.  DIR then also receives <stem>_mask.png, the region of the last
step (m times the gate), and <stem>.npz `mask_area`, its mean.  The pixel term is not renormalised by the region's area.
Without these options nothing changes.

With --texture [T] (default 512) the picture's colours are carried onto the fitted surface (op.texture): DIR also receives
<stem>_texture.png (T x T), <stem>_texture_weight.png (grey, weight x 255: how much every texel saw of the picture),
<stem>_textured.obj with <stem>_textured.mtl (the posed vertices of <stem>.obj with texture coordinates and the material
that names the texture), and <stem>.npz `texture_coverage`, the share of the layout's texels with a positive weight before
padding.  The layout is --uv FILE (face_model.load_uv: an .obj with vt lines and f a/t records over the model's faces, or an
.npz with vt and ft; FLAME's template comes in this way) or, without it, the cylindrical unwrap of the model's mean shape
(face_model.uv_layout, meant for face patches and convex heads).  --texture_from picture (the default) samples the file's
picture at its own resolution (the resized target covers the whole picture, so the same model coordinates project onto
it); render samples the generator's image of the fit.  A texel counts while it faces the camera (--texture_facing LO,HI on
the z of its normal; 0.1,0.4 and the depth slack 4 / side of the z-buffer are starting values, not tuned on any trained
checkpoint, like --lmk_weight) and is not hidden (the posed mesh's z-buffer, square, of side min(1024, max(size, T))).
--texture_pad N (default 8, at most 64) grows the charts by N texels so that a renderer's filter finds no black beside
them; --texture_fill mean (the default) paints what is left with the mean colour, none leaves it black.  Without --texture
nothing changes.

The textured head can be drawn (op.texture.uv_map / sample: the layout's coordinates rasterised over the fitted mesh, then a
bilinear look-up of the texture that is differentiable in the texture; three options, all of which need --texture and
without which nothing changes).  --texture_check draws the written texture (after padding and fill) on the fitted mesh at
the fitted pose and camera at the fit's resolution: <stem>_rerender.png, and <stem>.npz `rerender_error`, the mean absolute
difference to the fit's target over the pixels that are covered and where the look-up of the bake's weight is positive
(`rerender_covered` and `rerender_counted` are the two counts).  --turntable N writes N renders <stem>_turn_KK.png over
background -1 of the camera-space mesh turned about the vertical axis through its centroid, the yaws spaced evenly in
[-DEG, DEG] (--turntable_yaw, default 30; one render: yaw 0), projected by the fitted camera when there is one.
--texture_refine STEPS runs Adam (optim.FlatAdam) on the texture alone, from the padded bake, on the sum over the covered
pixels of (render - target)^2; the mesh, the uv map and its tap list are fixed, texels no tap reaches keep their padded
value, the refined texture is the one written, and <stem>.npz gains `texture_refine_loss` [STEPS] (the loss before every
step) and, with --texture_check, `rerender_error_before`.  --texture_lr's default 0.02 is a starting value, not tuned on any
trained checkpoint.  With --multiview the merged texture is refined over all views of the subject at once (one texture
under V uv maps) and checked on every view: NAME_identity.npz `merged_texture_refine_loss`, `merged_rerender_error` [V]
(with `merged_rerender_covered`, `merged_rerender_counted` and, after a refinement, `merged_rerender_error_before`): the
number the merge's sharpness and the facing gate can be tuned against; --turntable also writes NAME_merged_turn_KK.png, the
identity mesh (pose 0, no camera) with the merged texture.
--texture_mip [BIAS] (without it nothing changes) sends every one of these draws, the look-up of the bake's weight in
--texture_check and --relight's picture included, through the texture's mip pyramid (op.texture.sample_mip: a trilinear
look-up at the level of detail of the uv map's footprint plus BIAS, default 0), so a texture drawn smaller than it is no
longer aliases.  Refinement keeps level 0 as the parameter and rebuilds the pyramid in every step; the level of detail and
the tap list are computed once.  <stem>.npz gains `texture_mip`, the bias; the written texture files stay level 0.

With --light (it needs --texture, as its five companions do) every bake is separated into an albedo and a light (op.light:
Lambertian shading under second-order spherical harmonics, nine coefficients per colour channel, or one white light with
--light_mono).  After the bake the posed normals are carried to the texels, the light is fitted in closed form under a
constant-albedo assumption (--light_ridge L, default 0.001, on its non-constant coefficients; the fitted shading has
weighted mean 1, so the albedo keeps the picture's exposure) and divided out of the bake (not below --light_floor S,
default 0.05); padding and fill run on the albedo.  <stem>_texture.png, the one the .mtl names, is then the albedo;
<stem>_texture_lit.png is the plain bake, padded likewise; <stem>_shading.png is the fitted light on a mid-grey head at the
fit's resolution; <stem>.npz gains `light` [Cl, 9] and `light_residual`, the weighted rms over the fitted texels of what
a constant albedo under the fitted light leaves of the bake (with --multiview also `texture_lit` beside `texture`, which is
the albedo).  --texture_check draws albedo times light, so `rerender_error` keeps its meaning and is comparable with a run
without --light, and writes the plain bake's error beside it (`rerender_error_lit`).  --turntable turns the normals with
the mesh while the light stays fixed in the camera's frame, so the shading moves over the face.  --relight FILE (an .npy or
text file of 9 or 9 C numbers) writes <stem>_relit.png, the fitted pose under that light, and the turntable frames use it.
--texture_refine runs Adam on the albedo and the light together, the light in a second group with --light_lr (default
0.005); the .npz holds `light`, the refined one, and `light_fit`, the closed-form one.  With --multiview every view has
its own light, the views' albedos are what is merged, the merged check shades the merged albedo with each view's light,
joint refinement keeps one albedo and V lights, the merged turntable uses view 0's light and NAME_identity.npz gains
`lights` [V, Cl, 9].  The floor, the ridge and the light's learning rate are starting values, not tuned on any picture.
Without --light nothing changes.

With --multiview V the IMAGE arguments are taken in consecutive groups of V, each group V pictures of one subject (their
count must be a multiple of V).  It implies --batch V: a group is fitted as one batched LatentInverter with
shared_identity=K, so the views share the leading K coefficients (K = the face model's n_identity: shape before
expression, FLAME's 300 identity columns, FaceWarehouse's identity logits; --identity_dims K overrides it) while latent,
pose, expression / joints, landmarks and masks stay per view; the first group builds the inverter, the following ones
`reset` it.  Every view keeps its own prior term, so the shared coefficients' prior enters V times (the objective is the
sum of the V single-view objectives under the constraint).  Per view, the files are those of --batch, and every .npz also
holds `subject` and `view`.  Per subject NAME (--subject for a single group, else the stem of the group's first view) DIR
also receives NAME_identity.obj, the model's mesh at the shared coefficients with every other coefficient and the pose at
0, with normals, and NAME_identity.npz with `identity` [K], `views` (the stems) and `loss` (the views' summed history).
With --texture the V bakes are merged per texel (op.texture.merge: weights (w_v / max w)^(2^S), --merge_sharpness S in 0..4,
default 2), then padded and filled as a single bake is: NAME_merged_texture.png, NAME_merged_texture_weight.png,
NAME_merged_texture_views.png (grey: the view every texel took most from, 255 where no view saw it) and NAME_merged.obj
with NAME_merged.mtl, the identity mesh carrying the merged texture.  NAME_identity.npz then also holds
`merged_coverage` beside `texture_coverage` [V], the views' own (the gain of the merge is their difference), and the
merge before padding: `merged_texture` [C, T, T], `merged_weight` [T, T] and `merged_best` [T, T]; every view's .npz
holds its bake before padding, `texture` [C, T, T] and `texture_weight` [T, T] (float32; 4 MB per view at T = 512), so a
merge can be repeated at another sharpness without a new fit.  Not built: exposure or colour matching between the views,
mirror fill, choosing the views automatically.  Without --multiview nothing changes.

With --camera_distance D (D > 0: the camera's distance from the plane z = 0 of pose space in half-picture-widths, which is
the focal length in that unit) or --camera_fov DEG (the full field of view across the picture) the fit sees the mesh through
a perspective camera with kappa = 1 / D = tan(DEG / 2) (op.camera: one node between the posed mesh and every consumer; a
close-up taken from 35 cm and cropped to 1.5 face widths has D near 3).  --fit_camera fits kappa together with the pose, one
value per picture (per view with --multiview), with the learning rate --camera_lr (a starting value, not tuned); kappa is not
constrained and a negative fit is reported as it is.  kappa is only weakly determined by the image terms alone: it wants
--lmk.  <stem>.obj, <stem>_textured.obj and the merged .obj then hold the camera-space mesh (pose applied, not projected),
while <stem>_normal.png, the landmarks, the mask, the depth buffer and the bake use the projected mesh the fit saw;
<stem>.npz also holds `camera` (kappa) and `camera_distance` (1 / kappa), NAME_identity.npz the views' `camera` [V].  The
depth translation and the scale trade off along a flat direction under a camera (inversion.LatentInverter's note), so
compare projections, kappa and angles between fits, not raw t_z or scale.  Not built: a principal-point offset (the crop is
assumed centred on the optical axis), a closed-form perspective pose start (the orthographic one is the start), lens
distortion.  Without these options nothing changes.

With --silhouette_dir DIR the fit has a silhouette term (fit_parts.Silhouette): DIR/<stem>.png or .npy (read
and resized as --mask_dir's files; every picture needs one) against the coverage of the mesh, antialiased along its
silhouette edges (op.edge.coverage), so the outline pulls on the vertices that form it; per row
--silhouette_weight * sum (coverage - silhouette)^2 / (H W), in the one captured step (weight 1.0: an untuned starting
value).  <stem>_coverage.png is the fitted mesh's coverage, <stem>.npz gains `silhouette_loss` (the term at the fitted
state) and `silhouette_iou` (both thresholded at 0.5).  It works with --batch, --multiview and all three face models.
--photo_edges (with --photo) lets the outline take part in the photometric term: the render is composited over the picture
and antialiased along the silhouette before it is compared.  --render_aa antialiases the --turntable renders the same way
(the relit ones after the shading); --texture_check's re-render is not antialiased (its views carry no mesh).  Without
these options nothing changes.

Images are PNG / JPG (PIL) or .npy in [-1, 1] (HWC or CHW), resized on the host.  The 3DMM is the Basel Face Model with
--bfm (face_model.load_bfm), FLAME with --flame (face_model.load_flame, op.skin), the FaceWarehouse bilinear blendshape
model with --facewarehouse (face_model.load_facewarehouse, op.blend), else the synthetic model `train --mesh` trains with (train.SyntheticFaceSource).  Without
--lpips-trunk the perceptual trunk is the deterministic synthetic fill and the result is not a meaningful
reconstruction (stderr says so).
"""
import argparse
import os
import sys

import numpy as np
import torch

from . import checkpoint, generate, inversion, lpips, utils_3d


def load_picture(path):
    """[1, 3, H, W] float32 of the file's picture at its own resolution, on the host (in [-1, 1] for PNG / JPG; an .npy
    as it is)."""
    if path.lower().endswith(".npy"):
        a = np.load(path).astype(np.float32)
        if a.ndim == 4:
            a = a[0]
        if a.ndim == 2:
            a = a[:, :, None]
        if a.shape[0] in (1, 3) and a.shape[-1] not in (1, 3):       # CHW
            a = a.transpose(1, 2, 0)
        x = torch.from_numpy(np.ascontiguousarray(a)).permute(2, 0, 1)[None]
    else:
        from PIL import Image

        im = Image.open(path).convert("RGB")
        x = torch.from_numpy(np.asarray(im, np.float32) / 127.5 - 1.0).permute(2, 0, 1)[None]
    if x.shape[1] == 1:
        x = x.expand(-1, 3, -1, -1)
    return x[:, :3]


def load_image(path, size, with_shape=False):
    """[1, 3, size, size] float32 in [-1, 1] on the host (with_shape: and the (H, W) of the file's picture)."""
    x = load_picture(path)
    shape = (int(x.shape[-2]), int(x.shape[-1]))
    if shape != (size, size):
        x = torch.nn.functional.interpolate(x, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
    x = x.clamp(-1, 1).contiguous()
    return (x, shape) if with_shape else x


def face_model(bfm, device, seed=0, flame=None, facewarehouse=None, beta_shape=.01):
    """(model, tri) on `device`: the Basel model of --bfm, FLAME of --flame, FaceWarehouse of --facewarehouse, else
    train.SyntheticFaceSource's."""
    if facewarehouse or flame or bfm:
        from .face_model import load_bfm, load_facewarehouse, load_flame

        if facewarehouse:
            model, tri = load_facewarehouse(facewarehouse, beta_shape)
        else:
            model, tri = load_flame(flame) if flame else load_bfm(bfm)
        return model.to(device), tri.to(device)
    from .train import SyntheticFaceSource

    src = SyntheticFaceSource(device, seed=seed)
    return src.model, src.tri


class LandmarkGuide:
    """The landmark options of one run: the reader of --lmk, the embedding and the weights; `lookup` gives what the
    inverter takes for a picture."""

    def __init__(self, lmk_file, face, index_file=None, weight=1.0, beta=1.0, contour=1.0, dynamic=False, lines_file=None,
                 axis=None, vis=None):
        from . import align
        from .face_model import landmark_embedding

        if not os.path.isfile(lmk_file):
            raise SystemExit("reconstruct: landmark file %s not found" % lmk_file)
        self.reader = align.LandmarksReader(lmk_file)
        self.file = lmk_file
        model, tri = face
        if index_file:
            self.embedding = landmark_embedding(index_file, tri)
        else:
            self.embedding = getattr(model, "landmarks", None)
        if self.embedding is None:
            raise SystemExit("reconstruct: --lmk needs the face model's landmarks and this model names none: pass "
                             "--lmk_index FILE (vertex indices, or faces and barycentric weights)")
        self.count = int(self.embedding[0].shape[0])
        self.weight, self.beta, self.contour = float(weight), float(beta), float(contour)
        if self.contour < 0:
            raise SystemExit("reconstruct: --lmk_contour must not be negative")
        self.missing = 0
        self.seen = 0
        self.dynamic = self._dynamic_args(face, dynamic, lines_file, axis, vis)

    def _dynamic_args(self, face, dynamic, lines_file, axis, vis):
        """LatentInverter's landmark_lines / landmark_axis / landmark_vis of --lmk_dynamic, --lmk_lines, --lmk_axis and
        --lmk_vis; {} without them."""
        from .face_model import contour_lines, landmark_vertices, load_contour_lines

        out = {}
        if vis is not None:
            try:
                lo, hi = (float(x) for x in vis.split(","))
            except ValueError:
                raise SystemExit("reconstruct: --lmk_vis takes LO,HI")
            if not lo <= hi:
                raise SystemExit("reconstruct: --lmk_vis needs LO <= HI")
            out["landmark_vis"] = (lo, hi)
        if not (dynamic or lines_file):
            if axis is not None:
                raise SystemExit("reconstruct: --lmk_axis needs --lmk_dynamic or --lmk_lines")
            return out
        model, tri = face
        if axis is None and self.count != 68:
            raise SystemExit("reconstruct: --lmk_axis I,J is required with %d landmarks (its default, 27,8, is of a "
                             "68-point set)" % self.count)
        try:
            i, j = (27, 8) if axis is None else (int(x) for x in axis.split(","))
        except ValueError:
            raise SystemExit("reconstruct: --lmk_axis takes two landmark numbers I,J")
        if not (0 <= i < self.count and 0 <= j < self.count and i != j):
            raise SystemExit("reconstruct: --lmk_axis names two different landmarks in [0, %d)" % self.count)
        main = landmark_vertices(self.embedding)
        out["landmark_axis"] = (int(main[i]), int(main[j]))
        with torch.no_grad():
            dev = tri.device
            v, n = model.mesh(torch.zeros(1, model.n_coeff, device=dev), torch.zeros(1, 7, device=dev), tri)[:2]
        try:
            if lines_file:
                out["landmark_lines"] = load_contour_lines(lines_file, self.count, int(v.shape[1]))
            else:
                if self.count != 68:
                    raise SystemExit("reconstruct: --lmk_dynamic takes landmarks 0-16 of a 68-point set for the jaw line; "
                                     "with %d landmarks pass --lmk_lines FILE" % self.count)
                out["landmark_lines"] = contour_lines(v[0].cpu(), self.embedding, normals=n[0].cpu())
        except (ValueError, OSError) as e:
            raise SystemExit("reconstruct: %s" % e)
        return out

    def lookup(self, path, shape, size):
        """(landmarks [L, 2] in pixel indices of the size x size target, conf [L], the file's landmarks in the picture's
        own pixels or None) of the picture at `path`, whose (H, W) is `shape`."""
        from . import align

        self.seen += 1
        lmk = self.reader.detect(path)
        if lmk is None:
            self.missing += 1
            return np.zeros((self.count, 2)), np.zeros(self.count), None
        if lmk.shape[0] != self.count:
            raise SystemExit("reconstruct: %s lists %d landmarks for %s, the model's embedding has %d"
                             % (self.file, lmk.shape[0], path, self.count))
        conf = np.ones(self.count)
        if self.count == 68:
            conf[:17] = self.contour
        return align.scale_landmarks(lmk, shape, (size, size)), conf, lmk

    def inverter_args(self, landmarks, conf):
        return dict(landmarks=np.stack(landmarks), landmark_conf=np.stack(conf), landmark_weight=self.weight,
                    landmark_beta=self.beta, landmark_embedding=self.embedding, **self.dynamic)

    def summary(self):
        return "landmarks: %d of %d images are not listed in %s and were fitted without them" % (
            self.missing, self.seen, self.file)


def read_triangulation(path):
    """int64 [T, 3], 0-based landmark numbers: the `f` lines of an .obj (1-based, their first three entries; `a/b/c`
    entries count by their vertex), or an .npy / .txt of [T, 3] (0-based)."""
    if not os.path.isfile(path):
        raise SystemExit("reconstruct: --mask_tri file %s not found" % path)
    try:
        if path.lower().endswith(".obj"):
            rows = [[int(tok.split("/")[0]) - 1 for tok in line.split()[1:4]]
                    for line in open(path) if line.split()[:1] == ["f"]]
            tri = np.asarray(rows, np.int64).reshape(-1, 3)
        else:
            raw = np.load(path) if path.lower().endswith(".npy") else np.loadtxt(path, ndmin=2)
            if not np.all(np.round(raw) == raw):
                raise ValueError("not whole numbers")
            tri = np.asarray(raw, np.int64).reshape(-1, 3)
    except (ValueError, IndexError) as e:
        raise SystemExit("reconstruct: --mask_tri %s does not hold triangles [T, 3]: %s" % (path, e))
    if tri.shape[0] == 0 or tri.min() < 0:
        raise SystemExit("reconstruct: --mask_tri %s holds no triangle, or a landmark number below its first" % path)
    return tri


def load_mask(path, size):
    """[1, 1, size, size] float32 in [0, 1] of a grey .png (0-255) or .npy ([0, 1]; whole-number types 0-255), resized by
    the resize load_image applies to the picture."""
    if path.lower().endswith(".npy"):
        a = np.load(path)
        scale = 255.0 if a.dtype.kind in "ui" else 1.0
        a = a.astype(np.float32) / scale
        a = a.reshape(a.shape[-2:]) if a.ndim > 2 and a.size == a.shape[-2] * a.shape[-1] else a
        if a.ndim != 2:
            raise SystemExit("reconstruct: mask %s is not a grey picture [H, W]" % path)
    else:
        from PIL import Image

        a = np.asarray(Image.open(path).convert("L"), np.float32) / 255.0
    x = torch.from_numpy(np.ascontiguousarray(a))[None, None]
    if tuple(x.shape[-2:]) != (size, size):
        x = torch.nn.functional.interpolate(x, size=(size, size), mode="bilinear", align_corners=False, antialias=True)
    if not bool(torch.isfinite(x).all()):
        raise SystemExit("reconstruct: mask %s is not finite" % path)
    return x.clamp(0, 1).contiguous()


class MaskGuide:
    """The region options of one run; `lookup` gives the mask the inverter takes for a picture, or None when only the mesh
    gate is on."""

    def __init__(self, use_lmk=False, tri_file=None, margin=0, mask_dir=None, mesh=False, count=None):
        self.use_lmk, self.margin, self.dir, self.mesh = bool(use_lmk), int(margin), mask_dir, bool(mesh)
        if abs(self.margin) > 32:
            raise SystemExit("reconstruct: --mask_margin lies in [-32, 32]")
        self.tri = read_triangulation(tri_file) if tri_file else None
        if self.tri is not None and count is not None and self.tri.max() >= count:
            raise SystemExit("reconstruct: --mask_tri names landmark %d, the model's embedding has %d"
                             % (int(self.tri.max()) + 1, count))
        if mask_dir and not os.path.isdir(mask_dir):
            raise SystemExit("reconstruct: --mask_dir %s is not a directory" % mask_dir)
        self.missing = self.seen = 0

    per_picture = property(lambda self: self.use_lmk or bool(self.dir))

    def lookup(self, path, look, size):
        """look: LandmarkGuide.lookup's triple (the landmarks in the size x size target's pixels, conf, the file's)."""
        from .op.region import landmark_region

        if not self.per_picture:
            return None
        mask = torch.ones(1, 1, size, size)
        if self.use_lmk:
            listed = look[2] is not None                 # (every listed landmark counts, whatever --lmk_contour weighs)
            mask = landmark_region(np.asarray(look[0], np.float64)[None], np.full((1, len(look[0])), float(listed)),
                                   (size, size), tris=self.tri, margin=self.margin)
        if self.dir:
            self.seen += 1
            stem = os.path.splitext(os.path.basename(path))[0]
            found = [f for f in (os.path.join(self.dir, stem + ext) for ext in (".png", ".npy")) if os.path.isfile(f)]
            if found:
                mask = mask * load_mask(found[0], size)
            else:
                self.missing += 1
        return mask

    def inverter_args(self, masks):
        return dict(mask=None if masks[0] is None else torch.cat(masks, 0), mask_mesh=self.mesh)

    def summary(self):
        return "masks: %d of %d images have no file in %s and were fitted without one" % (self.missing, self.seen, self.dir)


def load_silhouette(directory, path, size):
    """[1, size, size] in [0, 1]: the silhouette of the picture `path`, DIR/<stem>.png or .npy, read as a mask is."""
    stem = os.path.splitext(os.path.basename(path))[0]
    found = [f for f in (os.path.join(directory, stem + ext) for ext in (".png", ".npy")) if os.path.isfile(f)]
    if not found:
        raise SystemExit("reconstruct: --silhouette_dir %s has no %s.png or %s.npy" % (directory, stem, stem))
    return load_mask(found[0], size)[:, 0]


def silhouette_outputs(inv, index, out_dir, stem):
    """Writes <stem>_coverage.png, the antialiased coverage of the fitted mesh, and returns the .npz entries
    `silhouette_loss` (the term at the fitted state) and `silhouette_iou` (coverage and silhouette thresholded at 0.5)."""
    from .op.edge import coverage

    k = slice(index, index + 1)
    with torch.no_grad():
        v, _, tri = inv.fitted_mesh()
        alpha = coverage(v[k].contiguous(), inv.sil.tri, inv.sil.hw)[0]
        want = inv.sil.mask[index]
        loss = float(((alpha - want) ** 2).sum()) * inv.sil.scale
        a, m = alpha > 0.5, want > 0.5
        union = int((a | m).sum())
        iou = float((a & m).sum()) / union if union else 1.0
    pix = np.round(alpha.cpu().numpy().astype(np.float64).clip(0, 1) * 255.0).astype(np.uint8)
    TextureGuide.save_grey(pix, os.path.join(out_dir, stem + "_coverage.png"))
    return {"silhouette_loss": np.float64(loss), "silhouette_iou": np.float64(iou)}


def mask_outputs(inv, index, out_dir, stem):
    """Writes <stem>_mask.png, the region of the last step's forward (the mask, times the mesh gate), and returns the
    .npz entry `mask_area`, its mean."""
    m = inv.mask_fit[index, 0].detach().cpu().numpy().astype(np.float64)
    pix = np.round(m * 255.0).astype(np.uint8)
    try:
        from PIL import Image

        Image.fromarray(pix).save(os.path.join(out_dir, stem + "_mask.png"))
    except ImportError:
        with open(os.path.join(out_dir, stem + "_mask.pgm"), "wb") as f:
            f.write(b"P5 %d %d 255\n" % (pix.shape[1], pix.shape[0]) + pix.tobytes())
    return {"mask_area": np.float64(m.mean())}


def landmark_outputs(inv, index, conf, listed, shape):
    """The landmark entries of sample `index`'s .npz: the fit's landmarks and the file's in pixel indices of the input
    picture (H, W) = shape, and their mean distance over the landmarks with a positive weight."""
    from . import align

    from .op.landmark import landmark_points, project

    size = tuple(int(x) for x in inv.target.shape[-2:])
    term = inv.landmark                                  # fit_parts.LandmarkTerm: the embedding and the pose-aware settings
    # of the mesh that is written (the saved pose and coeff): inv.landmarks_fit is the last forward's, one Adam step behind
    with torch.no_grad():
        v = inv.fitted_mesh()[0][index:index + 1]
        p = project(landmark_points(v, term.index, term.bary), size)[0]
    fit = align.scale_landmarks(p.cpu().numpy().astype(np.float64), size, shape)
    more = {}
    if term.dynamic:
        # the pose-aware term: the jaw landmarks are those the contour lines select on the written mesh
        from .op.landmark import landmark_dynamic_composite

        with torch.no_grad():
            n = inv.fitted_mesh()[1][index:index + 1]
            zero = torch.zeros(1, p.shape[0], device=v.device)
            _, pd, sel, gate = landmark_dynamic_composite(v, term.index, term.bary, torch.zeros_like(p)[None], zero,
                                                          size, normals=n, lines=term.lines, axis=term.axis, vis=term.vis)
        fit = align.scale_landmarks(pd[0].cpu().numpy().astype(np.float64), size, shape)
        more = {"contour_vertices": sel[0].cpu().numpy().astype(np.int64),
                "lmk_visibility": gate[0].cpu().numpy().astype(np.float64)}
    if listed is None:
        return dict(more, landmarks=fit, landmarks_target=np.full_like(fit, np.nan), lmk_error=np.float64(np.nan))
    on = conf > 0
    err = np.sqrt(((fit - listed) ** 2).sum(1))[on].mean() if on.any() else np.nan
    return dict(more, landmarks=fit, landmarks_target=np.asarray(listed, np.float64), lmk_error=np.float64(err))


def texture_rerender(tex, weight, views, light=None, mip=None):
    """With views a list of (uvmap [1, S, S, 2], cover [1, S, S], target [1, C, S, S]), per view (image [1, C, S, S] over
    background -1, error, covered, counted): the texture tex [1, C, T, T] drawn on the view's uv map; error is the mean
    absolute difference to the view's target over the `counted` pixels, those that are covered and where the look-up of
    the bake's weight [1, 1, T, T] is positive.  light: per view (gamma [1, Cl, 9], normals [1, 3, S, S]); tex is then an
    albedo and the image is op.light.shade of its look-up.  mip: None, or the lod bias of the mip-mapped look-up
    (op.texture.sample_mip), which then draws the texture and looks the weight up."""
    from .op import light as lighting, texture

    def look(t, uvmap, cover, background):
        if mip is None:
            return texture.sample(t, uvmap, cover, background)
        return texture.sample_mip(t, uvmap, cover, bias=float(mip), background=background)

    out = []
    with torch.no_grad():
        for i, (uvmap, cover, target) in enumerate(views):
            img = look(tex, uvmap, cover, -1.0)
            if light is not None:
                img = lighting.shade(img, light[i][1], cover, light[i][0], -1.0, -1.0)
            on = cover & (look(weight, uvmap, cover, 0.0)[:, 0] > 0)
            n = int(on.sum())
            err = float(((img - target).abs() * on.unsqueeze(1)).sum()) / max(n * int(img.shape[1]), 1)
            out.append((img, err, int(cover.sum()), n))
    return out


def texture_refine(tex, views, steps, lr=0.02, light=None, light_lr=0.005, mip=None):
    """(tex' [1, C, T, T], loss [STEPS]; the loss before every step) with views a list of (uvmap [1, S, S, 2], cover
    [1, S, S], target [1, C, S, S]): Adam (optim.FlatAdam) on the texture alone from tex, on the sum over the views' covered
    pixels of (render - target)^2; one texture for all views (Bt = 1).  The uv maps are fixed, so the tap list is built
    once; a texel no tap reaches has gradient 0 in every step and keeps its value bit for bit.  lr's default is a
    starting value, not tuned on any trained checkpoint.
    light: per view (gamma [1, Cl, 9], normals [1, 3, S, S]); tex is then an albedo, the render is op.light.shade of its
    look-up, and Adam runs on the albedo and the V lights together, the lights as a second FlatAdam group with light_lr
    (0.005: a starting value, not tuned) whose gradient the shading node writes into the group's buffer (ggamma_out; on
    the host it comes through autograd).  Returns (tex', loss, gamma' [V, Cl, 9]).
    mip: None, or the lod bias of the mip-mapped look-up: level 0 stays the parameter, the pyramid is rebuilt in every
    step (op.texture.mip_build), the lod and the 8-tap list are computed once, and a step's gradient reaches every texel
    under a drawn pixel's footprint, not the four the bilinear look-up reads."""
    from . import optim
    from .op import light as lighting, texture

    uvmap = torch.cat([u for u, _, _ in views], 0).contiguous()
    cover = torch.cat([c for _, c, _ in views], 0).contiguous()
    target = torch.cat([t for _, _, t in views], 0)
    p = tex.detach().clone().contiguous().requires_grad_(True)
    offs, total = optim.flat_layout([p])
    flat_g = torch.zeros(total, dtype=p.dtype, device=p.device)
    opt = optim.FlatAdam([p], flat_g, lr=float(lr))
    slot = optim.flat_views(flat_g, [p], offs)[0]
    tsize = (int(p.shape[-2]), int(p.shape[-1]))
    if mip is None:
        texture.tap_plan(uvmap, cover, tsize, 1)

        def look(background):
            return texture.sample(p, uvmap, cover, background)
    else:
        lod = texture.mip_lod(uvmap, cover, tsize, None, float(mip))
        texture.mip_tap_plan(uvmap, cover, lod, tsize, None, 1)

        def look(background):
            return texture.mip_sample(texture.mip_build(p), tsize, uvmap, cover, lod, background)
    on = cover.unsqueeze(1).to(p.dtype)
    losses = []
    if light is not None:
        normals = torch.cat([n for _, n in light], 0).contiguous()
        q = torch.cat([gam for gam, _ in light], 0).detach().clone().contiguous()
        direct = lighting.native_ok(p, normals, q)                   # the kernels write the light's gradient themselves
        q.requires_grad_(not direct)
        light_g = torch.zeros(optim.flat_layout([q])[1], dtype=q.dtype, device=q.device)
        light_opt = optim.FlatAdam([q], light_g, lr=float(light_lr), step_from=opt)
        light_slot = optim.flat_views(light_g, [q], [0])[0]
    for _ in range(int(steps)):
        if light is None:
            diff = (look(0.0) - target) * on
            loss = (diff * diff).sum()
            (g,) = torch.autograd.grad(loss, p)
        else:
            flat = look(-1.0)
            render = lighting.shade(flat, normals, cover, q, -1.0, -1.0, ggamma_out=light_g if direct else None)
            diff = (render - target) * on
            loss = (diff * diff).sum()
            if direct:
                (g,) = torch.autograd.grad(loss, p)
            else:
                g, gq = torch.autograd.grad(loss, (p, q))
                light_slot.copy_(gq)
        slot.copy_(g)
        opt.step()
        if light is not None:
            light_opt.step()
        losses.append(loss.detach())
    history = torch.stack(losses).cpu().numpy().astype(np.float64)
    if light is not None:
        return p.detach().clone(), history, q.detach().clone()
    return p.detach().clone(), history


class TextureGuide:
    """The texture options of one run: the layout and its texel map (built once), and `outputs`, which bakes one fitted
    sample and writes its files."""

    def __init__(self, face, size, uv_file=None, source="picture", facing="0.1,0.4", passes=8, fill="mean", check=False,
                 turntable=0, turntable_yaw=30.0, refine=0, refine_lr=0.02, light=None, mip=None, render_aa=False):
        """render_aa: the turntable's draws are antialiased along the mesh's silhouette edges (op.edge).
        light: None (the texture is the plain bake) or a dict with any of mono (one white light), floor (unshade's),
        ridge (the fit's), lr (the light's learning rate under refinement) and relight (a file of 9 or 9 C numbers):
        every bake is then separated into an albedo and a light (op.light).  mip: None, or the lod bias with which
        every draw goes through the mip-mapped look-up (--texture_mip)."""
        from .face_model import load_uv, uv_layout
        from .op import texture

        model, tri = face
        self.light = None
        if light is not None:
            self.light = dict(mono=bool(light.get("mono", False)), floor=float(light.get("floor", 0.05)),
                              ridge=float(light.get("ridge", 1e-3)), lr=float(light.get("lr", 0.005)), relight=None)
            if not self.light["floor"] > 0 or not self.light["ridge"] >= 0 or not self.light["lr"] > 0:
                raise SystemExit("reconstruct: --light_floor and --light_lr are positive, --light_ridge is not negative")
            if light.get("relight"):
                self.light["relight"] = self.read_light(light["relight"])
        self.lights = []                                                 # (--multiview: the views' (gamma, normal map))
        self.mip = None if mip is None else float(mip)
        self.render_aa = bool(render_aa)
        if self.mip is not None and not np.isfinite(self.mip):
            raise SystemExit("reconstruct: --texture_mip takes a finite bias")
        self.size = int(size)
        if not 1 <= self.size <= 8192:
            raise SystemExit("reconstruct: --texture T lies in [1, 8192]")
        try:
            lo, hi = (float(x) for x in facing.split(","))
        except ValueError:
            raise SystemExit("reconstruct: --texture_facing takes LO,HI")
        if not lo <= hi:
            raise SystemExit("reconstruct: --texture_facing needs LO <= HI")
        self.facing, self.source, self.fill = (lo, hi), source, fill
        self.check, self.turntable, self.turntable_yaw = bool(check), int(turntable), float(turntable_yaw)
        self.refine_steps, self.refine_lr = int(refine), float(refine_lr)
        if self.turntable < 0 or self.refine_steps < 0 or not self.refine_lr > 0:
            raise SystemExit("reconstruct: --turntable and --texture_refine are not negative, --texture_lr is positive")
        self.views = []                                                  # (--multiview: what the merged texture is checked on)
        self.view_size = None                                            # the fit's resolution, known with the first sample
        self.passes = int(passes)
        if not 0 <= self.passes <= texture.MAX_PASSES:
            raise SystemExit("reconstruct: --texture_pad lies in [0, %d]" % texture.MAX_PASSES)
        dev = tri.device
        try:
            if uv_file:
                if not os.path.isfile(uv_file):
                    raise SystemExit("reconstruct: --uv file %s not found" % uv_file)
                uv, tri_uv = load_uv(uv_file, tri)
                keep = None
            else:
                with torch.no_grad():
                    v = model.mesh(torch.zeros(1, model.n_coeff, device=dev), torch.zeros(1, 7, device=dev), tri)[0]
                uv, tri_uv, keep = uv_layout(v[0].cpu(), tri)
            self.uv, self.tri_uv = uv, tri_uv                            # (on the host: what the .obj lists)
            self._layout = (uv.to(dev), tri_uv, keep)                    # (kept: the map's cache key holds their addresses)
            self.face, self.coeff = texture.texel_map(self._layout[0], tri_uv, self.size, keep)
        except (ValueError, OSError) as e:
            raise SystemExit("reconstruct: %s" % e)

    def finish(self, tex, weight):
        """The texture as it is written: padded and filled (tex [1, C, T, T] of a bake or a merge, with its weight)."""
        from .op import texture

        out, filled = texture.pad(tex, weight, self.passes)
        if self.fill == "mean":
            out = texture.fill_mean(out, weight, filled)
        return out

    renders = property(lambda self: self.check or self.refine_steps > 0)

    @staticmethod
    def read_light(path):
        """A light from an .npy or a text file of 9 numbers (one white light) or 9 C: float32 [Cl, 9] on the host."""
        try:
            values = np.load(path) if path.endswith(".npy") else np.loadtxt(path)
            values = np.asarray(values, np.float64).reshape(-1)
        except (OSError, ValueError) as e:
            raise SystemExit("reconstruct: --relight %s: %s" % (path, e))
        if values.size == 0 or values.size % 9 or not np.isfinite(values).all():
            raise SystemExit("reconstruct: --relight takes a file of 9 or 9 C finite numbers, got %d" % values.size)
        return torch.from_numpy(values.reshape(-1, 9).astype(np.float32))

    def separate(self, tex, weight, n, tri):
        """(albedo [1, C, T, T], gamma [1, Cl, 9], residual): the bake tex with its weight split into an albedo and the
        closed-form light of op.light.fit on the texels' normals (the camera-space vertex normals n [1, nv, 3] carried
        through the texel map); residual is the weighted rms of tex - shade(mean intensity, normals, gamma) over the
        fitted texels: what a constant albedo under the fitted light leaves unexplained."""
        from .op import light as lighting

        with torch.no_grad():
            tn = lighting.texel_attribute(n.to(tex.dtype).contiguous(), tri, self.face, self.coeff)
            gamma = lighting.fit(tex, tn, weight, mono=self.light["mono"], ridge=self.light["ridge"])
            on = (weight[:, 0] > 0).contiguous()
            albedo = lighting.unshade(tex, tn, on, gamma, floor=self.light["floor"])
            total = weight.sum().clamp_min(1e-12)
            mean = ((tex * weight).sum((2, 3), keepdim=True) / total).expand_as(tex).contiguous()
            diff = (tex - lighting.shade(mean, tn, on, gamma, -1.0, -1.0)) * on.unsqueeze(1)
            residual = float(torch.sqrt((weight * diff * diff).sum() / (total * tex.shape[1])))
        return albedo, gamma, residual

    def normals_at(self, vd, n, tri, size):
        """The normal map [1, 3, S, S] the shading reads: the camera-space normals n drawn over the mesh vd as the camera
        sees it (projected when there is a camera)."""
        from .op import light as lighting

        with torch.no_grad():
            return lighting.normal_map(vd.contiguous(), n.to(vd.dtype).contiguous(), tri, size)

    def view(self, inv, index):
        """(uvmap [1, S, S, 2], cover [1, S, S], target [1, 3, S, S]) of sample `index`: the uv map of the fitted mesh at the
        fitted pose and camera at the fit's resolution, and the fit's target.  The mesh is fixed from here on, so the tap
        list of the map is built once."""
        from .op import texture

        k = slice(index, index + 1)
        v, _, tri = inv.fitted_mesh()
        with torch.no_grad():
            uvmap, cover = texture.uv_map(v[k].contiguous(), tri, self._layout[0], self.tri_uv, int(inv.target.shape[-1]),
                                          self._layout[2])
        return uvmap, cover, inv.target[k].to(uvmap.dtype).contiguous()

    def checked(self, tex, weight, views, prefix="", light=None):
        """(tex as it is written, .npz entries, the re-rendered images): --texture_refine and --texture_check on the padded
        texture tex over `views`; the entries' names start with `prefix`.  light: per view [gamma, normal map] (tex is an
        albedo); refinement replaces the gammas in place by the refined ones."""
        entries, before = {}, None
        if self.check and self.refine_steps:
            before = texture_rerender(tex, weight, views, light, mip=self.mip)
        if self.refine_steps and light is None:
            tex, loss = texture_refine(tex, views, self.refine_steps, self.refine_lr, mip=self.mip)
            entries[prefix + "texture_refine_loss"] = loss
        elif self.refine_steps:
            tex, loss, gammas = texture_refine(tex, views, self.refine_steps, self.refine_lr, light, self.light["lr"],
                                               mip=self.mip)
            entries[prefix + "texture_refine_loss"] = loss
            for i, pair in enumerate(light):
                pair[0] = gammas[i:i + 1].contiguous()
        images = []
        if self.check:
            after = texture_rerender(tex, weight, views, light, mip=self.mip)
            one = len(views) == 1 and not prefix
            pick = (lambda col: np.float64(col[0])) if one else (lambda col: np.asarray(col, np.float64))
            entries[prefix + "rerender_error"] = pick([r[1] for r in after])
            entries[prefix + "rerender_covered"] = pick([r[2] for r in after])
            entries[prefix + "rerender_counted"] = pick([r[3] for r in after])
            if before is not None:
                entries[prefix + "rerender_error_before"] = pick([r[1] for r in before])
            images = [r[0] for r in after]
        return tex, entries, images

    def turn(self, tex, v, tri, size, kappa, out_dir, prefix, light=None):
        """Writes the --turntable renders <prefix>_turn_KK.png: the mesh v [1, nv, 3] turned about the vertical axis through
        its centroid by yaws spaced evenly in [-DEG, DEG] (one render: 0), projected by the camera kappa [1] when there is
        one, drawn with tex over background -1.  light = (gamma [1, Cl, 9], n [1, nv, 3]): tex is an albedo; the normals
        turn with the mesh and the light stays fixed in the camera's frame, so the shading moves over the head."""
        from .op import camera, light as lighting, texture

        n = self.turntable
        yaws = np.linspace(-self.turntable_yaw, self.turntable_yaw, n) if n > 1 else np.zeros(1)
        with torch.no_grad():
            centre = v.mean(1, keepdim=True)
            for j, deg in enumerate(yaws):
                angle = torch.tensor([np.deg2rad(deg), 0.0, 0.0], dtype=v.dtype, device=v.device)
                turned = torch.matmul(v - centre, utils_3d.euler_mat(angle)) + centre
                if kappa is not None:
                    turned = camera.project(turned.contiguous(), kappa)
                img, cover = texture.render(turned.contiguous(), tri, self._layout[0], self.tri_uv, tex, size, -1.0,
                                            self._layout[2], mip=self.mip, antialias=self.render_aa and light is None)
                if light is not None:
                    nmap = self.normals_at(turned, torch.matmul(light[1].to(v.dtype), utils_3d.euler_mat(angle)), tri, size)
                    img = lighting.shade(img, nmap, cover, light[0], -1.0, -1.0)
                    if self.render_aa:                           # (after the shading: the outline blends lit colours)
                        from .op.edge import antialias

                        img = antialias(img, turned.contiguous(), tri)
                generate.save_image(img.clamp(-1, 1).cpu(), os.path.join(out_dir, "%s_turn_%02d.png" % (prefix, j)))

    @staticmethod
    def save_grey(grey, path):
        try:
            from PIL import Image

            Image.fromarray(grey).save(path)
        except ImportError:
            with open(os.path.splitext(path)[0] + ".pgm", "wb") as f:
                f.write(b"P5 %d %d 255\n" % (grey.shape[1], grey.shape[0]) + grey.tobytes())

    def start(self, inv, index, path):
        """(texture [1, C, T, T], bake, weight) of sample `index` at the inverter's current state: the bake, padded and
        filled as it would be written: what --photo starts from."""
        from .op import texture

        k = slice(index, index + 1)
        v, n, tri = inv.fitted_mesh()
        v, n = v[k].contiguous(), n[k].contiguous()
        picture = inv.image[k] if self.source == "render" else load_picture(path).to(v.device)
        side = min(1024, max(int(inv.target.shape[-1]), self.size))
        with torch.no_grad():
            zbuf = texture.depth_buffer(v, tri, side)
            tex, weight = texture.bake(v, n, tri, self.face, self.coeff, picture.to(v.dtype).contiguous(), zbuf,
                                       facing=self.facing)
            return self.finish(tex, weight), tex, weight

    def outputs(self, inv, index, out_dir, stem, path, keep=None, photo=None):
        """Writes the four texture files of sample `index` and returns the .npz entry `texture_coverage`.  keep: a list
        that receives the bake before padding, (tex [1, C, T, T], weight [1, 1, T, T]), and makes the returned entries
        hold it too (`texture`, `texture_weight`): the views of --multiview, merged afterwards.  photo: the texture
        [1, C, T, T] of the photometric phase (--photo); it stands where the padded bake would, and where the bake of the
        final mesh has weight it is what a light is separated from and what the views hand to the merge."""
        from .op import texture

        k = slice(index, index + 1)
        v, n, tri = inv.fitted_mesh()
        v, n = v[k].contiguous(), n[k].contiguous()
        self.view_size = int(inv.target.shape[-1])
        # (under a camera the bake reads the projected mesh and the .obj lists the camera-space one)
        vo, no = (t[k] for t in inv.fitted_mesh(projected=False)[:2]) if inv.camera is not None else (v, n)
        if self.source == "render":
            picture = inv.image[k]
        else:
            picture = load_picture(path).to(v.device)                    # its own resolution, uploaded once
        side = min(1024, max(int(inv.target.shape[-1]), self.size))
        with torch.no_grad():
            zbuf = texture.depth_buffer(v, tri, side)
            tex, weight = texture.bake(v, n, tri, self.face, self.coeff, picture.to(v.dtype).contiguous(), zbuf,
                                       facing=self.facing)
            cover = float(texture.coverage(self.face, weight)[0])
            if photo is not None:
                out = photo.to(tex.dtype).contiguous()
                tex = torch.where(weight > 0, out, torch.zeros_like(out))
            else:
                out = self.finish(tex, weight)
        more = {} if self.mip is None else {"texture_mip": np.float64(self.mip)}
        lit = pair = None
        if self.light is not None:
            # the bake splits into an albedo and a light; from here on `out` is the albedo and `lit` the plain bake
            lit, baked = out, tex
            tex, gamma, residual = self.separate(baked, weight, no, tri)
            with torch.no_grad():
                out = self.finish(tex, weight)
            pair = [gamma, self.normals_at(v, no, tri, self.view_size)]
            more["light_residual"] = np.float64(residual)
        if self.renders or (self.light is not None and self.light["relight"] is not None):
            views = [self.view(inv, index)]
        if self.renders:
            out, entries, images = self.checked(out, weight, views, light=None if pair is None else [pair])
            more.update(entries)
            if images:
                generate.save_image(images[0].clamp(-1, 1).cpu(), os.path.join(out_dir, stem + "_rerender.png"))
            if pair is not None and self.check:
                more["rerender_error_lit"] = np.float64(texture_rerender(lit, weight, views, mip=self.mip)[0][1])
            if keep is not None:
                self.views.append(views[0])
        shown = pair
        if pair is not None:
            from .op import light as lighting

            more["light"] = pair[0][0].cpu().numpy()
            if self.refine_steps:
                more["light_fit"] = gamma[0].cpu().numpy()
            if keep is not None:
                self.lights.append([gamma, pair[1]])                     # (the closed-form light: what the albedo was made with)
            with torch.no_grad():
                drawn = (pair[1] != 0).any(1).contiguous()
                grey = lighting.shade(torch.zeros_like(pair[1]), pair[1], drawn, pair[0], -1.0, -1.0)
                generate.save_image(grey.clamp(-1, 1).cpu(), os.path.join(out_dir, stem + "_shading.png"))
                generate.save_image(lit.clamp(-1, 1).cpu(), os.path.join(out_dir, stem + "_texture_lit.png"))
                if self.light["relight"] is not None:
                    other = self.light["relight"].to(out.device)
                    if other.shape[0] not in (1, out.shape[1]):
                        raise SystemExit("reconstruct: --relight holds %d lights, the texture has %d channels"
                                         % (other.shape[0], out.shape[1]))
                    shown = [other[None].contiguous(), pair[1]]
                    uvmap, seen, _ = views[0]
                    flat = (texture.sample(out, uvmap, seen, -1.0) if self.mip is None else
                            texture.sample_mip(out, uvmap, seen, bias=self.mip, background=-1.0))
                    relit = lighting.shade(flat, pair[1], seen, shown[0], -1.0, -1.0)
                    generate.save_image(relit.clamp(-1, 1).cpu(), os.path.join(out_dir, stem + "_relit.png"))
        if self.turntable:
            self.turn(out, vo.contiguous(), tri, int(inv.target.shape[-1]),
                      inv.camera.detach()[k].contiguous() if inv.camera is not None else None, out_dir, stem,
                      None if shown is None else (shown[0], no.contiguous()))
        generate.save_image(out.clamp(-1, 1).cpu(), os.path.join(out_dir, stem + "_texture.png"))
        grey = np.round(weight[0, 0].cpu().numpy().astype(np.float64) * 255.0).astype(np.uint8)
        try:
            from PIL import Image

            Image.fromarray(grey).save(os.path.join(out_dir, stem + "_texture_weight.png"))
        except ImportError:
            with open(os.path.join(out_dir, stem + "_texture_weight.pgm"), "wb") as f:
                f.write(b"P5 %d %d 255\n" % (grey.shape[1], grey.shape[0]) + grey.tobytes())
        utils_3d.save_textured_obj(os.path.join(out_dir, stem + "_textured.obj"), vo[0].cpu().numpy(), tri.cpu().numpy(),
                                   self.uv.numpy(), self.tri_uv.numpy(), no[0].cpu().numpy(), stem + "_texture.png")
        if keep is not None:
            keep.append((tex, weight))                                   # (with a light: the view's albedo is what is merged)
            if pair is not None:
                more["texture_lit"] = baked[0].cpu().numpy()
            return dict(more, texture_coverage=np.float64(cover), texture=tex[0].cpu().numpy(),
                        texture_weight=weight[0, 0].cpu().numpy())
        return dict(more, texture_coverage=np.float64(cover))

    def merged_outputs(self, bakes, sharpness, out_dir, name, v, n, tri):
        """Merges the views' bakes (`outputs`' keep list), writes the subject's NAME_merged_texture.png, _weight.png,
        _views.png and NAME_merged.obj / .mtl on the mesh v, n [1, nv, 3], and returns the entries of NAME_identity.npz."""
        from .op import texture

        with torch.no_grad():
            tex, weight, best = texture.merge(torch.cat([t for t, _ in bakes], 0), torch.cat([w for _, w in bakes], 0),
                                              sharpness)
            cover = float(texture.coverage(self.face, weight)[0])
            out = self.finish(tex, weight)
        more = {}
        lights = None
        if self.light is not None:
            # every view keeps its own light; the merged albedo is shaded with each view's (and refined under all of them)
            lights, self.lights = self.lights[-len(bakes):], []
        if self.renders:
            # the merged texture on every view's own mesh and target: the number the merge is tuned against
            views, self.views = self.views[-len(bakes):], []
            out, more, _ = self.checked(out, weight, views, "merged_", light=lights)
        if lights is not None:
            more["lights"] = torch.cat([pair[0] for pair in lights], 0).cpu().numpy()
        if self.turntable:
            shown = None
            if lights is not None:
                gamma = lights[0][0] if self.light["relight"] is None else self.light["relight"].to(v.device)[None].contiguous()
                shown = (gamma, n)
            self.turn(out, v, tri, int(self.view_size), None, out_dir, name + "_merged", shown)
        generate.save_image(out.clamp(-1, 1).cpu(), os.path.join(out_dir, name + "_merged_texture.png"))
        grey = np.round(weight[0, 0].cpu().numpy().astype(np.float64) * 255.0).astype(np.uint8)
        self.save_grey(grey, os.path.join(out_dir, name + "_merged_texture_weight.png"))
        self.save_grey(np.ascontiguousarray(best.cpu().numpy()), os.path.join(out_dir, name + "_merged_texture_views.png"))
        utils_3d.save_textured_obj(os.path.join(out_dir, name + "_merged.obj"), v[0].cpu().numpy(), tri.cpu().numpy(),
                                   self.uv.numpy(), self.tri_uv.numpy(), n[0].cpu().numpy(), name + "_merged_texture.png")
        return dict(more, merged_coverage=np.float64(cover), merged_texture=tex[0].cpu().numpy(),
                    merged_weight=weight[0, 0].cpu().numpy(), merged_best=best.cpu().numpy())


def reconstruct(g, percept, face, target, steps, lr=0.05, pose_lr=0.01, coeff_lr=0.01, shape_reg=0.0,
                n_mean_latent=4096, **inverter_args):
    """Fits one image; returns the inverter (w, pose, coeff, image, fitted_mesh()) and the loss history (host).
    inverter_args: LatentInverter's further keywords (landmarks, mask, camera)."""
    inv = inversion.LatentInverter(g, percept, target, None, lr=lr, pose_lr=pose_lr, n_mean_latent=n_mean_latent,
                                   face=face, fit_shape=True, coeff_lr=coeff_lr, shape_reg=shape_reg, **inverter_args)
    hist = inv.run(steps)
    return inv, hist.cpu().numpy()


def reconstruct_batch(g, percept, face, target, steps, lr=0.05, pose_lr=0.01, coeff_lr=0.01, shape_reg=0.0,
                      n_mean_latent=4096, inv=None, shared_identity=None, **inverter_args):
    """Fits the B images of target [B, 3, H, W] together; `inv` (an inverter of the same batch from an earlier call) is
    re-targeted instead of built anew.  Returns the inverter and the loss history [steps, B] (host).  inverter_args:
    LatentInverter's further keywords (landmarks, mask, camera; a re-targeted inverter takes landmarks, landmark_conf and
    mask from them and keeps the rest as it was built).  shared_identity=K: the images are views of one subject and share
    the leading K coefficients (a re-targeted inverter keeps the K it was built with)."""
    if inv is None:
        more = {} if shared_identity is None else {"shared_identity": shared_identity}
        inv = inversion.LatentInverter(g, percept, target, None, lr=lr, pose_lr=pose_lr, n_mean_latent=n_mean_latent,
                                       face=face, fit_shape=True, coeff_lr=coeff_lr, shape_reg=shape_reg, **more,
                                       **inverter_args)
    elif inverter_args:
        inv.reset(target, inverter_args.get("landmarks"), inverter_args.get("landmark_conf"),
                  **({"mask": inverter_args["mask"]} if inverter_args.get("mask") is not None else {}),
                  **({"silhouette": inverter_args["silhouette"]} if inverter_args.get("silhouette") is not None else {}))
    else:
        inv.reset(target)
    hist = inv.run(steps)
    return inv, hist.cpu().numpy().reshape(steps, -1)


def write_outputs(inv, hist, out_dir, stem, index=0, extras=None):
    """The five files of sample `index` of the inverter (hist: its loss history [steps]; extras: further .npz entries)."""
    from .op.rasterize import rasterize

    k = slice(index, index + 1)
    # the camera-space mesh is what is written; the normal map draws what the generator saw: under a camera the projected
    # vertices with the camera-space normals
    v, n, tri = inv.fitted_mesh(projected=False)
    v, n = v[k], n[k]
    vd = inv.fitted_mesh()[0][k] if inv.camera is not None else v
    coeff = inv.coeff.detach()[k]
    pose = inv.pose.detach().view(-1, 7)[index]
    with torch.no_grad():
        zero = torch.zeros_like(pose).view(1, 7)
        vc, nc = inv.face_model.mesh(coeff, zero, tri)[:2]
        size = int(inv.target.shape[-1])
        normal_map = rasterize(vd.contiguous(), n.contiguous(), tri, size, size, channel_major=True)
    tri_h = tri.cpu().numpy()
    utils_3d.save_obj(os.path.join(out_dir, stem + ".obj"), v[0].cpu().numpy(), tri_h, vn=n[0].cpu().numpy())
    utils_3d.save_obj(os.path.join(out_dir, stem + "_canonical.obj"), vc[0].cpu().numpy(), tri_h,
                      vn=nc[0].cpu().numpy())
    generate.save_image(inv.image[k].cpu(), os.path.join(out_dir, stem + "_render.png"))
    generate.save_image(normal_map.cpu(), os.path.join(out_dir, stem + "_normal.png"))
    if inv.camera is not None:
        kappa = float(inv.camera.detach()[index])
        extras = dict(extras or {}, camera=np.float64(kappa),
                      camera_distance=np.float64(1.0 / kappa if kappa != 0 else np.inf))
    np.savez(os.path.join(out_dir, stem + ".npz"), w=inv.w.detach()[k].cpu().numpy(), coeff=coeff.cpu().numpy(),
             pose=pose.cpu().numpy(), loss=hist, **inv.face_model.fit_extras(coeff), **(extras or {}))


def subject_outputs(inv, hist, out_dir, name, stems, covers=None, painter=None, bakes=None, sharpness=2):
    """The per-subject files of a --multiview group: NAME_identity.obj (the model's mesh at the shared coefficients, every
    other coefficient and the pose 0) and NAME_identity.npz; with a painter also the merged texture's files.  hist
    [steps, V]: the views' loss histories; covers: the views' `texture_coverage`."""
    k = inv.shared_identity
    coeff = inv.coeff.detach()
    shared = coeff[0, :k]
    with torch.no_grad():
        only = torch.zeros_like(coeff[:1])
        only[0, :k] = shared
        v, n = inv.face_model.mesh(only, torch.zeros(1, 7, device=coeff.device, dtype=coeff.dtype), inv.tri)[:2]
    utils_3d.save_obj(os.path.join(out_dir, name + "_identity.obj"), v[0].cpu().numpy(), inv.tri.cpu().numpy(),
                      vn=n[0].cpu().numpy())
    entries = {"identity": shared.cpu().numpy(), "views": np.asarray(stems), "loss": hist.sum(1)}
    if inv.camera is not None:
        entries["camera"] = inv.camera.detach()[:len(stems)].cpu().numpy().astype(np.float64)
    if painter is not None:
        entries.update(painter.merged_outputs(bakes, sharpness, out_dir, name, v.contiguous(), n.contiguous(), inv.tri))
        entries["texture_coverage"] = np.asarray(covers, np.float64)
    np.savez(os.path.join(out_dir, name + "_identity.npz"), **entries)
    return entries


def main(argv=None):
    ap = argparse.ArgumentParser(description="Face reconstruction: fit W+, pose and 3DMM coefficients to images")
    ap.add_argument("--size", type=int, default=256, help="output image size of the generator [%(default)d]")
    ap.add_argument("--steps", type=int, default=400, help="Adam iterations per image [%(default)d]")
    ap.add_argument("--lr", type=float, default=0.05, help="learning rate of the W+ latent [%(default)g]")
    ap.add_argument("--pose_lr", type=float, default=0.01, help="learning rate of the pose [%(default)g]")
    ap.add_argument("--coeff_lr", type=float, default=0.01, help="learning rate of the 3DMM coefficients [%(default)g]")
    ap.add_argument("--shape_reg", type=float, default=1e-3,
                    help="weight of the coefficient prior: sum (coeff / sigma)^2, or the Dirichlet / Beta prior of "
                         "--facewarehouse, which with a --beta_shape below 1 (the default) is unbounded below and pushes "
                         "the identity away from the mean: use --beta_shape >= 1 or --shape_reg 0 there [%(default)g]")
    which = ap.add_mutually_exclusive_group()
    which.add_argument("--bfm", default=None, metavar="BFM.mat", help="Basel Face Model (.mat); default: synthetic 3DMM")
    which.add_argument("--flame", default=None, metavar="FLAME.{pkl,mat}",
                       help="FLAME skinned model: shape and the neck / jaw / eye rotations are fitted")
    which.add_argument("--facewarehouse", default=None, metavar="FW.mat",
                       help="FaceWarehouse bilinear blendshape model: identity and expression weights are fitted")
    ap.add_argument("--beta_shape", type=float, default=.01,
                    help="with --facewarehouse: Dirichlet concentration of the identity prior; the reference's .01 is "
                         "not a proper prior (see --shape_reg) [%(default)g]")
    ap.add_argument("--lpips-trunk", default=None, metavar="PATH",
                    help="torchvision vgg16 (or vgg16().features) state dict for the LPIPS trunk")
    ap.add_argument("--n_mean_latent", type=int, default=4096, help="latents averaged for the starting W+ [%(default)d]")
    ap.add_argument("--batch", type=int, default=None,
                    help="images fitted together in one batched inverter (one captured graph) [1]")
    ap.add_argument("--multiview", type=int, default=None, metavar="V",
                    help="the images are consecutive groups of V views of one subject each: a group is fitted together "
                         "(as --batch V) with the identity coefficients shared by its views")
    ap.add_argument("--identity_dims", type=int, default=None, metavar="K",
                    help="with --multiview: how many leading coefficients the views share [the face model's n_identity]")
    ap.add_argument("--subject", default=None, metavar="NAME",
                    help="with --multiview and a single group: the name of the subject's files [the first view's stem]")
    ap.add_argument("--merge_sharpness", type=int, default=None, metavar="S",
                    help="with --multiview and --texture: the views' textures are blended with the weights "
                         "(w / max w)^(2^S), S in 0..4 [2]")
    ap.add_argument("--lmk", default=None, metavar="LANDMARKS.txt",
                    help="landmark file (one picture per line: its name and x y pairs in its pixels): guides the fit")
    ap.add_argument("--lmk_index", default=None, metavar="FILE",
                    help="the model's landmarks: .npy / .txt of vertex indices, or .npz with faces and bary; default: the "
                         "face model's own (a Basel file's landmarks68)")
    ap.add_argument("--lmk_weight", type=float, default=1.0,
                    help="weight of the landmark term; a starting value, not tuned on a trained checkpoint [%(default)g]")
    ap.add_argument("--lmk_beta", type=float, default=1.0, help="smooth-L1 threshold of the term in pixels [%(default)g]")
    ap.add_argument("--lmk_contour", type=float, default=1.0,
                    help="weight of landmarks 0-16 (the jaw line) of a 68-point set [%(default)g]")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--lmk_dynamic", action="store_true",
                     help="the jaw landmarks (0-16 of a 68-point set) slide along the posed mesh's silhouette: contour "
                          "lines built from the model's mean shape")
    how.add_argument("--lmk_lines", default=None, metavar="FILE",
                     help="hand-made contour lines: .npz with line_lmk, side, cand_off and cand")
    ap.add_argument("--lmk_axis", default=None, metavar="I,J",
                    help="with contour lines: the two landmarks whose vertices span the face's up direction [27,8 of a "
                         "68-point set; required for other landmark counts]")
    ap.add_argument("--lmk_vis", default=None, metavar="LO,HI",
                    help="fade a landmark out as the z of its normal falls from HI to LO (turned away from the camera); off "
                         "unless given; 0,0.2 is a starting value, untuned like --lmk_weight")
    ap.add_argument("--mask_lmk", action="store_true",
                    help="the image loss sees only the filled polygon of --lmk's landmarks (their convex hull)")
    ap.add_argument("--mask_tri", default=None, metavar="FILE",
                    help="with --mask_lmk: a landmark triangulation to fill instead of the hull: .obj (f lines, 1-based) or "
                         ".npy / .txt of [T, 3] (0-based)")
    ap.add_argument("--mask_margin", type=int, default=0, metavar="R",
                    help="with --mask_lmk: grow (R > 0) or shrink (R < 0) the polygon by R pixels, |R| <= 32 [%(default)d]")
    ap.add_argument("--mask_dir", default=None, metavar="DIR",
                    help="masks of the pictures: DIR/<stem>.png or .npy, grey in [0, 1]; a missing file is all ones")
    ap.add_argument("--mask_mesh", action="store_true",
                    help="gate the region in every step by the fitted mesh's coverage of the picture")
    ap.add_argument("--texture", type=int, nargs="?", const=512, default=None, metavar="T",
                    help="bake a T x T texture of the picture on the fitted mesh and write a textured .obj [512 when given "
                         "without a number]")
    ap.add_argument("--uv", default=None, metavar="FILE",
                    help="with --texture: the layout, an .obj with vt lines and f a/t records over the model's faces, or an "
                         ".npz with vt and ft; default: a cylindrical unwrap of the model's mean shape")
    ap.add_argument("--texture_from", default=None, choices=("picture", "render"),
                    help="with --texture: sample the file's picture at its own resolution, or the generator's image of the "
                         "fit [picture]")
    ap.add_argument("--texture_facing", default=None, metavar="LO,HI",
                    help="with --texture: a texel fades out as the z of its normal falls from HI to LO; 0.1,0.4 is a "
                         "starting value, untuned like --lmk_weight [0.1,0.4]")
    ap.add_argument("--texture_pad", type=int, default=None, metavar="N",
                    help="with --texture: grow the charts by N texels (0..64) [8]")
    ap.add_argument("--texture_fill", default=None, choices=("mean", "none"),
                    help="with --texture: paint the texels still unfilled with the mean colour, or leave them black [mean]")
    ap.add_argument("--texture_check", action="store_true",
                    help="with --texture: draw the written texture on the fitted mesh at the fit's resolution "
                         "(<stem>_rerender.png) and report its mean absolute difference to the target (rerender_error)")
    ap.add_argument("--turntable", type=int, default=None, metavar="N",
                    help="with --texture: write N renders <stem>_turn_KK.png of the textured mesh turned about its vertical "
                         "axis")
    ap.add_argument("--turntable_yaw", type=float, default=None, metavar="DEG",
                    help="with --turntable: the yaws are spaced evenly in [-DEG, DEG] [30]")
    ap.add_argument("--texture_refine", type=int, default=None, metavar="STEPS",
                    help="with --texture: STEPS Adam steps on the texture alone against the target, from the padded bake "
                         "(or merge); the refined texture is the one written")
    ap.add_argument("--texture_lr", type=float, default=None, metavar="LR",
                    help="with --texture_refine: Adam's learning rate; a starting value, not tuned [0.02]")
    ap.add_argument("--texture_mip", type=float, nargs="?", const=0.0, default=None, metavar="BIAS",
                    help="with --texture: every draw of --texture_check, --turntable, --relight and --texture_refine looks "
                         "the texture up through its mip pyramid (trilinear; BIAS is added to the level of detail [0])")
    ap.add_argument("--photo", type=float, nargs="?", const=1.0, default=None, metavar="WEIGHT",
                    help="with --texture: after the fit and the bake, run --photo_steps iterations of the fit with a "
                         "photometric term of this weight (the textured mesh against the picture; the texture, the pose, "
                         "the coefficients and the camera move), starting from the bake, and write every output from the "
                         "state after them [%(const)g; this and the two below are untuned starting values]")
    ap.add_argument("--photo_steps", type=int, default=None, metavar="N",
                    help="iterations of the photometric phase [100; untuned]")
    ap.add_argument("--photo_lr", type=float, default=None, metavar="LR",
                    help="learning rate of the texture in the photometric phase [0.01; untuned]")
    ap.add_argument("--photo_edges", action="store_true",
                    help="with --photo: the term compares the render composited over the picture and antialiased along "
                         "the mesh's silhouette edges (op.edge), so the outline takes part in it")
    ap.add_argument("--render_aa", action="store_true",
                    help="with --turntable: the renders (relit ones included) are antialiased along the mesh's silhouette "
                         "edges (op.texture.render(antialias=True)); --texture_check's re-render is not (its views "
                         "carry no mesh)")
    ap.add_argument("--silhouette_dir", default=None, metavar="DIR",
                    help="fit the mesh's outline to a silhouette: DIR/<stem>.png or .npy (grey, read and resized as "
                         "--mask_dir's files) against the antialiased coverage of the mesh (op.edge.coverage); writes "
                         "<stem>_coverage.png and the .npz entries silhouette_loss and silhouette_iou")
    ap.add_argument("--silhouette_weight", type=float, default=None, metavar="W",
                    help="weight of the silhouette term [1.0; an untuned starting value]")
    ap.add_argument("--light", action="store_true",
                    help="with --texture: separate every bake into an albedo and a light (second-order spherical "
                         "harmonics, fitted in closed form); <stem>_texture.png is then the albedo")
    ap.add_argument("--light_mono", action="store_true",
                    help="with --light: one white light for all colour channels instead of one per channel")
    ap.add_argument("--light_floor", type=float, default=None, metavar="S",
                    help="with --light: the shading is not divided out below S; a starting value, not tuned [0.05]")
    ap.add_argument("--light_ridge", type=float, default=None, metavar="L",
                    help="with --light: the ridge on the light's non-constant coefficients, relative to the fitted "
                         "weight; a starting value, not tuned [0.001]")
    ap.add_argument("--light_lr", type=float, default=None, metavar="LR",
                    help="with --light and --texture_refine: Adam's learning rate of the light; a starting value, not "
                         "tuned [0.005]")
    ap.add_argument("--relight", default=None, metavar="FILE",
                    help="with --light: an .npy or text file of 9 or 9 C numbers, another light; <stem>_relit.png is the "
                         "fitted pose under it and the --turntable frames use it")
    cam = ap.add_mutually_exclusive_group()
    cam.add_argument("--camera_distance", type=float, default=None, metavar="D",
                     help="perspective camera at distance D > 0 from the plane z = 0 of pose space, in half-picture-widths "
                          "(the focal length in that unit): kappa = 1 / D; default: orthographic")
    cam.add_argument("--camera_fov", type=float, default=None, metavar="DEG",
                     help="perspective camera by its full field of view across the picture, 0 <= DEG < 180: kappa = tan(DEG / 2)")
    ap.add_argument("--fit_camera", action="store_true",
                    help="fit kappa = 1 / distance with the pose, one value per picture, from the start --camera_distance or "
                         "--camera_fov gives; it wants --lmk")
    ap.add_argument("--camera_lr", type=float, default=None,
                    help="learning rate of kappa; a starting value, not tuned [0.01]")
    ap.add_argument("--gpu", type=int, default=0, help="use gpu id")
    ap.add_argument("--seed", type=int, default=0, help="random seed (mean latent, noise)")
    ap.add_argument("--out", default="reconstruct", metavar="DIR", help="output directory [%(default)s]")
    ap.add_argument("ckpt", metavar="CHECKPOINT", help="checkpoint holding g_ema of a GeneratorWithMap")
    ap.add_argument("images", metavar="IMAGE", nargs="+", help="PNG / JPG, or .npy in [-1, 1] (HWC or CHW)")
    args = ap.parse_args(argv)
    if args.multiview is None:
        if args.identity_dims is not None or args.subject is not None or args.merge_sharpness is not None:
            ap.error("--identity_dims, --subject and --merge_sharpness need --multiview")
    else:
        if args.multiview < 1:
            ap.error("--multiview must be at least 1")
        if args.batch is not None and args.batch != args.multiview:
            ap.error("--multiview V implies --batch V and conflicts with --batch %d" % args.batch)
        if len(args.images) % args.multiview:
            raise SystemExit("reconstruct: --multiview %d takes the images in groups of %d views, got %d images"
                             % (args.multiview, args.multiview, len(args.images)))
        if args.subject is not None and len(args.images) != args.multiview:
            ap.error("--subject names the files of a single group; with several groups each takes its first view's stem")
        if args.merge_sharpness is not None and args.texture is None:
            ap.error("--merge_sharpness needs --texture")
        if args.merge_sharpness is not None and not 0 <= args.merge_sharpness <= 4:
            ap.error("--merge_sharpness lies in 0..4")
        args.batch = args.multiview
    if args.batch is None:
        args.batch = 1
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    if args.lmk_index and not args.lmk:
        ap.error("--lmk_index needs --lmk")
    if (args.lmk_dynamic or args.lmk_lines or args.lmk_axis or args.lmk_vis) and not args.lmk:
        ap.error("--lmk_dynamic, --lmk_lines, --lmk_axis and --lmk_vis need --lmk")
    if args.mask_lmk and not args.lmk:
        ap.error("--mask_lmk needs --lmk")
    if (args.mask_tri or args.mask_margin) and not args.mask_lmk:
        ap.error("--mask_tri and --mask_margin need --mask_lmk")
    if args.texture is None and (args.uv or args.texture_from or args.texture_facing or args.texture_pad is not None
                                 or args.texture_fill):
        ap.error("--uv, --texture_from, --texture_facing, --texture_pad and --texture_fill need --texture")
    if args.texture is None and (args.texture_check or args.turntable is not None or args.texture_refine is not None):
        ap.error("--texture_check, --turntable and --texture_refine need --texture")
    if args.texture is None and args.texture_mip is not None:
        ap.error("--texture_mip needs --texture")
    if args.photo is None and (args.photo_steps is not None or args.photo_lr is not None):
        ap.error("--photo_steps and --photo_lr need --photo")
    if args.render_aa and not args.turntable:
        ap.error("--render_aa needs --turntable")
    if args.photo_edges and args.photo is None:
        ap.error("--photo_edges needs --photo")
    if args.silhouette_dir is None and args.silhouette_weight is not None:
        ap.error("--silhouette_weight needs --silhouette_dir")
    if args.silhouette_dir is not None:
        if not os.path.isdir(args.silhouette_dir):
            ap.error("--silhouette_dir %s is not a directory" % args.silhouette_dir)
        args.silhouette_weight = 1.0 if args.silhouette_weight is None else args.silhouette_weight
        if not (args.silhouette_weight >= 0 and np.isfinite(args.silhouette_weight)):
            ap.error("--silhouette_weight takes a finite weight that is not negative")
    if args.photo is not None:
        if args.texture is None:
            ap.error("--photo needs --texture")
        if not (args.photo >= 0 and np.isfinite(args.photo)):
            ap.error("--photo takes a finite weight that is not negative")
        args.photo_steps = 100 if args.photo_steps is None else args.photo_steps
        args.photo_lr = 0.01 if args.photo_lr is None else args.photo_lr
        if args.photo_steps < 1 or not args.photo_lr >= 0:
            ap.error("--photo_steps is at least 1 and --photo_lr is not negative")
    if args.texture is None and (args.light or args.light_mono or args.light_floor is not None
                                 or args.light_ridge is not None or args.light_lr is not None or args.relight):
        ap.error("--light, --light_mono, --light_floor, --light_ridge, --light_lr and --relight need --texture")
    if not args.light and (args.light_mono or args.light_floor is not None or args.light_ridge is not None
                           or args.light_lr is not None or args.relight):
        ap.error("--light_mono, --light_floor, --light_ridge, --light_lr and --relight need --light")
    if args.light_lr is not None and args.texture_refine is None:
        ap.error("--light_lr needs --texture_refine")
    if args.turntable_yaw is not None and args.turntable is None:
        ap.error("--turntable_yaw needs --turntable")
    if args.texture_lr is not None and args.texture_refine is None:
        ap.error("--texture_lr needs --texture_refine")
    camera_args = {}
    if args.camera_distance is not None or args.camera_fov is not None:
        if args.camera_distance is not None:
            if not (args.camera_distance > 0 and np.isfinite(args.camera_distance)):
                ap.error("--camera_distance must be positive")
            kappa = 1.0 / args.camera_distance
        else:
            if not 0 <= args.camera_fov < 180:
                ap.error("--camera_fov lies in [0, 180) degrees")
            kappa = float(np.tan(np.deg2rad(args.camera_fov) / 2))
        camera_args = dict(camera=kappa, fit_camera=args.fit_camera,
                           camera_lr=0.01 if args.camera_lr is None else args.camera_lr)
    elif args.fit_camera or args.camera_lr is not None:
        ap.error("--fit_camera and --camera_lr need --camera_distance or --camera_fov (the start of the fit)")
    torch.manual_seed(args.seed)
    if torch.cuda.is_available() and 0 <= args.gpu < torch.cuda.device_count():
        device = torch.device("cuda:%d" % args.gpu)
        torch.cuda.set_device(device)
        torch.cuda.manual_seed(args.seed)
    else:
        device = torch.device("cpu")
    g = checkpoint.load_generator(args.ckpt, args.size, 512, 8, device=device, with_map=True)
    percept = lpips.PNetLin()
    if args.lpips_trunk:
        percept.net.load_trunk_state_dict(torch.load(args.lpips_trunk, map_location="cpu", weights_only=False))
    else:
        sys.stderr.write("warning: no --lpips-trunk given: the LPIPS VGG16 trunk is the deterministic synthetic fill, "
                         "so this is not a meaningful reconstruction\n")
    percept = percept.to(device)
    face = face_model(args.bfm, device, seed=args.seed, flame=args.flame, facewarehouse=args.facewarehouse,
                      beta_shape=args.beta_shape)
    guide = (LandmarkGuide(args.lmk, face, args.lmk_index, args.lmk_weight, args.lmk_beta, args.lmk_contour,
                           args.lmk_dynamic, args.lmk_lines, args.lmk_axis, args.lmk_vis) if args.lmk else None)
    masker = (MaskGuide(args.mask_lmk, args.mask_tri, args.mask_margin, args.mask_dir, args.mask_mesh,
                        guide.count if guide else None)
              if (args.mask_lmk or args.mask_dir or args.mask_mesh) else None)
    painter = (TextureGuide(face, args.texture, args.uv, args.texture_from or "picture", args.texture_facing or "0.1,0.4",
                            8 if args.texture_pad is None else args.texture_pad, args.texture_fill or "mean",
                            check=args.texture_check, turntable=args.turntable or 0,
                            turntable_yaw=30.0 if args.turntable_yaw is None else args.turntable_yaw,
                            refine=args.texture_refine or 0,
                            refine_lr=0.02 if args.texture_lr is None else args.texture_lr,
                            light=({k: v for k, v in (("mono", args.light_mono), ("floor", args.light_floor),
                                                      ("ridge", args.light_ridge), ("lr", args.light_lr),
                                                      ("relight", args.relight)) if v is not None}
                                   if args.light else None), mip=args.texture_mip, render_aa=args.render_aa)
               if args.texture is not None else None)
    shared = None
    if args.multiview is not None:
        shared = face[0].n_identity if args.identity_dims is None else args.identity_dims
        if not 1 <= shared <= face[0].n_coeff:
            raise SystemExit("reconstruct: the views share K coefficients with 1 <= K <= %d (the model's), got %d: pass "
                             "--identity_dims K" % (face[0].n_coeff, shared))
    os.makedirs(args.out, exist_ok=True)
    results = []

    def load(path):
        """(target on the host, what the landmark file says about the picture: LandmarkGuide.lookup's triple, or None,
        the picture's mask or None)."""
        if guide is None:
            return load_image(path, args.size), None, masker.lookup(path, None, args.size) if masker else None
        x, shape = load_image(path, args.size, with_shape=True)
        look = guide.lookup(path, shape, args.size) + (shape,)
        return x, look, masker.lookup(path, look, args.size) if masker else None

    photo_args = {}
    if args.photo is not None:
        photo_args = dict(photometric=painter._layout, photo_size=args.texture, photo_weight=args.photo,
                          photo_lr=args.photo_lr)
        if args.photo_edges:
            photo_args["photo_edges"] = True

    def silhouette_args(paths):
        """--silhouette_dir: the inverter's silhouette= [B, H, W] of these pictures (and its weight)."""
        return dict(silhouette=torch.cat([load_silhouette(args.silhouette_dir, path, args.size) for path in paths], 0),
                    silhouette_weight=args.silhouette_weight)

    def photo_error(tex, view):
        """The mean absolute difference between the texture drawn on a view and the view's target, over the covered
        pixels (texture_rerender's error with every texel counted)."""
        return texture_rerender(tex, torch.ones_like(tex[:, :1]), [view])[0][1]

    def photo_phase(inv, paths):
        """--photo: the bake of every sample at the fitted state (one merged texture when the rows are views of one
        subject) into the inverter's texture, then the photometric iterations.  Returns per sample the .npz entries
        photo_loss, photo_error_before and photo_error_after, and the texture [1, C, T, T] to write."""
        from .op import texture

        n = len(paths)
        starts = [painter.start(inv, i, path) for i, path in enumerate(paths)]
        with torch.no_grad():
            if inv.photo.bt == 1 and inv.batch > 1:
                merged, weight, _ = texture.merge(torch.cat([t for _, t, _ in starts], 0),
                                                  torch.cat([w for _, _, w in starts], 0),
                                                  2 if args.merge_sharpness is None else args.merge_sharpness)
                first = painter.finish(merged, weight)
            else:
                first = torch.cat([t for t, _, _ in starts] + [starts[-1][0]] * (inv.batch - n), 0)
        pick = (lambda t, i: t) if inv.photo.bt == 1 else (lambda t, i: t[i:i + 1])
        before = [photo_error(pick(first, i), painter.view(inv, i)) for i in range(n)]
        inv.set_texture(first)
        hist = inv.run(args.photo_steps, photometric=True).cpu().numpy().reshape(args.photo_steps, -1)
        final = inv.texture.clone()
        out = []
        for i in range(n):
            tex = pick(final, i).contiguous()
            out.append((dict(photo_loss=np.ascontiguousarray(hist[:, i]), photo_error_before=np.float64(before[i]),
                             photo_error_after=np.float64(photo_error(tex, painter.view(inv, i)))), tex))
        return out

    def more(inv, index, stem, extras, path, keep=None, photo=None):
        """The .npz entries with the region's and the texture's (and their files written), when there are any.  photo:
        (entries, texture) of the photometric phase."""
        if masker is not None:
            extras = dict(extras or {}, **mask_outputs(inv, index, args.out, stem))
        if args.silhouette_dir is not None:
            extras = dict(extras or {}, **silhouette_outputs(inv, index, args.out, stem))
        if painter is not None and photo is not None:
            extras = dict(extras or {}, **photo[0], **painter.outputs(inv, index, args.out, stem, path, keep, photo[1]))
        elif painter is not None:
            extras = dict(extras or {}, **painter.outputs(inv, index, args.out, stem, path, keep))
        return extras

    def closing():
        if guide:
            print(guide.summary(), flush=True)
        if masker and masker.dir:
            print(masker.summary(), flush=True)

    def tail(extras):
        if extras is None:
            return ""
        return ", landmarks %s" % ("not listed" if np.isnan(extras["lmk_error"]) else "%.3f px" % float(extras["lmk_error"]))

    if args.batch == 1 and shared is None:
        for path in args.images:
            stem = os.path.splitext(os.path.basename(path))[0]
            target, look, mask = load(path)
            lmk_args = guide.inverter_args([look[0]], [look[1]]) if guide else {}
            if masker:
                lmk_args.update(masker.inverter_args([mask]))
            lmk_args.update(camera_args)
            lmk_args.update(photo_args)
            if args.silhouette_dir is not None:
                lmk_args.update(silhouette_args([path]))
            inv, hist = reconstruct(g, percept, face, target.to(device), args.steps, args.lr, args.pose_lr, args.coeff_lr,
                                    args.shape_reg, args.n_mean_latent, **lmk_args)
            photo = photo_phase(inv, [path])[0] if args.photo is not None else None
            extras = landmark_outputs(inv, 0, look[1], look[2], look[3]) if guide else None
            write_outputs(inv, hist, args.out, stem, extras=more(inv, 0, stem, extras, path, photo=photo))
            print("%s: loss %.4f -> %.4f over %d steps, |coeff| %.4f%s" % (
                path, float(hist[0]), float(hist[-1]), len(hist), float(inv.coeff.detach().norm()), tail(extras)),
                flush=True)
            results.append((stem, hist))
        closing()
        return results
    inv = None
    for start in range(0, len(args.images), args.batch):
        group = args.images[start:start + args.batch]
        loaded = [load(path) for path in group]
        targets = [x for x, _, _ in loaded]
        targets += targets[-1:] * (args.batch - len(group))          # padding: fitted, then discarded
        looks = [look for _, look, _ in loaded]
        looks += looks[-1:] * (args.batch - len(group))
        masks = [m for _, _, m in loaded]
        masks += masks[-1:] * (args.batch - len(group))
        lmk_args = guide.inverter_args([k[0] for k in looks], [k[1] for k in looks]) if guide else {}
        if masker:
            lmk_args.update(masker.inverter_args(masks))
        lmk_args.update(camera_args)
        if inv is None:
            lmk_args.update(photo_args)
        if args.silhouette_dir is not None:
            lmk_args.update(silhouette_args(group + group[-1:] * (args.batch - len(group))))
        inv, hist = reconstruct_batch(g, percept, face, torch.cat(targets, 0).to(device), args.steps, args.lr,
                                      args.pose_lr, args.coeff_lr, args.shape_reg, args.n_mean_latent, inv=inv,
                                      shared_identity=shared, **lmk_args)
        stems = [os.path.splitext(os.path.basename(path))[0] for path in group]
        name = (args.subject or stems[0]) if shared is not None else None
        bakes = [] if shared is not None and painter is not None else None
        covers = []
        photos = photo_phase(inv, group) if args.photo is not None else None
        for i, path in enumerate(group):
            stem = stems[i]
            h = np.ascontiguousarray(hist[:, i])
            lmk = landmark_outputs(inv, i, looks[i][1], looks[i][2], looks[i][3]) if guide else None
            extras = more(inv, i, stem, lmk, path, bakes, None if photos is None else photos[i])
            if shared is not None:
                extras = dict(extras or {}, subject=np.asarray(name), view=np.int64(i))
                if painter is not None:
                    covers.append(float(extras["texture_coverage"]))
            write_outputs(inv, h, args.out, stem, index=i, extras=extras)
            print("%s: loss %.4f -> %.4f over %d steps, |coeff| %.4f%s" % (
                path, float(h[0]), float(h[-1]), len(h), float(inv.coeff.detach()[i].norm()), tail(lmk)), flush=True)
            results.append((stem, h))
        if shared is not None:
            entries = subject_outputs(inv, hist[:, :len(group)], args.out, name, stems, covers, painter, bakes,
                                      2 if args.merge_sharpness is None else args.merge_sharpness)
            print("%s: %d views share %d coefficients, |identity| %.4f%s" % (
                name, len(group), shared, float(np.linalg.norm(entries["identity"])),
                ", merged texture covers %.3f (views: %s)" % (float(entries["merged_coverage"]), " ".join(
                    "%.3f" % c for c in covers)) if painter is not None else ""), flush=True)
    closing()
    return results


if __name__ == "__main__":
    main()
