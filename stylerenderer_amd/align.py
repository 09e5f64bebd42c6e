"""Landmark face alignment (reference utils_face.py): a landmark file reader, the closed-form pose solvers, and the warp
of a picture onto a canvas on which its landmarks meet a template's.  Host numpy; the warp is op.warp_affine, on the
host or on the device according to the picture it is given.

    LandmarksReader(file).detect(path)            the landmarks [L, 2] a text file lists for a picture, or None
    solve_affine(src, dst)                        least-squares 2-D similarity src -> dst, 2x3
    solve_ortho(src3d, dst2d)                     scaled orthographic fit, 3x4
    pose_from_landmarks(pts, lmk, size_hw)        that fit as the fitting loop's pose [7] (inversion.LatentInverter)
    scale_landmarks(lmk, src_hw, dst_hw)          pixel indices of a picture -> of its resized copy
    euler_mat_inv(R, type)                        Euler angles of a rotation matrix
    alignment_matrix(template, lmk, canvas_hw)    3x3 T: canvas index coordinates -> picture index coordinates
    template_from_bfm(mat_or_dict, n)             the 3-D template: the model's landmark vertices on its mean shape
    align(img, lmk, template, canvas, border)     (the canvas image, T)
    Aligner(reader, template, canvas, border)     what align_faces and prepare_data --align share

Not reproduced from the reference:
  * the solvers' `max_iter > 0` refinements (scipy leastsq).  solve_ortho's needs cv2.Rodrigues, and unpacks its
    (R, jacobian) pair from the R alone; solve_affine's runs the optimiser and then writes the STARTING point x0 back
    instead of the result x, and ends with `T[:2, :] = x0[2:4]`, which overwrites both rows of the matrix with the
    translation.  Only the closed forms (max_iter = 0, the default the reference's own tool uses) exist here.
  * a token that is empty (two spaces in a row) makes the reference's reader raise IndexError; here it is skipped.
  * the dlib / external-program / PFLD landmark detectors, grabcut and network skin segmentation and the recognition
    feature: their libraries and weights are not part of this package.  Landmarks come from a file.
"""
import os

import numpy as np

from .op import warp

NAME_EXTS = (".png", ".jpg", ".bmp")


class LandmarksReader:
    """A text file with one picture per line: tokens separated by single spaces; a token whose last character is a digit
    is a number, the first token of more than four characters ending in .png / .jpg / .bmp (any case) is the picture's
    name; lines without a name are dropped.  `names` is sorted, `data` [P, 2 L] follows it."""

    def __init__(self, file_name):
        with open(file_name, "r") as f:
            lines = [ln for ln in f.read().splitlines() if ln]
        names, rows = [], []
        for ln in lines:
            tokens = [t for t in ln.split(" ") if t]
            found = [t for t in tokens if len(t) > 4 and t[-4:].lower() in NAME_EXTS]
            if not found:
                continue
            names.append(found[0])
            rows.append([float(t) for t in tokens if "0" <= t[-1] <= "9"])
        order = np.argsort(names, kind="stable") if names else []
        self.names = [names[i] for i in order]
        self.data = np.array([rows[i] for i in order], np.float64)

    def __len__(self):
        return len(self.names)

    def detect(self, img_name):
        """[L, 2] of the first name (in sorted order) that `img_name` ends with, or None."""
        for i, name in enumerate(self.names):
            if img_name.endswith(name):
                return self.data[i].reshape(-1, 2)
        return None


def _pinv_apply(a, b, eps):
    """pinv(a) b through the SVD; singular values <= eps are not inverted (kept as they are, like the reference)."""
    u, w, vt = np.linalg.svd(a, full_matrices=False)
    w_inv = np.where(w > eps, 1.0 / np.where(w > eps, w, 1.0), w)
    return vt.T.dot((u.T.dot(b).T * w_inv).T)


def solve_affine(src, dst, eps=1e-9):
    """Least-squares similarity (rotation, uniform scale, translation) with dst ~ A src + t, as [[a, -b, tx],
    [b, a, ty]].  src, dst [n, 2]."""
    src = np.asarray(src, np.float64)[:, :2]
    dst = np.asarray(dst, np.float64)[:, :2]
    n = len(src)
    J = np.zeros((2 * n, 4), np.float64)
    J[0::2, 0], J[0::2, 1], J[0::2, 2] = src[:, 0], -src[:, 1], 1.0
    J[1::2, 0], J[1::2, 1], J[1::2, 3] = src[:, 1], src[:, 0], 1.0
    a, b, tx, ty = _pinv_apply(J, dst.reshape(-1), eps)
    return np.array([[a, -b, tx], [b, a, ty]], np.float64)


def solve_ortho(src, dst, eps=1e-9, weights=None):
    """Scaled orthographic fit dst ~ w (R src)[:2] + t of src [n, 3] to dst [n, 2]: the least-squares 3x2 linear map of
    the centred points, its nearest scaled rotation (SVD, completed to det +1), and the translation that maps mean to
    mean.  Returns the reference's 3x4 layout: [:3, :3] = w R, [:2, 3] = t, [2, 3] = 1 / max(w, eps).  `weights` [n]
    >= 0 (not in the reference) makes the means and the least squares weighted; a point of weight 0 does not count."""
    src = np.asarray(src, np.float64)
    dst = np.asarray(dst, np.float64)
    if weights is None:
        src_mean, dst_mean = src.mean(0), dst.mean(0)
        M = _pinv_apply(src - src_mean, dst - dst_mean, eps)        # [3, 2]: dst_ ~ src_ M
    else:
        wt = np.asarray(weights, np.float64).reshape(-1, 1)
        src_mean, dst_mean = (wt * src).sum(0) / wt.sum(), (wt * dst).sum(0) / wt.sum()
        M = _pinv_apply(np.sqrt(wt) * (src - src_mean), np.sqrt(wt) * (dst - dst_mean), eps)
    u, _, vt = np.linalg.svd(M)
    v3 = np.eye(3)
    v3[:2, :2] = vt
    if np.linalg.det(v3) * np.linalg.det(u) < 0:
        v3[2, 2] = -1.0
    Rt = u.dot(v3)                                                   # R transposed: columns are R's rows
    w = (M * Rt[:, :2]).sum() / (Rt[:, :2] * Rt[:, :2]).sum()
    T = np.zeros((3, 4), np.float64)
    T[:, :3] = (w * Rt).T
    T[:2, 3] = dst_mean - src_mean.dot(w * Rt[:, :2])
    T[2, 3] = 1.0 / max(w, eps)
    return T


def euler_mat_inv(R, type="yxz", eps=1e-9):
    """Euler angles [3] of rotation matrix R for an axis order such as 'yxz' (three distinct axes) or 'zxz' (first =
    last), with the reference's sign conventions and its handling of the two degenerate poses."""
    R = np.asarray(R)
    ax = [ord(t) - ord("x") for t in type.lower()]
    sign = 2 * ((ax[0] - ax[1]) % 3) - 3
    proper = ax[0] == ax[2] and ax[0] != ax[1]
    if proper:
        i, j = ax[0], ax[1]
        k = 3 - i - j
        D = max(min(R[i, i], 1), -1)
        r = np.array([np.arctan2(R[i, j], sign * R[i, k]), np.arccos(D), np.arctan2(R[j, i], -sign * R[k, i])], R.dtype)
    elif set(ax) <= {0, 1, 2}:
        i, j, k = ax
        D = max(min(R[k, i], 1), -1)
        r = np.array([np.arctan2(sign * R[k, j], R[k, k]), np.arcsin(-sign * D), np.arctan2(sign * R[j, i], R[i, i])])
    else:
        return np.zeros(3, R.dtype)
    if 1 - D <= eps:
        r[2] = np.arctan2(-sign * R[j, k], R[j, j]) - r[0]
    elif 1 + D <= eps:
        r[2] = np.arctan2(sign * R[j, k], R[j, j]) + r[0]
    return r


def pose_from_landmarks(model_pts, lmk, size_hw, weights=None):
    """pose [7] = (yaw, pitch, roll, tx, ty, 0, log-scale), float64, of inversion.LatentInverter's convention
    v = v0 @ (e^s R_yxz) + t, under which the model's landmark points model_pts [L, 3] (on its mean shape) project onto
    the landmarks lmk [L, 2], given in pixel index coordinates of an (H, W) = size_hw picture.  The rasterizer's
    projection x = (1 + v.x) W / 2 - 1/2, y = (1 - v.y) H / 2 - 1/2 (y flipped) is undone first, then solve_ortho's
    closed form gives the scaled rotation and the translation and euler_mat_inv the angles; no iteration.  weights [L]
    >= 0: the weighted fit (0: the landmark is missing)."""
    h, w = _hw(size_hw)
    pts = np.asarray(model_pts, np.float64)
    lmk = np.asarray(lmk, np.float64)
    if pts.ndim != 2 or pts.shape[1] != 3 or lmk.shape != (len(pts), 2):
        raise ValueError("align: model points %s and landmarks %s do not pair up" % (pts.shape, lmk.shape))
    if weights is not None:
        weights = np.asarray(weights, np.float64).reshape(-1)
        if weights.shape != (len(pts),) or (weights < 0).any() or not weights.sum() > 0:
            raise ValueError("align: weights must be [L], not negative and not all zero")
    ndc = np.stack(((lmk[:, 0] + 0.5) * 2 / w - 1, 1 - (lmk[:, 1] + 0.5) * 2 / h), 1)
    T = solve_ortho(pts, ndc, weights=weights)
    scale = 1.0 / T[2, 3]
    # ndc ~ pts @ M[:, :2] + t with M = T[:3, :3].T = e^s R
    angles = euler_mat_inv(T[:3, :3].T / scale, "yxz")
    return np.array([angles[0], angles[1], angles[2], T[0, 3], T[1, 3], 0.0, np.log(scale)], np.float64)


def pose_from_landmarks_contour(v_mean, embedding, lines, axis, lmk, size_hw, weights=None):
    """pose_from_landmarks for landmarks whose jaw line follows the silhouette: two passes, no iteration to convergence.
    Pass 1 is pose_from_landmarks on the embedding's static points of the mean shape v_mean [nv, 3].  The mean shape is
    then posed with that result, every contour line of `lines` selects its vertex by op.landmark's rule (the candidate
    furthest out across the face, `axis` = (i_up, i_down)), and pass 2 solves again with the selected vertices in place of
    the static jaw points.  Returns (pose [7] float64, sel int64 [C] the selected vertices).  Host float64."""
    import torch

    from .op.landmark import check_lines, contour_select, landmark_points
    from .utils_3d import euler_mat

    v = torch.from_numpy(np.asarray(v_mean, np.float64).reshape(1, -1, 3))
    idx, bary = (torch.as_tensor(t) for t in embedding)
    pts = landmark_points(v, idx, bary.double())[0].numpy()
    first = pose_from_landmarks(pts, lmk, size_hw, weights)
    tables = check_lines(lines, len(pts), v.shape[1])
    if len(tables[0]) == 0:
        return first, np.zeros(0, np.int64)
    p = torch.from_numpy(first)
    posed = v @ (torch.exp(p[6]) * euler_mat(p[:3], "yxz")) + p[3:6]
    sel = contour_select(posed, tables, (int(axis[0]), int(axis[1])))[1][0].numpy()
    pts2 = pts.copy()
    pts2[tables[0]] = v[0].numpy()[sel]
    return pose_from_landmarks(pts2, lmk, size_hw, weights), sel


def scale_landmarks(lmk, src_hw, dst_hw):
    """Pixel index coordinates [..., 2] of a picture of (H, W) = src_hw -> of the same picture resized to dst_hw:
    x' = (x + 1/2) W' / W - 1/2 (pixel centres, as the resize of reconstruct.load_image places them)."""
    (h0, w0), (h1, w1) = _hw(src_hw), _hw(dst_hw)
    lmk = np.asarray(lmk, np.float64)
    return np.stack(((lmk[..., 0] + 0.5) * w1 / w0 - 0.5, (lmk[..., 1] + 0.5) * h1 / h0 - 0.5), -1)


def _hw(canvas):
    if isinstance(canvas, (tuple, list)):
        h, w = canvas
        return int(h), int(w)
    return int(canvas), int(canvas)


def alignment_matrix(template, lmk, canvas_hw):
    """3x3 T from canvas index coordinates to picture index coordinates, so that the template lands on `lmk` [L, 2].
    template [L, 2]: pixels of the canvas; T is solve_affine(template, lmk).  template [L, 3]: model coordinates in
    [-1, 1], y up, projected to the canvas by x = (1 + x) W / 2, y = (1 - y) H / 2, z = -z (W + H) / 4; of
    solve_ortho's pose only the scale cbrt(det), the in-plane ('yxz') roll and the translation are kept: yaw and pitch
    stay in the picture."""
    template = np.asarray(template, np.float64)
    lmk = np.asarray(lmk, np.float64)
    if template.ndim != 2 or template.shape[1] not in (2, 3) or lmk.shape != (len(template), 2):
        raise ValueError("align: template %s and landmarks %s do not pair up" % (template.shape, lmk.shape))
    if template.shape[1] == 2:
        return np.concatenate((solve_affine(template, lmk), [[0.0, 0.0, 1.0]]), 0)
    h, w = _hw(canvas_hw)
    base = np.stack(((1 + template[:, 0]) * w / 2, (1 - template[:, 1]) * h / 2, -template[:, 2] * (w + h) / 4), 1)
    P = solve_ortho(base, lmk)
    f = np.cbrt(np.linalg.det(P[:3, :3]))
    roll = euler_mat_inv(P[:3, :3] / f, "yxz")[2]
    c, s = f * np.cos(roll), f * np.sin(roll)
    return np.array([[c, -s, P[0, 3]], [s, c, P[1, 3]], [0.0, 0.0, 1.0]], np.float64)


def template_from_bfm(mat_or_dict, n=68):
    """[n, 3] template of a Basel-Face-Model .mat (a path, or the loaded dict): the vertices its `landmarks<n>` entry
    names (indices based like `tri`: tri.min() is subtracted) on the centred, 1e-5-scaled mean shape."""
    if isinstance(mat_or_dict, (str, os.PathLike)):
        import scipy.io as sio

        data = sio.loadmat(mat_or_dict)
    else:
        data = mat_or_dict
    key = "landmarks%d" % n
    if key not in data.keys():
        raise KeyError("align: the face model has no '%s' entry.  The reference then renders the mean face and runs a "
                       "landmark detector on the rendering; no detector exists in this package, so the model file must "
                       "name its landmark vertices (or pass a 2-D --template instead)" % key)
    v = (np.asarray(data["v"], np.float64) - np.asarray(data["v"], np.float64).mean(1).reshape(-1, 1)).T * 1e-5
    tri = np.asarray(data["tri"][0, 0]).astype(np.int64)
    idx = np.asarray(data[key]).reshape(-1).astype(np.int64) - tri.min()
    return v[idx]


def align(img, lmk, template, canvas, border="reflect"):
    """uint8 [H, W, C] picture (array: host, device tensor: kernel) with landmarks lmk [L, 2] -> (the canvas = (h, w)
    image on which the landmarks sit on the template, T of alignment_matrix)."""
    h, w = _hw(canvas)
    T = alignment_matrix(template, lmk, (h, w))
    return warp.warp_affine(img, warp.from_index_transform(T), (h, w), border), T


def read_template(file_name):
    """A one-row landmark file -> [L, 2] (pixels of the canvas it was made for)."""
    reader = LandmarksReader(file_name)
    if len(reader) != 1:
        raise ValueError("align: a template file holds one row of landmarks, %s has %d" % (file_name, len(reader)))
    return reader.data[0].reshape(-1, 2)


class Aligner:
    """Template, canvas and border of one run.  template None: the landmarks of the first readable picture of `files`
    that has any, on a canvas of that picture's shape (the reference's `base_img = img`).  canvas None with a template:
    that picture's shape as well."""

    def __init__(self, reader, template=None, canvas=None, border="reflect", files=(), read_image=None):
        self.reader, self.border = reader, border
        if border not in warp.BORDERS:
            raise ValueError("align: border must be one of %s" % ", ".join(warp.BORDERS))
        if template is None or canvas is None:
            first = None
            for f in files:
                lmk = reader.detect(f)
                img = read_image(f) if lmk is not None else None
                if img is not None:
                    first = (lmk, img.shape[:2])
                    break
            if first is None:
                raise ValueError("align: no readable picture with landmarks to take the %s from" %
                                 ("template" if template is None else "canvas"))
            if template is None:
                template = first[0]
            canvas = first[1] if canvas is None else canvas
        self.template = np.asarray(template, np.float64)
        self.canvas = _hw(canvas)

    def has(self, path):
        return self.reader.detect(path) is not None

    def matrix(self, path):
        """The op.warp_affine matrix of a picture, or None when the file lists no landmarks for it."""
        lmk = self.reader.detect(path)
        if lmk is None:
            return None
        return warp.from_index_transform(alignment_matrix(self.template, lmk, self.canvas))


def add_arguments(ap, size_flag):
    """The template / border flags align_faces and prepare_data share."""
    ap.add_argument("--bfm", type=str, default="", help="Basel Face Model .mat with a landmarks68 entry: the 3-D template")
    ap.add_argument("--template", type=str, default="", help="one-row landmark file in pixels of the S x S canvas")
    ap.add_argument(size_flag, type=int, default=0, help="side S of the square canvas")
    ap.add_argument("--border", type=str, default="reflect", choices=sorted(warp.BORDERS))


def aligner_from_args(lmk_file, bfm, template, size, border, files, read_image):
    for word, what in (("dlib", "the dlib library and its shape predictor"), ("exe", "the external tracking program"),
                       ("torch", "the PFLD detector's weights")):
        if not os.path.exists(lmk_file) and word in lmk_file.lower():
            raise SystemExit("align: --lmk %s needs %s, which this package does not have; pass a landmark .txt file"
                             % (lmk_file, what))
    if not os.path.isfile(lmk_file):
        raise SystemExit("align: landmark file %s not found" % lmk_file)
    if bfm and template:
        raise SystemExit("align: --bfm and --template exclude each other")
    reader = LandmarksReader(lmk_file)
    tpl = None
    if bfm:
        tpl = template_from_bfm(bfm, reader.data.shape[1] // 2 if len(reader) else 68)
    elif template:
        if size <= 0:
            raise SystemExit("align: --template needs the canvas size it was made for")
        tpl = read_template(template)
    return Aligner(reader, tpl, size if size > 0 else None, border, files, read_image)
