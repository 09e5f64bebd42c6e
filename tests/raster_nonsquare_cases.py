"""Shared inputs and references of the rasterizer's non-square tests (tests/test_rasterize_nonsquare_cpu.py,
tests/test_rasterize_nonsquare_gpu.py, test_ops_gpu.test_rasterize_ab_switches_change_no_bit, tests/poison_cases.py).

The rasterizer keeps the reference's swapped call convention: on an h x w image x spans h columns and y
spans w rows, and sample (x, y) lands on buffer entry x + y w.
  * h > w: a sample with x >= w lands on pixel (x - w, y + 1) — one row further down, up to ceil(h / w) - 1 rows deep —
    so several samples of one triangle may share a pixel.  The sequential sweep keeps the largest depth; between
    triangles the earlier one wins a tie (`zB < z` is strict), within a triangle the sample earlier in box order
    (smaller y, i.e. the aliased one).
  * w > h: samples with x + y w >= h w are dropped.
The reference of every test is the C oracle (oracle/rasterize_oracle_impl.h) through oracle/raster.py; this module
computes it once per case (`case`, cached) and nothing here reads a device result.

The per-element gradient measure.  Element i of a gradient is a sum of per-pixel terms; with
  S_i (grad_v)   = sum over the pixels and weights that contribute to i of  sum_ch |grad_out tex| * |dcoeff|,
  S_i (grad_tex) = sum over those pixels of |grad_out| * |coeff|                                   (float64)
a result passes when |got_i - want_i| <= tol * S_i for every i.  (With perspective and h > w the own-pixel Jacobian of
an aliased sample is evaluated outside its triangle and reaches 1e6: "relative to the largest element" would accept
almost anything there.)  tol is measured from the reference alone (`accumulation_error`): the oracle's fp32 per-pixel
terms summed in float32 in pixel order against the same terms summed in float64, the largest difference in units of S_i
over all CASES of both meshes, both projections and c = 3, 6; tol = 4 x that — the margin for another fixed summation
order and the analytically collapsed orthographic Jacobian of the kernels.  tests/test_rasterize_nonsquare_cpu.py
re-measures and holds MEASURED_F32 to it.  fp64 runs the same operations at double precision, so its bound is the fp32
one scaled by the ratio of the unit roundoffs, 2^-29.
"""
import functools

import numpy as np

import raster

TALL = [(20, 12), (33, 17), (40, 12)]         # h > w: aliasing one, one and three rows deep
WIDE = [(12, 20), (12, 40)]                   # w > h: dropped rows
DEGENERATE = [(16, 1), (1, 16)]
SIZES = TALL + WIDE + DEGENERATE
MESHES = ["ab", "flat"]
CHANNELS = [3, 6]

# accumulation_error() over SIZES x {orthographic, perspective} x MESHES x CHANNELS (float32), largest value: measured on
# the reference alone (grad_tex 1.79e-7, grad_v 4.23e-8, both at 40 x 12, perspective, ab, c = 6), rounded up
MEASURED_F32 = 1.8e-7
TOL_F32 = 4 * MEASURED_F32
TOL_F64 = TOL_F32 * 2.0 ** -29
EPS = 1e-6


def ab_mesh(h, w, persp, on_image=True):
    """(v [2, nv, 3], tri [nf, 3]): a closed fan of 32 triangles around one vertex (valence 32 > 24: the wave-summed
    branch of the vertex gather), a 6 x 6 grid of cells of two small triangles each, and one screen-filling triangle
    (bounding box > 64 pixels: k_grad_big) whose depth crosses the other two parts.  Every z is negative (perspective
    accepts it); the second sample is the first one shrunk, shifted and tilted in depth.

    The mesh is laid out on x = -1 .. 1, which on an h x w image spans h columns.  on_image=True maps it, when
    h > w, onto the w columns the image has, x -> (x + 1) w / h - 1: no sample aliases into a later row.  on_image=False
    leaves it where it is: with h > w the geometry right of column w aliases, with w > h rows are dropped.  For the
    perspective projection x and y are then multiplied by -z: the division brings the same layout to the screen."""
    ang = 2.0 * np.pi * np.arange(32) / 32
    fan = [(-0.45, 0.40, -0.70)] + [(-0.45 + 0.25 * np.cos(a), 0.40 + 0.25 * np.sin(a), -0.72 + 0.05 * np.sin(3 * a))
                                    for a in ang]
    tri = [(0, 1 + k, 1 + (k + 1) % 32) for k in range(32)]
    g0 = len(fan)
    grid = [(0.10 + 0.1 * i, -0.70 + 0.1 * j, -0.70 + 0.02 * ((3 * i + 5 * j) % 7)) for j in range(7) for i in range(7)]
    for j in range(6):
        for i in range(6):
            a = g0 + 7 * j + i
            tri += [(a, a + 1, a + 8), (a, a + 8, a + 7)]
    b0 = g0 + len(grid)
    big = [(-0.95, -0.90, -0.90), (0.95, -0.90, -0.55), (0.0, 0.95, -0.75)]
    tri.append((b0, b0 + 1, b0 + 2))
    v0 = np.array(fan + grid + big, np.float32)
    v1 = v0 * np.array([0.9, 0.85, 1.0], np.float32) + np.array([0.06, -0.04, 0.0], np.float32)
    v1[:, 2] += 0.1 * v0[:, 0]
    v = np.stack([v0, v1])
    if on_image and h > w:
        v[..., 0] = (v[..., 0] + 1) * np.float32(w / h) - 1
    if persp:
        v[..., :2] *= -v[..., 2:]
    return v, np.array(tri, np.int64)


AB_HUB, AB_GRID0, AB_BIG0 = 0, 33, 33 + 49       # first vertex of the fan's hub, the grid and the large triangle


def flat_mesh(persp):
    """(v [2, 6, 3], tri [2, 2, 3]): two overlapping triangles wider than the screen, every vertex at z = -0.5, so every
    sample of both has the same depth up to the rounding of its weights' sum (exactly -0.5 wherever that sum rounds to
    1: most samples).  Sample 0 lists the triangle of vertices 0-2 first, sample 1 lists it second: between triangles
    the one listed earlier wins a tie, within a triangle the sample earlier in box order does."""
    a = [(-1.30, -1.20, -0.5), (1.40, -1.10, -0.5), (-0.20, 1.50, -0.5)]
    b = [(-1.40, 1.10, -0.5), (-0.90, -1.30, -0.5), (1.50, 0.40, -0.5)]
    v0 = np.array(a + b, np.float32)
    v = np.stack([v0, v0])
    if persp:
        v[..., :2] *= -v[..., 2:]
    tri = np.array([[(0, 1, 2), (3, 4, 5)], [(3, 4, 5), (0, 1, 2)]], np.int64)
    return v, tri


def mesh(name, h, w, persp):
    return ab_mesh(h, w, persp, on_image=False) if name == "ab" else flat_mesh(persp)


def det_normal(shape, seed):
    from stylerenderer_amd import synth

    return synth.det_normal(shape, seed)


class Case:
    """Inputs (float32; `.astype(np.float64)` gives the fp64 run's) and the oracle's results of one (size, projection,
    mesh, channel count)."""

    def __init__(self, h, w, persp, name, c):
        self.h, self.w, self.persp, self.name, self.c = h, w, persp, name, c
        self.v, self.tri = mesh(name, h, w, persp)
        self.tex = det_normal((2, self.v.shape[1], c), 91)
        self.go = det_normal((2, h, w, c), 92)

    @functools.lru_cache(maxsize=None)
    def oracle(self, dtype=np.float32):
        """dict: index, coeff, zbuf, attr, dcoeff, grad_v, grad_tex (float64-accumulated, rounded once), s_v, s_tex."""
        v, tex, go = self.v.astype(dtype), self.tex.astype(dtype), self.go.astype(dtype)
        index, coeff, zbuf = raster.forward_buffers(v, self.tri, self.h, self.w, self.persp, EPS)
        dcoeff = raster.backward_dcoeff(v, index, self.persp, EPS)
        grad_v, grad_tex = raster.rasterize_grads(v, tex, self.tri, go, self.h, self.w, self.persp, EPS)
        s_v, s_tex = scales(index, coeff, dcoeff, tex, go)
        out = dict(index=index, coeff=coeff, zbuf=zbuf, attr=raster.rasterize(v, tex, self.tri, self.h, self.w, self.persp, EPS),
                   dcoeff=dcoeff, grad_v=grad_v, grad_tex=grad_tex, s_v=s_v, s_tex=s_tex)
        for a in out.values():
            a.setflags(write=False)
        return out


@functools.lru_cache(maxsize=None)
def case(h, w, persp, name, c):
    return Case(h, w, persp, name, c)


def _terms(index, coeff, dcoeff, tex, go, dtype):
    """Per-pixel terms in `dtype`: (rows [npix * 3], vertex terms [npix * 3, 3], attribute terms [npix * 3, c])."""
    c = tex.shape[-1]
    flat = np.ascontiguousarray(tex).reshape(-1, c).astype(dtype)
    g = go.astype(dtype)
    taken = flat[index.reshape(-1)].reshape(index.shape + (c,))
    dl_dw = (g[..., None, :] * taken).sum(-1, dtype=dtype)
    per_vert = np.einsum("...i,...ij->...j", dl_dw, dcoeff.astype(dtype)).astype(dtype)
    per_tex = g[..., None, :] * coeff[..., None].astype(dtype)
    return index.reshape(-1), per_vert.reshape(-1, 3), per_tex.reshape(-1, c)


def scales(index, coeff, dcoeff, tex, go):
    """(S of grad_v [b, nv, 3], S of grad_tex [b, nv, c]) in float64 — module docstring."""
    c = tex.shape[-1]
    flat = np.ascontiguousarray(tex).reshape(-1, c).astype(np.float64)
    g = np.abs(go.astype(np.float64))
    taken = np.abs(flat[index.reshape(-1)].reshape(index.shape + (c,)))
    dl_dw = (g[..., None, :] * taken).sum(-1)
    per_vert = np.einsum("...i,...ij->...j", dl_dw, np.abs(dcoeff.astype(np.float64)))
    s_v = np.zeros((flat.shape[0], 3))
    np.add.at(s_v, index.reshape(-1), per_vert.reshape(-1, 3))
    s_tex = np.zeros((flat.shape[0], c))
    np.add.at(s_tex, index.reshape(-1), (g[..., None, :] * np.abs(coeff[..., None].astype(np.float64))).reshape(-1, c))
    return s_v.reshape(tex.shape[:-1] + (3,)), s_tex.reshape(tex.shape)


def accumulation_error(cs):
    """(grad_v, grad_tex): the oracle's float32 per-pixel terms of case `cs` summed in float32 in pixel order against the
    same terms summed in float64, largest difference in units of S_i."""
    o = cs.oracle()
    rows, tv, tt = _terms(o["index"], o["coeff"], o["dcoeff"], cs.tex, cs.go, np.float32)
    worst = []
    for terms, s in ((tv, o["s_v"]), (tt, o["s_tex"])):
        n = s.reshape(-1, terms.shape[1]).shape[0]
        lo = np.zeros((n, terms.shape[1]), np.float32)
        hi = np.zeros((n, terms.shape[1]), np.float64)
        np.add.at(lo, rows, terms)                          # unbuffered: one float32 addition per term, in pixel order
        np.add.at(hi, rows, terms.astype(np.float64))
        worst.append(in_units(lo, hi, s.reshape(n, -1)))
    return tuple(worst)


def in_units(got, want, s):
    """max_i |got_i - want_i| / S_i; an element nothing contributes to (S_i = 0) must be equal."""
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64)).reshape(-1)
    s = s.reshape(-1)
    if (diff[s == 0] != 0).any():
        return np.inf
    return float((diff[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0


def all_cases():
    return [(h, w, persp, name, c) for h, w in SIZES for persp in (False, True) for name in MESHES for c in CHANNELS]


def case_id(p):
    h, w, persp, name, c = p
    return "%dx%d-%s-%s-c%d" % (h, w, "persp" if persp else "ortho", name, c)
