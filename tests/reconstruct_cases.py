"""Inputs of the face-reconstruction fixtures (tests/golden/reconstruct_*.npz / .obj), rebuilt from fixed keys by the
generator (make_golden_reconstruct.py) and by the tests alike: nothing but the results is stored."""
import numpy as np

from stylerenderer_amd import synth

REG_WEIGHT = 0.01
CASES = {
    # name: (mesh, shape dims, expression dims, batch, stored vertex sample or None = all)
    "small": ("ellipsoid", 8, 6, 3, None),
    "face": ("face", 80, 64, 1, 1024),
}


def mesh(kind):
    return synth.uv_ellipsoid(16, 14) if kind == "ellipsoid" else synth.face_sized_mesh()


def case(name):
    """(v0 [nv,3], tri [nf,3], w_shape [ds,3nv], w_exp [de,3nv], coeff [B,d] / sigma, pose [B,7], gv [B,nv,3],
    gn [B,nv,3], vertex sample index) as float64 / int64 arrays.  Coefficients are given in units of sigma (the
    model's defaults: 1 for shape, 0.01 for expression)."""
    kind, ds, de, b, ns = CASES[name]
    v0, tri = mesh(kind)
    nv = v0.shape[0]
    key = 7100 + 50 * list(CASES).index(name)
    # per-vertex bases small against the mesh (a few % of its size at 1 sigma): non-degenerate normals
    wsh = 0.01 / np.sqrt(ds) * synth.det_uniform((ds, 3 * nv), key + 1)
    wex = 1.0 / np.sqrt(de) * synth.det_uniform((de, 3 * nv), key + 2)
    coeff = synth.det_normal((b, ds + de), key + 3)
    pose = synth.det_normal((b, 7), key + 4) * np.array([0.4, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1], np.float32)
    gv = synth.det_normal((b, nv, 3), key + 5)
    gn = synth.det_normal((b, nv, 3), key + 6)
    idx = np.arange(nv) if ns is None else synth.sample_index(nv, ns)
    return v0, tri, wsh, wex, coeff, pose.astype(np.float32), gv, gn, idx


def sigmas(ds, de):
    return np.array([1.0] * ds + [0.01] * de, np.float32)


def obj_inputs():
    """(v [6,3], vt [6,2], vn [6,3], tri [5,3]) of the save_obj fixtures: float32 values as float64."""
    v = synth.det_uniform((6, 3), 7301).astype(np.float64) * 2
    vt = (synth.det_uniform((6, 2), 7302).astype(np.float64) + 1) / 2
    vn = synth.det_uniform((6, 3), 7303).astype(np.float64)
    tri = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [1, 5, 4]], np.int64)
    return v, vt, vn, tri


OBJ_FORMS = ("full", "vt", "vn", "plain")


def obj_args(form):
    v, vt, vn, tri = obj_inputs()
    return {"full": dict(vt=vt, vn=vn), "vt": dict(vt=vt), "vn": dict(vn=vn), "plain": {}}[form], v, tri
