"""Inputs of the skinning fixtures (tests/golden/flame_skin.npz), rebuilt from fixed keys by the generator
(make_golden_flame.py) and by the tests alike: nothing but the results is stored."""
import numpy as np

from stylerenderer_amd import synth

REG_WEIGHT = 0.01
NJ = 5                                            # FLAME's tree: root, neck, then jaw and the two eyeballs on the neck
CASES = {
    # name: (mesh, shape dims, batch, stored vertex sample or None = all, root mark of kintree_table)
    "small": ("ellipsoid", 40, 3, None, -1),
    "face": ("face", 48, 1, 1024, 2 ** 32 - 1),
}
RODRIGUES_VECTORS = np.array([[0.0, 0.0, 0.0], [1e-9, 0.0, 0.0], [6e-10, -5e-10, 4e-10], [0.3, -0.2, 0.1],
                              [-1.1, 0.4, 0.9], [0.0, 2.5, 0.0], [1e-3, 2e-3, -1e-3]], np.float64)


def mesh(kind):
    return synth.uv_ellipsoid(16, 14) if kind == "ellipsoid" else synth.face_sized_mesh()


def kintree(root):
    kt = np.array([[0, 0, 1, 1, 1], [0, 1, 2, 3, 4]], np.int64)
    kt[0, 0] = root
    return kt.astype(np.uint32) if root > 0 else kt


def flame_dict(name):
    """A FLAME-shaped dict (the keys and layouts of the licensed file) on a synthetic mesh."""
    kind, ds, _, _, root = CASES[name]
    v0, tri = mesh(kind)
    nv = v0.shape[0]
    key = 7500 + 50 * list(CASES).index(name)
    size = float(np.abs(v0).max())
    shapedirs = (0.02 * size / np.sqrt(ds) * synth.det_uniform((nv, 3, ds), key + 1)).astype(np.float64)
    posedirs = (0.01 * size * synth.det_uniform((nv, 3, 9 * (NJ - 1)), key + 2)).astype(np.float64)
    jr = np.abs(synth.det_uniform((NJ, nv), key + 3)).astype(np.float64) ** 8          # a few vertices dominate a joint
    jr = jr / jr.sum(1, keepdims=True)
    weights = np.abs(synth.det_uniform((nv, NJ), key + 4)).astype(np.float64)          # normalised by the constructor
    return {"v_template": v0.astype(np.float64), "shapedirs": shapedirs, "posedirs": posedirs, "J_regressor": jr,
            "kintree_table": kintree(root), "weights": weights, "f": (tri + 1).astype(np.uint32)}


def case(name):
    """(dict, tri [nf,3], coeff [B, ds + 12], pose [B,7], gv [B,nv,3], gn [B,nv,3], vertex sample index); float32 values
    as float64 where they are coefficients."""
    kind, ds, b, ns, _ = CASES[name]
    d = flame_dict(name)
    nv = d["v_template"].shape[0]
    key = 7500 + 50 * list(CASES).index(name)
    beta = synth.det_normal((b, ds), key + 5)
    theta = synth.det_normal((b, 3 * (NJ - 1)), key + 6) * 0.25
    if b > 1:
        theta[1, 3:6] = 0.0                       # an exactly zero joint rotation: the series branch of rodrigues
    coeff = np.concatenate([beta, theta], 1).astype(np.float32)
    pose = (synth.det_normal((b, 7), key + 7) * np.array([0.4, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1], np.float32)).astype(np.float32)
    gv = synth.det_normal((b, nv, 3), key + 8)
    gn = synth.det_normal((b, nv, 3), key + 9)
    idx = np.arange(nv) if ns is None else synth.sample_index(nv, ns)
    tri = (d["f"].astype(np.int64) - 1)
    return d, tri, coeff, pose, gv, gn, idx


def block_errors(got, want, ds):
    """Relative errors of a coefficient gradient [B, ds + 3 np] per block, each against its own magnitude: the shape block,
    and the largest of the joints' (max |diff| / max |want| over a joint's three angles, all samples).  One max-norm over
    the whole vector would let FLAME's eye-roll prior (sigma 1e-5 degrees: entries ~1e11) hide every other entry."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)

    def rel(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))

    joints = [rel(got[:, k:k + 3], want[:, k:k + 3]) for k in range(ds, want.shape[1], 3)]
    return {"beta": rel(got[:, :ds], want[:, :ds]), "theta": max(joints)}


def elementwise_error(got, want):
    """Largest |got - want| / |want| over the entries with want != 0; entries with want == 0 must be exactly 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    if np.any(got[zero] != 0):
        return float("inf")
    return float((np.abs(got - want)[~zero] / np.abs(want)[~zero]).max())
