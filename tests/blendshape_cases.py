"""Inputs of the blendshape fixtures (tests/golden/blendshape.npz), rebuilt from fixed keys by the generator
(make_golden_blendshape.py) and by the tests alike: nothing but the results is stored.  numpy only.

The kernels of csrc/blend.hip have one shape-selected path, the four-column load against the single-column tail of a row
(3 nv % 4 in {0, 1, 2, 3}), and sample blocks of 8.  The cases sit on every side:

    name      nv   3nv%4  ds  de   B  beta_shape  what it is there for
    small     40     0     5   3   3     .01      the loader's beta, rows 16-byte aligned
    odd       41     3     4   2   1     1.5      a three-column tail, a proper prior
    two       42     2     3   4   8     2.0      rows 8-byte aligned (FaceWarehouse's own 3 nv % 4), a full sample block
    one       43     1     2   2   9     .01      a one-column tail, B = 9 crosses the sample block
    noid      40     0     0   3   3     1.0      ds = 0: one identity
    noexp     41     3     4   0   3     .01      de = 0: the neutral expression alone
    large     40     0     2   4   3  1.5, 2, 3    coefficients of magnitude up to 30 (the last identity's logit, their
                                                  negated sum, then stays below fp32's exp range in the reference).
                                                  Unequal concentrations: with equal ones the prior's gradient at an
                                                  identity whose weight and the last one's both vanish is the difference
                                                  of two equal numbers, exactly 0 in the reference's own float32 run
                                                  (entry-by-entry error 1), which no float32 bar can hold
    face     mesh    -    12   6   1     1.0      the face-sized mesh (train --mesh's), a vertex sample stored
"""
import numpy as np

from stylerenderer_amd import synth

REG_WEIGHT = 0.01
CASES = {
    # name: (vertices or "face", ds, de, batch, beta_shape, coefficient scale, stored vertex sample or None = all)
    "small": (40, 5, 3, 3, .01, 1.0, None),
    "odd": (41, 4, 2, 1, 1.5, 1.0, None),
    "two": (42, 3, 4, 8, 2.0, 1.0, None),
    "one": (43, 2, 2, 9, .01, 1.0, None),
    "noid": (40, 0, 3, 3, 1.0, 1.0, None),
    "noexp": (41, 4, 0, 3, .01, 1.0, None),
    "large": (40, 2, 4, 3, [1.5, 2.0, 3.0], 30.0, None),
    "face": ("face", 12, 6, 1, 1.0, 1.0, 1024),
}
BETA_FORMS = {"scalar": (.5, [2, 3]), "short": ([.5, 2.0], [2, 3, 4]), "full": ([.5, 1, 2, 3], [1, 2, 3, 4, 5, 6])}
BETA_DIMS = (3, 3)                                # ds, de of the constructor's three beta argument forms


def ring_mesh(nv):
    """nv >= 3 points on a bumpy closed strip and a triangle strip over them (every vertex in a triangle)."""
    t = np.arange(nv, dtype=np.float64)
    v = np.stack([np.cos(0.61 * t) * (1 + 0.1 * np.sin(1.7 * t)), np.sin(0.61 * t), 0.3 * np.cos(0.37 * t) + 0.02 * t], 1)
    tri = np.stack([np.arange(nv - 2), np.arange(1, nv - 1), np.arange(2, nv)], 1)
    return v.astype(np.float32), np.concatenate([tri, [[nv - 1, 0, nv // 2]]]).astype(np.int64)


def mesh(kind):
    if kind == "face":
        v0, tri = synth.face_sized_mesh()
        return v0.astype(np.float32), tri.astype(np.int64)
    return ring_mesh(kind)


def facewarehouse_dict(nv_or_mesh, ds, de, key, tri_rows=False, base=1):
    """A FaceWarehouse-shaped dict: v [3, nv], p [3 nv, de + 1, ds + 1], tri (1-based [nf, 3]; [3, nf] with tri_rows)."""
    v0, tri = nv_or_mesh if isinstance(nv_or_mesh, tuple) else mesh(nv_or_mesh)
    nv = v0.shape[0]
    size = max(float(np.abs(v0).max()), 1e-3)
    p = v0.reshape(-1, 1, 1).astype(np.float64) + 0.1 * size * synth.det_uniform((3 * nv, de + 1, ds + 1), key).astype(np.float64)
    t = (tri + base).astype(np.int32)
    return {"v": np.ascontiguousarray(v0.T.astype(np.float64)), "p": p, "tri": t.T.copy() if tri_rows else t}


def key_of(name):
    return 8800 + 40 * list(CASES).index(name)


def case(name):
    """(dict, tri [nf, 3], beta_shape, coeff [B, ds + de], pose [B, 7], gv [B, nv, 3], gn [B, nv, 3], vertex sample)."""
    kind, ds, de, b, beta_shape, scale, ns = CASES[name]
    key = key_of(name)
    d = facewarehouse_dict(kind, ds, de, key + 1)
    nv = d["v"].shape[1]
    coeff = (scale * synth.det_uniform((b, ds + de), key + 2)).astype(np.float32)
    if scale > 1:
        coeff[0, 0] = scale                        # the extremes themselves
        coeff[1, -1] = -scale
    pose = (synth.det_normal((b, 7), key + 3) * np.array([0.4, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1], np.float32)).astype(np.float32)
    gv = synth.det_normal((b, nv, 3), key + 4)
    gn = synth.det_normal((b, nv, 3), key + 5)
    idx = np.arange(nv) if ns is None else synth.sample_index(nv, ns)
    return d, d["tri"].astype(np.int64) - 1, beta_shape, coeff, pose, gv, gn, idx


def elementwise_error(got, want):
    """Largest |got - want| / |want| over the entries with want != 0; entries with want == 0 must be exactly 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    zero = want == 0
    if np.any(got[zero] != 0):
        return float("inf")
    if zero.all():
        return 0.0
    return float((np.abs(got - want)[~zero] / np.abs(want)[~zero]).max())
