"""Cases of tests/golden/fid_*.npz (written by tests/make_golden_fid.py from the reference's inception.py and fid.py),
shared by the fixture writer and the tests: every input is a pure function of integer keys (synth.det_*), so the GPU
machine rebuilds the reference's inputs without storing them."""
import numpy as np

from stylerenderer_amd import synth

# name -> (batch, size, key): 299^2 is fed as is, 256^2 is resized down, 64^2 up
NET_CASES = {"s299": (2, 299, 9501), "s256": (2, 256, 9502), "s64": (3, 64, 9503)}

# calc_fid cases: name -> (n_sample, n_real, dim, key).  n > dim gives full-rank covariances; n < dim a singular one
FID_CASES = {"full": (2100, 2200, 2048, 9601), "singular": (1000, 2200, 2048, 9602)}


def images(name):
    """Smooth images in [-1, 1]: a few low-frequency waves per channel plus a little det_normal texture."""
    b, s, key = NET_CASES[name]
    y, x = np.meshgrid(np.linspace(-1, 1, s), np.linspace(-1, 1, s), indexing="ij")
    ph = synth.det_uniform((b, 3, 3), key) * 3.0
    img = np.zeros((b, 3, s, s), np.float64)
    for i in range(b):
        for c in range(3):
            img[i, c] = np.sin(ph[i, c, 0] * 3 * x + ph[i, c, 1] * 2 * y + ph[i, c, 2])
    img += 0.1 * synth.det_normal((b, 3, s, s), key + 1)
    return np.clip(img, -1, 1).astype(np.float32)


def features(n, d, key, offset=0.0):
    """ReLU-like float32 features [n, d] with a per-dimension scale, the shape of pooled Inception features."""
    z = synth.det_normal((n, d), key)
    scale = 0.5 + np.abs(synth.det_normal((d,), key + 1))
    return (np.abs(z + offset) * scale).astype(np.float32)


def fid_inputs(name):
    """(sample features, real features) of a calc_fid case."""
    n, n_real, d, key = FID_CASES[name]
    return features(n, d, key), features(n_real, d, key + 10, offset=0.3)


def stats(f):
    f = f.astype(np.float64)
    return f.mean(0), np.cov(f, rowvar=False)
