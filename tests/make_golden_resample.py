"""Writes tests/golden/resample.npz: what Pillow's resampler gives on seeded inputs (run by hand: python
tests/make_golden_resample.py; needs Pillow, nothing of this package).

The inputs are not stored: a test redraws them with golden_input() below's rule, np.random.RandomState(seed).randint
(kind "binary": only 0 and 255, which drives the sums under the negative lobes of bicubic / lanczos below 0 and above
255, into the clip).  Stored per case and filter: the resized uint8 image; for the 1024 x 683 pyramid only a SHA-256 of
the bytes and the top-left 16 x 16 corner.  The archive carries its own table of cases (key "meta", JSON).
"""
import hashlib
import json
import os

import numpy as np

FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")
# name, seed, kind, (h, w, c) -> (oh, ow) [, window (oy0, ox0, oh', ow')]
CASES = [
    dict(name="down", seed=1, kind="random", shape=(131, 97, 3), size=(32, 32)),
    dict(name="up", seed=2, kind="random", shape=(64, 64, 3), size=(96, 128)),
    dict(name="odd", seed=3, kind="random", shape=(200, 300, 3), size=(43, 64)),
    dict(name="skip_h", seed=4, kind="random", shape=(50, 50, 3), size=(20, 50)),
    dict(name="skip_v", seed=5, kind="random", shape=(50, 50, 3), size=(50, 20)),
    dict(name="thin", seed=6, kind="random", shape=(40, 1, 3), size=(17, 5)),
    dict(name="gray", seed=7, kind="random", shape=(33, 47, 1), size=(20, 80)),
    dict(name="four", seed=8, kind="random", shape=(20, 30, 4), size=(7, 13)),
    dict(name="binary", seed=9, kind="binary", shape=(45, 60, 3), size=(18, 24)),
    dict(name="binary_up", seed=10, kind="binary", shape=(12, 9, 3), size=(40, 31)),
    # centre crop to 32: 64 x 74 -> 32 x 37, difference 5 -> left = round(2.5) = 2 (half to even)
    dict(name="crop", seed=11, kind="random", shape=(64, 74, 3), size=(32, 37), window=(0, 2, 32, 32)),
]
PYRAMID = dict(name="pyramid", seed=12, kind="random", shape=(683, 1024, 3), sizes=(128, 256, 512))


def golden_input(case):
    rs = np.random.RandomState(case["seed"])
    a = rs.randint(0, 256, size=tuple(case["shape"])).astype(np.uint8)
    if case["kind"] == "binary":
        a = np.where(a > 127, 255, 0).astype(np.uint8)
    return a


def pillow_resize(a, size, name, window=None):
    from PIL import Image

    flt = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC,
           "lanczos": Image.LANCZOS}[name]
    c = a.shape[2]
    # "CMYK" is four plain 8-bit channels (an "RGBA" resize would premultiply alpha around the resampler)
    im = Image.fromarray(a[:, :, 0] if c == 1 else a, {1: "L", 3: "RGB", 4: "CMYK"}[c])
    oh, ow = size
    out = np.asarray(im.resize((ow, oh), flt)).reshape(oh, ow, c)
    if window is not None:
        oy0, ox0, wh, ww = window
        out = out[oy0:oy0 + wh, ox0:ox0 + ww]
    return np.ascontiguousarray(out)


def center_crop_geometry(h, w, size):
    """torchvision resize(size) + center_crop(size)."""
    oh, ow = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
    return (oh, ow), (int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0)), size, size)


def main():
    out = {"meta": np.array(json.dumps({"filters": FILTERS, "cases": CASES, "pyramid": PYRAMID}))}
    for case in CASES:
        a = golden_input(case)
        for f in FILTERS:
            out["%s/%s" % (case["name"], f)] = pillow_resize(a, case["size"], f, case.get("window"))
    a = golden_input(PYRAMID)
    for s in PYRAMID["sizes"]:
        size, window = center_crop_geometry(a.shape[0], a.shape[1], s)
        for f in FILTERS:
            r = pillow_resize(a, size, f, window)
            out["pyramid/%d/%s/sha256" % (s, f)] = np.array(hashlib.sha256(r.tobytes()).hexdigest())
            out["pyramid/%d/%s/corner" % (s, f)] = r[:16, :16].copy()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
