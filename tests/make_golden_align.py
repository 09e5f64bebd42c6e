"""Writes tests/golden/align.npz (run by hand: python tests/make_golden_align.py REFERENCE/utils_face.py; needs Pillow
and the reference's utils_face.py, nothing of this package).

Warp part: what Pillow's Image.transform(size, Image.AFFINE, a, Image.BILINEAR) gives on seeded inputs (redrawn by
golden_input() below, not stored), the mask "sample point inside the source" of every case and its share.  Pillow
defines a value only under that mask (elsewhere it writes 0), so a case compared with Pillow under border = reflect or
replicate must lie mostly inside: the generator asserts share >= 0.5 for those (a condition on the inputs, not a
tolerance).  For the 1024^2 case only a SHA-256 and the top-left 16 x 16 corner are stored.

Solver part: the outputs of the reference's solve_affine, solve_ortho and euler_mat_inv (max_iter = 0) on seeded
68-point sets, and of its LandmarksReader on SAMPLE_TEXT.  The reference file neither parses nor imports as a whole, so
the four definitions are cut out of it by their first and last lines at run time and executed; none of its text is here.
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np


def _centred(A, shape, size, shift=(0.0, 0.0)):
    """Pillow matrix with linear part A that takes the centre of the output to the centre of the source + shift."""
    A = np.asarray(A, np.float64)
    (h, w), (oh, ow) = shape[:2], size
    t = np.array([w / 2.0 + shift[0], h / 2.0 + shift[1]]) - A.dot([ow / 2.0, oh / 2.0])
    return [float(v) for v in (A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1])]


def _rot(deg, s=1.0):
    c, sn = np.cos(np.deg2rad(deg)) * s, np.sin(np.deg2rad(deg)) * s
    return [[c, -sn], [sn, c]]


EVERY = ("constant", "reflect", "replicate")
# name, seed, kind, source (h, w, c), output (oh, ow), matrix, the borders compared with Pillow
CASES = [
    dict(name="shift", seed=21, kind="random", shape=(48, 64, 3), size=(48, 64), borders=EVERY,
         matrix=[1.0, 0.0, 3.37, 0.0, 1.0, -2.81]),
    dict(name="rotate", seed=22, kind="random", shape=(90, 120, 3), size=(60, 60), borders=EVERY,
         matrix=_centred(_rot(17.0), (90, 120), (60, 60), (4.3, -3.1))),
    dict(name="x0.3", seed=23, kind="random", shape=(40, 50, 3), size=(100, 140), borders=EVERY,
         matrix=_centred(_rot(-8.0, 0.3), (40, 50), (100, 140), (0.7, 1.9))),
    dict(name="x2.5", seed=24, kind="random", shape=(200, 300, 3), size=(64, 96), borders=EVERY,
         matrix=_centred(_rot(31.0, 2.5), (200, 300), (64, 96), (-11.5, 7.25))),
    dict(name="general", seed=25, kind="random", shape=(77, 131, 3), size=(45, 83), borders=EVERY,
         matrix=_centred([[1.21, 0.43], [-0.17, 0.78]], (77, 131), (45, 83), (2.6, -1.4))),
    dict(name="gray", seed=26, kind="random", shape=(33, 47, 1), size=(30, 41), borders=EVERY,
         matrix=_centred(_rot(-25.0, 0.8), (33, 47), (30, 41), (1.5, 0.5))),
    dict(name="four", seed=27, kind="random", shape=(20, 30, 4), size=(17, 23), borders=EVERY,
         matrix=_centred(_rot(12.0, 1.1), (20, 30), (17, 23), (-0.9, 0.4))),
    dict(name="thin", seed=28, kind="random", shape=(40, 1, 3), size=(40, 5), borders=EVERY,
         matrix=[0.1, 0.0, 0.2, 0.02, 0.9, 1.0]),
    dict(name="binary", seed=29, kind="binary", shape=(45, 60, 3), size=(50, 52), borders=EVERY,
         matrix=_centred(_rot(40.0, 0.7), (45, 60), (50, 52), (0.25, -0.75))),
    dict(name="odd", seed=30, kind="random", shape=(31, 29, 3), size=(13, 27), borders=EVERY,
         matrix=_centred(_rot(90.0), (31, 29), (13, 27), (0.5, 0.5))),
    # most of the output falls outside the source: Pillow is the yardstick under border = constant only
    dict(name="outside", seed=31, kind="random", shape=(24, 32, 3), size=(64, 80), borders=("constant",),
         matrix=_centred(_rot(-33.0, 1.6), (24, 32), (64, 80), (9.0, -5.0))),
]
BIG = dict(name="big", seed=32, kind="random", shape=(1024, 1024, 3), size=(1024, 1024), borders=EVERY,
           matrix=_centred(_rot(10.0, 0.9), (1024, 1024), (1024, 1024), (13.5, -8.25)))

SAMPLE_TEXT = "\n".join([
    "pics/zeta.png 10 20 30.5 40.25 -5 6e1",
    "",
    "1 2 3 4 5 6",                                    # no name: dropped
    "alpha.JPG 1.5 2.5 3.5 4.5 5.5 6.5 trailing",
    "7 8 9 10 11 12 sub/mid.bmp",
    "note beta.jpg 0 0 100 0 50 80",
    ".png 1 1 1 1 1 1",                              # four characters: too short for a name
]) + "\n"
SAMPLE_QUERIES = ["/data/pics/zeta.png", "zeta.png", "alpha.JPG", "alpha.jpg", "/a/sub/mid.bmp", "xbeta.jpg", "x.png",
                  "none.png"]
EULER_TYPES = ("yxz", "xyz", "zyx", "zxy", "zxz", "yxy")


def golden_input(case):
    rs = np.random.RandomState(case["seed"])
    a = rs.randint(0, 256, size=tuple(case["shape"])).astype(np.uint8)
    if case["kind"] == "binary":
        a = np.where(a > 127, 255, 0).astype(np.uint8)
    return a


def inside_mask(case):
    """Where the sample point of Pillow's affine transform lies in [0, W) x [0, H), float64 like Pillow."""
    m = case["matrix"]
    (h, w), (oh, ow) = case["shape"][:2], case["size"]
    xs = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    ys = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    xin = m[0] * xs + m[1] * ys + m[2]
    yin = m[3] * xs + m[4] * ys + m[5]
    return (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)


def pillow_transform(a, matrix, size):
    from PIL import Image

    c = a.shape[2]
    # "CMYK" is four plain 8-bit channels, as in make_golden_resample.py
    im = Image.fromarray(a[:, :, 0] if c == 1 else a, {1: "L", 3: "RGB", 4: "CMYK"}[c])
    oh, ow = size
    out = im.transform((ow, oh), Image.AFFINE, tuple(matrix), resample=Image.BILINEAR)
    return np.ascontiguousarray(np.asarray(out).reshape(oh, ow, c))


def landmark_sets():
    """Seeded 68-point sets: a 2-D pair related by a similarity plus noise, a 3-D set and a noisy scaled orthographic
    view of it, and a few rotation matrices."""
    rs = np.random.RandomState(40)
    src2 = rs.uniform(20.0, 236.0, (68, 2))
    th, s = 0.4, 1.7
    A = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    dst2 = src2.dot(A.T) + [31.0, -12.0] + rs.normal(0.0, 1.5, (68, 2))
    src3 = rs.uniform(-1.0, 1.0, (68, 3)) * [90.0, 110.0, 60.0] + [128.0, 128.0, 0.0]
    rots = []
    for angles in ([0.3, -0.2, 0.5], [-1.1, 0.7, 2.4], [0.05, 1.2, -0.9], [2.0, -0.4, -2.8]):
        cx, cy, cz = np.cos(angles)
        sx, sy, sz = np.sin(angles)
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        rots.append(Ry.dot(Rx).dot(Rz))
    rots = np.stack(rots)
    dst3 = 1.3 * src3.dot(rots[0].T)[:, :2] + [40.0, 25.0] + rs.normal(0.0, 1.0, (68, 2))
    return src2, dst2, src3, dst3, rots


def reference_definitions(path):
    """The reference's solvers and reader, executed from the slices of its file that define them."""
    with open(path, "r") as f:
        lines = f.read().splitlines()
    heads = ("class LandmarksReader", "def solve_ortho", "def solve_affine", "def euler_mat_inv")
    ns = {"np": np, "os": os, "BASE_DIR": "."}
    for head in heads:
        first = [i for i, ln in enumerate(lines) if ln.startswith(head)][0]
        last = first + 1
        while last < len(lines) and (not lines[last] or lines[last][0] in " \t"):
            last += 1
        exec(compile("\n".join(lines[first:last]), head, "exec"), ns)
    return ns


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_align.py REFERENCE/utils_face.py")
    out = {"meta": np.array(json.dumps({"cases": CASES, "big": BIG}))}
    for case in CASES + [BIG]:
        mask = inside_mask(case)
        share = float(mask.mean())
        if any(b != "constant" for b in case["borders"]):
            assert share >= 0.5, (case["name"], share)
        r = pillow_transform(golden_input(case), case["matrix"], case["size"])
        assert not r[~mask].any()
        name = case["name"]
        out[name + "/share"] = np.array(share)
        if case is BIG:
            out[name + "/sha256"] = np.array(hashlib.sha256(r.tobytes()).hexdigest())
            out[name + "/corner"] = r[:16, :16].copy()
            out[name + "/inside"] = np.packbits(mask)
        else:
            out[name + "/pillow"] = r
            out[name + "/inside"] = mask
        print("%-8s inside %.3f" % (name, share))

    ref = reference_definitions(sys.argv[1])
    src2, dst2, src3, dst3, rots = landmark_sets()
    out["solve_affine"] = ref["solve_affine"](src2, dst2)
    out["solve_ortho"] = ref["solve_ortho"](src3, dst3)
    for t in EULER_TYPES:
        out["euler/" + t] = np.stack([np.asarray(ref["euler_mat_inv"](R, t), np.float64) for R in rots])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "lmk.txt")
        with open(path, "w") as f:
            f.write(SAMPLE_TEXT)
        reader = ref["LandmarksReader"](path)
    out["reader/names"] = np.array(reader.names)
    out["reader/data"] = np.asarray(reader.data, np.float64)
    for i, q in enumerate(SAMPLE_QUERIES):
        hit = reader.detect(q)
        out["reader/detect/%d" % i] = np.zeros((0, 2)) if hit is None else np.asarray(hit, np.float64)

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
