"""CPU: op.warp_affine's host definition against the stored Pillow outputs (every byte; under reflect / replicate every
byte whose sample point lies inside the source, the region on which Pillow defines a value) and against a plain
per-pixel loop (every byte, outside included); align.py's solvers and reader against the stored outputs of the
reference's; the two command-line tools on a small folder, host path, lossless payloads."""
import hashlib
import math
import os

import numpy as np
import pytest
import torch

from make_golden_align import BIG, CASES, EULER_TYPES, SAMPLE_QUERIES, SAMPLE_TEXT, golden_input, landmark_sets
from stylerenderer_amd import align, align_faces, dataset, prepare_data
from stylerenderer_amd.op import resample, warp

from prepare_data_cases import make_folder

# Solver bar (relative to the largest entry): the inputs are 68 well-spread points, so two LAPACK-level evaluations of
# the same closed form differ by about 1e-13, while a wrong convention (a transposed rotation, a swapped sign) is O(1).
# 1e-9 keeps four orders of margin on either side.
SOLVER_RTOL = 1e-9


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want).max() / np.abs(want).max()
    print("relative error %.3g" % err)
    return err <= SOLVER_RTOL


# ---- warp_affine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_definition_equals_pillow_fixture(golden, case):
    g = golden("align")
    a, name = golden_input(case), case["name"]
    want, inside = g[name + "/pillow"], g[name + "/inside"]
    got = warp.warp_affine(a, case["matrix"], case["size"], "constant")
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want)
    for border in case["borders"]:
        if border == "constant":
            continue
        assert float(g[name + "/share"]) >= 0.5
        got = warp.warp_affine(a, case["matrix"], case["size"], border)
        assert np.array_equal(got[inside], want[inside]), border


def test_big_case_digest(golden):
    g = golden("align")
    a = golden_input(BIG)
    got = warp.warp_affine(a, BIG["matrix"], BIG["size"], "constant")
    assert np.array_equal(got[:16, :16], g["big/corner"])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(g["big/sha256"])
    inside = np.unpackbits(g["big/inside"])[:got.shape[0] * got.shape[1]].reshape(got.shape[:2]).astype(bool)
    refl = warp.warp_affine(a, BIG["matrix"], BIG["size"], "reflect")
    assert np.array_equal(refl[inside], got[inside])
    assert refl[~inside].any()


def loop_warp(a, m, oh, ow, border, fill=0):
    """The definition, one pixel at a time in Python floats (IEEE doubles, no fused multiply-add)."""
    h, w, c = a.shape

    def index(i, size):
        if border == "reflect":
            i = i % (2 * size)
            return i if i < size else 2 * size - 1 - i
        return min(max(i, 0), size - 1)

    out = np.zeros((oh, ow, c), np.uint8)
    for y in range(oh):
        for x in range(ow):
            xs, ys = x + .5, y + .5
            xin = m[0] * xs + m[1] * ys + m[2]
            yin = m[3] * xs + m[4] * ys + m[5]
            if border == "constant" and not (0.0 <= xin < w and 0.0 <= yin < h):
                out[y, x] = fill
                continue
            xf, yf = xin - .5, yin - .5
            x0, y0 = math.floor(xf), math.floor(yf)
            dx, dy = xf - x0, yf - y0
            for ch in range(c):
                p00, p01 = float(a[index(y0, h), index(x0, w), ch]), float(a[index(y0, h), index(x0 + 1, w), ch])
                p10, p11 = float(a[index(y0 + 1, h), index(x0, w), ch]), float(a[index(y0 + 1, h), index(x0 + 1, w), ch])
                v1 = p00 + (p01 - p00) * dx
                v2 = p10 + (p11 - p10) * dx
                out[y, x, ch] = int(v1 + (v2 - v1) * dy)
    return out


@pytest.mark.parametrize("name", ["outside", "four"])
def test_borders_equal_a_plain_loop(name):
    """Outside pixels included: `outside` reaches several periods of the reflection on every side."""
    case = [c for c in CASES if c["name"] == name][0]
    a = golden_input(case)
    oh, ow = case["size"]
    m = list(case["matrix"])
    if name == "four":              # push it off the source: a shift of the whole width, both signs of the index
        m[2] -= 40.0
        m[5] += 25.0
    for border, fill in (("reflect", 0), ("replicate", 0), ("constant", 200)):
        got = warp.warp_affine(a, m, (oh, ow), border, fill)
        assert np.array_equal(got, loop_warp(a, m, oh, ow, border, fill)), border


def test_batch_with_per_image_matrices_equals_single_calls():
    rs = np.random.RandomState(5)
    a = rs.randint(0, 256, (5, 30, 41, 3)).astype(np.uint8)
    mats = np.stack([[np.cos(t) * s, -np.sin(t) * s, 3.0 + t, np.sin(t) * s, np.cos(t) * s, -2.0 * t]
                     for t, s in zip((0.0, 0.2, -0.4, 1.0, 2.5), (1.0, 0.7, 1.3, 0.5, 2.0))])
    for border in ("reflect", "replicate", "constant"):
        got = warp.warp_affine(a, mats, (26, 37), border)
        assert got.shape == (5, 26, 37, 3)
        for i in range(5):
            assert np.array_equal(got[i], warp.warp_affine(a[i], mats[i], (26, 37), border))
        shared = warp.warp_affine(a, mats[1], (26, 37), border)
        assert np.array_equal(shared[3], warp.warp_affine(a[3], mats[1], (26, 37), border))
    t = warp.warp_affine(torch.from_numpy(a), mats, (26, 37))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), warp.warp_affine(a, mats, (26, 37)))


def test_f32_chw_is_to_unit_chw_of_the_bytes():
    case = [c for c in CASES if c["name"] == "general"][0]
    a = golden_input(case)
    u8 = warp.warp_affine(a, case["matrix"], case["size"])
    f32 = warp.warp_affine(a, case["matrix"], case["size"], out="f32_chw")
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (3,) + tuple(case["size"])
    assert torch.equal(f32, resample.to_unit_chw(u8[None])[0])
    assert torch.equal(f32, dataset.to_unit_tensor(u8))


def test_arguments_are_checked():
    a = np.zeros((4, 4, 3), np.uint8)
    eye = [1.0, 0, 0, 0, 1.0, 0]
    assert np.array_equal(warp.warp_affine(a + 7, eye, 4), a + 7)
    for bad in (dict(border="wrap"), dict(out="f16"), dict(fill=256)):
        with pytest.raises(ValueError):
            warp.warp_affine(a, eye, 4, **bad)
    with pytest.raises(ValueError):
        warp.warp_affine(a.astype(np.float32), eye, 4)
    with pytest.raises(ValueError):
        warp.warp_affine(a[:, :, :2], eye, 4)
    with pytest.raises(ValueError):
        warp.warp_affine(a, np.zeros((2, 6)), 4)
    with pytest.raises(ValueError):
        warp.warp_affine(a, [1.0, 0, float("nan"), 0, 1.0, 0], 4)


def test_from_index_transform_is_the_index_convention():
    """An index-coordinate shift by whole pixels moves whole pixels; a scale by 2 about index 0 samples index 2 i."""
    rs = np.random.RandomState(6)
    a = rs.randint(0, 256, (12, 15, 3)).astype(np.uint8)
    m = warp.from_index_transform([[1.0, 0.0, 3.0], [0.0, 1.0, 2.0]])
    assert np.array_equal(warp.warp_affine(a, m, (10, 12)), a[2:, 3:])
    m = warp.from_index_transform(np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 1.0]]))
    assert np.array_equal(warp.warp_affine(a, m, (6, 7)), a[0:12:2, 0:14:2])
    with pytest.raises(ValueError):
        warp.from_index_transform(np.ones((3, 3)))


# ---- solvers and reader ----------------------------------------------------------------------------------------------
def test_solvers_equal_the_reference(golden):
    g = golden("align")
    src2, dst2, src3, dst3, rots = landmark_sets()
    assert close(align.solve_affine(src2, dst2), g["solve_affine"])
    assert close(align.solve_ortho(src3, dst3), g["solve_ortho"])
    for t in EULER_TYPES:
        assert close(np.stack([align.euler_mat_inv(R, t) for R in rots]), g["euler/" + t]), t


def test_reader_equals_the_reference(golden, tmp_path):
    g = golden("align")
    path = tmp_path / "lmk.txt"
    path.write_text(SAMPLE_TEXT)
    reader = align.LandmarksReader(str(path))
    assert reader.names == [str(n) for n in g["reader/names"]]
    assert np.array_equal(reader.data, g["reader/data"])
    for i, q in enumerate(SAMPLE_QUERIES):
        hit, want = reader.detect(q), g["reader/detect/%d" % i]
        if want.shape[0] == 0:
            assert hit is None, q
        else:
            assert np.array_equal(hit, want), q
    assert reader.detect("alpha.JPG").shape == (3, 2) and reader.detect("none.png") is None


def similarity(th, s, tx, ty):
    return np.array([[s * np.cos(th), -s * np.sin(th), tx], [s * np.sin(th), s * np.cos(th), ty], [0.0, 0.0, 1.0]])


def test_alignment_matrix_recovers_a_known_similarity():
    rs = np.random.RandomState(7)
    template = rs.uniform(30.0, 220.0, (68, 2))
    T = similarity(-0.35, 1.9, 41.0, 17.5)
    lmk = template.dot(T[:2, :2].T) + T[:2, 2]
    got = align.alignment_matrix(template, lmk, (256, 256))
    assert got.shape == (3, 3) and close(got, T)
    with pytest.raises(ValueError):
        align.alignment_matrix(template, lmk[:60], (256, 256))


def test_3d_template_keeps_roll_scale_translation_only():
    """A 3-D template seen under yaw, pitch and roll: the alignment is the same as under the roll alone."""
    rs = np.random.RandomState(8)
    template = rs.uniform(-1.0, 1.0, (68, 3)) * [0.7, 0.8, 0.4]
    H, W = 240, 200
    base = np.stack(((1 + template[:, 0]) * W / 2, (1 - template[:, 1]) * H / 2, -template[:, 2] * (W + H) / 4), 1)
    yaw, pitch, roll, s, t = 0.3, -0.2, 0.45, 1.4, np.array([25.0, -10.0])

    def view(yaw, pitch):
        cy, sy, cx, sx, cz, sz = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        R = Rz.dot(Rx).dot(Ry)              # roll applied last: it is the in-plane part
        centre = base.mean(0)
        return s * (base - centre).dot(R.T)[:, :2] + centre[:2] + t

    T = align.alignment_matrix(template, view(yaw, pitch), (H, W))
    assert np.array_equal(T[2], [0.0, 0.0, 1.0])
    c, sn = T[0, 0], T[1, 0]
    assert close([T[0, 1], T[1, 1]], [-sn, c])                              # a similarity
    assert close([np.hypot(c, sn), np.arctan2(sn, c)], [s, roll])           # scale and roll; yaw and pitch are gone
    flat = align.alignment_matrix(template, view(0.0, 0.0), (H, W))
    assert close(flat[:2, :2], T[:2, :2])
    # and with no yaw / pitch it is the 2-D answer
    assert close(flat, align.alignment_matrix(base[:, :2], view(0.0, 0.0), (H, W)))


def test_template_from_bfm():
    rs = np.random.RandomState(9)
    v = rs.normal(0.0, 1e5, (3, 50))
    tri = np.empty((1, 1), object)
    tri[0, 0] = rs.randint(1, 51, (3, 80))
    tri[0, 0][0, 0] = 1
    idx = rs.randint(1, 51, (68, 1)).astype(np.float64)
    model = {"v": v, "tri": tri, "landmarks68": idx}
    got = align.template_from_bfm(model)
    want = ((v - v.mean(1, keepdims=True)).T * 1e-5)[idx.reshape(-1).astype(int) - 1]
    assert got.shape == (68, 3) and np.array_equal(got, want)
    with pytest.raises(KeyError, match="detector"):
        align.template_from_bfm({"v": v, "tri": tri})


def test_align_puts_the_landmarks_on_the_template():
    rs = np.random.RandomState(10)
    img = np.zeros((120, 110, 3), np.uint8)
    template = np.array([[20.0, 20.0], [44.0, 20.0], [32.0, 40.0], [24.0, 50.0], [40.0, 50.0]])
    T = similarity(0.5, 1.2, 30.0, 5.0)
    lmk = np.rint(template.dot(T[:2, :2].T) + T[:2, 2])
    for i, (x, y) in enumerate(lmk.astype(int)):
        img[y - 1:y + 2, x - 1:x + 2] = 60 + 40 * i
    out, got = align.align(img, lmk, template, 64)
    assert out.shape == (64, 64, 3) and got.shape == (3, 3)
    for i, (x, y) in enumerate(template.astype(int)):
        assert abs(int(out[y, x, 0]) - (60 + 40 * i)) < 40, i           # the blob of landmark i, blurred by the warp


# ---- command-line tools ----------------------------------------------------------------------------------------------
SIZES = (16, 32)


def flat_folder(root, png_only=False):
    """make_folder's pictures in ONE folder (align_faces writes basenames, so sorted order survives it), with the
    truncated file; png_only: every picture re-saved as <name>.png, so that align_faces' output is lossless.
    Returns (folder, readable paths sorted)."""
    from PIL import Image

    good = make_folder(os.path.join(root, "nested"))
    flat = os.path.join(root, "flat")
    os.makedirs(flat)
    out = []
    for f in good:
        if png_only:
            out.append(os.path.join(flat, os.path.splitext(os.path.basename(f))[0] + ".png"))
            Image.fromarray(dataset.read_image(f)).save(out[-1])
        else:
            out.append(os.path.join(flat, os.path.basename(f)))
            with open(f, "rb") as src, open(out[-1], "wb") as dst:
                dst.write(src.read())
    whole = open(out[0], "rb").read()
    with open(os.path.join(flat, "broken.png" if png_only else "broken.jpg"), "wb") as f:
        f.write(whole[:len(whole) // 3])
    return flat, sorted(out)


def make_landmarks(root, files, seed=3, skip=("five.png",)):
    """A landmark file for `files` (but `skip`) and for the truncated file, rows in shuffled order: five points, a fixed
    shape under a similarity of its own per picture.  Also a template file for a 40 x 40 (or larger) canvas."""
    rs = np.random.RandomState(seed)
    shape = np.array([[12.0, 12.0], [28.0, 12.0], [20.0, 22.0], [14.0, 30.0], [26.0, 30.0]])
    rows = []
    for f in files:
        if os.path.basename(f) in skip:
            continue
        th, s = rs.uniform(-0.5, 0.5), rs.uniform(0.8, 1.3)
        pts = shape.dot(np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]).T * s) + rs.uniform(0.0, 8.0, 2)
        rows.append(os.path.basename(f) + " " + " ".join("%.4f" % v for v in pts.reshape(-1)))
    broken = [n for n in os.listdir(root) if n.startswith("broken")][0]
    rows.append(broken + " " + " ".join("%d" % v for v in range(10)))
    rs.shuffle(rows)
    path = os.path.join(root, "landmarks.txt")
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    tpl = os.path.join(root, "template.txt")
    with open(tpl, "w") as f:
        f.write("template.png " + " ".join("%.2f" % v for v in (shape * 1.2).reshape(-1)) + "\n")
    return path, tpl


def store_payloads(path):
    store = dataset.open_store(path)
    return {k: store.get(k) for k in store.keys()}


def test_align_faces_writes_the_pictures_that_have_landmarks(tmp_path, capsys):
    src, good = flat_folder(str(tmp_path))
    lmk, tpl = make_landmarks(src, good)
    out = str(tmp_path / "aligned")
    assert align_faces.main(["--lmk", lmk, "--template", tpl, "--size", "48", "--gpu", "-1", "--n_worker", "3",
                             "--output", out, src]) == 0
    said = capsys.readouterr().out
    assert "aligned 5 pictures to 48 x 48" in said and "1 without landmarks, 1 unreadable" in said
    assert sorted(os.listdir(out)) == sorted(os.path.basename(f) for f in good if not f.endswith("five.png"))
    reader, template = align.LandmarksReader(lmk), align.read_template(tpl)
    for f in good:
        if f.lower().endswith((".png", ".bmp")) and not f.endswith("five.png"):         # lossless: the bytes of align()
            want, _ = align.align(dataset.read_image(f), reader.detect(f), template, 48)
            assert np.array_equal(dataset.read_image(os.path.join(out, os.path.basename(f))), want)


def test_align_faces_without_a_template_takes_the_first_picture(tmp_path, capsys):
    src, good = flat_folder(str(tmp_path))
    lmk, _ = make_landmarks(src, good, skip=())
    out = str(tmp_path / "aligned")
    assert align_faces.main(["--lmk", lmk, "--gpu", "-1", "--output", out, src]) == 0
    first = dataset.read_image(good[0])
    assert "aligned 6 pictures to %d x %d" % first.shape[:2] in capsys.readouterr().out
    reader = align.LandmarksReader(lmk)
    for f in good:
        got = dataset.read_image(os.path.join(out, os.path.basename(f)))
        assert got.shape == first.shape
        if f.lower().endswith((".png", ".bmp")):
            want, _ = align.align(dataset.read_image(f), reader.detect(f), reader.detect(good[0]), first.shape[:2])
            assert np.array_equal(got, want)


@pytest.mark.parametrize("word", ["dlib", "exec", "torch"])
def test_align_faces_names_the_missing_detector(tmp_path, word):
    with pytest.raises(SystemExit, match="does not have"):
        align_faces.main(["--lmk", word, "--output", str(tmp_path / "o"), str(tmp_path)])


def test_prepare_data_align_equals_prepare_data_over_align_faces(tmp_path, capsys):
    src, good = flat_folder(str(tmp_path), png_only=True)
    lmk, tpl = make_landmarks(src, good)
    aligned, two_step, one_step = str(tmp_path / "aligned"), str(tmp_path / "two"), str(tmp_path / "one")
    common = ["--size", ",".join(str(s) for s in SIZES), "--n_worker", "3", "--gpu", "-1", "--format", "png"]
    assert align_faces.main(["--lmk", lmk, "--template", tpl, "--size", "40", "--gpu", "-1", "--output", aligned, src]) == 0
    assert prepare_data.main(["--out", two_step] + common + [aligned]) == 0
    capsys.readouterr()
    assert prepare_data.main(["--out", one_step, "--align", lmk, "--template", tpl, "--align_size", "40"] + common
                             + [src]) == 0
    said = capsys.readouterr().out
    assert "6 of 7 pictures have landmarks, 1 skipped" in said
    assert "stored 5 images" in said and "skipped 1 unreadable" in said
    one, two = store_payloads(one_step), store_payloads(two_step)
    assert one[b"length"] == b"5" and len(one) == 1 + 5 * len(SIZES)
    assert one == two
    # the default canvas is the largest --size
    assert prepare_data.main(["--out", str(tmp_path / "d"), "--align", lmk, "--template", tpl] + common + [src]) == 0
    assert "aligning to 32 x 32" in capsys.readouterr().out


def test_prepare_data_without_align_is_unchanged(tmp_path):
    """The store of a run without --align equals what the tool's documented pipeline writes: every readable file, sorted,
    resize_center_crop of the decoded picture, encoded by dataset.encode_image."""
    src = str(tmp_path / "src")
    good = make_folder(src)
    out = str(tmp_path / "store")
    assert prepare_data.main(["--out", out, "--size", "16,32", "--n_worker", "3", "--gpu", "-1", "--format", "png",
                              src]) == 0
    want = {b"length": str(len(good)).encode()}
    for i, f in enumerate(good):
        for s in SIZES:
            want[dataset.make_key(s, i, len(good))] = dataset.encode_image(
                resample.resize_center_crop(dataset.read_image(f), s, "lanczos"), "PNG", None)
    assert store_payloads(out) == want
    with pytest.raises(SystemExit):
        prepare_data.main(["--out", out, "--template", "t.txt", "--gpu", "-1", src])
