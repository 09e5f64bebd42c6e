"""CPU: python -m stylerenderer_amd.prepare_data on a small folder (host resampling, lossless payloads), read back
through dataset.MultiResolutionDataset and compared with Pillow's own resize + crop of every file."""
import os

import numpy as np
import pytest

from stylerenderer_amd import dataset, prepare_data
from stylerenderer_amd.op import resample

from prepare_data_cases import make_folder, pillow_levels

PIL = pytest.importorskip("PIL")
SIZES = (16, 32)


def run_cli(src, out, *extra):
    assert prepare_data.main(["--out", out, "--size", ",".join(str(s) for s in SIZES), "--n_worker", "3", *extra, src]) == 0


def test_cli_writes_a_store_the_dataset_reads(tmp_path, capsys):
    from PIL import Image

    src, out = str(tmp_path / "src"), str(tmp_path / "store")
    good = make_folder(src)
    run_cli(src, out, "--gpu", "-1", "--format", "npy")
    assert "skipped 1 unreadable" in capsys.readouterr().out
    # keys and length: compact indices over the readable files, in sorted order
    want_keys = {b"length"} | {dataset.make_key(s, i, len(good)) for s in SIZES for i in range(len(good))}
    assert set(dataset.open_store(out).keys()) == want_keys
    assert dataset.open_store(out).get(b"length") == str(len(good)).encode()
    for s in SIZES:
        ds = dataset.MultiResolutionDataset(out, transform=lambda a: a, resolution=s)
        assert len(ds) == len(good)
        for i, path in enumerate(good):
            assert np.array_equal(ds[i], pillow_levels(path, s, Image.LANCZOS)), (s, path)
        unit = dataset.MultiResolutionDataset(out, resolution=s)[0]
        assert tuple(unit.shape) == (3, s, s)


def test_resample_names_mean_what_they_say(tmp_path):
    from PIL import Image

    src = str(tmp_path / "src")
    good = make_folder(src)
    run_cli(src, str(tmp_path / "box"), "--gpu", "-1", "--format", "npy", "--resample", "box")
    run_cli(src, str(tmp_path / "lanczos"), "--gpu", "-1", "--format", "npy", "--resample", "lanczos")
    run_cli(src, str(tmp_path / "pillow"), "--gpu", "-1", "--format", "npy", "--host_resampler", "pillow")
    box = dataset.MultiResolutionDataset(str(tmp_path / "box"), transform=lambda a: a, resolution=16)
    lan = dataset.MultiResolutionDataset(str(tmp_path / "lanczos"), transform=lambda a: a, resolution=16)
    pil = dataset.MultiResolutionDataset(str(tmp_path / "pillow"), transform=lambda a: a, resolution=16)
    for i, path in enumerate(good):
        assert np.array_equal(box[i], pillow_levels(path, 16, Image.BOX))       # what the reference's tool computes
        assert not np.array_equal(box[i], lan[i])
        assert np.array_equal(pil[i], lan[i])
    with pytest.raises(ValueError, match="nearest"):
        prepare_data.main(["--out", str(tmp_path / "n"), "--resample", "nearest", "--gpu", "-1", src])


def test_jpeg_store_uses_the_quality(tmp_path):
    src = str(tmp_path / "src")
    good = make_folder(src)
    run_cli(src, str(tmp_path / "q100"), "--gpu", "-1")
    run_cli(src, str(tmp_path / "q30"), "--gpu", "-1", "--quality", "30")
    hi, lo = dataset.open_store(str(tmp_path / "q100")), dataset.open_store(str(tmp_path / "q30"))
    key = dataset.make_key(32, 0, len(good))
    assert hi.get(key)[:2] == b"\xff\xd8" and len(lo.get(key)) < len(hi.get(key))
    img = dataset.MultiResolutionDataset(str(tmp_path / "q100"), transform=lambda a: a, resolution=32)[0]
    assert img.shape == (32, 32, 3)
    a = np.zeros((8, 8, 3), np.uint8)
    assert dataset.encode_image(a) == dataset.encode_image(a, "JPEG", None)           # default unchanged
    assert dataset.encode_image(a, "JPEG", 100) != dataset.encode_image(a)


def test_key_padding_follows_the_readable_count():
    """Zero padding comes from the number of STORED images (make_key's rule), also when the file count needs more."""
    store = {}

    class Writer:
        put = staticmethod(store.__setitem__)

        @staticmethod
        def rename(old, new):
            store[new] = store.pop(old)

    import stylerenderer_amd.dataset as d

    real = d.read_image
    files = ["f%06d" % i for i in range(100001)]
    img = np.zeros((4, 4, 3), np.uint8)
    d.read_image = lambda p: img if p < "f000003" else None
    try:
        stored, skipped, _ = prepare_data.prepare(Writer, files, sizes=(2,), fmt="npy", n_worker=2)
    finally:
        d.read_image = real
    assert (stored, skipped) == (3, 100001 - 3)
    assert set(store) == {b"length", b"2-00000", b"2-00001", b"2-00002"}


def test_img_dataset_listing_and_items(tmp_path):
    src = str(tmp_path / "src")
    good = make_folder(src)
    ds = dataset.ImgDataset(src, resolution=16)
    listed = [p for p, label in ds.imgs]
    assert all(label == 0 for _, label in ds.imgs)
    assert sorted(listed) == sorted(good + [os.path.join(src, "a", "broken.jpg")])         # by name: '.txt' is out
    # breadth first: the top folder's files, then its sub-folders', then theirs
    depth = [p[len(src):].count(os.sep) for p in listed]
    assert depth == sorted(depth)
    flat = dataset.ImgDataset(src, recurrent=False)
    assert [p for p, _ in flat.imgs] == [os.path.join(src, "five.png")]
    assert [p for p, _ in dataset.ImgDataset(os.path.join(src, "five.png")).imgs] == [os.path.join(src, "five.png")]
    assert dataset.ImgDataset(os.path.join(src, "notes.txt")).imgs == []
    assert dataset.ImgDataset(os.path.join(src, "missing")).imgs == []
    assert len(dataset.ImgDataset(src, exts=".png").imgs) == 4                              # any letter case
    i = listed.index(os.path.join(src, "five.png"))
    item = ds[i]
    want = dataset.to_unit_tensor(resample.resize_center_crop(dataset.read_image(listed[i]), 16, "lanczos"))
    assert tuple(item.shape) == (3, 16, 16) and (item == want).all()
    with pytest.raises(IOError):
        ds[listed.index(os.path.join(src, "a", "broken.jpg"))]
