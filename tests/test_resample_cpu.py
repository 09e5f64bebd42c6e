"""CPU: the host restatement of Pillow's 8-bit resampler (op/resample.py) against the stored Pillow outputs and, where
Pillow is installed, against Pillow itself.  Every comparison is exact."""
import hashlib

import numpy as np
import pytest
import torch

from make_golden_resample import CASES, FILTERS, PYRAMID, center_crop_geometry, golden_input
from stylerenderer_amd import dataset
from stylerenderer_amd.op import resample


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_path_equals_fixture(golden, case):
    g = golden("resample")
    a = golden_input(case)
    for f in FILTERS:
        got = resample.resize_u8(a, case["size"], f, window=case.get("window"))
        want = g["%s/%s" % (case["name"], f)]
        assert got.dtype == np.uint8 and got.shape == want.shape
        assert np.array_equal(got, want), (case["name"], f)


def test_fixture_reaches_the_clip(golden):
    """The 0 / 255 inputs overshoot under the negative lobes: without the clip the bytes would wrap."""
    g = golden("resample")
    a = golden_input([c for c in CASES if c["name"] == "binary_up"][0]).astype(np.float64)
    for f in ("bicubic", "lanczos"):
        k, b = resample.coefficients(a.shape[1], 31, f)
        raw = np.stack([a[:, b[x, 0]:b[x, 0] + b[x, 1], 0] @ k[x, :b[x, 1]] for x in range(31)]) / 2.0 ** 22
        assert raw.min() < -1 and raw.max() > 256
        out = g["binary_up/%s" % f]
        assert out.min() == 0 and out.max() == 255


def test_center_crop_geometry_rounds_half_to_even():
    assert resample.center_crop_geometry(64, 74, 32) == ((32, 37), (0, 2, 32, 32))        # difference 5 -> 2
    assert resample.center_crop_geometry(74, 64, 32) == ((37, 32), (2, 0, 32, 32))
    assert resample.center_crop_geometry(64, 70, 32) == ((32, 35), (0, 2, 32, 32))        # difference 3 -> 2
    assert resample.center_crop_geometry(683, 1024, 128) == ((128, 191), (0, 32, 128, 128))
    for h, w, s in [(683, 1024, 256), (1024, 683, 512), (99, 99, 40)]:
        assert resample.center_crop_geometry(h, w, s) == center_crop_geometry(h, w, s)


def test_center_crop_equals_fixture(golden):
    g = golden("resample")
    case = [c for c in CASES if c["name"] == "crop"][0]
    a = golden_input(case)
    for f in FILTERS:
        assert np.array_equal(resample.resize_center_crop(a, 32, f), g["crop/%s" % f])


def test_pyramid_digests_and_single_calls(golden):
    g = golden("resample")
    a = golden_input(PYRAMID)
    for f in ("box", "lanczos"):
        levels = resample.resize_pyramid(a, PYRAMID["sizes"], f)
        assert sorted(levels) == sorted(PYRAMID["sizes"])
        for s in PYRAMID["sizes"]:
            assert levels[s].shape == (s, s, 3)
            assert hashlib.sha256(levels[s].tobytes()).hexdigest() == str(g["pyramid/%d/%s/sha256" % (s, f)])
            assert np.array_equal(levels[s][:16, :16], g["pyramid/%d/%s/corner" % (s, f)])
            assert np.array_equal(levels[s], resample.resize_center_crop(a, s, f))


def test_equals_live_pillow_on_fresh_shapes():
    pytest.importorskip("PIL")
    from make_golden_resample import pillow_resize

    rs = np.random.RandomState(2024)
    for i in range(12):
        h, w, oh, ow = (int(v) for v in rs.randint(1, 160, size=4))
        c = (1, 3, 4)[i % 3]
        a = rs.randint(0, 256, size=(h, w, c)).astype(np.uint8)
        if i % 4 == 0:
            a = np.where(a > 127, 255, 0).astype(np.uint8)
        oy0, ox0 = int(rs.randint(0, oh)), int(rs.randint(0, ow))
        win = (oy0, ox0, int(rs.randint(1, oh - oy0 + 1)), int(rs.randint(1, ow - ox0 + 1)))
        for f in FILTERS:
            assert np.array_equal(resample.resize_u8(a, (oh, ow), f), pillow_resize(a, (oh, ow), f)), (h, w, oh, ow, c, f)
            assert np.array_equal(resample.resize_u8(a, (oh, ow), f, window=win), pillow_resize(a, (oh, ow), f, win))


def test_table_invariants():
    for n_in, n_out in [(97, 32), (64, 128), (300, 64), (1, 5), (1024, 128), (683, 512), (50, 50), (7, 1000)]:
        for f in FILTERS:
            k, b = resample.coefficients(n_in, n_out, f)
            support = {"box": .5, "bilinear": 1., "hamming": 1., "bicubic": 2., "lanczos": 3.}[f] * max(n_in / n_out, 1.)
            ksize = int(np.ceil(support)) * 2 + 1
            assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == (n_out, ksize) and b.shape == (n_out, 2)
            assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all()
            assert (b[:, 1] <= ksize).all()
            assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()
            rows = k.astype(np.int64).sum(1)
            assert (np.abs(rows - (1 << 22)) <= ksize).all()
            for x in range(n_out):
                assert not k[x, b[x, 1]:].any()
            assert np.abs(k.astype(np.int64)).max() < (1 << 23)          # the 24-bit multiply-add holds
    assert resample.coefficients(97, 32, "lanczos")[0] is resample.coefficients(97, 32, "LANCZOS")[0]     # cached


def test_f32_chw_is_to_unit_tensor():
    a = golden_input(CASES[0])
    u8 = resample.resize_u8(a, (32, 32), "lanczos")
    f32 = resample.resize_u8(a, (32, 32), "lanczos", out="f32_chw")
    want = dataset.to_unit_tensor(u8)
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (3, 32, 32)
    assert torch.equal(f32.view(torch.int32), want.view(torch.int32))
    every = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    assert torch.equal(resample.resize_u8(every, (16, 16), "box", out="f32_chw").view(torch.int32),
                       dataset.to_unit_tensor(np.repeat(every, 3, 2))[:1].view(torch.int32))


def test_batches_tensors_and_identity():
    rs = np.random.RandomState(5)
    a = rs.randint(0, 256, size=(3, 21, 34, 3)).astype(np.uint8)
    got = resample.resize_u8(a, (10, 13), "bicubic")
    for i in range(3):
        assert np.array_equal(got[i], resample.resize_u8(a[i], (10, 13), "bicubic"))
    t = resample.resize_u8(torch.from_numpy(a), (10, 13), "bicubic")
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), got)
    assert np.array_equal(resample.resize_u8(a, (21, 34), "lanczos"), a)                  # both passes skipped
    assert np.array_equal(resample.resize_u8(a, (21, 34), "lanczos", window=(2, 3, 5, 7)), a[:, 2:7, 3:10])


def test_rejects_nearest_and_bad_arguments():
    a = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError, match="nearest"):
        resample.resize_u8(a, 4, "nearest")
    with pytest.raises(ValueError, match="nearest"):
        resample.coefficients(8, 4, "NEAREST")
    with pytest.raises(ValueError):
        resample.resize_u8(a, 4, "area")
    with pytest.raises(ValueError):
        resample.resize_u8(a.astype(np.float32), 4)
    with pytest.raises(ValueError):
        resample.resize_u8(np.zeros((8, 8, 2), np.uint8), 4)
    with pytest.raises(ValueError):
        resample.resize_u8(a, 4, window=(0, 0, 5, 4))
    with pytest.raises(ValueError):
        resample.resize_u8(a, 4, out="f16")


def test_entry_point_validates_without_gpu():
    """sr_resample_u8 checks sizes, tables and the window before any launch."""
    import ctypes

    from stylerenderer_amd import _lib

    L = _lib.lib()
    k, b = resample.coefficients(16, 8, "bilinear")
    bh = b.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    assert L.sr_resample_u8_scratch_bytes(2, 16, 16, 3, 8, 8, bh, 0, 0, 8, 8) == 2 * 16 * 24
    assert L.sr_resample_u8_scratch_bytes(2, 16, 16, 3, 8, 8, bh, 2, 1, 3, 5) == 2 * (int(b[4, 0] + b[4, 1]) - int(b[2, 0])) * 16
    assert L.sr_resample_u8_scratch_bytes(2, 16, 16, 3, 16, 8, None, 0, 0, 16, 8) == 0
    assert L.sr_resample_u8_scratch_bytes(2, 16, 16, 2, 8, 8, bh, 0, 0, 8, 8) == -1
    assert L.sr_resample_u8_scratch_bytes(2, 16, 16, 3, 8, 8, bh, 0, 0, 9, 8) == -1
    args = (None, None, None, 0, None, None, None, 0)
    assert L.sr_resample_u8(None, None, 0, 16, 16, 3, 8, 8, *args, 0, 0, 8, 8, 0, 1, None, None) == 0     # empty batch
    assert L.sr_resample_u8(None, None, 1, 16, 16, 3, 8, 8, *args, 0, 0, 8, 8, 0, 1, None, None) == -1    # NULL images
    assert L.sr_resample_u8(None, None, 1, 16, 16, 2, 8, 8, *args, 0, 0, 8, 8, 0, 1, None, None) == -1    # C = 2
    assert L.sr_resample_u8(None, None, 1, 16, 16, 3, 8, 8, *args, 0, 0, 8, 8, 2, 1, None, None) == -1    # output form
    assert L.sr_resample_u8(1, 1, 1, 16, 16, 3, 8, 8, *args, 0, 0, 8, 8, 0, 1, None, None) == -1          # tables missing
