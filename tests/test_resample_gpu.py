"""GPU: the sr_resample_u8 kernels against the stored Pillow outputs and the host restatement, bit for bit."""
import hashlib

import numpy as np
import pytest
import torch

from make_golden_resample import CASES, FILTERS, PYRAMID, golden_input
from stylerenderer_amd import dataset
from stylerenderer_amd.op import resample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_fixture_and_host(golden, case):
    g = golden("resample")
    a = golden_input(case)
    rs = np.random.RandomState(100 + case["seed"])
    batch = np.stack([a] + [rs.randint(0, 256, size=a.shape).astype(np.uint8) for _ in range(4)])
    for f in FILTERS:
        want = g["%s/%s" % (case["name"], f)]
        one = resample.resize_u8(torch.from_numpy(a).to(DEV), case["size"], f, window=case.get("window"))
        assert one.dtype == torch.uint8 and np.array_equal(one.cpu().numpy(), want), (case["name"], f, "N = 1")
        host = resample.resize_u8(batch, case["size"], f, window=case.get("window"))
        assert np.array_equal(host[0], want)
        for form in ("u8_hwc", "f32_chw"):
            got = resample.resize_u8(torch.from_numpy(batch).to(DEV), case["size"], f, window=case.get("window"), out=form)
            ref = torch.from_numpy(host) if form == "u8_hwc" else resample.to_unit_chw(host)
            assert same_bits(got.cpu(), ref), (case["name"], f, form, "N = 5")
        # the 32-bit multiply instantiations
        got = resample.resize_u8(torch.from_numpy(batch).to(DEV), case["size"], f, window=case.get("window"),
                                 _force_mul32=True)
        assert np.array_equal(got.cpu().numpy(), host), (case["name"], f, "mul32")


def test_windows_of_every_pass_combination():
    rs = np.random.RandomState(7)
    for (h, w, c), size, win in [((45, 61, 3), (20, 33), (3, 5, 11, 17)), ((45, 61, 3), (45, 33), (3, 5, 11, 17)),
                                 ((45, 61, 3), (20, 61), (3, 5, 11, 17)), ((45, 61, 3), (45, 61), (3, 5, 11, 17)),
                                 ((45, 61, 3), (45, 61), None), ((30, 40, 4), (30, 40), (1, 4, 20, 8)),
                                 ((30, 40, 1), (70, 90), (9, 1, 50, 77)), ((64, 64, 4), (16, 16), (2, 3, 9, 10)),
                                 ((64, 64, 4), (64, 16), None), ((64, 67, 1), (16, 67), (0, 1, 16, 65))]:
        a = rs.randint(0, 256, size=(2, h, w, c)).astype(np.uint8)
        for f in ("box", "lanczos"):
            for form in ("u8_hwc", "f32_chw"):
                host = resample.resize_u8(a, size, f, window=win, out=form)
                got = resample.resize_u8(torch.from_numpy(a).to(DEV), size, f, window=win, out=form).cpu()
                assert same_bits(got, host if form == "f32_chw" else torch.from_numpy(host)), ((h, w, c), size, win, f, form)


def test_unstaged_horizontal_pass_on_a_very_wide_row():
    """One tile's input span beyond the LDS budget: the horizontal kernel reads global memory directly."""
    rs = np.random.RandomState(8)
    a = rs.randint(0, 256, size=(1, 3, 20000, 4)).astype(np.uint8)
    for f in ("box", "bilinear"):
        host = resample.resize_u8(a, (2, 8), f)
        assert np.array_equal(resample.resize_u8(torch.from_numpy(a).to(DEV), (2, 8), f).cpu().numpy(), host)


def test_unaligned_source_view():
    """A batch whose storage does not start on a dword: staging takes the first and last bytes singly."""
    rs = np.random.RandomState(9)
    flat = torch.from_numpy(rs.randint(0, 256, size=(1 + 2 * 31 * 29 * 3,)).astype(np.uint8)).to(DEV)
    x = flat[1:].view(2, 31, 29, 3)
    assert x.data_ptr() % 4 == 1
    for size in [(12, 10), (31, 10), (12, 29), (50, 60)]:
        host = resample.resize_u8(x.cpu().numpy(), size, "bicubic")
        assert np.array_equal(resample.resize_u8(x, size, "bicubic").cpu().numpy(), host), size


def test_f32_form_is_to_unit_tensor():
    every = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1).repeat(1, 1, 1, 3)
    got = resample.resize_u8(every.to(DEV), (16, 16), "lanczos", out="f32_chw").cpu()
    assert same_bits(got[0], dataset.to_unit_tensor(every[0].numpy()))
    a = golden_input(CASES[0])
    got = resample.resize_u8(torch.from_numpy(a).to(DEV), (32, 32), "lanczos", out="f32_chw").cpu()
    assert same_bits(got, dataset.to_unit_tensor(resample.resize_u8(a, (32, 32), "lanczos")))


def test_non_default_stream_and_captured_graph(golden):
    g = golden("resample")
    case = CASES[0]
    a = torch.from_numpy(golden_input(case)).to(DEV)
    want = torch.from_numpy(g["down/lanczos"])
    resample.resize_u8(a, case["size"], "lanczos")                  # tables on the device before anything is captured
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = resample.resize_u8(a, case["size"], "lanczos")
    side.synchronize()
    assert torch.equal(got.cpu(), want)

    static = a.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_u8 = resample.resize_u8(static, case["size"], "lanczos")
        out_f32 = resample.resize_u8(static, case["size"], "lanczos", out="f32_chw")
    other = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=tuple(a.shape)).astype(np.uint8))
    for src in (a.cpu(), other):                                    # two replays on two inputs
        static.copy_(src.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        host = resample.resize_u8(src.numpy(), case["size"], "lanczos")
        assert np.array_equal(out_u8.cpu().numpy(), host)
        assert same_bits(out_f32.cpu(), dataset.to_unit_tensor(host))
    assert torch.equal(torch.from_numpy(resample.resize_u8(a.cpu().numpy(), case["size"], "lanczos")), want)


def test_pyramid_digests(golden):
    g = golden("resample")
    a = torch.from_numpy(golden_input(PYRAMID)).to(DEV)
    for f in FILTERS:
        levels = resample.resize_pyramid(a, PYRAMID["sizes"], f)
        for s in PYRAMID["sizes"]:
            got = levels[s].cpu().numpy()
            assert got.shape == (s, s, 3)
            assert np.array_equal(got[:16, :16], g["pyramid/%d/%s/corner" % (s, f)]), (s, f)
            assert hashlib.sha256(got.tobytes()).hexdigest() == str(g["pyramid/%d/%s/sha256" % (s, f)]), (s, f)


def test_square_1024_pyramid_equals_host():
    a = np.random.RandomState(21).randint(0, 256, size=(2, 1024, 1024, 3)).astype(np.uint8)
    dev = resample.resize_pyramid(torch.from_numpy(a).to(DEV), (128, 256, 512, 1024), "lanczos")
    host = resample.resize_pyramid(a, (128, 256, 512, 1024), "lanczos")
    for s in host:
        assert np.array_equal(dev[s].cpu().numpy(), host[s]), s
