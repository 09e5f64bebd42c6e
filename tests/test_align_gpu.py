"""GPU: the sr_warp_affine_u8 kernel against the stored Pillow outputs and the host definition, bit for bit: every case,
every border, both output forms, N = 1 and N = 5 with five matrices, the 1024^2 case by hash; a captured graph; the two
command-line tools with --gpu 0 against --gpu -1."""
import hashlib
import os

import numpy as np
import pytest
import torch

from make_golden_align import BIG, CASES, golden_input
from stylerenderer_amd import align_faces, dataset, prepare_data
from stylerenderer_amd.op import resample, warp

from test_align_cpu import flat_folder, make_landmarks

pytestmark = pytest.mark.gpu
DEV = "cuda"
BORDERS = ("constant", "reflect", "replicate")


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_strict_native_is_on():
    assert os.environ.get("SR_STRICT_NATIVE") == "1"


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_fixture_and_host(golden, case):
    g = golden("align")
    a, name = golden_input(case), case["name"]
    want, inside = g[name + "/pillow"], g[name + "/inside"]
    x = torch.from_numpy(a).to(DEV)
    for border in BORDERS:
        host = warp.warp_affine(a, case["matrix"], case["size"], border, fill=0)
        got = warp.warp_affine(x, case["matrix"], case["size"], border, fill=0)
        assert got.dtype == torch.uint8 and got.device.type == "cuda"
        got = got.cpu().numpy()
        assert np.array_equal(got, host), border                              # every byte, outside included
        if border == "constant":
            assert np.array_equal(got, want)
        elif border in case["borders"]:
            assert np.array_equal(got[inside], want[inside]), border
        f32 = warp.warp_affine(x, case["matrix"], case["size"], border, out="f32_chw").cpu()
        assert same_bits(f32, resample.to_unit_chw(host[None])[0]), border
    filled = warp.warp_affine(x, case["matrix"], case["size"], "constant", fill=137).cpu().numpy()
    assert np.array_equal(filled, warp.warp_affine(a, case["matrix"], case["size"], "constant", fill=137))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_batch_of_five_matrices(case):
    """N = 5: the case's picture and four redrawn ones, the case's matrix and four perturbed ones (one of them pushes
    the output off the source, another is not aligned to anything)."""
    rs = np.random.RandomState(100 + case["seed"])
    a = np.stack([golden_input(case)] + [rs.randint(0, 256, size=tuple(case["shape"])).astype(np.uint8) for _ in range(4)])
    m = np.array(case["matrix"])
    mats = np.stack([m, m * [1, 1, 1, 1, 1, 1] + [0, 0, 0.37, 0, 0, -0.61], m * 1.7, m * [1, -1, 1, -1, 1, 1],
                     m + [0, 0, 3.0 * case["shape"][1], 0, 0, -2.0 * case["shape"][0]]])
    x = torch.from_numpy(a).to(DEV)
    for border in BORDERS:
        host = warp.warp_affine(a, mats, case["size"], border)
        got = warp.warp_affine(x, mats, case["size"], border)
        assert np.array_equal(got.cpu().numpy(), host), border
        # the matrices as a device tensor, and one matrix shared by the batch
        got = warp.warp_affine(x, torch.from_numpy(mats).to(DEV), case["size"], border, out="f32_chw")
        assert same_bits(got.cpu(), resample.to_unit_chw(host)), border
        got = warp.warp_affine(x, mats[2], case["size"], border)
        assert np.array_equal(got.cpu().numpy(), warp.warp_affine(a, mats[2], case["size"], border)), border


def test_big_case_by_hash(golden):
    g = golden("align")
    a = golden_input(BIG)
    x = torch.from_numpy(a).to(DEV)
    got = warp.warp_affine(x, BIG["matrix"], BIG["size"], "constant").cpu().numpy()
    assert np.array_equal(got[:16, :16], g["big/corner"])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(g["big/sha256"])
    for border in ("reflect", "replicate"):
        got = warp.warp_affine(x, BIG["matrix"], BIG["size"], border).cpu().numpy()
        assert np.array_equal(got, warp.warp_affine(a, BIG["matrix"], BIG["size"], border)), border
    f32 = warp.warp_affine(x, BIG["matrix"], BIG["size"], "reflect", out="f32_chw").cpu()
    assert same_bits(f32, resample.to_unit_chw(warp.warp_affine(a, BIG["matrix"], BIG["size"], "reflect")[None])[0])


def test_unaligned_views_take_the_unpacked_stores():
    """A source that starts at an odd byte and outputs whose rows are not dword multiples: byte / float stores."""
    rs = np.random.RandomState(11)
    flat = torch.from_numpy(rs.randint(0, 256, 1 + 2 * 21 * 33 * 3).astype(np.uint8)).to(DEV)
    x = flat[1:].view(2, 21, 33, 3)
    assert x.data_ptr() % 4 == 1 and x.is_contiguous()
    a = x.cpu().numpy()
    m = [0.9, -0.3, 4.2, 0.3, 0.9, -1.1]
    for size in ((19, 31), (7, 2), (5, 64), (16, 65)):
        for out in ("u8_hwc", "f32_chw"):
            got = warp.warp_affine(x, m, size, "reflect", out=out).cpu()
            host = warp.warp_affine(a, m, size, "reflect", out=out)
            assert torch.equal(got, torch.as_tensor(host)), (size, out)


def test_captured_graph_replays_on_a_second_picture():
    case = CASES[1]
    a = golden_input(case)
    other = np.random.RandomState(12).randint(0, 256, size=a.shape).astype(np.uint8)
    static = torch.from_numpy(a).to(DEV)
    mats = torch.tensor(case["matrix"], dtype=torch.float64, device=DEV)
    warp.warp_affine(static, mats, case["size"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_u8 = warp.warp_affine(static, mats, case["size"], "reflect")
        out_f32 = warp.warp_affine(static, mats, case["size"], "replicate", out="f32_chw")
    for src in (a, other):
        static.copy_(torch.from_numpy(src).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out_u8.cpu().numpy(), warp.warp_affine(src, case["matrix"], case["size"], "reflect"))
        assert same_bits(out_f32.cpu(), warp.warp_affine(src, case["matrix"], case["size"], "replicate", out="f32_chw"))


def read_all(path):
    return {name: open(os.path.join(path, name), "rb").read() for name in sorted(os.listdir(path))}


def test_tools_on_the_device_equal_the_host(tmp_path):
    src, good = flat_folder(str(tmp_path))
    lmk, tpl = make_landmarks(src, good)
    for gpu, tag in (("0", "dev"), ("-1", "host")):
        assert align_faces.main(["--lmk", lmk, "--template", tpl, "--size", "48", "--gpu", gpu, "--n_worker", "4",
                                 "--output", str(tmp_path / ("aligned_" + tag)), src]) == 0
        assert prepare_data.main(["--out", str(tmp_path / ("store_" + tag)), "--size", "16,32,64", "--format", "npy",
                                  "--gpu", gpu, "--n_worker", "4", "--align", lmk, "--template", tpl, src]) == 0
    for kind in ("aligned_", "store_"):
        dev, host = read_all(str(tmp_path / (kind + "dev"))), read_all(str(tmp_path / (kind + "host")))
        assert sorted(dev) == sorted(host) and len(host) >= 5
        for name in host:
            assert dev[name] == host[name], (kind, name)
    assert len(read_all(str(tmp_path / "store_host"))) == 3 * 5 + 1
    assert dataset.open_store(str(tmp_path / "store_dev")).get(b"length") == b"5"
