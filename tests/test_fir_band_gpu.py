"""Whole-row band kernels of the up-sampling layers' blur tail (csrc/upfirdn2d.hip k_fir4_band_fwd, k_fir4_band_nba_bwd).

The band kernels replace k_fir4_tile<true, false> and k_fir4_nba_bwd<true> where the 2^k side is at least 64 wide, the
pad is the up-sampling layers' and every pointer is 16-byte aligned; SR_FIR_BAND=0 keeps the tiled kernels.  Checked
here, on shapes small enough for a few seconds in all:
  * forward: bit for bit upfirdn2d followed by noise_bias_act, the numpy oracle's order, and the tiled kernel;
  * backward: the gradient bit for bit the two-kernel form and the tiled one-pass kernel; the three sums against float64
    at the bar of test_conv_gpu.test_upsampling_tail_backward_in_one_pass_equals_the_two_kernels (2e-6 of the sum of
    absolute products); a second run inside poisoned buffers (NaN scratch, NaN guards around every input and output:
    the first plane's band reads in front of the tensor, the last plane's behind it) bit-identical;
  * below the edge and on inputs shifted by 4 bytes: the tiled kernels, same bits;
  * Generator(64): image bit-identical with the switch unset and 0, parameter gradients at the bar of
    test_model_gpu.test_full_gradient_tensors_gpu_vs_own_cpu_path.
The switch is read once per process: the tiled kernels' results come from ONE child process shared by every test."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import poison
from util import bits_equal, kernel_ran, launched_kernels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE, GAIN = 0.2, math.sqrt(2.0)
# (b, c, H, W) of the wide (2^k + 1) side.  41 x 65: non-square, 41 rows do not divide by the band height, and the
# plane size is 1 mod 4: planes 0 - 3 start at the four 16-byte residues.  73 x 129: 72 / 73 rows over bands of 32.
SHAPES = [(2, 3, 41, 65), (1, 5, 73, 129), (3, 2, 65, 65)]
BIG = (1, 2, 257, 257)
NOISES = ("bnoise", "noise1", "nonoise")
CASES = [(s, nz, bias) for s in SHAPES for nz in NOISES for bias in (True, False)] + [(BIG, "bnoise", True)]


def _key(case):
    shape, nz, bias = case
    return "%s-%s-%s" % ("x".join(map(str, shape)), nz, "bias" if bias else "nobias")


def _blur():
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
    return (k1[None, :] * k1[:, None] / 64.0 * 4.0).to(DEV)


def _inputs(case):
    """Host tensors of one case (fixed by the case alone)."""
    (b, c, h, w), nz, bias = case
    g = torch.Generator().manual_seed(b * 1000003 + c * 10007 + h * 101 + w + NOISES.index(nz) * 7 + bias)
    oh, ow = h - 1, w - 1
    t = {"x": torch.randn(b, c, h, w, generator=g), "gy": torch.randn(b, c, oh, ow, generator=g)}
    t["noise"] = None if nz == "nonoise" else torch.randn(b if nz == "bnoise" else 1, 1, oh, ow, generator=g)
    t["nw"] = None if nz == "nonoise" else torch.randn(1, generator=g)
    t["bias"] = torch.randn(c, generator=g) if bias else None
    return t


def _dev(t):
    return {k: (None if v is None else v.to(DEV)) for k, v in t.items()}


def _forward(d, k):
    from stylerenderer_amd.op.fused_elem import _BlurNBA

    return _BlurNBA.apply(d["x"], k, (1, 1), d["noise"], d["nw"], d["bias"], SLOPE, GAIN)


def _backward(d, y, k, frozen=False):
    from stylerenderer_amd.op import conv as cv
    from stylerenderer_amd.op.upfirdn2d import flipped

    return cv._blur_nba_bwd(d["gy"], y, flipped(k), 1, tuple(d["x"].shape), d["noise"], d["nw"], d["bias"], SLOPE, GAIN,
                            not frozen)


def _run_case(case):
    d, k = _dev(_inputs(case)), _blur()
    y = _forward(d, k)
    g257, gb, gnw, rdot = _backward(d, y, k)
    return {"y": y, "g257": g257, "gb": gb, "gnw": gnw, "rdot": rdot}


def _model_run():
    """Generator(64), batch 2: image and every parameter gradient of <image, proj>."""
    from stylerenderer_amd import model, synth
    from test_model_cpu import noise_list

    g = model.Generator(64, 64, 2)
    synth.fill_state_dict(g.state_dict(), salt=5)
    noise = [n.to(DEV) for n in noise_list(g, 70)]
    g = g.to(DEV)
    z = torch.from_numpy(synth.det_normal((2, 64), 6)).to(DEV)
    proj = torch.from_numpy(synth.det_normal((2, 3, 64, 64), 7)).to(DEV)
    img, _ = g([z], noise=noise)
    params = dict(g.named_parameters())
    grads = torch.autograd.grad((img * proj).sum(), list(params.values()), allow_unused=True)
    out = {"image": img.detach()}
    out.update({"grad:" + n: o for n, o in zip(params, grads) if o is not None})
    return out


def _dump(path):
    """Everything the tests compare with, from the process this runs in (the child: SR_FIR_BAND=0)."""
    out = {}
    for case in CASES:
        out.update({_key(case) + "|" + n: v.cpu().numpy() for n, v in _run_case(case).items()})
    out.update({"model|" + n: v.cpu().numpy() for n, v in _model_run().items()})
    np.savez(path, **out)


_CHILD = r"""
import sys
sys.path[:0] = sys.argv[2:]
import test_fir_band_gpu as T
T._dump(sys.argv[1])
"""


@pytest.fixture(scope="module")
def tiled(tmp_path_factory):
    """The same calls with the switch off (the tiled kernels), computed once."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    dst = str(tmp_path_factory.mktemp("fir_band") / "tiled.npz")
    run = subprocess.run([sys.executable, "-c", _CHILD, dst, here, root, os.path.join(root, "oracle")],
                         env=dict(os.environ, SR_FIR_BAND="0"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    return dict(np.load(dst))


def _np(t):
    return t.detach().cpu().numpy()


def test_planes_of_the_41x65_case_start_at_all_four_residues():
    b, c, h, w = SHAPES[0]
    assert (h * w) % 4 == 1 and b * c >= 4
    assert {(p * h * w) % 4 for p in range(4)} == {0, 1, 2, 3}
    # and the narrow side's band geometry: 16 lanes per row, 16 lane rows of 4 rows: one band of 40, two of 20 / 21
    assert 4 * (256 // ((w - 1) // 4)) == 64


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_band_forward_bit_for_bit(case, tiled):
    import ops_np
    from stylerenderer_amd.op.fused_elem import noise_bias_act
    from stylerenderer_amd.op.upfirdn2d import upfirdn2d

    t = _inputs(case)
    d, k = _dev(t), _blur()
    y, names = launched_kernels(lambda: _forward(d, k))
    assert kernel_ran(names, "k_fir4_band_fwd") and not kernel_ran(names, "k_fir4_tile"), names
    assert bool(torch.isfinite(y).all())
    # the two operators (without a bias the fused kernels add 0.0f: a zero bias is the same arithmetic)
    bias = d["bias"] if d["bias"] is not None else torch.zeros(t["x"].shape[1], device=DEV)
    want = noise_bias_act(upfirdn2d(d["x"], k, pad=(1, 1)), d["noise"], d["nw"], bias, SLOPE, GAIN)
    assert torch.equal(y, want)
    # the numpy oracle's tap order, then the tail's order in float32: (f + nw * noise) + bias, select, gain
    f = ops_np.upfirdn2d(t["x"].numpy(), ops_np.make_blur_kernel((1, 3, 3, 1), 4.0), 1, 1, (1, 1))
    assert f.dtype == np.float32
    v = f
    if t["noise"] is not None:
        v = v + t["nw"].numpy()[0] * t["noise"].numpy()
    v = v + _np(bias)[None, :, None, None]
    oracle = np.where(v > 0, v, v * np.float32(SLOPE)) * np.float32(GAIN)
    assert oracle.dtype == np.float32 and bits_equal(_np(y), oracle)
    assert bits_equal(_np(y), tiled[_key(case) + "|y"])


def _check(got, want, mag, bar, what):
    got = got.detach().cpu().double()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    ratio = float(((got - want).abs() / (mag + 1e-30)).max())
    print("%s: %.3e of the absolute-product sum (bar %.1e)" % (what, ratio, bar))
    assert ratio <= bar, "%s: error %.3e of the absolute-product sum (bar %.1e)" % (what, ratio, bar)


@pytest.mark.parametrize("case", CASES, ids=_key)
def test_band_backward_gradient_sums_and_poisoned_rerun(case, tiled, monkeypatch):
    from stylerenderer_amd.op import conv as cv
    from stylerenderer_amd.op.upfirdn2d import flipped, upfirdn2d_op

    t = _inputs(case)
    d, k = _dev(t), _blur()
    b, c, h, w = case[0]
    oh, ow = h - 1, w - 1
    y = _forward(d, k)
    (g257, gb, gnw, rdot), names = launched_kernels(lambda: _backward(d, y, k))
    assert kernel_ran(names, "k_fir4_band_nba_bwd") and not kernel_ran(names, "k_fir4_nba_bwd"), names
    assert kernel_ran(names, "k_rowdot_finish") == (math.ceil(h / (4 * (256 // (ow // 4)))) > 1), names
    # gradient: the two-kernel form and the tiled one-pass kernel, bit for bit
    gm, gb0, gnw0, rdot0 = cv._nba_bwd_dot(d["gy"], y, d["noise"], d["nw"], d["bias"], SLOPE, GAIN, True)
    g0 = upfirdn2d_op(gm.reshape(-1, oh, ow, 1), flipped(k), 1, 1, 1, 1, 2, 2, 2, 2).view(b, c, h, w)
    assert torch.equal(g257, g0)
    assert bits_equal(_np(g257), tiled[_key(case) + "|g257"])
    # the three sums against float64 (as test_dispatch_edges_gpu holds the tiled kernel's)
    yd = y.cpu().double()
    nzd = torch.zeros(1, 1, oh, ow, dtype=torch.float64) if t["noise"] is None else t["noise"].double()
    nwd = torch.zeros(1, dtype=torch.float64) if t["nw"] is None else t["nw"].double()
    bd = torch.zeros(c, dtype=torch.float64) if t["bias"] is None else t["bias"].double()
    gpre = t["gy"].double() * torch.where(yd > 0, 1.0, SLOPE) * GAIN
    pre = torch.where(yd > 0, yd / GAIN, yd / (SLOPE * GAIN))
    blur = pre - nwd * nzd - bd[None, :, None, None]
    blur_mag = pre.abs() + (nwd * nzd).abs() + bd.abs()[None, :, None, None]
    _check(gb, gpre.sum((0, 2, 3)), gpre.abs().sum((0, 2, 3)), 2e-6, "gb")
    if t["noise"] is not None:
        _check(gnw, (gpre * nzd).sum().reshape(1), (gpre * nzd).abs().sum().reshape(1), 2e-6, "gnw")
    _check(rdot, (gpre * blur).sum((2, 3)), (gpre.abs() * blur_mag).sum((2, 3)), 2e-6, "rdot")
    # frozen parameters: NULL gbias / gnoise_w, same gradient and row-dots
    f257, fb, fnw, frdot = _backward(d, y, k, frozen=True)
    assert fb.numel() == 0 and fnw.numel() == 0 and torch.equal(f257, g257) and torch.equal(frdot, rdot)
    # again inside poisoned buffers: NaN scratch and outputs, NaN guards directly in front of the first plane and
    # behind the last plane of every input and output
    with poison.poisoned(monkeypatch) as log:
        pd = {n: (None if v is None else poison.embed(v, log)) for n, v in d.items()}
        pk = poison.embed(k, log)
        py = _forward(pd, pk)
        again = _backward(pd, py, pk)
    live = [v for v in pd.values() if v is not None]
    poison.check(log, [py] + [o for o in again if o.numel()], live + [pk])
    assert torch.equal(py, y)
    assert all(torch.equal(u, v) for u, v in zip(again, (g257, gb, gnw, rdot)))


def _shifted(t):
    buf = torch.empty(t.numel() + 1, device=DEV)
    buf[1:] = t.reshape(-1)
    return buf[1:].view(t.shape)


def test_below_the_edge_and_shifted_inputs_take_the_tiled_kernels():
    k = _blur()
    small = ((2, 3, 33, 33), "bnoise", True)                        # 32 wide: below the edge
    d = _dev(_inputs(small))

    def both(dd):
        yy = _forward(dd, k)
        return yy, _backward(dd, yy, k)

    _, names = launched_kernels(lambda: both(d))
    assert kernel_ran(names, "k_fir4_tile", "<true, false>") and kernel_ran(names, "k_fir4_nba_bwd", "<true>"), names
    assert not kernel_ran(names, "k_fir4_band_fwd") and not kernel_ran(names, "k_fir4_band_nba_bwd"), names
    # 65 wide, every tensor aligned: the bands; the input (forward) or the gradient (backward) 4 bytes off: the tiles
    case = (SHAPES[0], "bnoise", True)
    d = _dev(_inputs(case))
    y = _forward(d, k)
    want = _backward(d, y, k)
    ds = dict(d, x=_shifted(d["x"]), gy=_shifted(d["gy"]))
    assert ds["x"].data_ptr() % 16 == 4 and ds["gy"].data_ptr() % 16 == 4
    (ys, got), names = launched_kernels(lambda: (_forward(ds, k), _backward(ds, y, k)))
    assert kernel_ran(names, "k_fir4_tile", "<true, false>") and kernel_ran(names, "k_fir4_nba_bwd", "<false>"), names
    assert not kernel_ran(names, "k_fir4_band_fwd") and not kernel_ran(names, "k_fir4_band_nba_bwd"), names
    assert torch.equal(ys, y) and torch.equal(got[0], want[0])


def test_generator_64_image_bit_identical_and_gradients_at_the_model_bar(tiled):
    got, names = launched_kernels(_model_run)
    # the 32 -> 64 up-sampling layer is on the band path, forward and backward
    assert sum("k_fir4_band_fwd" in n for n in names) >= 1, names
    assert sum("k_fir4_band_nba_bwd" in n for n in names) >= 1, names
    assert bits_equal(_np(got["image"]), tiled["model|image"])
    keys = sorted(k for k in got if k.startswith("grad:"))
    assert keys == sorted(k[len("model|"):] for k in tiled if k.startswith("model|grad:")) and len(keys) > 20
    for n in keys:
        want = tiled["model|" + n]
        scale = float(np.abs(want).max())
        # test_full_gradient_tensors_gpu_vs_own_cpu_path: 2e-5 of the tensor's scale, 5x for the scalar noise strengths
        bar = 2e-5 * (5 if want.size == 1 else 1)
        err = float(np.abs(_np(got[n]).astype(np.float64) - want).max())
        assert err <= bar * scale + 1e-9, "%s: |err| %.3e = %.3e of the tensor's scale (bar %.1e)" % (
            n, err, err / max(scale, 1e-30), bar)
