"""GPU: the texture look-up kernels (csrc/texture_sample.hip) against the host float32 definition of op.texture, bit for
bit — forward, the uv map's gradient, the texture's gradient; tapless texels in poisoned memory; reruns; float64; graph
capture with a prebuilt tap list; `uv_map` on the device; `reconstruct` with the render flags on the device."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, graphs, model, synth
from stylerenderer_amd.op import texture
from test_texture_cpu import scene_batch
from test_texture_sample_cpu import SHIFTS, float64_bound, float64_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


# ---- the cases and their host reference, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_map(isize, b_n):
    """The uv map of the shifted exact scenes at isize^2 (uncovered pixels, border-clamped taps at the charts' outer
    edges), with the special values written over its first pixels: NaN, infinity, outside [0, 1], exactly 0 and 1."""
    v, _, tri, uv, tri_uv = scene_batch(SHIFTS[:b_n])
    uvmap, cover = texture.uv_map(v, tri, uv, tri_uv, isize)
    uvmap, cover = uvmap.clone(), cover.clone()
    cover[0, 0, :6] = True
    uvmap[0, 0, 0] = torch.tensor([float("nan"), 0.5])
    uvmap[0, 0, 1] = torch.tensor([0.5, float("-inf")])
    uvmap[0, 0, 2] = torch.tensor([-0.3, 1.4])
    uvmap[0, 0, 3] = torch.tensor([1.7, -0.2])
    uvmap[0, 0, 4] = torch.tensor([0.0, 1.0])
    uvmap[0, 0, 5] = torch.tensor([1.0, 0.0])
    return uvmap, cover


@functools.lru_cache(maxsize=None)
def host_case(tsize, isize, b_n, c_n, bt):
    """(tex, uvmap, cover, g, out, gtex, guv): the inputs and the host float32 composite's results."""
    uvmap, cover = host_map(isize, b_n)
    seed = 100 + 7 * tsize[1] + isize
    tex = torch.from_numpy(synth.det_uniform((bt, c_n) + tsize, seed).astype(np.float32))
    g = torch.from_numpy(synth.det_uniform((b_n, c_n, isize, isize), seed + 1).astype(np.float32))
    t, m = tex.clone().requires_grad_(True), uvmap.clone().requires_grad_(True)
    out = texture.sample_composite(t, m, cover, 0.25)
    gtex, guv = torch.autograd.grad(out, (t, m), g)
    return tex, uvmap, cover, g, out.detach(), gtex, guv


def device_run(tex, uvmap, cover, g, background=0.25):
    t, m = tex.to(DEV).requires_grad_(True), uvmap.to(DEV).requires_grad_(True)
    out = texture.sample(t, m, cover.to(DEV), background)
    gtex, guv = torch.autograd.grad(out, (t, m), g.to(DEV))
    return out.detach(), gtex, guv


def tapless(uvmap, cover, tsize, bt):
    off, _ = texture.tap_plan(uvmap, cover, tsize, bt)
    n = bt * tsize[0] * tsize[1]
    return (off[1:n + 1] == off[:n]).view(bt, 1, *tsize)


# ---- bit for bit -------------------------------------------------------------------------------------------------------
# (8, 8): 16-byte stores of the bake's kind; (33, 65) at 16^2: minification, most texels without taps; (4, 4) at 33^2:
# magnification, tap lists of hundreds of entries.  16: the 16-byte path; 33: the scalar path with a tail.
@pytest.mark.parametrize("tsize", [(8, 8), (33, 65), (4, 4)])
@pytest.mark.parametrize("isize", [16, 33])
def test_sample_equals_the_host_bit_for_bit(tsize, isize):
    for b_n in (1, 3):
        for c_n in (1, 3):
            for bt in sorted({1, b_n}):
                tex, uvmap, cover, g, want, want_t, want_uv = host_case(tsize, isize, b_n, c_n, bt)
                out, gtex, guv = device_run(tex, uvmap, cover, g)
                assert out.is_cuda and tuple(out.shape) == (b_n, c_n, isize, isize)
                assert tuple(gtex.shape) == tuple(tex.shape) and tuple(guv.shape) == tuple(uvmap.shape)
                bad = (int((out.cpu() != want).sum()), int((guv.cpu() != want_uv).sum()), int((gtex.cpu() != want_t).sum()))
                print("sample", tsize, isize, "B", b_n, "C", c_n, "Bt", bt, "mismatches (out, grad_uv, grad_tex)", bad,
                      "uncovered", int((~cover).sum()), "tapless texels", int(tapless(uvmap, cover, tsize, bt).sum()))
                assert torch.equal(out.cpu(), want), bad
                assert torch.equal(guv.cpu(), want_uv), bad
                assert torch.equal(gtex.cpu(), want_t), bad
    # what the shapes are there for
    uvmap, cover = host_map(isize, 3)
    assert 0 < int((~cover).sum()) < cover.numel()
    empty = tapless(uvmap, cover, tsize, 1)
    if tsize == (33, 65) and isize == 16:
        assert int(empty.sum()) > 0.5 * empty.numel()
    if tsize == (4, 4):
        assert int(empty.sum()) == 0
    sx = uvmap[..., 0][cover] * tsize[1] - 0.5
    assert bool(((sx < 0) & (sx >= -1)).any())                               # border-clamped taps


def test_tapless_texels_are_zero_in_poisoned_memory_and_reruns_are_equal():
    tsize, isize = (33, 65), 16
    tex, uvmap, cover, g, want, want_t, _ = host_case(tsize, isize, 3, 3, 1)
    empty = tapless(uvmap, cover, tsize, 1).expand(1, 3, -1, -1)
    assert int(empty.sum()) > 0
    t, m, c, gd = tex.to(DEV).requires_grad_(True), uvmap.to(DEV), cover.to(DEV), g.to(DEV)
    out = texture.sample(t, m, c, 0.25)
    junk = torch.full(tuple(tex.shape), float("nan"), device=DEV)           # fill, free, call: the block comes back
    torch.cuda.synchronize()
    del junk
    (gtex,) = torch.autograd.grad(out, t, gd)
    assert bool(torch.isfinite(gtex).all())
    assert bool((gtex.cpu()[empty] == 0).all())
    assert torch.equal(gtex.cpu(), want_t)
    junk = torch.full(tuple(want.shape), float("nan"), device=DEV)
    torch.cuda.synchronize()
    del junk
    assert torch.equal(texture.sample(t.detach(), m, c, 0.25).cpu(), want)
    first = device_run(tex, uvmap, cover, g)
    second = device_run(tex, uvmap, cover, g)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


def test_float64_is_refused_under_strict_native():
    tex, uvmap, cover, _, _, _, _ = host_case((8, 8), 16, 1, 1, 1)
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        texture.sample(tex.double().to(DEV), uvmap.double().to(DEV), cover.to(DEV))


# ---- float64 -----------------------------------------------------------------------------------------------------------
def test_sample_against_float64():
    tex, uvmap, cover, d = float64_case(torch.float32, DEV)
    tex64, uv64, cover64, _ = float64_case(torch.float64)
    out = texture.sample(tex, uvmap, cover, -1.0).cpu()
    out64 = texture.sample(tex64, uv64, cover64, -1.0)
    agree = cover.cpu() == cover64
    on = agree & cover64
    err = float((out.double() - out64).permute(1, 0, 2, 3)[:, on].abs().max())
    print("float64: error", err, "bound", float64_bound(d), "pixels left out", int((~agree).sum()), "of", agree.numel())
    assert int((~agree).sum()) <= 0.005 * agree.numel()
    assert int(on.sum()) > 0.3 * on.numel()
    assert err <= float64_bound(d)


# ---- uv_map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [16, 33, (12, 16)])
def test_uv_map_on_the_device_is_the_hosts(size):
    v, _, tri, uv, tri_uv = scene_batch(SHIFTS)
    want, want_c = texture.uv_map(v, tri, uv, tri_uv, size)
    got, got_c = texture.uv_map(v.to(DEV), tri.to(DEV), uv.to(DEV), tri_uv, size)
    assert got.is_cuda and got_c.dtype == torch.bool
    assert torch.equal(got_c.cpu(), want_c) and torch.equal(got.cpu(), want)
    # a curved mesh with a layout that leaves faces out
    v0, tri0 = synth.uv_ellipsoid(16, 14)
    uv0, tri_uv0, keep = face_model.uv_layout(v0, tri0)
    vp = torch.from_numpy(synth.random_poses(v0, 2)).float()
    tri_t = torch.from_numpy(tri0)
    want, want_c = texture.uv_map(vp, tri_t, uv0, tri_uv0, size, keep)
    got, got_c = texture.uv_map(vp.to(DEV), tri_t.to(DEV), uv0.to(DEV), tri_uv0, size, keep.to(DEV))
    print("uv_map", size, "mismatches (cover, uv)", int((got_c.cpu() != want_c).sum()), int((got.cpu() != want).sum()))
    assert torch.equal(got_c.cpu(), want_c) and torch.equal(got.cpu(), want)
    assert 0 < int(want_c.sum()) < want_c.numel()


# ---- capture -----------------------------------------------------------------------------------------------------------
def test_sample_forward_and_backward_under_graph_capture():
    tex, uvmap, cover, g, _, _, _ = host_case((33, 65), 33, 3, 3, 1)
    t = tex.to(DEV).requires_grad_(True)
    m = uvmap.to(DEV).requires_grad_(True)
    c, gd = cover.to(DEV), g.to(DEV)
    texture.tap_plan(m, c, (33, 65), 1)                                     # the list is built before the capture
    torch.cuda.synchronize()
    out = {}

    def body():
        y = texture.sample(t, m, c, 0.25)
        out["gtex"], out["guv"] = torch.autograd.grad(y, (t, m), gd)
        out["y"] = y.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    for k in range(2):
        with torch.no_grad():
            t.copy_(torch.from_numpy(synth.det_uniform(tuple(tex.shape), 300 + k).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = {name: x.clone() for name, x in out.items()}
        y = texture.sample(t, m, c, 0.25)
        gtex, guv = torch.autograd.grad(y, (t, m), gd)
        assert torch.equal(got["y"], y.detach()) and torch.equal(got["gtex"], gtex) and torch.equal(got["guv"], guv)
    assert float(gtex.abs().max()) > 0 and float(guv.abs().max()) > 0


# ---- command line ------------------------------------------------------------------------------------------------------
def test_reconstruct_cli_with_the_render_flags_on_the_device(tmp_path):
    g = model.GeneratorWithMap(32, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_b.npy")
    np.save(img, synth.det_uniform((32, 32, 3), 19))                     # HWC
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "32", "--steps", "4", "--n_mean_latent", "64",
           "--texture", "64", "--texture_check", "--turntable", "3", "--texture_refine", "4", "--out", out, ckpt, img]
    env = dict(os.environ, PYTHONPATH=ROOT, SR_STRICT_NATIVE="1")
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(
        ["face_b.obj", "face_b_canonical.obj", "face_b_render.png", "face_b_normal.png", "face_b.npz",
         "face_b_texture.png", "face_b_texture_weight.png", "face_b_textured.obj", "face_b_textured.mtl",
         "face_b_rerender.png", "face_b_turn_00.png", "face_b_turn_01.png", "face_b_turn_02.png"])
    r = np.load(os.path.join(out, "face_b.npz"))
    assert r["texture_refine_loss"].shape == (4,) and np.isfinite(r["texture_refine_loss"]).all()
    assert 0 < int(r["rerender_counted"]) <= int(r["rerender_covered"]) <= 32 * 32
    assert 0 <= float(r["rerender_error"]) <= 2 and 0 <= float(r["rerender_error_before"]) <= 2
