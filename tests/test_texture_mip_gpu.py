"""GPU: the mip-mapped look-up's kernels (csrc/texture_mip.hip) against the host float32 definitions of op.texture, bit for
bit — the pyramid and its gradient, the level of detail, the look-up with both gradients, the chain down to the texture;
full writes into poisoned buffers; reruns; lod 0 against the plain sampler; graph capture with a prebuilt lod and tap list;
float64 under strict mode; `reconstruct --texture_mip` on the device."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import graphs, model, synth
from stylerenderer_amd.op import texture
from stylerenderer_amd.op._dispatch import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (8, 8): four levels down to 1 x 1; (12, 20): three levels, odd top; (33, 65): one level; (72, 40): 3 x 2 tiles of the
# build kernel with partial tiles, four levels; (128, 64): seven levels, so two build launches, and a 2 x 1 top
TSIZES = [(8, 8), (12, 20), (33, 65), (72, 40), (128, 64)]
ISIZES = [16, 33]                          # 16: the 16-byte path; 33: scalar stores, a tail, unaligned rows
COMBOS = [(1, 1, 1), (1, 3, 1), (3, 1, 1), (3, 1, 3), (3, 3, 1), (3, 3, 3)]          # (B, C, Bt)


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


# ---- the cases and their host reference, computed once -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_map(isize, b_n):
    """A uv map whose density changes across the picture (u = 1/2 + 0.62 t |t| over t in [-1, 1]: magnified in the middle,
    minified towards the sides, beyond [0, 1] at the rim, so border-clamped taps and positions past the clamp), at another
    scale per sample, with the right third moved into a far chart (a seam), holes in the cover and the special values
    written over its first pixels: NaN, infinity, numbers whose difference overflows."""
    n = isize
    t = (torch.arange(n, dtype=torch.float64) + 0.5) / n * 2 - 1
    r = torch.from_numpy(synth.det_uniform((b_n, n, n, 2), 500 + n)).double()
    maps = []
    for b in range(b_n):
        scale = (0.62, 0.2, 1.4)[b]
        u = 0.5 + scale * (t * t.abs()).view(1, n).expand(n, n) + 0.004 * r[b, ..., 0]
        v = 0.5 - scale * 0.8 * t.view(n, 1).expand(n, n) + 0.004 * r[b, ..., 1]
        u = torch.where(torch.arange(n).view(1, n) >= (2 * n) // 3, u - 0.45, u)
        maps.append(torch.stack((u, v), -1))
    uvmap = torch.stack(maps).float().contiguous()
    cover = torch.from_numpy(synth.det_uniform((b_n, n, n), 501 + n)) > -0.6
    cover[0, 0, :6] = True
    uvmap[0, 0, 0] = torch.tensor([float("nan"), 0.5])
    uvmap[0, 0, 1] = torch.tensor([0.5, float("-inf")])
    uvmap[0, 0, 2] = torch.tensor([3e38, -3e38])
    uvmap[0, 0, 3] = torch.tensor([-3e38, 3e38])
    uvmap[0, 0, 4] = torch.tensor([0.0, 1.0])
    uvmap[0, 0, 5] = torch.tensor([1.0, 0.0])
    return uvmap, cover


@functools.lru_cache(maxsize=None)
def host_case(tsize, isize, b_n, c_n, bt):
    """The inputs and the host float32 composite's results, as a dict."""
    uvmap, cover = host_map(isize, b_n)
    seed = 700 + 7 * tsize[1] + isize
    tex = torch.from_numpy(synth.det_uniform((bt, c_n) + tsize, seed).astype(np.float32))
    g = torch.from_numpy(synth.det_uniform((b_n, c_n, isize, isize), seed + 1).astype(np.float32))
    layout = texture.mip_layout(tsize)
    p = layout[-1][0] + layout[-1][1] * layout[-1][2]
    gp = torch.from_numpy(synth.det_uniform((bt, c_n, p), seed + 2).astype(np.float32))
    t, m = tex.clone().requires_grad_(True), uvmap.clone().requires_grad_(True)
    pyr = texture.mip_build_composite(t)
    (build_g,) = torch.autograd.grad(pyr, t, gp, retain_graph=True)
    lod = texture.mip_lod_composite(uvmap, cover, tsize)
    q = pyr.detach().clone().requires_grad_(True)
    out = texture.mip_sample_composite(q, tsize, m, cover, lod, 0.25)
    gpyr, guv = torch.autograd.grad(out, (q, m), g)
    (gtex,) = torch.autograd.grad(pyr, t, gpyr)
    return dict(tex=tex, uvmap=uvmap, cover=cover, g=g, gp=gp, layout=layout, pyr=pyr.detach(), build_g=build_g, lod=lod,
                out=out.detach(), gpyr=gpyr, guv=guv, gtex=gtex)


def device_case(case, tsize):
    t, m = case["tex"].to(DEV).requires_grad_(True), case["uvmap"].to(DEV).requires_grad_(True)
    c = case["cover"].to(DEV)
    pyr = texture.mip_build(t)
    (build_g,) = torch.autograd.grad(pyr, t, case["gp"].to(DEV), retain_graph=True)
    lod = texture.mip_lod(m.detach(), c, tsize)
    q = pyr.detach().clone().requires_grad_(True)
    out = texture.mip_sample(q, tsize, m, c, lod, 0.25)
    gpyr, guv = torch.autograd.grad(out, (q, m), case["g"].to(DEV))
    # the chain, as `sample_mip` runs it
    chained = texture.sample_mip(t, m, c, background=0.25)
    (gtex,) = torch.autograd.grad(chained, t, case["g"].to(DEV))
    return dict(pyr=pyr.detach(), build_g=build_g, lod=lod, out=out.detach(), gpyr=gpyr, guv=guv, gtex=gtex,
                chained=chained.detach())


NAMES = ("pyr", "build_g", "lod", "out", "guv", "gpyr", "gtex")


# ---- bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tsize", TSIZES)
@pytest.mark.parametrize("isize", ISIZES)
def test_mip_equals_the_host_bit_for_bit(tsize, isize):
    for b_n, c_n, bt in COMBOS:
        case = host_case(tsize, isize, b_n, c_n, bt)
        got = device_case(case, tsize)
        assert all(got[k].is_cuda for k in NAMES)
        bad = {k: int((got[k].cpu() != case[k]).sum()) for k in NAMES}
        bad["chained"] = int((got["chained"].cpu() != case["out"]).sum())
        print("mip", tsize, isize, "B", b_n, "C", c_n, "Bt", bt, "mismatches", bad)
        for k in NAMES:
            assert tuple(got[k].shape) == tuple(case[k].shape), k
            assert torch.equal(got[k].cpu(), case[k]), (k, bad)
        assert torch.equal(got["chained"].cpu(), case["out"]), bad
    # what the shapes and the map are there for
    case = host_case(tsize, isize, 3, 3, 1)
    lod, cover, uvmap = case["lod"], case["cover"], case["uvmap"]
    n_l = len(case["layout"])
    assert 0 < int((~cover).sum()) < cover.numel()
    assert float(lod[0, 0, 2]) == n_l - 1 and float(lod[0, 0, 3]) == n_l - 1 and float(lod[0, 0, 0]) == 0
    assert bool(torch.isfinite(case["out"]).all()) and bool(torch.isfinite(case["guv"]).all())
    assert bool(torch.isfinite(case["gpyr"]).all())
    if n_l > 1:
        levels = set(torch.floor(lod[cover]).long().tolist())
        frac = lod[cover] - torch.floor(lod[cover])
        assert len(levels) >= min(n_l, 3), levels                                # several levels in play
        assert int((frac != 0).sum()) > 0 and int((frac == 0).sum()) > 0         # trilinear and one-level pixels
    else:
        assert bool((lod == 0).all())
    sx = uvmap[..., 0][cover] * tsize[1] - 0.5
    assert bool(((sx < 0) & (sx >= -1)).any()) or bool((sx < -1).any())      # border-clamped taps


# ---- full writes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tsize,isize", [((72, 40), 16), ((128, 64), 33), ((33, 65), 33)])
def test_every_output_is_written_in_full_into_poisoned_buffers(tsize, isize):
    b_n, c_n, bt = 3, 3, 1
    case = host_case(tsize, isize, b_n, c_n, bt)
    layout = case["layout"]
    n_l, p = len(layout), case["pyr"].shape[2]
    th, tw = tsize
    tex, uvmap, cover, g = (case[k].to(DEV).contiguous() for k in ("tex", "uvmap", "cover", "g"))
    nan = float("nan")
    run = native(tex)
    pyr = torch.full((bt, c_n, p), nan, device=DEV)
    run.sr_mip_build_fwd(pyr, tex, bt * c_n, th, tw, n_l)
    assert torch.equal(pyr.cpu(), case["pyr"])                                   # (NaN anywhere would differ)
    gtex = torch.full(tuple(tex.shape), nan, device=DEV)
    run.sr_mip_build_bwd(gtex, case["gp"].to(DEV), bt, c_n, th, tw, n_l)
    assert torch.equal(gtex.cpu(), case["build_g"])
    lod = torch.full((b_n, isize, isize), nan, device=DEV)
    run.sr_mip_lod(lod, uvmap, cover, b_n, isize, isize, th, tw, n_l, 0.0)
    assert torch.equal(lod.cpu(), case["lod"])
    dims = (b_n, bt, c_n, isize, isize, th, tw, n_l)
    out = torch.full((b_n, c_n, isize, isize), nan, device=DEV)
    run.sr_mip_sample_fwd(out, pyr, uvmap, cover, lod, *dims, 0.25)
    assert torch.equal(out.cpu(), case["out"])
    guv = torch.full(tuple(uvmap.shape), nan, device=DEV)
    run.sr_mip_sample_bwd_uv(guv, g, pyr, uvmap, cover, lod, *dims)
    assert torch.equal(guv.cpu(), case["guv"])
    off, entries = texture.mip_tap_plan(uvmap, cover, lod, tsize, None, bt)
    gpyr = torch.full((bt, c_n, p), nan, device=DEV)
    run.sr_mip_sample_bwd_pyr(gpyr, g, uvmap, cover, lod, off, entries, *dims)
    assert torch.equal(gpyr.cpu(), case["gpyr"])
    empty = (off[1:bt * p + 1] == off[:bt * p]).view(bt, 1, p).expand(bt, c_n, p).cpu()
    assert int(empty.sum()) > 0
    assert bool((gpyr.cpu()[empty] == 0).all())                                  # tapless elements: exactly 0
    # the chain's level-0 texels without a tap in any level above them take exactly 0 as well
    t = tex.clone().requires_grad_(True)
    (chain_g,) = torch.autograd.grad(texture.sample_mip(t, uvmap, cover, background=0.25), t, g)
    assert torch.equal(chain_g.cpu(), case["gtex"]) and bool(torch.isfinite(chain_g).all())
    if n_l == 1:
        assert int((chain_g == 0).sum()) > 0


def test_reruns_are_bit_identical():
    case = host_case((72, 40), 33, 3, 3, 3)
    first, second = device_case(case, (72, 40)), device_case(case, (72, 40))
    for k in first:
        assert torch.equal(first[k], second[k]), k


def test_lod_zero_on_the_device_is_the_device_sampler():
    for tsize, isize in (((12, 20), 33), ((128, 64), 16)):
        case = host_case(tsize, isize, 3, 3, 1)
        t, m = case["tex"].to(DEV).requires_grad_(True), case["uvmap"].to(DEV).requires_grad_(True)
        c, g = case["cover"].to(DEV), case["g"].to(DEV)
        want = texture.sample(t, m, c, 0.25)
        want_t, want_uv = torch.autograd.grad(want, (t, m), g)
        got = texture.sample_mip(t, m, c, lod=torch.zeros(tuple(c.shape), device=DEV), background=0.25)
        got_t, got_uv = torch.autograd.grad(got, (t, m), g)
        assert torch.equal(got, want) and torch.equal(got_uv, want_uv) and torch.equal(got_t, want_t)
        assert float(got_t.abs().max()) > 0


def test_float64_is_refused_under_strict_native():
    case = host_case((8, 8), 16, 1, 1, 1)
    tex, uvmap, cover = case["tex"].double().to(DEV), case["uvmap"].double().to(DEV), case["cover"].to(DEV)
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        texture.mip_build(tex)
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        texture.mip_lod(uvmap, cover, (8, 8))
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        texture.mip_sample(case["pyr"].double().to(DEV), (8, 8), uvmap, cover, case["lod"].double().to(DEV))
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        texture.sample_mip(tex, uvmap, cover)


# ---- capture -----------------------------------------------------------------------------------------------------------
def test_build_and_look_up_with_both_backwards_under_graph_capture():
    tsize = (128, 64)
    case = host_case(tsize, 33, 3, 3, 1)
    t = case["tex"].to(DEV).requires_grad_(True)
    m = case["uvmap"].to(DEV).requires_grad_(True)
    c, gd = case["cover"].to(DEV), case["g"].to(DEV)
    lod = texture.mip_lod(m.detach(), c, tsize)                               # the lod and the list: before the capture
    texture.mip_tap_plan(m, c, lod, tsize, None, 1)
    torch.cuda.synchronize()
    out = {}

    def body():
        y = texture.mip_sample(texture.mip_build(t), tsize, m, c, lod, 0.25)
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
            t.copy_(torch.from_numpy(synth.det_uniform(tuple(case["tex"].shape), 900 + k).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = {name: x.clone() for name, x in out.items()}
        y = texture.mip_sample(texture.mip_build(t), tsize, m, c, lod, 0.25)
        gtex, guv = torch.autograd.grad(y, (t, m), gd)
        assert torch.equal(got["y"], y.detach()) and torch.equal(got["gtex"], gtex) and torch.equal(got["guv"], guv)
    assert float(gtex.abs().max()) > 0 and float(guv.abs().max()) > 0


# ---- command line ------------------------------------------------------------------------------------------------------
def test_reconstruct_cli_with_texture_mip_on_the_device(tmp_path):
    g = model.GeneratorWithMap(32, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_b.npy")
    np.save(img, synth.det_uniform((32, 32, 3), 19))                     # HWC
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "32", "--steps", "4", "--n_mean_latent", "64",
           "--texture", "64", "--texture_check", "--turntable", "2", "--texture_refine", "2", "--texture_mip",
           "--out", out, ckpt, img]
    env = dict(os.environ, PYTHONPATH=ROOT, SR_STRICT_NATIVE="1")
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(
        ["face_b.obj", "face_b_canonical.obj", "face_b_render.png", "face_b_normal.png", "face_b.npz",
         "face_b_texture.png", "face_b_texture_weight.png", "face_b_textured.obj", "face_b_textured.mtl",
         "face_b_rerender.png", "face_b_turn_00.png", "face_b_turn_01.png"])
    r = np.load(os.path.join(out, "face_b.npz"))
    assert float(r["texture_mip"]) == 0.0
    assert r["texture_refine_loss"].shape == (2,) and np.isfinite(r["texture_refine_loss"]).all()
    assert 0 < int(r["rerender_counted"]) <= int(r["rerender_covered"]) <= 32 * 32
    assert 0 <= float(r["rerender_error"]) <= 2 and 0 <= float(r["rerender_error_before"]) <= 2
