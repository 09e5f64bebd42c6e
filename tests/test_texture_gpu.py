"""GPU: the texture kernels (csrc/texture.hip) against the host float32 definitions of op.texture, bit for bit; the
ordinary case against float64; a round trip through the rasterizer; bake and padding under graph capture; `reconstruct
--texture` on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, graphs, model, synth
from stylerenderer_amd.op import texture
from stylerenderer_amd.op.rasterize import rasterize
from test_texture_cpu import (affine_picture, decisions_differ, expected_weight, ordinary_case, pad_case, scene_batch)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = [(0.0, 0.0), (0.5, 0.125), (-0.3, -0.6)]                        # the samples of a batch are shifted copies


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


# ---- the exact scene -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(8, 8), (33, 65)])                     # 8: the 16-byte stores; 65: scalar, with a tail
@pytest.mark.parametrize("batch", [1, 3])
def test_bake_equals_the_host_bit_for_bit_on_the_exact_scene(size, batch):
    v, n, tri, uv, tri_uv = scene_batch(SHIFTS[:batch])
    face, coeff = texture.texel_map(uv, tri_uv, size)
    zbuf = texture.depth_buffer(v, tri, (48, 64))
    zbuf_d = texture.depth_buffer(v.to(DEV), tri.to(DEV), (48, 64))
    assert torch.equal(zbuf_d.cpu(), zbuf)
    face_d, coeff_d = face.to(DEV), coeff.to(DEV)
    for psize in ((5, 7), (48, 64)):
        for c_n in (1, 3):
            img = affine_picture(c_n, *psize, batch=batch)
            want_t, want_w = texture.bake(v, n, tri, face, coeff, img, zbuf, facing=(0.0, 0.5), z_bias=1.0 / 64)
            tex, weight = texture.bake(v.to(DEV), n.to(DEV), tri.to(DEV), face_d, coeff_d, img.to(DEV), zbuf_d,
                                       facing=(0.0, 0.5), z_bias=1.0 / 64)
            assert tex.is_cuda and tuple(tex.shape) == (batch, c_n) + size and tuple(weight.shape) == (batch, 1) + size
            bad_w = int((weight.cpu() != want_w).sum())
            bad_t = int((tex.cpu() != want_t).sum())
            print("exact scene", size, batch, psize, c_n, "weight mismatches", bad_w, "tex mismatches", bad_t)
            assert torch.equal(weight.cpu(), want_w), (psize, c_n, bad_w)
            assert torch.equal(tex.cpu(), want_t), (psize, c_n, bad_t)
    # and the closed form, on the device's own result
    for s in range(batch):
        want, sure = expected_weight(face, size, SHIFTS[s], (48, 64), (48, 64))
        assert torch.equal(weight[s, 0].cpu()[sure].double(), want[sure])


# ---- the ordinary case -----------------------------------------------------------------------------------------------
def test_bake_on_the_ordinary_case_against_float64():
    args, d, _ = ordinary_case(torch.float32, DEV)
    args32, _, _ = ordinary_case(torch.float32)
    args64, _, _ = ordinary_case(torch.float64)
    assert torch.equal(args["face"].cpu(), args32["face"]) and torch.equal(args["coeff"].cpu(), args32["coeff"])
    assert torch.equal(args["zbuf"].cpu(), args32["zbuf"])
    differ, live, p64 = decisions_differ(args32, args64)
    n_live = int(live.sum()) * differ.shape[0]
    assert int(differ.sum()) <= 0.005 * n_live
    tex, weight = texture.bake(**args)
    bound = d * (48 + 64) * 2.0 ** -22 + 2.0 ** -22
    same = ~differ
    err_w = float((weight.cpu().double() - p64[1])[:, 0][same].abs().max())
    err_t = float((tex.cpu().double() - p64[0]).permute(1, 0, 2, 3)[:, same].abs().max())
    host_t, host_w = texture.bake(**args32)
    bad = (int((weight.cpu() != host_w).sum()), int((tex.cpu() != host_t).sum()))
    print("ordinary case: |weight - f64|", err_w, "|tex - f64|", err_t, "bound", bound, "differing decisions",
          int(differ.sum()), "of", n_live, "mismatches with the host float32 (weight, tex)", bad)
    assert err_w <= bound and err_t <= bound
    assert int(((weight.cpu() > 0) & same.unsqueeze(1)).sum()) > 0.1 * n_live
    # the host float32 definition, bit for bit: every operation is matched (division and square root included)
    assert torch.equal(weight.cpu(), host_w) and torch.equal(tex.cpu(), host_t), bad
    again_t, again_w = texture.bake(**args)                                 # reruns give the same bits
    assert torch.equal(again_t, tex) and torch.equal(again_w, weight)


@pytest.mark.parametrize("size", [(33, 65), 128])
def test_texel_map_on_the_device_is_the_hosts(size):
    v0, tri = synth.uv_ellipsoid(16, 14)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    face, coeff = texture.texel_map(uv, tri_uv, size, keep)
    uv_d = uv.to(DEV)
    face_d, coeff_d = texture.texel_map(uv_d, tri_uv, size, keep)
    assert face_d.is_cuda and face_d.dtype == torch.int32 and coeff_d.dtype == torch.float32
    assert torch.equal(face_d.cpu(), face) and torch.equal(coeff_d.cpu(), coeff)
    assert 0.5 < float((face >= 0).double().mean()) < 1 and int(face.max()) < tri.shape[0]
    assert not bool(keep[face[face >= 0].long()].logical_not().any())       # no seam face in the map


# ---- padding ---------------------------------------------------------------------------------------------------------
def pad_samples():
    """tex [4, 3, 33, 65], weight: sparse, nearly full, one texel, empty."""
    shape = (4, 3, 33, 65)
    tex = torch.from_numpy(synth.det_uniform(shape, 61).astype(np.float32))
    r = torch.from_numpy(synth.det_uniform((4, 1, 33, 65), 62))
    weight = torch.zeros(4, 1, 33, 65)
    weight[0] = (r[0] > 0.9).float() * 0.5
    weight[1] = (r[1] > -0.96).float()
    weight[2, 0, 20, 64] = 0.125                                             # in the last column
    return tex * (weight > 0), weight


@pytest.mark.parametrize("passes", [1, 3, 8, 64])
def test_pad_equals_the_host_bit_for_bit(passes):
    tex, weight = pad_samples()
    assert 0 < int((weight[0] > 0).sum()) < 400 and 0 < int((weight[1] == 0).sum()) < 200
    want, want_f = texture.pad(tex, weight, passes)
    tex_d, weight_d = tex.to(DEV), weight.to(DEV)
    got, filled = texture.pad(tex_d, weight_d, passes)
    assert got.is_cuda and filled.dtype == torch.uint8 and tuple(filled.shape) == tuple(weight.shape)
    assert torch.equal(filled.cpu(), want_f) and torch.equal(got.cpu(), want)
    assert torch.equal(tex_d.cpu(), tex) and torch.equal(weight_d.cpu(), weight)           # inputs untouched
    assert int(filled[3].sum()) == 0 and bool((got[3] == 0).all())
    small_t, small_w = pad_case("sparse")                                    # (9, 11), two samples
    got_s, filled_s = texture.pad(small_t.to(DEV), small_w.to(DEV), passes)
    want_s = texture.pad(small_t, small_w, passes)
    assert torch.equal(got_s.cpu(), want_s[0]) and torch.equal(filled_s.cpu(), want_s[1])


# ---- round trip through the rasterizer -------------------------------------------------------------------------------
def test_bake_recovers_a_rendered_attribute():
    """A picture rendered by op.rasterize from a per-vertex attribute that is affine in the layout's uv; baking it must
    give that affine function back at every texel that is seen, up to the picture's own pixel-to-pixel step."""
    v0, tri = synth.uv_ellipsoid(16, 14)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    abc = torch.tensor([[0.8, -0.3, 0.1], [-0.5, 0.6, 0.2], [0.2, 0.9, -0.4]], dtype=torch.float64)
    attr = (uv.double() @ abc[:, :2].t() + abc[:, 2]).float()                # [nv, 3]
    v = torch.from_numpy(v0)[None].to(DEV)
    n = torch.from_numpy(synth.vertex_normals(v0, tri))[None].to(DEV)
    tri_d = torch.from_numpy(tri).to(DEV)
    picture = rasterize(v, attr[None].to(DEV), tri_d, 64, 64, channel_major=True).contiguous()
    zbuf = texture.depth_buffer(v, tri_d, 64)
    size = 64
    face, coeff = texture.texel_map(uv.to(DEV), tri_uv, size, keep)
    tex, weight = texture.bake(v, n, tri_d, face, coeff, picture, zbuf, facing=(0.3, 0.3))
    assert sorted(weight.unique().tolist()) == [0.0, 1.0]
    # which texels qualify: weight 1 and all four sampled pixels covered by the mesh (read off the z-buffer)
    face_h, coeff_h, zb, pic = face.cpu(), coeff.cpu().double(), zbuf[0].cpu(), picture[0].cpu().double()
    corners = torch.from_numpy(v0).double()[torch.from_numpy(tri)[face_h.long().clamp_min(0)]]      # [T, T, 3, 3]
    p = (coeff_h.unsqueeze(-1) * corners).sum(-2)
    sx, sy = (1 + p[..., 0]) * 32 - 0.5, (1 - p[..., 1]) * 32 - 0.5
    x0, y0 = torch.floor(sx).long(), torch.floor(sy).long()
    covered = zb > -1e30
    four = torch.ones_like(covered[0:1, 0:1]).expand(size, size).clone()
    for yy in (y0, y0 + 1):
        for xx in (x0, x0 + 1):
            four &= covered[yy.clamp(0, 63), xx.clamp(0, 63)]
    ok = (weight[0, 0].cpu() == 1) & four & (face_h >= 0)
    # D8: the largest difference between 8-neighbouring covered pixels
    d8 = 0.0
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        a = pic[:, :64 - dy, max(-dx, 0):64 - max(dx, 0)]
        b = pic[:, dy:, max(dx, 0):64 - max(-dx, 0)]
        both = covered[:64 - dy, max(-dx, 0):64 - max(dx, 0)] & covered[dy:, max(dx, 0):64 - max(-dx, 0)]
        d8 = max(d8, float(((a - b).abs() * both).max()))
    centres = texture.texel_centres(size)
    want = torch.einsum("yxk,ck->cyx", centres, abc[:, :2]) + abc[:, 2].view(3, 1, 1)
    err = float((tex[0].cpu().double() - want)[:, ok].abs().max())
    share = float(ok.sum()) / float((face_h >= 0).sum())
    print("round trip: error", err, "D8", d8, "qualifying share", share)
    assert share >= 0.25
    assert err <= d8 + 1e-5


# ---- capture ---------------------------------------------------------------------------------------------------------
def test_bake_and_pad_under_graph_capture():
    args, _, _ = ordinary_case(torch.float32, DEV, batch=2)
    out = {}

    def body():
        tex, weight = texture.bake(**args)
        out["tex"], out["weight"] = tex, weight
        out["pad"], out["filled"] = texture.pad(tex, weight, 3)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    # new inputs, in place: the mesh turned and moved (with its z-buffer), another picture
    v2 = args["v"].clone()
    v2[..., 0] = -v2[..., 0] + 0.05
    v2[..., 2] = v2[..., 2] * 0.9
    n2 = args["n"].clone()
    n2[..., 0] = -n2[..., 0]
    tri_flipped = args["tri"][:, [0, 2, 1]].contiguous()                     # (mirrored in x: the other winding faces +z)
    z2 = texture.depth_buffer(v2, tri_flipped, (48, 64))
    img2 = torch.flip(args["image"], dims=(1, 3)).contiguous() * 0.5
    args["v"].copy_(v2)
    args["n"].copy_(n2)
    args["zbuf"].copy_(z2)
    args["image"].copy_(img2)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.clone() for k, t in out.items()}
        tex, weight = texture.bake(**args)
        padded, filled = texture.pad(tex, weight, 3)
        assert torch.equal(got["tex"], tex) and torch.equal(got["weight"], weight)
        assert torch.equal(got["pad"], padded) and torch.equal(got["filled"], filled)
    assert int((weight > 0).sum()) > 0


# ---- command line ----------------------------------------------------------------------------------------------------
def test_reconstruct_cli_with_texture_on_the_device(tmp_path):
    g = model.GeneratorWithMap(256, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_b.npy")
    np.save(img, synth.det_uniform((256, 256, 3), 19))                   # HWC
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "256", "--steps", "8", "--n_mean_latent",
           "256", "--texture", "256", "--texture_from", "render", "--out", out, ckpt, img]
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(
        ["face_b.obj", "face_b_canonical.obj", "face_b_render.png", "face_b_normal.png", "face_b.npz",
         "face_b_texture.png", "face_b_texture_weight.png", "face_b_textured.obj", "face_b_textured.mtl"])
    from PIL import Image

    tex = np.asarray(Image.open(os.path.join(out, "face_b_texture.png")), np.float64)
    assert tex.shape == (256, 256, 3) and np.isfinite(tex).all() and tex.max() > tex.min()
    r = np.load(os.path.join(out, "face_b.npz"))
    assert 0 < float(r["texture_coverage"]) < 1
    assert r["loss"].shape == (8,) and np.isfinite(r["loss"]).all()
