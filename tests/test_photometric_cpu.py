"""CPU: the photometric term of the latent fit (fit_parts.Photometric, LatentInverter(photometric=...)): its rows against the
formula written out in numpy, its gradient against finite differences in float64, the plain iteration untouched by it, and a
planted scene in which the term pulls a perturbed pose back."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, fit_parts, inversion, lpips, model, synth
from stylerenderer_amd.op import texture
from test_inversion_cpu import tiny_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def scene(n_lat=6, n_lon=8):
    v0, tri0 = synth.uv_ellipsoid(n_lat, n_lon)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri0)
    return v0, torch.from_numpy(tri0), uv, tri_uv, keep


def affine_texture(bt, c_n, size, dtype=torch.float32):
    """A texture affine in uv (bilinear sampling reproduces it between texel centres), different per channel and row."""
    uvc = texture.texel_centres(size, dtype)                                  # [T, T, 2]
    rows = []
    for b in range(bt):
        rows.append(torch.stack([0.2 * (c + 1) + (0.5 + 0.1 * c) * uvc[..., 0] - (0.3 + 0.05 * b) * uvc[..., 1]
                                 for c in range(c_n)]))
    return torch.stack(rows)


# ---- the term's values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_n", [1, 2])
@pytest.mark.parametrize("with_mask", [False, True])
def test_rows_equal_the_formula(b_n, with_mask):
    v0, tri, uv, tri_uv, keep = scene()
    size, t_size, c_n, weight = 12, 8, 3, 0.7
    v = torch.from_numpy(synth.random_poses(v0, b_n, seed=3)).double()
    target = torch.from_numpy(synth.det_uniform((b_n, c_n, size, size), 11)).double()
    mask = (torch.from_numpy(synth.det_uniform((b_n, 1, size, size), 12)).double() * 0.5 + 0.5) if with_mask else None
    for bt in sorted({1, b_n}):
        term = fit_parts.Photometric((uv, tri_uv, keep), tri, target, t_size, weight, bt == 1, "cpu")
        assert term.bt == bt and tuple(term.texture.shape) == (bt, c_n, t_size, t_size)
        tex = torch.from_numpy(synth.det_uniform((bt, c_n, t_size, t_size), 13 + bt)).double()
        term.texture = tex.clone().requires_grad_(True)
        rows = term(v, target, mask)
        # the formula, written out
        render, cover = texture.render(v, tri, uv, tri_uv, tex, size, 0.0, keep)
        r, t, on = render.numpy(), target.numpy(), cover.numpy().astype(np.float64)[:, None]
        if with_mask:
            on = on * mask.numpy()
        want = np.array([weight * (on[b] * (r[b] - t[b]) ** 2).sum() / (c_n * size * size) for b in range(b_n)])
        print("rows", rows.detach().numpy(), "formula", want)
        assert rows.dtype == torch.float64 and tuple(rows.shape) == (b_n,)
        np.testing.assert_allclose(rows.detach().numpy(), want, rtol=1e-12, atol=0)
        assert 0 < int(cover.sum()) < cover.numel() and float(rows.detach().min()) > 0
        assert torch.equal(term.render_fit, render) and torch.equal(term.cover_fit, cover)


def test_gradcheck_through_uv_map_and_sample():
    v0, tri, uv, tri_uv, keep = scene()
    size, t_size, c_n = 8, 4, 2
    v = torch.from_numpy(synth.random_poses(v0, 1, seed=5)).double()
    target = torch.from_numpy(synth.det_uniform((1, c_n, size, size), 21)).double()
    term = fit_parts.Photometric((uv, tri_uv, keep), tri, target, t_size, 1.0, True, "cpu")
    tex = torch.from_numpy(synth.det_uniform((1, c_n, t_size, t_size), 22)).double()
    # the definition has a one-sided derivative where a coordinate sits on a texel boundary: keep the scene away from them
    with torch.no_grad():
        uvmap, cover = texture.uv_map(v, tri, uv, tri_uv, size, keep)
        sx = (uvmap[..., 0] * t_size - 0.5)[cover]
        sy = ((1 - uvmap[..., 1]) * t_size - 0.5)[cover]
        gap = min(float((sx - sx.round()).abs().min()), float((sy - sy.round()).abs().min()))
    print("gradcheck: covered", int(cover.sum()), "distance to the next texel boundary", gap)
    assert int(cover.sum()) > 8 and gap > 1e-4

    def f(vv, tt):
        term.texture = tt
        return term(vv, target).sum()

    assert torch.autograd.gradcheck(f, (v.clone().requires_grad_(True), tex.clone().requires_grad_(True)), eps=1e-6,
                                    atol=1e-6, rtol=1e-4)


# ---- the inverter ------------------------------------------------------------------------------------------------------------
@pytest.fixture
def one_thread():
    """Bit-for-bit comparisons of two host runs: torch's multi-threaded host backward is not reproducible from run to run
    (two identical inverters differ in the last bit of the latent after one step), a single thread is."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def planted(photometric, photo_lr=0.0, **kw):
    g, mesh = tiny_setup()
    net = lpips.PNetLin()
    v0, tri0 = synth.uv_ellipsoid(10, 12)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri0)
    layout = (uv, tri_uv, keep)
    noise = [torch.from_numpy(synth.det_normal((1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)), 40 + i))
             for i in range(g.num_layers)]
    true_pose = torch.tensor([0.2, -0.05, 0.0, 0.05, -0.03, 0.0, 0.0])
    tex = affine_texture(1, 3, 16)
    helper = inversion.LatentInverter(g, net, torch.zeros(1, 3, 16, 16), mesh, noise=noise, n_mean_latent=64)
    with torch.no_grad():
        helper.pose.copy_(true_pose)
        target = texture.render(helper.posed_mesh()[0], mesh[2], uv, tri_uv, tex, 16, 0.0, keep)[0]
    inv = inversion.LatentInverter(g, net, target, mesh, noise=noise, n_mean_latent=64,
                                   photometric=layout if photometric else None, photo_size=16, photo_lr=photo_lr, **kw)
    return inv, true_pose, tex


def test_the_plain_iteration_is_untouched(one_thread):
    a, _, _ = planted(False, lr=0.05, pose_lr=0.02)
    b, _, tex = planted(True, lr=0.05, pose_lr=0.02, photo_lr=0.01)
    assert a.photo is None and a.texture is None and not a.with_photometric
    b.set_texture(tex)
    ha, hb = a.run(6), b.run(6)
    assert torch.equal(ha, hb) and torch.equal(a.w.detach(), b.w.detach()) and torch.equal(a.pose.detach(), b.pose.detach())
    assert torch.equal(b.texture, tex)                                        # the plain iteration does not step the texture
    with pytest.raises(ValueError):
        a.run(2, photometric=True)
    with pytest.raises(ValueError):
        a.set_texture(tex)
    # after photometric steps the plain iteration is still the plain iteration: no term in its loss
    b.run(2, photometric=True)
    assert not b._photo_on
    before = b.texture.clone()
    b.run(1)
    assert torch.equal(b.texture, before)


def test_planted_scene_the_term_pulls_the_pose_back():
    # the term dominates the objective (weight), the latent barely moves (lr), the texture is the true one and stays.  The
    # region is the target's own silhouette: a pixel the moving mesh newly covers outside it would enter the term with a
    # jump (coverage is not differentiable), inside it the term is smooth in the pose
    inv, true_pose, tex = planted(True, lr=1e-5, pose_lr=0.002, photo_weight=1e3, photo_lr=0.0, mask=torch.ones(1, 1, 16, 16))
    inv.region.set((inv.target.abs().sum(1, keepdim=True) > 0).float())
    start = true_pose + torch.tensor([0.12, 0.0, 0.0, 0.0, 0.06, 0.0, 0.0])   # yaw and translation off
    with torch.no_grad():
        inv.pose.copy_(start)
    inv.set_texture(tex)
    terms, w0 = [], inv.w.detach().clone()
    for _ in range(30):
        inv.run(1, photometric=True)
        terms.append(float(inv.photo.rows.detach()))
    err0 = float((start - true_pose).norm())
    err = float((inv.pose.detach() - true_pose).norm())
    print("planted: term", terms[0], "->", terms[-1], "pose error", err0, "->", err)
    assert np.isfinite(terms).all() and terms[-1] < terms[0]
    assert err < err0
    assert torch.equal(inv.texture, tex)                                      # photo_lr = 0
    assert float((inv.w.detach() - w0).abs().max()) < 1e-2
    # reset puts the texture and its Adam back at 0
    inv.reset(inv.target)
    assert float(inv.texture.abs().max()) == 0.0 and len(inv._photo_optim.state) == 0


def test_the_texture_takes_adam_steps_and_set_texture_restarts_them(one_thread):
    inv, _, tex = planted(True, lr=0.01, pose_lr=0.0, photo_lr=0.05)
    inv.set_texture(tex * 0.5)
    h = inv.run(8, photometric=True)
    assert np.isfinite(h.numpy()).all()
    moved = inv.texture.clone()
    assert float((moved - tex * 0.5).abs().max()) > 0
    first = float(h[0])
    inv.reset(inv.target)
    inv.set_texture(tex * 0.5)
    again = inv.run(8, photometric=True)
    assert torch.equal(again, h) and torch.equal(inv.texture, moved) and float(again[0]) == first
    with pytest.raises(ValueError):
        inv.set_texture(torch.zeros(1, 3, 8, 8))


# ---- the tool ------------------------------------------------------------------------------------------------------------------
BASE_FILES = ["face_b.obj", "face_b_canonical.obj", "face_b_render.png", "face_b_normal.png", "face_b.npz",
              "face_b_texture.png", "face_b_texture_weight.png", "face_b_textured.obj", "face_b_textured.mtl"]


def run_tool(tmp_path, name, flags, env_more=None, size=16, images=1, timeout=600):
    """Runs `reconstruct` at size^2 on deterministic pictures; returns (process, output directory)."""
    ckpt = str(tmp_path / "g.pt")
    if not os.path.exists(ckpt):
        g = model.GeneratorWithMap(size, 512, 8)
        synth.fill_state_dict(g.state_dict(), salt=5)
        torch.save({"g_ema": g.state_dict()}, ckpt)
    paths = []
    for k, stem in enumerate(["face_b", "face_c"][:images]):
        paths.append(str(tmp_path / (stem + ".npy")))
        np.save(paths[-1], synth.det_uniform((size, size, 3), 19 + k))       # HWC
    out = str(tmp_path / name)
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", str(size), "--steps", "3", "--n_mean_latent",
           "16", "--texture", "32", "--out", out] + list(flags) + [ckpt] + paths
    # one host thread: torch's multi-threaded host backward is not reproducible from run to run (see one_thread)
    env = dict(dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="1", MKL_NUM_THREADS="1"), **(env_more or {}))
    return subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=timeout), out


def test_reconstruct_with_photo_writes_its_entries_and_without_it_nothing_changes(tmp_path):
    res, out = run_tool(tmp_path, "photo", ["--photo", "--photo_steps", "3"])
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(BASE_FILES)
    r = np.load(os.path.join(out, "face_b.npz"))
    assert r["photo_loss"].shape == (3,) and np.isfinite(r["photo_loss"]).all()
    assert 0 <= float(r["photo_error_before"]) <= 2 and 0 <= float(r["photo_error_after"]) <= 2
    assert r["loss"].shape == (3,)
    # without --photo: the arrays of a run that never imports the new code (the photometric part and the planner are
    # made unimportable in the child: fit_parts.Photometric and op.texture.TapPlanner raise when touched)
    plain, out_a = run_tool(tmp_path, "plain", [])
    guard = tmp_path / "guard"
    guard.mkdir()
    (guard / "sitecustomize.py").write_text(
        "import stylerenderer_amd.fit_parts as f, stylerenderer_amd.op.texture as t\n"
        "def _no(*a, **k):\n    raise RuntimeError('the new code ran without --photo')\n"
        "f.Photometric = _no\nt.TapPlanner = _no\nt.explode = _no\nt._explode_corners = _no\n")
    other, out_b = run_tool(tmp_path, "guarded", [], {"PYTHONPATH": str(guard) + os.pathsep + ROOT})
    assert plain.returncode == 0 and other.returncode == 0, (plain.stderr[-2000:], other.stderr[-2000:])
    assert sorted(os.listdir(out_a)) == sorted(os.listdir(out_b)) == sorted(BASE_FILES)
    a, b = np.load(os.path.join(out_a, "face_b.npz")), np.load(os.path.join(out_b, "face_b.npz"))
    assert sorted(a.files) == sorted(b.files) and not any(k.startswith("photo") for k in a.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    bad, _ = run_tool(tmp_path, "bad", ["--photo_steps", "3"])
    assert bad.returncode != 0 and "--photo" in bad.stderr
