"""CPU: the perspective camera node (op.camera) — the composite's gradients, the identity at kappa = 0, n_view, the tie to
the rasterizer's perspective mode, pose and kappa recovered from landmarks, the inverter's camera options and
`reconstruct --camera_distance`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import align, face_model, reconstruct, synth, train, utils_3d
from stylerenderer_amd.op import camera, landmark
from stylerenderer_amd.op.rasterize import forward as raster_forward
from test_landmark_cpu import _inverter, tiny_landmarks, tiny_problem
from test_reconstruct_cpu import _env

POSE = (0.3, -0.2, 0.1, 0.05, -0.03, 0.0, -0.2)
FRONTAL = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -0.2)
_SRC = {}


def mean_shape():
    """(v [nv, 3] float64, tri int64 [nf, 3]) of train.SyntheticFaceSource(face_sized=False)'s mean shape."""
    if not _SRC:
        src = train.SyntheticFaceSource(torch.device("cpu"), face_sized=False)
        _SRC["v"], _SRC["tri"] = src.model.fc.bias.detach().view(-1, 3).double(), src.tri.contiguous()
    return _SRC["v"], _SRC["tri"]


def posed(pts, pose):
    """pts [n, 3] under pose [7] (a tensor: differentiable), in pts' float type."""
    return pts @ (torch.exp(pose[6]) * utils_3d.euler_mat(pose[:3], "yxz")) + pose[3:6]


def small_case(dtype=torch.float64):
    """B = 2, nv = 7, kappa = (0, 0.3); vertex 4 of row 1 has q0 = 1 - 0.3 * 3.5 < QMIN."""
    v = torch.from_numpy(synth.det_uniform((2, 7, 3), 81)).to(dtype)
    v[1, 4, 2] = 3.5
    n = torch.nn.functional.normalize(torch.from_numpy(synth.det_normal((2, 7, 3), 82)).to(dtype), dim=-1)
    return v, torch.tensor([0.0, 0.3], dtype=dtype), n


# ---- 1, 2, 3: the composite --------------------------------------------------------------------------------------------
def test_composite_passes_gradcheck_and_gradgradcheck():
    v, kappa, n = small_case()
    assert float(1 - kappa[1] * v[1, 4, 2]) < camera.QMIN
    v.requires_grad_(True)
    kappa.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, k: camera.project(a, k), (v, kappa))
    assert torch.autograd.gradcheck(lambda a, k: camera.project(a, k, normals=n)[0], (v, kappa))
    assert torch.autograd.gradgradcheck(lambda a, k: camera.project(a, k), (v, kappa))
    # the clamped vertex: divided by QMIN, no kappa t term in its gradient and nothing added to gkappa
    g = torch.from_numpy(synth.det_normal((2, 7, 3), 83)).double()
    vp = camera.project(v, kappa)
    assert torch.equal(vp[1, 4].detach(), v[1, 4].detach() / camera.QMIN)
    gv, gk = torch.autograd.grad((vp * g).sum(), (v, kappa))
    assert torch.equal(gv[1, 4], g[1, 4] / camera.QMIN)
    terms = camera.kappa_terms(v.detach(), kappa.detach(), g)
    assert float(terms[1, 4]) == 0.0 and int((terms[1] != 0).sum()) == 6
    assert torch.allclose(gk, terms.sum(1), rtol=1e-15, atol=0)
    # an unclamped vertex does carry the term
    assert float((gv[1, 0, 2] - g[1, 0, 2] / (1 - 0.3 * v.detach()[1, 0, 2])).abs()) > 1e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_kappa_zero_is_the_identity_bit_for_bit(dtype):
    v, _, n = small_case(dtype)
    v[0, 2] = torch.tensor([-0.0, 0.0, -0.0], dtype=dtype)
    n[0, 3] = torch.tensor([0.0, -0.0, -0.0], dtype=dtype)
    kappa = torch.zeros(2, dtype=dtype)
    v.requires_grad_(True)
    vp, nview = camera.project(v, kappa, normals=n)
    as_bits = lambda t: t.detach().contiguous().view(torch.int32 if dtype == torch.float32 else torch.int64)  # noqa: E731
    assert torch.equal(as_bits(vp), as_bits(v)) and torch.equal(as_bits(nview), as_bits(n))
    assert not nview.requires_grad
    g = torch.from_numpy(synth.det_normal((2, 7, 3), 84)).to(dtype)
    (gv,) = torch.autograd.grad((vp * g).sum(), v)
    assert torch.equal(gv, g)


def test_view_normals_keep_the_norm_and_their_z_is_the_cosine_to_the_ray():
    v, _, n = small_case()
    n = n * torch.linspace(0.5, 2.0, 7, dtype=torch.float64).view(1, 7, 1)          # not unit: the norm is kept, whatever
    kappa = torch.tensor([0.4, -0.1], dtype=torch.float64)
    vp, nview = camera.project(v, kappa, normals=n)
    k = kappa.view(2, 1)
    d = torch.stack((-k * vp[..., 0], -k * vp[..., 1], torch.ones_like(vp[..., 0])), -1)
    d = d / d.norm(dim=-1, keepdim=True)
    assert float((nview[..., 2] - (n * d).sum(-1)).abs().max()) <= 1e-14
    assert float((nview.norm(dim=-1) - n.norm(dim=-1)).abs().max()) <= 1e-14
    assert float((nview - n).abs().max()) > 1e-3
    same = camera.project(v, torch.zeros(2, dtype=torch.float64), normals=n)[1]
    assert torch.equal(same, n)


def test_project_refuses_what_does_not_pair_up():
    v, kappa, n = small_case()
    for bad in (lambda: camera.project(v, kappa[:1]), lambda: camera.project(v, kappa.float()),
                lambda: camera.project(v[0], kappa), lambda: camera.project(v, kappa, normals=n[:, :5]),
                lambda: camera.project(v, 0.3)):
        with pytest.raises(ValueError):
            bad()


# ---- 4: the rasterizer's perspective mode ------------------------------------------------------------------------------
def perspective_tie(v, tri, kappa, size):
    """Asserts the tie between `project` + the orthographic rasterizer and the rasterizer's own perspective mode on the
    posed mesh v [1, nv, 3] (any device); returns (covered pixels, differing pixels, worst coefficient difference / bound)."""
    k = torch.full((1,), kappa, dtype=v.dtype, device=v.device)
    vp = camera.project(v, k).contiguous()
    idx_o, c_o = raster_forward(vp, tri, size, size, False)
    vcam = torch.stack((v[..., 0], v[..., 1], kappa * v[..., 2] - 1), -1).contiguous()
    idx_p, c_p = raster_forward(vcam, tri, size, size, True)
    cov_o, cov_p = (c_o != 0).any(-1), (c_p != 0).any(-1)
    both = cov_o & cov_p & (idx_o == idx_p).all(-1)
    covered = int((cov_o | cov_p).sum())
    differ = int(((cov_o | cov_p) & ~both).sum())
    assert covered > 0.05 * size * size
    # the project's cap on differing pixels between two rasterizations of one surface
    assert differ <= 0.005 * covered, (covered, differ)
    q = (1 - kappa * v[0, :, 2])[idx_o[0]]                                       # [H, W, 3]: q at the winner's corners
    bound = (q.max(-1).values - q.min(-1).values) / q.min(-1).values
    if v.dtype == torch.float32:
        bound = bound + 8 * 2.0 ** -24
    diff = (c_p / c_p.sum(-1, keepdim=True) - c_o)[0].abs().max(-1).values
    ratio = float((diff[both[0]] / bound[both[0]].clamp_min(1e-300)).max())
    assert bool((diff[both[0]] <= bound[both[0]]).all()), ratio
    return covered, differ, ratio


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kappa", [0.1, 0.25, 0.4])
def test_projection_then_orthographic_raster_is_the_rasterizers_perspective_mode(kappa, dtype):
    v0, tri = mean_shape()
    v = posed(v0, torch.tensor(POSE, dtype=torch.float64)).to(dtype)[None].contiguous()
    covered, differ, ratio = perspective_tie(v, tri, kappa, 32)
    print("kappa %.2f %s: %d covered, %d differ, coefficient difference %.3f of the bound" % (kappa, dtype, covered, differ, ratio))


# ---- 5: recovery -------------------------------------------------------------------------------------------------------
def fit_landmarks(pts, lmk, hw, fit_kappa):
    """L-BFGS on (pose, kappa) from the orthographic closed-form start; returns (pose [7], kappa, mean distance in px)."""
    start = align.pose_from_landmarks(pts.numpy(), lmk.numpy(), hw)
    pose = torch.tensor(start, dtype=torch.float64, requires_grad=True)
    kappa = torch.zeros(1, dtype=torch.float64, requires_grad=fit_kappa)

    def points():
        return landmark.project(camera.project(posed(pts, pose)[None], kappa), hw)[0]

    opt = torch.optim.LBFGS([pose] + ([kappa] if fit_kappa else []), lr=1.0, max_iter=500, tolerance_grad=1e-15,
                            tolerance_change=1e-18, history_size=30, line_search_fn="strong_wolfe")

    def closure():
        opt.zero_grad()
        loss = ((points() - lmk) ** 2).sum()
        loss.backward()
        return loss

    for _ in range(4):
        opt.step(closure)
    with torch.no_grad():
        dist = float(((points() - lmk) ** 2).sum(1).sqrt().mean())
    return pose.detach().numpy(), float(kappa.detach()), dist


@pytest.mark.parametrize("pose", [POSE, FRONTAL])
@pytest.mark.parametrize("kappa", [0.1, 0.25])
def test_pose_and_kappa_come_back_from_landmarks(kappa, pose):
    v0, _ = mean_shape()
    pts = v0[np.linspace(0, len(v0) - 1, 24).round().astype(np.int64)]
    hw = (64, 64)
    true = torch.tensor(pose, dtype=torch.float64)
    with torch.no_grad():
        lmk = landmark.project(camera.project(posed(pts, true)[None], torch.tensor([kappa], dtype=torch.float64)), hw)[0]
    got, k, dist = fit_landmarks(pts, lmk, hw, True)
    _, _, ortho = fit_landmarks(pts, lmk, hw, False)
    print("kappa %.2f: with kappa fitted %.3g px, kappa %.9f, angles %s; orthographic %.3f px"
          % (kappa, dist, k, got[:3], ortho))
    assert dist <= 1e-6 and abs(k - kappa) <= 1e-6
    assert np.abs(got[:3] - np.array(pose[:3])).max() <= 1e-6
    assert ortho >= 0.1


# ---- 6: the inverter -----------------------------------------------------------------------------------------------------
def _state(inv, hist):
    return [hist] + [t.detach().clone() for t in (inv.w, inv.pose, inv.coeff)]


def test_inverter_camera_options():
    problem = tiny_problem()
    emb, lmk = tiny_landmarks(problem[2])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # the CPU path's threaded reductions are not run-to-run identical
    try:
        plain = _inverter(problem)
        want = _state(plain, plain.run(5))
        assert plain.camera is None
        fixed = _inverter(problem, camera=0.0)
        got = _state(fixed, fixed.run(5))
        assert fixed.camera.shape == (1,) and not fixed.camera.requires_grad
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        kw = dict(camera=0.25, fit_camera=True, camera_lr=0.02, landmarks=lmk, landmark_embedding=emb,
                  landmark_vis=(0.0, 0.2))
        inv = _inverter(problem, **kw)
        assert inv.camera.requires_grad and float(inv.camera.detach()) == 0.25
        first = _state(inv, inv.run(4)) + [inv.camera.detach().clone()]
        assert abs(float(inv.camera.detach()) - 0.25) > 1e-3                              # fit_camera moves kappa
        # what the consumers saw against the camera-space mesh
        v, n, _ = inv.fitted_mesh()
        vc, nc, _ = inv.fitted_mesh(projected=False)
        wv, wn = camera.project(vc, inv.camera.detach(), normals=nc)
        assert torch.equal(v, wv) and torch.equal(n, wn) and float((v - vc).abs().max()) > 1e-3
        inv.reset(problem[4], landmarks=lmk)
        assert float(inv.camera.detach()) == 0.25
        again = _state(inv, inv.run(4)) + [inv.camera.detach().clone()]
        for a, b in zip(again, first):
            assert torch.equal(a, b)
    finally:
        torch.set_num_threads(threads)
    for bad in (dict(camera=[0.1, 0.2]), dict(camera=float("nan")), dict(camera=torch.tensor([float("inf")])),
                dict(fit_camera=True), dict(camera="near")):
        with pytest.raises(ValueError):
            _inverter(problem, **bad)


def test_batched_inverter_takes_one_kappa_per_row(tmp_path):
    g, mesh, face, noise, target = tiny_problem()
    targets = torch.cat([target, target.flip(3)], 0).contiguous()
    inv = _inverter((g, mesh, face, noise, targets), camera=[0.1, 0.3], fit_camera=True, shared_identity=8)
    hist = inv.run(2)
    assert inv.camera.shape == (2,) and hist.shape == (2, 2)
    k = inv.camera.detach()
    assert abs(float(k[0]) - 0.1) > 0 and abs(float(k[1]) - 0.3) > 0 and abs(float(k[0] - k[1])) > 0.1
    # the subject's file of `reconstruct --multiview` lists the views' kappa; the views' own files each theirs
    entries = reconstruct.subject_outputs(inv, hist.numpy(), str(tmp_path), "who", ["a", "b"])
    assert np.array_equal(entries["camera"], k.double().numpy())
    assert np.array_equal(np.load(str(tmp_path / "who_identity.npz"))["camera"], k.double().numpy())
    reconstruct.write_outputs(inv, hist.numpy()[:, 1], str(tmp_path), "b", index=1)
    r = np.load(str(tmp_path / "b.npz"))
    assert float(r["camera"]) == float(k[1]) and abs(float(r["camera_distance"]) * float(k[1]) - 1) <= 1e-12
    one = _inverter((g, mesh, face, noise, targets), camera=0.2)
    assert torch.equal(one.camera, torch.full((2,), 0.2))
    with pytest.raises(ValueError):
        _inverter((g, mesh, face, noise, targets), camera=[0.1, 0.2, 0.3])


# ---- 7: command line -----------------------------------------------------------------------------------------------------
def _obj_vertices(path):
    return np.array([[float(x) for x in line.split()[1:4]] for line in open(path) if line.startswith("v ")])


def run_camera_cli(tmp_path, env, size=16, steps=4, more=(), without=True):
    """`reconstruct --camera_distance 4 --fit_camera --lmk ...` on one 24 x 32 picture and, with `without`, the same
    without the camera flags; checks the files (shared with the GPU suite, which fits at 256)."""
    from PIL import Image

    from stylerenderer_amd import model

    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    path = str(tmp_path / "face_a.png")
    pix = (127.5 * (synth.det_uniform((24, 32, 3), 9) + 1)).clip(0, 255).astype(np.uint8)
    Image.fromarray(pix).save(path)
    v0, _ = synth.face_sized_mesh()
    verts = np.linspace(0, len(v0) - 1, 9).round().astype(np.int64)
    index = str(tmp_path / "index.txt")
    np.savetxt(index, verts, fmt="%d")
    pts = torch.from_numpy(v0[verts].astype(np.float64))
    with torch.no_grad():
        seen = camera.project(posed(pts, torch.tensor(POSE, dtype=torch.float64))[None],
                              torch.tensor([0.3], dtype=torch.float64))
        lmk = align.scale_landmarks(landmark.project(seen, (size, size))[0].numpy(), (size, size), (24, 32))
    lmk_file = str(tmp_path / "lmk.txt")
    with open(lmk_file, "w") as f:
        f.write("face_a.png " + " ".join("%.6f" % x for x in lmk.reshape(-1)) + "\n")
    base = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", str(size), "--steps", str(steps), "--n_mean_latent",
            "64", "--lmk", lmk_file, "--lmk_index", index, "--lmk_vis", "0,0.2"] + list(more)
    out = str(tmp_path / "out")
    res = subprocess.run(base + ["--camera_distance", "4", "--fit_camera", "--camera_lr", "0.02", "--out", out, ckpt, path],
                         env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    r = np.load(os.path.join(out, "face_a.npz"))
    kappa = float(r["camera"])
    assert r["camera"].shape == () and np.isfinite(kappa) and 1e-5 < abs(kappa - 0.25) < 0.2
    assert abs(float(r["camera_distance"]) - 1 / kappa) <= 1e-12
    fm, tri = reconstruct.face_model(None, torch.device("cpu"), seed=0)                     # (--seed's default)
    with torch.no_grad():
        v = fm.mesh(torch.from_numpy(r["coeff"]), torch.from_numpy(r["pose"]).view(1, 7), tri)[0]
        vp = camera.project(v, torch.tensor([kappa], dtype=torch.float32))
    # (the fit ran on `device`, this mesh on the host: the two model nodes agree to float32 rounding, the file to its digits)
    tol = 2e-5
    written = _obj_vertices(os.path.join(out, "face_a.obj"))
    assert np.abs(written - v[0].double().numpy()).max() <= tol
    assert np.abs(written - vp[0].double().numpy()).max() > 100 * tol            # not the projected mesh
    idx, bary = face_model.landmark_embedding(verts)
    with torch.no_grad():
        want = [align.scale_landmarks(landmark.project(landmark.landmark_points(m, idx, bary), (size, size))[0].double().numpy(),
                                      (size, size), (24, 32)) for m in (vp, v)]
    assert np.abs(r["landmarks"] - want[0]).max() <= 1e-3                        # the projected mesh's landmarks
    assert np.abs(r["landmarks"] - want[1]).max() > 0.05
    assert r["lmk_visibility"].shape == (9,)
    if not without:
        return res
    off = str(tmp_path / "off")
    res = subprocess.run(base + ["--out", off, ckpt, path], env=env, cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    r0 = np.load(os.path.join(off, "face_a.npz"))
    assert "camera" not in r0.files and "camera_distance" not in r0.files
    assert sorted(os.listdir(off)) == sorted(os.listdir(out))
    return res


def test_reconstruct_cli_with_a_camera(tmp_path):
    run_camera_cli(tmp_path, _env())
    # the flags' rules
    for flags in (["--fit_camera"], ["--camera_distance", "0"], ["--camera_distance", "3", "--camera_fov", "40"]):
        res = subprocess.run([sys.executable, "-m", "stylerenderer_amd.reconstruct"] + flags + ["x.pt", "x.png"], env=_env(),
                             cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert res.returncode == 2, (flags, res.stderr[-500:])
