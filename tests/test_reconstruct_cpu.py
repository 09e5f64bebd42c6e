"""CPU: face reconstruction — the morphable-mesh node's composite path against the reference (fixture of
make_golden_reconstruct.py), utils_3d.save_obj against the reference's files, the inverter's fit_shape mode, the
`reconstruct` CLI end to end and `train --bfm`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reconstruct_cases as rc
from stylerenderer_amd import face_model, inversion, lpips, synth, utils_3d
from stylerenderer_amd.op import morph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# nominal relative bars; the bar used is 4x the reference's own fp32-vs-fp64 error, at least nominal, at most 10x nominal
NOMINAL = {"v": 1e-6, "n": 1e-4, "gcoeff": 1e-4, "gpose": 1e-4}


def bar(golden, name, key):
    return min(10 * NOMINAL[key], max(NOMINAL[key], 4 * float(golden["%s_%s_err32" % (name, key)])))


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())


def build_case(name, device="cpu", dtype=torch.float32):
    """(model, tri, coeff, pose, gv, gn, idx) of a fixture case as tensors."""
    v0, tri, wsh, wex, cu, pose, gv, gn, idx = rc.case(name)
    _, ds, de, _, _ = rc.CASES[name]
    model = face_model.LinearMorphableModel(v0.shape[0], ds, de, v0, wsh, wex).to(device=device, dtype=dtype)
    coeff = (torch.from_numpy(cu).to(dtype) * model.sigma.detach().cpu()).to(device)
    t = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)           # noqa: E731
    return model, torch.from_numpy(tri).to(device), coeff, t(pose), t(gv), t(gn), idx


def node_outputs(model, tri, coeff, pose, gv, gn, idx):
    """v, n at the sample and the gradients of sum(v gv) + sum(n gn) + REG_WEIGHT regulation(coeff), through morph_mesh."""
    c = coeff.clone().requires_grad_(True)
    p = pose.clone().requires_grad_(True)
    v, n, reg = morph.morph_mesh(model, c, p, tri, rc.REG_WEIGHT)
    loss = (v * gv).sum() + (n * gn).sum() + reg
    gc, gp = torch.autograd.grad(loss, (c, p))
    out = {"v": v.detach()[:, idx], "n": n.detach()[:, idx], "gcoeff": gc, "gpose": gp}
    return {k: x.cpu().double().numpy() for k, x in out.items()}


@pytest.mark.parametrize("name", list(rc.CASES))
def test_composite_node_matches_the_reference(golden, name):
    g = golden("reconstruct_morph")
    got = node_outputs(*build_case(name))
    for key in NOMINAL:
        want = g["%s_%s" % (name, key)]
        assert got[key].shape == want.shape
        err = rel(got[key], want)
        assert err <= bar(g, name, key), (name, key, err, bar(g, name, key))
    # the float64 composite is the reference's algebra: equal up to float64 rounding of another summation order
    got64 = node_outputs(*build_case(name, dtype=torch.float64))
    for key in NOMINAL:
        assert rel(got64[key], g["%s_%s" % (name, key)]) < 1e-7, key


def test_regulation_term_is_the_models():
    model, tri, coeff, pose, _, _, _ = build_case("small")
    _, _, reg = morph.morph_mesh(model, coeff, pose, tri, 0.5)
    assert torch.allclose(reg, 0.5 * model.regulation(coeff), rtol=1e-6)


@pytest.mark.parametrize("form", rc.OBJ_FORMS)
def test_save_obj_writes_the_references_text(tmp_path, form):
    kw, v, tri = rc.obj_args(form)
    path = str(tmp_path / "m.obj")
    assert utils_3d.save_obj(path, v, tri, **kw)
    with open(os.path.join(GOLDEN, "reconstruct_obj_%s.obj" % form), "rb") as f:
        want = f.read()
    with open(path, "rb") as f:
        assert f.read() == want
    # tensors are accepted too
    kw_t = {k: torch.from_numpy(a) for k, a in kw.items()}
    utils_3d.save_obj(path, torch.from_numpy(v), torch.from_numpy(tri), **kw_t)
    with open(path, "rb") as f:
        assert f.read() == want


def test_save_obj_face_records():
    kw, v, tri = rc.obj_args("full")
    first = {form: [l for l in open(os.path.join(GOLDEN, "reconstruct_obj_%s.obj" % form)).read().splitlines()
                    if l.startswith("f ")][0] for form in rc.OBJ_FORMS}
    assert first == {"full": "f 1/1/1 2/2/2 3/3/3", "vt": "f 1/1 2/2 3/3", "vn": "f 1//1 2//2 3//3", "plain": "f 1 2 3"}


# ---- inverter --------------------------------------------------------------------------------------------------------
def tiny_face(device="cpu"):
    v0, tri = synth.uv_ellipsoid(10, 12)
    nv = v0.shape[0]
    ds, de = 8, 6
    wsh = 0.02 * synth.det_uniform((ds, 3 * nv), 11)
    wex = 2.0 * synth.det_uniform((de, 3 * nv), 12)
    fm = face_model.LinearMorphableModel(nv, ds, de, v0, wsh, wex).to(device)
    return fm, torch.from_numpy(tri).to(device)


def tiny_problem(device="cpu"):
    from test_inversion_cpu import tiny_setup

    g, mesh = tiny_setup(device)
    fm, tri = tiny_face(device)
    noise = [torch.from_numpy(synth.det_normal((1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)), 40 + i)).to(device)
             for i in range(g.num_layers)]
    with torch.no_grad():
        c_true = torch.from_numpy(synth.det_normal((1, 14), 3)).to(device) * fm.sigma
        p_true = torch.tensor([[0.2, -0.1, 0.05, 0.03, -0.02, 0.0, 0.05]], device=device)
        v, n, _ = morph.morph_mesh(fm, c_true, p_true, tri)
        w_true = g.style(torch.from_numpy(synth.det_normal((1, 32), 5)).to(device)).unsqueeze(1).repeat(1, g.n_latent, 1)
        target, _, _ = g([w_true], (v.contiguous(), n.contiguous(), tri), input_is_latent=True, noise=noise)
    return g, mesh, (fm, tri), noise, target


def test_fit_shape_lowers_the_loss_and_moves_coefficients_latent_and_pose():
    g, _, face, noise, target = tiny_problem()
    torch.manual_seed(3)
    inv = inversion.LatentInverter(g, lpips.PNetLin(), target, None, lr=0.05, pose_lr=0.02, noise=noise,
                                   n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3)
    assert torch.equal(inv.coeff, torch.zeros(1, 14))
    hist = inv.run(25).numpy()
    assert np.isfinite(hist).all() and hist[-1] < 0.8 * hist[0]
    assert float(inv.coeff.detach().abs().max()) > 1e-3
    assert float(inv.pose.detach().abs().max()) > 1e-3
    assert float((inv.w.detach() - inv.w.detach()[:, :1]).abs().max()) > 0
    v, n, tri = inv.fitted_mesh()
    assert v.shape == (1, 110, 3) and n.shape == v.shape and not v.requires_grad and torch.equal(tri, face[1])
    want, _, _ = morph.morph_mesh(face[0], inv.coeff.detach(), inv.pose.detach().view(1, 7), tri)
    assert torch.equal(v, want)


def test_fit_shape_off_is_bit_identical_to_the_plain_inverter():
    g, mesh, face, noise, target = tiny_problem()
    runs = []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # the CPU path's threaded reductions are not run-to-run identical
    try:
        for extra in ({}, {"face": face, "fit_shape": False, "coeff_lr": 0.3, "shape_reg": 0.5}):
            torch.manual_seed(3)
            inv = inversion.LatentInverter(g, lpips.PNetLin(), target, mesh, lr=0.05, pose_lr=0.02, noise=noise,
                                           n_mean_latent=64, **extra)
            runs.append((inv.run(6).numpy(), inv.w.detach().clone(), inv.pose.detach().clone()))
            assert inv.coeff is None
    finally:
        torch.set_num_threads(threads)
    assert np.array_equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_fit_shape_needs_a_face_model():
    g, mesh, _, noise, target = tiny_problem()
    with pytest.raises(ValueError):
        inversion.LatentInverter(g, lpips.PNetLin(), target, mesh, noise=noise, n_mean_latent=8, fit_shape=True)


# ---- command line ----------------------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


def _obj_counts(path):
    kinds = {}
    for line in open(path):
        k = line.split(" ", 1)[0]
        kinds[k] = kinds.get(k, 0) + 1
    return kinds


def test_reconstruct_cli_end_to_end(tmp_path):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_a.npy")
    np.save(img, synth.det_uniform((3, 24, 24), 9))                      # CHW, resized to 16 on the host
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "4", "--n_mean_latent",
           "64", "--out", out, ckpt, img]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "--lpips-trunk" in res.stderr and "not a meaningful reconstruction" in res.stderr
    names = sorted(os.listdir(out))
    assert names == sorted(["face_a.obj", "face_a_canonical.obj", "face_a_render.png", "face_a_normal.png",
                            "face_a.npz"])
    v0, tri = synth.face_sized_mesh()                                    # train.SyntheticFaceSource's mesh
    nv, nf = v0.shape[0], tri.shape[0]
    for obj in ("face_a.obj", "face_a_canonical.obj"):
        assert _obj_counts(os.path.join(out, obj)) == {"v": nv, "vn": nv, "f": nf}
    r = np.load(os.path.join(out, "face_a.npz"))
    assert r["w"].shape == (1, g.n_latent, 512) and r["coeff"].shape == (1, 144) and r["pose"].shape == (7,)
    assert r["loss"].shape == (4,) and np.isfinite(r["loss"]).all()
    assert float(np.abs(r["coeff"]).max()) > 0


def _write_tiny_bfm(path):
    import scipy.io as sio

    v0, tri = synth.uv_ellipsoid(16, 14)
    nv = v0.shape[0]
    cell = np.empty((1, 1), dtype=object)
    cell[0, 0] = (tri + 1).astype(np.float64)                            # MATLAB: 1-based, in a cell
    sio.savemat(path, {"v": (v0.T * 1e5).astype(np.float64),
                       "w_shape": 1e3 * synth.det_uniform((3 * nv, 5), 21).astype(np.float64),
                       "w_exp": 1e3 * synth.det_uniform((3 * nv, 4), 22).astype(np.float64),
                       "sigma_shape": np.ones((5, 1)), "tri": cell})
    return nv, tri.shape[0]


def test_bfm_file_loads_in_the_load_bfm_contract(tmp_path):
    path = str(tmp_path / "tiny.mat")
    nv, nf = _write_tiny_bfm(path)
    m, tri = face_model.load_bfm(path)
    assert m.dim == [5, 4, 3 * nv] and tuple(tri.shape) == (nf, 3) and int(tri.min()) == 0
    from stylerenderer_amd import train

    src = train.BfmFaceSource(torch.device("cpu"), path)
    v, n, t = src.sample(2)
    assert v.shape == (2, nv, 3) and n.shape == v.shape and t is src.tri


def test_train_cli_with_bfm(tmp_path):
    path = str(tmp_path / "tiny.mat")
    _write_tiny_bfm(path)
    cmd = [sys.executable, "-m", "stylerenderer_amd.train", "--size", "16", "--latent", "32", "--n_mlp", "2",
           "--batch", "2", "--iter", "1", "--mesh", "--bfm", path]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.count("iter ") == 1
