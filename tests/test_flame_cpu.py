"""CPU: the FLAME skinned face model — utils_3d.rodrigues, LinearBlendSkinningModel / load_flame and the skinning node's
composite path against the reference (fixture of make_golden_flame.py), the inverter with a skinned model (single and
batched), `reconstruct --flame` and `train --mesh --flame`."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import flame_cases as fc
from stylerenderer_amd import face_model, inversion, lpips, synth, utils_3d
from stylerenderer_amd.op import skin
from test_reconstruct_batch_cpu import first_gradients
from test_reconstruct_cpu import NOMINAL, _env, _obj_counts, bar, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_case(name, device="cpu", dtype=torch.float32):
    """(model, tri, coeff, pose, gv, gn, idx) of a fixture case as tensors."""
    d, tri, coeff, pose, gv, gn, idx = fc.case(name)
    model, t = face_model.load_flame(d)
    assert np.array_equal(t.numpy(), tri)
    to = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)           # noqa: E731
    return model.to(device=device, dtype=dtype), t.to(device), to(coeff), to(pose), to(gv), to(gn), idx


def node_outputs(model, tri, coeff, pose, gv, gn, idx, reg_weight=fc.REG_WEIGHT, node=None):
    """v, n at the sample, the gradients of L = sum(v gv) + sum(n gn) + REG_WEIGHT regulation(coeff), and the coefficient
    gradient's two parts: of the data term alone and of regulation(coeff) alone (through the node's `reg` output)."""
    node = node or skin.skin_mesh
    c = coeff.clone().requires_grad_(True)
    p = pose.clone().requires_grad_(True)
    v, n, reg = node(model, c, p, tri, reg_weight)
    loss = (v * gv).sum() + (n * gn).sum() + reg
    gc, gp = torch.autograd.grad(loss, (c, p))
    v1, n1, reg1 = node(model, c, p, tri, 1.0)
    (gc_data,) = torch.autograd.grad((v1 * gv).sum() + (n1 * gn).sum(), c, retain_graph=True)
    (gc_prior,) = torch.autograd.grad(reg1, c)
    out = {"v": v.detach()[:, idx], "n": n.detach()[:, idx], "gcoeff": gc, "gpose": gp, "gcoeff_data": gc_data,
           "gcoeff_prior": gc_prior}
    return {k: x.cpu().double().numpy() for k, x in out.items()}


def rule(nominal, err32):
    """test_reconstruct_cpu's rule for an fp32 bar: 4x the reference's own fp32 error, at least nominal, at most 10x."""
    return min(10 * nominal, max(nominal, 4 * float(err32)))


def check_against_fixture(g, name, got, float64=False):
    """Every output against the fixture.  fp32: test_reconstruct_cpu's bars; float64: 1e-7.  The coefficient gradient is
    checked as a whole (the issue's L) and, because the eye-roll prior dominates that max-norm, block by block: the data
    term's shape block and each joint's angles against their own magnitude, the prior's gradient entry by entry."""
    ds = fc.CASES[name][1]
    for key in NOMINAL:
        want = g["%s_%s" % (name, key)]
        assert got[key].shape == want.shape
        err, lim = rel(got[key], want), 1e-7 if float64 else bar(g, name, key)
        print(name, key, "rel", err, "bar", lim)
        assert err < lim if float64 else err <= lim, (name, key, err, lim)
    for blk, err in fc.block_errors(got["gcoeff_data"], g[name + "_gcoeff_data"], ds).items():
        lim = 1e-7 if float64 else rule(NOMINAL["gcoeff"], g["%s_gcoeff_data_%s_err32" % (name, blk)])
        print(name, "gcoeff_data", blk, "rel", err, "bar", lim)
        assert err <= lim, (name, blk, err, lim)
    err = fc.elementwise_error(got["gcoeff_prior"], g[name + "_gcoeff_prior"])
    lim = 1e-7 if float64 else rule(NOMINAL["gcoeff"], g[name + "_gcoeff_prior_elem_err32"])
    print(name, "gcoeff_prior elementwise rel", err, "bar", lim)
    assert err <= lim, (name, err, lim)


# ---- rodrigues -------------------------------------------------------------------------------------------------------
def _rodrigues_grad(r):
    G = torch.from_numpy(np.arange(9, dtype=np.float64).reshape(1, 3, 3) / 4 - 1).to(r.dtype)
    R = utils_3d.rodrigues(r)
    (g,) = torch.autograd.grad((R * G).sum(), r)
    return R.detach(), g


def test_rodrigues_matches_the_reference_with_both_series_inputs(golden):
    g = golden("flame_skin")
    r = torch.from_numpy(fc.RODRIGUES_VECTORS).requires_grad_(True)
    n = np.linalg.norm(fc.RODRIGUES_VECTORS, axis=1)
    assert n[0] == 0 and 0 < n[1] <= 1e-8 and 0 < n[2] <= 1e-8
    R, gr = _rodrigues_grad(r)
    assert R.shape == (len(r), 3, 3) and torch.isfinite(gr).all()
    assert np.abs(R.numpy() - g["rodrigues_R"]).max() < 1e-14
    assert np.abs(gr.numpy() - g["rodrigues_grad"]).max() < 1e-13
    one = utils_3d.rodrigues(torch.from_numpy(fc.RODRIGUES_VECTORS[3]))
    assert one.shape == (3, 3) and np.abs(one.numpy() - g["rodrigues_R_single"]).max() < 1e-14
    R32, g32 = _rodrigues_grad(torch.from_numpy(fc.RODRIGUES_VECTORS.astype(np.float32)).requires_grad_(True))
    assert rel(R32, g["rodrigues_R"]) < 1e-6 and rel(g32, g["rodrigues_grad"]) < 1e-5


def test_rodrigues_gradcheck_and_second_order():
    r = torch.from_numpy(synth.det_normal((4, 3), 77).astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(utils_3d.rodrigues, (r,))
    assert torch.autograd.gradgradcheck(utils_3d.rodrigues, (r,))


# ---- model -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_composite_node_matches_the_reference(golden, name):
    g = golden("flame_skin")
    case32 = build_case(name)
    check_against_fixture(g, name, node_outputs(*case32))
    case64 = build_case(name, dtype=torch.float64)
    check_against_fixture(g, name, node_outputs(*case64), float64=True)
    assert rel(case64[0].regulation(case64[2]), g[name + "_reg"]) < 1e-7
    assert rel(case32[0].regulation(case32[2]), g[name + "_reg"]) < 1e-5
    # forward() is the unposed mesh: v = forward(x) lin + t
    model, tri, coeff, pose = case64[:4]
    lin = torch.exp(pose[:, 6]).view(-1, 1, 1) * utils_3d.euler_mat(pose[:, :3], "yxz")
    v = torch.matmul(model(coeff), lin) + pose[:, 3:6].view(-1, 1, 3)
    assert rel(v[:, case64[6]], g[name + "_v"]) < 1e-7


def test_the_block_metric_sees_each_block(golden):
    """The metric of check_against_fixture fails where one max-norm over the whole gradient could not: a data gradient of
    zero is off by 1 in every block, an error in one joint's angles only is seen at that joint's own scale, and a prior
    entry that should be exactly zero must be."""
    g = golden("flame_skin")
    for name in fc.CASES:
        ds = fc.CASES[name][1]
        want = g[name + "_gcoeff_data"]
        assert min(fc.block_errors(np.zeros_like(want), want, ds).values()) == 1.0
        for k in range(ds, want.shape[1], 3):
            off = want.copy()
            off[:, k:k + 3] *= 1.01
            e = fc.block_errors(off, want, ds)
            assert e["beta"] == 0.0 and 0.009 < e["theta"] < 0.011, (name, k, e)
        total = g[name + "_gcoeff"]
        assert rel(total - want, total) < 1e-4 * 10          # what the whole-vector max-norm alone would have let through
    assert fc.elementwise_error(np.array([[1.0, 0.0]]), np.array([[1.0, 0.0]])) == 0.0
    assert fc.elementwise_error(np.array([[1.0, 1e-3]]), np.array([[1.0, 0.0]])) == float("inf")


def test_series_branch_sample_is_in_the_small_case():
    _, _, coeff, *_ = fc.case("small")
    ds = fc.CASES["small"][1]
    assert (coeff[1, ds + 3:ds + 6] == 0).all() and np.abs(coeff[1, ds:ds + 3]).max() > 0


def test_state_dict_keys_attributes_and_to():
    model, _ = face_model.load_flame(fc.flame_dict("small"))
    assert set(model.state_dict()) == {"sigma", "pose_mean", "pose_cov"}
    ds = fc.CASES["small"][1]
    nv = fc.flame_dict("small")["v_template"].shape[0]
    assert model.dim == [ds, 3 * (fc.NJ - 1), 3 * nv] and list(model.parent) == [0, 1, 1, 1]
    assert tuple(model.fc[0].shape) == (ds + 9 * (fc.NJ - 1), 3 * nv) and tuple(model.fc[1].shape) == (3 * nv,)
    assert tuple(model.weight[0].shape) == (nv, fc.NJ) and tuple(model.weight[1].shape) == (fc.NJ, nv)
    assert tuple(model.pose_cov.shape) == (4, 3, 3) and tuple(model.pose_inv.shape) == (4, 3, 3)
    assert model.pose_cov_is_diagonal()
    deg = np.array([10, 30, 5, 10, 1, 1, 10, 10, 1e-5, 10, 10, 1e-5]) * np.pi / 180
    assert np.allclose(torch.diagonal(model.pose_cov, dim1=1, dim2=2).reshape(-1).numpy(), deg, rtol=1e-6)
    assert not any(t.requires_grad for t in model.fc + model.weight)
    m64 = model.to(torch.float64)
    assert all(t.dtype == torch.float64 for t in m64.fc + m64.weight + [m64.pose_inv])
    other, _ = face_model.load_flame(fc.flame_dict("small"))
    with torch.no_grad():
        other.pose_mean.add_(1.0)
    other.load_state_dict(face_model.load_flame(fc.flame_dict("small"))[0].state_dict())
    assert float(other.pose_mean.abs().max()) == 0
    x = model.random_input(5)
    assert x.shape == (5, ds + 12) and torch.isfinite(x).all()
    # effective sigma reproduces the prior for a diagonal covariance
    m32, _ = face_model.load_flame(fc.flame_dict("small"))
    c = torch.from_numpy(fc.case("small")[2])
    assert torch.allclose(((c / m32.effective_sigma()) ** 2).sum(), m32.regulation(c), rtol=1e-5)


def test_learnable_model_takes_the_composite_and_gets_gradients():
    d = fc.flame_dict("small")
    nv = d["v_template"].shape[0]
    m = face_model.LinearBlendSkinningModel(nv, fc.NJ, 40, d["v_template"], d["J_regressor"], d["kintree_table"],
                                            d["weights"], d["posedirs"], d["shapedirs"], learnable=True)
    assert all(t.requires_grad for t in m.fc + m.weight)
    m(m.random_input(2)).sum().backward()
    assert all(t.grad is not None for t in m.fc + m.weight)


def test_out_of_order_kintree_raises_and_both_root_marks_agree():
    d = fc.flame_dict("small")
    nv = d["v_template"].shape[0]
    args = (nv, fc.NJ, 40, d["v_template"], d["J_regressor"])
    rest = (d["weights"], d["posedirs"], d["shapedirs"])
    with pytest.raises(ValueError):
        face_model.LinearBlendSkinningModel(*args, np.array([[-1, 2, 0, 1, 1], [0, 1, 2, 3, 4]]), *rest)
    with pytest.raises(ValueError):
        face_model.LinearBlendSkinningModel(*args, np.array([[0, -1, 1, 1, 1], [1, 0, 2, 3, 4]]), *rest)
    a = face_model.LinearBlendSkinningModel(*args, fc.kintree(-1), *rest)
    b = face_model.LinearBlendSkinningModel(*args, fc.kintree(2 ** 32 - 1), *rest)
    assert fc.kintree(2 ** 32 - 1).dtype == np.uint32 and list(a.parent) == list(b.parent) == [0, 1, 1, 1]
    x = a.random_input(2)
    assert torch.equal(a(x), b(x))


def test_missing_weights_fall_back_to_the_nearest_joint():
    d = fc.flame_dict("small")
    nv = d["v_template"].shape[0]
    m = face_model.LinearBlendSkinningModel(nv, fc.NJ, 40, d["v_template"], d["J_regressor"], d["kintree_table"], None,
                                            d["posedirs"], d["shapedirs"])
    w = m.weight[0].numpy()
    assert ((w > 0).sum(1) <= 1).all() and np.allclose(w.sum(1)[w.sum(1) > 0], 1)
    joints = m.weight[1].numpy() @ d["v_template"].astype(np.float32)
    near = ((d["v_template"][:, None] - joints[None]) ** 2).sum(2).argmin(1)
    assert (w.argmax(1)[w.sum(1) > 0] == near[w.sum(1) > 0]).all()


def test_load_flame_from_dict_pickle_and_mat(tmp_path):
    import scipy.io as sio

    d = fc.flame_dict("small")
    pkl, mat = str(tmp_path / "flame.pkl"), str(tmp_path / "flame.mat")
    with open(pkl, "wb") as f:
        pickle.dump(d, f, protocol=2)
    sio.savemat(mat, d)
    ref, tri = face_model.load_flame(d)
    assert tri.dtype == torch.int64 and int(tri.min()) == 0 and tri.shape[1] == 3
    for path in (pkl, mat):
        m, t = face_model.load_flame(path)
        assert torch.equal(t, tri) and m.dim == ref.dim and list(m.parent) == list(ref.parent)
        for a, b in zip(m.fc + m.weight + [m.sigma, m.pose_cov], ref.fc + ref.weight + [ref.sigma, ref.pose_cov]):
            assert torch.equal(a, b)
    with pytest.raises(ValueError):
        face_model.load_flame(str(tmp_path / "flame.txt"))


# ---- inverter --------------------------------------------------------------------------------------------------------
def tiny_flame(device="cpu"):
    from stylerenderer_amd import train

    fm, t = face_model.load_flame(train.synthetic_flame_dict(8, mesh=synth.uv_ellipsoid(10, 12), shape_amplitude=0.02,
                                                             pose_amplitude=0.01))
    return fm.to(device), t.to(device)


FACES = ((5, 3, (0.2, -0.1, 0.05, 0.03, -0.02, 0.0, 0.05)), (21, 23, (-0.25, 0.08, 0.0, -0.04, 0.01, 0.0, -0.05)))


def flame_problem(device="cpu", faces=FACES):
    """(g, face, noise, targets [len(faces), 3, 16, 16]): images of the tiny generator on skinned meshes."""
    from test_inversion_cpu import tiny_setup

    g, _ = tiny_setup(device)
    fm, tri = tiny_flame(device)
    noise = [torch.from_numpy(synth.det_normal((1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)), 40 + i)).to(device)
             for i in range(g.num_layers)]
    ims = []
    with torch.no_grad():
        for ws, cs, p in faces:
            c = torch.from_numpy(synth.det_normal((1, 20), cs)).to(device) * 0.3
            v, n, _ = skin.skin_mesh(fm, c, torch.tensor([p], device=device), tri)
            w = g.style(torch.from_numpy(synth.det_normal((1, 32), ws)).to(device)).unsqueeze(1).repeat(1, g.n_latent, 1)
            img, _, _ = g([w], (v.contiguous(), n.contiguous(), tri), input_is_latent=True, noise=noise)
            ims.append(img)
    return g, (fm, tri), noise, torch.cat(ims, 0)


def make_inverter(g, face, noise, target, shape_reg=1e-3, **kw):
    torch.manual_seed(3)
    return inversion.LatentInverter(g, lpips.PNetLin(), target, None, lr=0.05, pose_lr=0.02, noise=noise,
                                    n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=shape_reg, **kw)


def test_inverter_with_a_skinned_model_moves_shape_joints_and_pose():
    # no prior here: FLAME's eye-roll sigma (1e-5 degrees) makes the prior of any Adam step of 0.05 rad dominate the loss
    g, face, noise, targets = flame_problem()
    inv = make_inverter(g, face, noise, targets[:1], shape_reg=0.0)
    assert inv.skinned and torch.equal(inv.coeff, torch.zeros(1, 20))
    hist = inv.run(8).numpy()
    assert np.isfinite(hist).all() and hist[-1] < hist[0]
    c = inv.coeff.detach()
    assert float(c[:, :8].abs().max()) > 1e-3 and float(c[:, 8:].abs().max()) > 1e-3
    assert float(inv.pose.detach().abs().max()) > 1e-3
    v, n, tri = inv.fitted_mesh()
    want, _, _ = skin.skin_mesh(face[0], c, inv.pose.detach().view(1, 7), tri)
    assert v.shape == (1, 110, 3) and torch.equal(v, want)


def test_batch_gradients_are_the_single_image_gradients():
    """As test_reconstruct_batch_cpu: d(sum_j L_j)/d x_b = dL_b/d x_b, fp32 summation order of batched CPU kernels only;
    the bar is that test's 1e-4.  The per-sample prior rows come from fit_loss_rows with the effective sigma."""
    g, face, noise, targets = flame_problem()
    batched = first_gradients(make_inverter(g, face, noise, targets))
    assert batched[3].shape == (2, 20)
    for b in range(2):
        single = first_gradients(make_inverter(g, face, noise, targets[b:b + 1]))
        for k, (got, want) in enumerate(zip(batched, single)):
            err = float((got[b:b + 1] - want).abs().max() / want.abs().max())
            print("sample", b, "term", k, "rel", err)
            assert err <= 1e-4, (b, k, err)
            assert float(want.abs().max()) > 0


def test_batched_rows_carry_the_prior():
    g, face, noise, targets = flame_problem()
    inv = make_inverter(g, face, noise, targets)
    with torch.no_grad():
        inv.coeff.copy_(torch.from_numpy(synth.det_normal((2, 20), 91)) * 0.1)
    total = inv.loss(inv.render())
    rows = inv._rows.detach()
    assert torch.allclose(rows.sum(), total.detach(), rtol=1e-5)
    inv0 = make_inverter(g, face, noise, targets)
    inv0.shape_reg = 0.0
    with torch.no_grad():
        inv0.coeff.copy_(inv.coeff)
    inv0.loss(inv0.render())
    want = torch.stack([1e-3 * face[0].regulation(inv.coeff.detach()[b:b + 1]) for b in range(2)])
    assert torch.allclose(rows - inv0._rows.detach(), want, rtol=1e-3, atol=1e-7)


def test_batched_fit_refuses_a_full_pose_covariance():
    g, face, noise, targets = flame_problem()
    fm, tri = face
    with torch.no_grad():
        fm.pose_cov[0, 0, 1] = 0.01
    with pytest.raises(ValueError):
        make_inverter(g, (fm, tri), noise, targets)
    make_inverter(g, (fm, tri), noise, targets[:1])                   # a single image goes through the node's own prior


# ---- recovery through the rasterizer ---------------------------------------------------------------------------------
RECOVERY_STEPS, RECOVERY_LR = 400, 0.02


def recovery_fit(device, dtype, steps=RECOVERY_STEPS, lr=RECOVERY_LR):
    """Normal map at 64^2 of a small skinned model at known (beta, theta, pose), the jaw clearly open; all three fitted
    from zero by Adam on the map's MSE.  Returns (relative error of [beta, theta], losses)."""
    from stylerenderer_amd import train
    from stylerenderer_amd.op.rasterize import rasterize

    ds = 4
    fm, t = face_model.load_flame(train.synthetic_flame_dict(ds, mesh=synth.uv_ellipsoid(24, 32), shape_amplitude=0.1,
                                                             pose_amplitude=0.01, key=931))
    fm, t = fm.to(device=device, dtype=dtype), t.to(device)
    truth = np.concatenate([0.8 * synth.det_normal((1, ds), 77), [[0.1, 0.15, 0.0, 0.45, 0.0, 0.0, 0, 0, 0, 0, 0, 0]]], 1)
    c_true = torch.from_numpy(truth).to(device=device, dtype=dtype)
    p_true = torch.tensor([[0.15, -0.1, 0.05, 0.02, -0.01, 0.0, 0.05]], device=device, dtype=dtype)

    def render(c, p):
        v, n, _ = skin.skin_mesh(fm, c, p, t)
        return rasterize(v.contiguous(), n.contiguous(), t, 64, 64, channel_major=True)

    with torch.no_grad():
        target = render(c_true, p_true)
    c = torch.zeros_like(c_true).requires_grad_(True)
    p = torch.zeros_like(p_true).requires_grad_(True)
    opt = torch.optim.Adam([c, p], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ((render(c, p) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return float((c.detach() - c_true).norm() / c_true.norm()), losses


def test_recovery_settings_meet_the_bar_with_the_float64_composite():
    """The step count and learning rate of the device test (test_flame_gpu) bring the float64 composite, the reference's
    algebra, below that test's bars: relative error of [beta, theta] < 0.1, loss below a tenth of its start."""
    err, losses = recovery_fit(torch.device("cpu"), torch.float64)
    print("float64 composite recovery: relative error", err, "loss", losses[0], "->", losses[-1])
    assert err < 0.1 and losses[-1] < 0.1 * losses[0]


# ---- command line ----------------------------------------------------------------------------------------------------
def _write_flame(path):
    d = fc.flame_dict("small")
    with open(path, "wb") as f:
        pickle.dump(d, f, protocol=2)
    return d["v_template"].shape[0], d["f"].shape[0]


def test_reconstruct_cli_with_flame(tmp_path):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_a.npy")
    np.save(img, synth.det_uniform((3, 24, 24), 9))
    flame = str(tmp_path / "flame.pkl")
    nv, nf = _write_flame(flame)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "4", "--n_mean_latent",
           "64", "--flame", flame, "--out", out, ckpt, img]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(["face_a.obj", "face_a_canonical.obj", "face_a_render.png",
                                              "face_a_normal.png", "face_a.npz"])
    for obj in ("face_a.obj", "face_a_canonical.obj"):
        assert _obj_counts(os.path.join(out, obj)) == {"v": nv, "vn": nv, "f": nf}
    r = np.load(os.path.join(out, "face_a.npz"))
    assert r["coeff"].shape == (1, 52) and r["pose"].shape == (7,) and r["joints"].shape == (4, 3)
    assert np.array_equal(r["joints"].reshape(-1), r["coeff"][0, 40:])
    assert r["loss"].shape == (4,) and np.isfinite(r["loss"]).all() and float(np.abs(r["joints"]).max()) > 0
    both = subprocess.run(cmd[:-2] + ["--bfm", "x.mat", ckpt, img], env=_env(), cwd=str(tmp_path), capture_output=True,
                          text=True, timeout=600)
    assert both.returncode != 0 and "not allowed with" in both.stderr


def test_train_cli_with_flame(tmp_path):
    flame = str(tmp_path / "flame.pkl")
    _write_flame(flame)
    cmd = [sys.executable, "-m", "stylerenderer_amd.train", "--size", "16", "--latent", "32", "--n_mlp", "2",
           "--batch", "2", "--iter", "2", "--mesh", "--flame", flame]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.count("iter ") == 2


def test_flame_face_source_has_the_sample_contract(tmp_path):
    from stylerenderer_amd import train

    flame = str(tmp_path / "flame.pkl")
    nv, _ = _write_flame(flame)
    src = train.FlameFaceSource(torch.device("cpu"), flame)
    v, n, t = src.sample(2)
    assert v.shape == (2, nv, 3) and n.shape == v.shape and t is src.tri and not v.requires_grad
