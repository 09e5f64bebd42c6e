"""CPU: the FaceWarehouse bilinear blendshape model — BlendShapeModel / load_facewarehouse and the blendshape node's
composite path against the reference (fixture of make_golden_blendshape.py), the sampler's moments, the inverter with a
blendshape model (single and batched), `reconstruct --facewarehouse` and `train --mesh --facewarehouse`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import blendshape_cases as bc
from stylerenderer_amd import face_model, inversion, lpips, synth
from stylerenderer_amd.op import blend
from test_reconstruct_batch_cpu import first_gradients
from test_reconstruct_cpu import NOMINAL, _env, _obj_counts, bar, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_case(name, device="cpu", dtype=torch.float32):
    """(model, tri, coeff, pose, gv, gn, idx) of a fixture case as tensors."""
    d, tri, beta_shape, coeff, pose, gv, gn, idx = bc.case(name)
    model, t = face_model.load_facewarehouse(d, beta_shape)
    assert np.array_equal(t.numpy(), tri)
    to = lambda a: torch.from_numpy(a).to(device=device, dtype=dtype)           # noqa: E731
    return model.to(device=device, dtype=dtype), t.to(device), to(coeff), to(pose), to(gv), to(gn), idx


def node_outputs(model, tri, coeff, pose, gv, gn, idx, reg_weight=bc.REG_WEIGHT, node=None):
    """v, n at the sample, reg, the gradients of L = sum(v gv) + sum(n gn) + REG_WEIGHT regulation(coeff), and the
    coefficient gradient's two parts: of the data term alone and of regulation(coeff) alone (through the node's `reg`)."""
    node = node or blend.blend_mesh
    c = coeff.clone().requires_grad_(True)
    p = pose.clone().requires_grad_(True)
    v, n, reg = node(model, c, p, tri, reg_weight)
    loss = (v * gv).sum() + (n * gn).sum() + reg
    gc, gp = torch.autograd.grad(loss, (c, p))
    v1, n1, reg1 = node(model, c, p, tri, 1.0)
    if c.shape[1]:
        (gc_data,) = torch.autograd.grad((v1 * gv).sum() + (n1 * gn).sum(), c, retain_graph=True)
        (gc_prior,) = torch.autograd.grad(reg1, c)
    else:
        gc_data = gc_prior = torch.zeros_like(c)
    out = {"v": v.detach()[:, idx], "n": n.detach()[:, idx], "gcoeff": gc, "gpose": gp, "gcoeff_data": gc_data,
           "gcoeff_prior": gc_prior, "reg": reg1.detach()}
    return {k: x.cpu().double().numpy() for k, x in out.items()}


def rule(nominal, err32):
    """test_reconstruct_cpu's rule for an fp32 bar: 4x the reference's own fp32 error, at least nominal, at most 10x."""
    return min(10 * nominal, max(nominal, 4 * float(err32)))


def check_against_fixture(g, name, got, float64=False):
    """Every output against the fixture.  fp32: test_reconstruct_cpu's bars; float64: 1e-7.  The coefficient gradient as
    a whole (the issue's L), in its two parts, and the prior's part entry by entry against its own magnitude; the prior
    value at the coefficient gradient's bar."""
    for key in NOMINAL:
        want = g["%s_%s" % (name, key)]
        assert got[key].shape == want.shape
        if want.size == 0:
            continue
        err, lim = rel(got[key], want), 1e-7 if float64 else bar(g, name, key)
        print(name, key, "rel", err, "bar", lim)
        assert err < lim if float64 else err <= lim, (name, key, err, lim)
    if got["gcoeff"].size:
        for key in ("gcoeff_data", "gcoeff_prior"):
            err = rel(got[key], g["%s_%s" % (name, key)])
            lim = 1e-7 if float64 else rule(NOMINAL["gcoeff"], g["%s_%s_err32" % (name, key)])
            print(name, key, "rel", err, "bar", lim)
            assert err <= lim, (name, key, err, lim)
        err = bc.elementwise_error(got["gcoeff_prior"], g[name + "_gcoeff_prior"])
        lim = 1e-7 if float64 else rule(NOMINAL["gcoeff"], g[name + "_gcoeff_prior_elem_err32"])
        print(name, "gcoeff_prior elementwise rel", err, "bar", lim)
        assert err <= lim, (name, err, lim)
    want = float(g[name + "_reg"])
    err = abs(float(got["reg"]) - want) / max(abs(want), 1e-30) if want != 0 else abs(float(got["reg"]))
    lim = 1e-7 if float64 else rule(NOMINAL["gcoeff"], g[name + "_reg_err32"])
    print(name, "reg rel", err, "bar", lim)
    assert err <= lim, (name, err, lim)


# ---- model -----------------------------------------------------------------------------------------------------------
def test_the_cases_sit_on_both_sides_of_every_threshold():
    rows = {name: c for name, c in bc.CASES.items() if c[0] != "face"}
    assert {3 * c[0] % 4 for c in rows.values()} == {0, 1, 2, 3}
    assert {c[3] for c in bc.CASES.values()} >= {1, 3, 8, 9}
    assert any(c[1] == 0 for c in rows.values()) and any(c[2] == 0 for c in rows.values())
    assert any(c[4] == .01 for c in rows.values()) and any(np.min(c[4]) >= 1 for c in rows.values())
    assert float(np.abs(bc.case("large")[3]).max()) == 30.0


@pytest.mark.parametrize("name", list(bc.CASES))
def test_composite_node_matches_the_reference(golden, name):
    g = golden("blendshape")
    case32 = build_case(name)
    check_against_fixture(g, name, node_outputs(*case32))
    case64 = build_case(name, dtype=torch.float64)
    check_against_fixture(g, name, node_outputs(*case64), float64=True)
    # forward() is the unposed mesh, and the per-sample priors add up to regulation
    model, tri, coeff, pose = case64[:4]
    _, _, reg, rows = blend.blend_mesh(model, coeff, pose, tri, 0.5, per_sample=True)
    assert rows.shape == (coeff.shape[0],) and torch.allclose(rows.sum(), reg, rtol=1e-12, atol=1e-12)
    for b in range(coeff.shape[0]):
        assert torch.allclose(rows[b], 0.5 * model.regulation(coeff[b:b + 1]), rtol=1e-12, atol=1e-12)
    assert model(coeff).shape == (coeff.shape[0], model.dim[2] // 3, 3)


def test_gradcheck_of_the_composite():
    d = bc.facewarehouse_dict(7, 3, 2, 4411)
    model, tri = face_model.load_facewarehouse(d, 1.5)
    model = model.to(torch.float64)
    c = torch.from_numpy(synth.det_normal((2, 5), 4412).astype(np.float64)).requires_grad_(True)
    p = (0.2 * torch.from_numpy(synth.det_normal((2, 7), 4413).astype(np.float64))).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c_, p_: blend.blend_composite(model, c_, p_, tri, 0.3), (c, p))


def test_constructor_accepts_both_axis_orders_and_pads_beta(golden):
    g = golden("blendshape")
    ds, de = bc.BETA_DIMS
    for form, (bsh, bex) in bc.BETA_FORMS.items():
        m = face_model.BlendShapeModel(4, ds, de, None, bsh, bex)
        assert m.beta.shape == (ds + 1 + 2 * de,) and np.array_equal(m.beta.double().numpy(), g["beta_" + form]), form
    bs = synth.det_uniform((3, 4, 15), 4420)                         # [ds + 1, de + 1, 3 nv]
    a = face_model.BlendShapeModel(5, 2, 3, bs)
    b = face_model.BlendShapeModel(5, 2, 3, np.transpose(bs, [2, 0, 1]))       # [3 nv, ds + 1, de + 1]
    assert torch.equal(a.weight, b.weight) and np.array_equal(a.weight.numpy(), bs)
    assert a.dim == [2, 3, 15] and not a.weight.requires_grad and not a.beta.requires_grad
    assert face_model.BlendShapeModel(5, 2, 3, bs, learnable=True).weight.requires_grad


def test_state_dict_is_the_references(golden):
    g = golden("blendshape")
    model = build_case("small")[0]
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_dict_keys"]] == ["beta", "weight"]
    for k, t in sd.items():
        assert tuple(t.shape) == tuple(g["state_dict_shape_" + k])
    other = face_model.BlendShapeModel(40, 5, 3)
    other.load_state_dict(sd)
    assert torch.equal(other.weight, model.weight) and torch.equal(other.beta, model.beta)


def test_loader_contract(tmp_path):
    import scipy.io as sio

    d = bc.facewarehouse_dict(40, 5, 3, 4430)
    model, tri = face_model.load_facewarehouse(d)
    assert model.dim == [5, 3, 120] and tuple(model.weight.shape) == (6, 4, 120)
    assert float(model.beta[:6].min()) == float(model.beta[:6].max()) == np.float32(.01)
    assert model.beta[6:].tolist() == [1, 10] * 3
    # mean-centring per axis, the vertex coordinate last
    centre = d["v"].mean(1)
    want = (d["p"] - np.tile(centre, 40).reshape(-1, 1, 1)).transpose(2, 1, 0).astype(np.float32)
    assert np.array_equal(model.weight.numpy(), want)
    assert tri.dtype == torch.int64 and tri.shape[1] == 3 and int(tri.min()) == 0
    assert np.array_equal(tri.numpy(), d["tri"].astype(np.int64) - 1)
    # tri transposed and on another base
    rows = bc.facewarehouse_dict(40, 5, 3, 4430, tri_rows=True, base=7)
    assert rows["tri"].shape[0] == 3 and torch.equal(face_model.load_facewarehouse(rows)[1], tri)
    # .mat round trip
    mat = str(tmp_path / "fw.mat")
    sio.savemat(mat, d)
    m2, t2 = face_model.load_facewarehouse(mat, beta_shape=2.0)
    assert torch.equal(t2, tri) and torch.equal(m2.weight, model.weight) and float(m2.beta[0]) == 2.0


def test_forward_at_zero_is_the_mean_identity_at_half_expressions():
    model = build_case("small")[0]
    xs, xe = model.mixing_weights(torch.zeros(1, 8))
    assert torch.allclose(xs, torch.full((1, 6), 1 / 6)) and torch.allclose(xe, torch.tensor([[-0.5, 0.5, 0.5, 0.5]]))
    want = torch.einsum("i,j,ijc->c", xs[0], xe[0], model.weight).view(1, 40, 3)
    assert torch.allclose(model(torch.zeros(1, 8)), want, atol=1e-6)


def test_learnable_model_takes_the_composite_and_gets_gradients():
    d = bc.facewarehouse_dict(40, 5, 3, 4430)
    bs = np.transpose(d["p"], [2, 1, 0])
    m = face_model.BlendShapeModel(40, 5, 3, bs, learnable=True)
    m(m.random_input(2)).sum().backward()
    assert m.weight.grad is not None and float(m.weight.grad.abs().max()) > 0


# ---- sampler ---------------------------------------------------------------------------------------------------------
N_SAMPLES = 40000


def test_random_input_reproduces_the_dirichlet_and_beta_moments():
    """N = 40 000 draws; the mean of each identity weight against beta_i / sum beta and of each expression weight against
    a / (a + b), within 5 standard errors sqrt(var / N) with the analytic variances beta_i (B - beta_i) / (B^2 (B + 1))
    and a b / ((a + b)^2 (a + b + 1))."""
    torch.manual_seed(5)
    bsh, bex = [2.0, 3.0, 5.0, 1.5], [2, 5, 4, 1, 1, 10]
    m = face_model.BlendShapeModel(4, 3, 3, None, bsh, bex)
    x = m.random_input(N_SAMPLES)
    assert x.shape == (N_SAMPLES, 6) and torch.isfinite(x).all() and x.device == m.beta.device
    xs, xe = m.mixing_weights(x.double())
    beta = np.array(bsh)
    total = beta.sum()
    mean, var = beta / total, beta * (total - beta) / (total ** 2 * (total + 1))
    err = np.abs(xs.mean(0).numpy() - mean) / np.sqrt(var / N_SAMPLES)
    print("identity: standard errors off", err)
    assert (err <= 5).all(), err
    a, b = np.array(bex[0::2], np.float64), np.array(bex[1::2], np.float64)
    mean, var = a / (a + b), a * b / ((a + b) ** 2 * (a + b + 1))
    err = np.abs(xe[:, 1:].mean(0).numpy() - mean) / np.sqrt(var / N_SAMPLES)
    print("expression: standard errors off", err)
    assert (err <= 5).all(), err


def test_random_input_is_finite_at_the_loaders_beta_and_full_size():
    """beta = .01: nearly every draw sits in one corner of the simplex; the mean alone is compared (5 standard errors of
    the analytic variance, N = 40 000)."""
    torch.manual_seed(6)
    m = face_model.BlendShapeModel(2, 149, 46, None, .01)
    x = m.random_input(N_SAMPLES)
    assert x.shape == (N_SAMPLES, 195) and torch.isfinite(x).all()
    xs, _ = m.mixing_weights(x.double())
    total = 1.5
    var = .01 * (total - .01) / (total ** 2 * (total + 1))
    err = np.abs(xs.mean(0).numpy() - 1 / 150) / np.sqrt(var / N_SAMPLES)
    print("identity at beta = .01: largest deviation in standard errors", err.max())
    assert (err <= 5).all(), err.max()
    assert face_model.BlendShapeModel(2, 3, 0).random_input(4).shape == (4, 3)
    assert face_model.BlendShapeModel(2, 0, 0).random_input(4).shape == (4, 0)


# ---- inverter --------------------------------------------------------------------------------------------------------
def tiny_blendshape(device="cpu", beta_shape=2.0):
    from stylerenderer_amd import train

    fm, t = face_model.load_facewarehouse(train.synthetic_facewarehouse_dict(5, 4, mesh=synth.uv_ellipsoid(10, 12),
                                                                             shape_amplitude=0.06,
                                                                             expression_amplitude=0.06), beta_shape)
    return fm.to(device), t.to(device)


FACES = ((5, 3, (0.2, -0.1, 0.05, 0.03, -0.02, 0.0, 0.05)), (21, 23, (-0.25, 0.08, 0.0, -0.04, 0.01, 0.0, -0.05)))


def blendshape_problem(device="cpu", faces=FACES, beta_shape=2.0):
    """(g, face, noise, targets [len(faces), 3, 16, 16]): images of the tiny generator on blendshape meshes."""
    from test_inversion_cpu import tiny_setup

    g, _ = tiny_setup(device)
    fm, tri = tiny_blendshape(device, beta_shape)
    noise = [torch.from_numpy(synth.det_normal((1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)), 40 + i)).to(device)
             for i in range(g.num_layers)]
    ims = []
    with torch.no_grad():
        for ws, cs, p in faces:
            c = torch.from_numpy(synth.det_normal((1, 9), cs)).to(device)
            v, n, _ = blend.blend_mesh(fm, c, torch.tensor([p], device=device), tri)
            w = g.style(torch.from_numpy(synth.det_normal((1, 32), ws)).to(device)).unsqueeze(1).repeat(1, g.n_latent, 1)
            img, _, _ = g([w], (v.contiguous(), n.contiguous(), tri), input_is_latent=True, noise=noise)
            ims.append(img)
    return g, (fm, tri), noise, torch.cat(ims, 0)


def make_inverter(g, face, noise, target, shape_reg=1e-3, **kw):
    torch.manual_seed(3)
    return inversion.LatentInverter(g, lpips.PNetLin(), target, None, lr=0.05, pose_lr=0.02, noise=noise,
                                    n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=shape_reg, **kw)


def test_inverter_with_a_blendshape_model_moves_identity_expression_and_pose():
    g, face, noise, targets = blendshape_problem()                   # beta_shape = 2: a prior that pulls to the mean
    inv = make_inverter(g, face, noise, targets[:1])
    assert inv.blended and not inv.skinned and torch.equal(inv.coeff, torch.zeros(1, 9))
    hist = inv.run(8).numpy()
    assert np.isfinite(hist).all() and hist[-1] < hist[0]
    c = inv.coeff.detach()
    assert float(c[:, :5].abs().max()) > 1e-3 and float(c[:, 5:].abs().max()) > 1e-3
    assert float(inv.pose.detach().abs().max()) > 1e-3
    v, n, tri = inv.fitted_mesh()
    want, _, _ = blend.blend_mesh(face[0], c, inv.pose.detach().view(1, 7), tri)
    assert v.shape == (1, 110, 3) and torch.equal(v, want)


def test_batch_gradients_are_the_single_image_gradients():
    """As test_reconstruct_batch_cpu: d(sum_j L_j)/d x_b = dL_b/d x_b, fp32 summation order of batched CPU kernels only;
    the bar is that test's 1e-4.  The coefficients start away from zero so that the prior's gradient is not zero."""
    g, face, noise, targets = blendshape_problem()
    start = torch.from_numpy(synth.det_normal((2, 9), 91)) * 0.3

    def grads(target, rows):
        inv = make_inverter(g, face, noise, target)
        with torch.no_grad():
            inv.coeff.copy_(start[rows])
        return first_gradients(inv)

    batched = grads(targets, slice(0, 2))
    assert batched[3].shape == (2, 9)
    for b in range(2):
        single = grads(targets[b:b + 1], slice(b, b + 1))
        for k, (got, want) in enumerate(zip(batched, single)):
            err = float((got[b:b + 1] - want).abs().max() / want.abs().max())
            print("sample", b, "term", k, "rel", err)
            assert err <= 1e-4, (b, k, err)
            assert float(want.abs().max()) > 0


def test_batched_rows_carry_each_samples_own_prior():
    g, face, noise, targets = blendshape_problem()
    inv = make_inverter(g, face, noise, targets)
    with torch.no_grad():
        inv.coeff.copy_(torch.from_numpy(synth.det_normal((2, 9), 91)) * 0.3)
    total = inv.loss(inv.render())
    rows = inv._rows.detach()
    assert torch.allclose(rows.sum(), total.detach(), rtol=1e-5)
    inv0 = make_inverter(g, face, noise, targets)
    inv0.shape_reg = 0.0
    with torch.no_grad():
        inv0.coeff.copy_(inv.coeff)
    inv0.loss(inv0.render())
    want = torch.stack([1e-3 * face[0].regulation(inv.coeff.detach()[b:b + 1]) for b in range(2)])
    assert float(want.abs().min()) > 1e-6 and float((want[0] - want[1]).abs()) > 1e-6
    assert torch.allclose(rows - inv0._rows.detach(), want, rtol=1e-3, atol=1e-7)


def test_fit_loss_rows_is_unchanged_without_prior_rows():
    from stylerenderer_amd.op import lpips_layer

    layers = [torch.from_numpy(synth.det_uniform((3,), 60 + i)).abs() for i in range(5)]
    m = torch.from_numpy(synth.det_uniform((3,), 70)).abs()
    rows, total = lpips_layer.fit_loss_rows(layers, m, 0.7)
    pr = torch.tensor([0.1, -0.2, 0.3])
    reg = pr.sum().requires_grad_(True)
    rows2, total2 = lpips_layer.fit_loss_rows(layers, m, 0.7, reg=reg, prior_rows=pr)
    assert torch.allclose(rows2, rows + pr) and torch.allclose(total2, total + reg) and not rows2.requires_grad
    total2.backward()
    assert float(reg.grad) == 1.0
    with pytest.raises(ValueError):
        lpips_layer.fit_loss_rows(layers, m, 0.7, prior_rows=pr)


# ---- command line ----------------------------------------------------------------------------------------------------
def _write_mat(path, name="small"):
    import scipy.io as sio

    d = bc.case(name)[0]
    sio.savemat(path, d)
    return d["v"].shape[1], d["tri"].shape[0]


def test_reconstruct_cli_with_facewarehouse(tmp_path):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_a.npy")
    np.save(img, synth.det_uniform((3, 24, 24), 9))
    mat = str(tmp_path / "fw.mat")
    nv, nf = _write_mat(mat)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "4", "--n_mean_latent",
           "64", "--facewarehouse", mat, "--beta_shape", "2", "--out", out, ckpt, img]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(["face_a.obj", "face_a_canonical.obj", "face_a_render.png",
                                              "face_a_normal.png", "face_a.npz"])
    for obj in ("face_a.obj", "face_a_canonical.obj"):
        assert _obj_counts(os.path.join(out, obj)) == {"v": nv, "vn": nv, "f": nf}
    r = np.load(os.path.join(out, "face_a.npz"))
    assert r["coeff"].shape == (1, 8) and r["pose"].shape == (7,)
    assert r["identity"].shape == (6,) and r["expression"].shape == (4,)
    assert abs(float(r["identity"].sum()) - 1) < 1e-5 and abs(float(r["expression"].sum()) - 1) < 1e-5
    assert (r["identity"] > 0).all() and float(np.abs(r["coeff"]).max()) > 0
    assert r["loss"].shape == (4,) and np.isfinite(r["loss"]).all()
    for other in (["--bfm", "x.mat"], ["--flame", "x.pkl"]):
        both = subprocess.run(cmd[:-2] + other + [ckpt, img], env=_env(), cwd=str(tmp_path), capture_output=True,
                              text=True, timeout=600)
        assert both.returncode != 0 and "not allowed with" in both.stderr


def test_train_cli_with_facewarehouse(tmp_path):
    mat = str(tmp_path / "fw.mat")
    _write_mat(mat)
    cmd = [sys.executable, "-m", "stylerenderer_amd.train", "--size", "16", "--latent", "32", "--n_mlp", "2",
           "--batch", "2", "--iter", "2", "--mesh", "--facewarehouse", mat]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.count("iter ") == 2


def test_facewarehouse_face_source_has_the_sample_contract():
    from stylerenderer_amd import train

    d = train.synthetic_facewarehouse_dict(5, 4, mesh=synth.uv_ellipsoid(10, 12))
    assert d["p"].shape == (330, 5, 6) and d["v"].shape == (3, 110)
    src = train.FaceWarehouseFaceSource(torch.device("cpu"), d)
    v, n, t = src.sample(2)
    assert v.shape == (2, 110, 3) and n.shape == v.shape and t is src.tri and not v.requires_grad
    assert torch.isfinite(v).all() and torch.isfinite(n).all()
