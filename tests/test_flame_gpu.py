"""GPU: the skinning node (csrc/skin.hip) against the reference fixture and its float64 composite, determinism and launch
hygiene, model.forward, recovery of shape / joint angles / pose through the rasterizer, and the inverter with a skinned
model at full size."""
import os

import numpy as np
import pytest
import torch

import flame_cases as fc
from stylerenderer_amd import face_model, inversion, lpips, model, synth, train
from stylerenderer_amd.op import skin
from test_flame_cpu import build_case, check_against_fixture, node_outputs, recovery_fit, rule
from test_reconstruct_cpu import NOMINAL, rel

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
BANNED = ("aten::mm", "aten::addmm", "aten::mv", "aten::linear", "aten::matmul", "aten::bmm", "aten::index_add_",
          "aten::index_add", "aten::addmv", "aten::baddbmm")


@pytest.fixture(autouse=True)
def strict_native(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


@pytest.mark.parametrize("name", list(fc.CASES))          # "small": B = 3 (one zero joint rotation), "face": B = 1
def test_node_matches_the_reference_and_reruns_bit_identically(golden, name):
    g = golden("flame_skin")
    case = build_case(name, device=DEV)
    assert case[2].shape[0] == fc.CASES[name][2]
    got = node_outputs(*case)
    check_against_fixture(g, name, got)
    again = node_outputs(*case)
    for key in got:
        assert np.array_equal(got[key], again[key]), key


def _against_float64_composite(model_, tri, coeff, pose, gv, gn, reg_weight):
    """The native node against the float64 composite on the device inputs, every output and the coefficient gradient
    block by block (flame_cases.block_errors), the prior's gradient entry by entry.  The bars are test_reconstruct_cpu's
    rule with the fp32 error of the composite itself (the reference's algebra, run on the host) in the fixture's place."""
    import copy

    ds = model_.dim[0]
    every = slice(None)
    args64 = [copy.deepcopy(model_).to(torch.float64), tri] + [t.double() for t in (coeff, pose, gv, gn)]
    want = node_outputs(*args64, every, reg_weight, node=skin.skin_composite)
    args32 = [copy.deepcopy(model_).cpu(), tri.cpu()] + [t.cpu() for t in (coeff, pose, gv, gn)]
    ref32 = node_outputs(*args32, every, reg_weight, node=skin.skin_composite)
    got = node_outputs(model_, tri, coeff, pose, gv, gn, every, reg_weight)
    for key in ("v", "n", "gpose"):
        err, lim = rel(got[key], want[key]), rule(NOMINAL[key], rel(ref32[key], want[key]))
        print(key, "rel", err, "bar", lim)
        assert err <= lim, (key, err, lim)
    for key in ("gcoeff_data", "gcoeff"):
        e32 = fc.block_errors(ref32[key], want[key], ds)
        for blk, err in fc.block_errors(got[key], want[key], ds).items():
            lim = rule(NOMINAL["gcoeff"], e32[blk])
            print(key, blk, "rel", err, "bar", lim)
            assert err <= lim, (key, blk, err, lim)
    err = fc.elementwise_error(got["gcoeff_prior"], want["gcoeff_prior"])
    lim = rule(NOMINAL["gcoeff"], fc.elementwise_error(ref32["gcoeff_prior"], want["gcoeff_prior"]))
    print("gcoeff_prior elementwise rel", err, "bar", lim)
    assert err <= lim, (err, lim)
    c = coeff.clone()
    _, _, r = skin.skin_mesh(model_, c, pose, tri, reg_weight)
    rw = reg_weight * args64[0].regulation(args64[2])
    assert abs(float(r) - float(rw)) <= 1e-5 * abs(float(rw)) if reg_weight else float(r) == 0.0


@pytest.mark.parametrize("reg_weight", [0.0, 0.3])
@pytest.mark.parametrize("name", list(fc.CASES))
def test_node_matches_its_float64_composite(name, reg_weight):
    model_, tri, coeff, pose, gv, gn, _ = build_case(name, device=DEV)
    _against_float64_composite(model_, tri, coeff, pose, gv, gn, reg_weight)


def _t(shape, key):
    return torch.from_numpy(synth.det_normal(shape, key)).to(DEV)


def test_node_at_batch_8():
    model_, tri, _, _, _, _, _ = build_case("small", device=DEV)
    nv = model_.dim[2] // 3
    coeff = torch.cat([_t((8, 40), 811), 0.25 * _t((8, 12), 812)], 1)
    pose = _t((8, 7), 813) * torch.tensor([0.4, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1], device=DEV)
    _against_float64_composite(model_, tri, coeff, pose, _t((8, nv, 3), 814), _t((8, nv, 3), 815), fc.REG_WEIGHT)


def test_node_with_unequal_shape_sigmas_and_a_full_pose_covariance():
    """sigma_shape from 0.5 to 2 and a non-symmetric 3x3 pose_cov per joint, at a reg_weight whose prior gradient is of
    the data gradient's size: c / sigma^2 against c / sigma, and theta Pinv Pinv^T against theta Pinv Pinv, differ here."""
    d = fc.flame_dict("small")
    nv, ds = d["v_template"].shape[0], 40
    cov = np.concatenate([0.3 * (np.eye(3) + 0.3 * synth.det_uniform((3, 3), 830 + j)) for j in range(fc.NJ - 1)])
    model_ = face_model.LinearBlendSkinningModel(nv, fc.NJ, ds, d["v_template"], d["J_regressor"], d["kintree_table"],
                                                 d["weights"], d["posedirs"], d["shapedirs"],
                                                 sigma_shape=np.linspace(0.5, 2.0, ds), sigma_pose=cov.reshape(-1),
                                                 mean_pose=0).to(DEV)
    assert not model_.pose_cov_is_diagonal() and float((model_.pose_cov - model_.pose_cov.transpose(1, 2)).abs().max()) > 0
    tri = torch.from_numpy(fc.case("small")[1]).to(DEV)
    coeff = torch.cat([_t((3, ds), 821), 0.25 * _t((3, 12), 822)], 1)
    pose = _t((3, 7), 823) * torch.tensor([0.4, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1], device=DEV)
    gv, gn = _t((3, nv, 3), 824), _t((3, nv, 3), 825)
    out = node_outputs(model_, tri, coeff, pose, gv, gn, slice(None), 0.05)
    data, prior = np.abs(out["gcoeff_data"]), 0.05 * np.abs(out["gcoeff_prior"])
    assert 0.01 < prior[:, :ds].max() / data[:, :ds].max() < 100 and 0.01 < prior[:, ds:].max() / data[:, ds:].max() < 100
    _against_float64_composite(model_, tri, coeff, pose, gv, gn, 0.05)


def test_forward_slices_batches_beyond_one_launch():
    """B (D + 12 nj) floats of coefficients and transforms exceed one launch's LDS from B = 91 on for this model."""
    model_, tri, _, _, _, _, _ = build_case("small", device=DEV)
    x = torch.cat([_t((100, 40), 841), 0.25 * _t((100, 12), 842)], 1)
    v = model_(x)
    want = torch.cat([model_(x[:50]), model_(x[50:])], 0)
    assert torch.equal(v, want)
    m64 = face_model.load_flame(fc.flame_dict("small"))[0].to(torch.float64)
    assert rel(v.cpu(), m64(x.cpu().double()).numpy()) <= 1e-5


def test_strict_mode_refuses_the_composite_on_device_tensors():
    model_, tri, coeff, pose, _, _, _ = build_case("small", device=DEV)
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        skin.skin_mesh(model_, coeff.double(), pose.double(), tri)
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        model_(coeff.double())


def _big_flame():
    fm, tri = face_model.load_flame(train.synthetic_flame_dict())
    return fm.to(DEV), tri.to(DEV)


def test_node_dispatches_no_library_gemm_or_scatter():
    from torch.utils._python_dispatch import TorchDispatchMode

    fm, tri = _big_flame()
    c = torch.zeros(1, 156, device=DEV, requires_grad=True)
    p = torch.zeros(1, 7, device=DEV, requires_grad=True)
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func._schema.name in BANNED:
                seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    skin.skin_mesh(fm, c, p, tri, 1e-3)                       # incidence lists and the prepared model outside the spy
    with Spy():
        v, n, r = skin.skin_mesh(fm, c, p, tri, 1e-3)
        (v.square().sum() + n.sum() + r).backward()
    assert not seen, seen
    assert c.grad is not None and p.grad is not None and torch.isfinite(c.grad).all() and torch.isfinite(p.grad).all()
    assert float(c.grad[:, 144:].abs().max()) > 0


def test_model_forward_is_the_nodes_vertices_at_zero_pose():
    fm, tri = _big_flame()
    x = fm.random_input(3)
    v = fm(x)
    want, _, _ = skin.skin_mesh(fm, x, torch.zeros(3, 7, device=DEV), tri)
    assert v.shape == want.shape and torch.equal(v, want)
    m64 = face_model.load_flame(train.synthetic_flame_dict())[0].to(torch.float64)
    assert rel(v.cpu(), m64(x.cpu().double()).numpy()) <= 1e-5
    xg = x.clone().requires_grad_(True)
    fm(xg).square().sum().backward()
    assert torch.isfinite(xg.grad).all() and float(xg.grad.abs().max()) > 0


# ---- recovery through the rasterizer ---------------------------------------------------------------------------------
def test_shape_joints_and_pose_recovered_through_the_rasterizer():
    """The bar is test_coefficients_recovered_through_the_rasterizer's: relative error of [beta, theta] < 0.1 and the
    loss below a tenth of its start.  Step count and learning rate were chosen so that the identical fit with the float64
    composite on the CPU meets it (test_flame_cpu.test_recovery_settings_meet_the_bar_with_the_float64_composite)."""
    err, losses = recovery_fit(DEV, torch.float32)
    print("recovery: relative error", err, "loss", losses[0], "->", losses[-1])
    assert losses[-1] < 0.1 * losses[0]
    assert err < 0.1, err


# ---- the inverter at full size -----------------------------------------------------------------------------------------
_G256 = {}


def _setup():
    """The 256^2 generator and a skinned model on the face-sized mesh with usable prior sigmas (0.3 rad on every joint
    axis: load_flame's eye-roll sigma of 1e-5 degrees would make the prior of any Adam step dominate the loss), so that
    the inverter tests run with the prior on, as test_reconstruct_batch_gpu does."""
    if "g" not in _G256:
        g = model.GeneratorWithMap(256, 512, 8)
        synth.fill_state_dict(g.state_dict(), salt=7)
        _G256["g"] = g.to(DEV)
        d = train.synthetic_flame_dict()
        fm = face_model.LinearBlendSkinningModel(d["v_template"].shape[0], 5, 144, d["v_template"], d["J_regressor"],
                                                 d["kintree_table"], d["weights"], d["posedirs"], d["shapedirs"],
                                                 sigma_shape=1, sigma_pose=0.3)
        _G256["face"] = (fm.to(DEV), torch.from_numpy((d["f"].astype(np.int64) - 1)).to(DEV))
    return _G256["g"], _G256["face"]


def _noise():
    g, _ = _setup()
    return [torch.from_numpy(synth.det_normal(tuple(n.shape), 300 + i)).to(DEV) for i, n in enumerate(g.make_noise())]


def _faces(n):
    """n targets rendered from different latents, shapes, joint angles and poses (cached)."""
    if ("t", n) not in _G256:
        g, (fm, tri) = _setup()
        noise = _noise()
        ims = []
        with torch.no_grad():
            for k in range(n):
                c = torch.from_numpy(synth.det_normal((1, 156), 8 + k)).to(DEV) * 0.2
                p = torch.tensor([[0.2 - 0.1 * k, -0.1 + 0.05 * k, 0.0, 0.02 * k, 0.0, 0.0, 0.0]], device=DEV)
                v, nn_, _ = skin.skin_mesh(fm, c, p, tri)
                w = g.style(torch.from_numpy(synth.det_normal((1, 512), 9 + k)).to(DEV)).unsqueeze(1).repeat(
                    1, g.n_latent, 1)
                ims.append(g([w], (v, nn_, tri), input_is_latent=True, noise=noise)[0])
        _G256[("t", n)] = torch.cat(ims, 0)
    return _G256[("t", n)]


def _inverter(target, use_graph):
    g, face = _setup()
    torch.manual_seed(11)
    return inversion.LatentInverter(g, lpips.PNetLin().to(DEV), target, None, lr=0.05, pose_lr=0.01, noise=_noise(),
                                    n_mean_latent=256, use_graph=use_graph, face=face, fit_shape=True, coeff_lr=0.05,
                                    shape_reg=1e-3)


def _state(inv, hist):
    return [hist.cpu()] + [t.detach().cpu().clone() for t in (inv.w, inv.pose, inv.coeff)]


def test_skinned_inversion_full_size_graph_equals_eager_and_reset_equals_fresh():
    faces = _faces(2)
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = _inverter(faces[:1].contiguous(), use_graph)
        runs[key] = _state(inv, inv.run(30)) + [inv.graph is not None]
        if use_graph:
            # reset to another image: the next run is a fresh inverter's on that image, bit for bit
            other = faces[1:].contiguous()
            inv.reset(other)
            got = _state(inv, inv.run(30))
            fresh = _inverter(other, True)
            want = _state(fresh, fresh.run(30))
            del fresh
            for a, b in zip(got, want):
                assert torch.equal(a, b)
            assert not torch.equal(got[0], runs["graph"][0])
        del inv
    assert runs["graph"][4] and not runs["eager"][4]
    for key in ("eager", "graph"):
        hist, _, _, coeff = runs[key][:4]
        assert torch.isfinite(hist).all() and hist[-1] < hist[0]
        assert float(coeff[:, :144].abs().max()) > 1e-3 and float(coeff[:, 144:].abs().max()) > 1e-3
    for i in range(4):
        assert torch.equal(runs["graph"][i], runs["eager"][i]), i


def _first_gradients(inv):
    value = inv.loss(inv.render())
    value.backward()
    loss = inv._rows if inv.batch > 1 else value.detach().view(1)
    return [loss.detach()] + [x.grad.detach().clone().view(inv.batch, -1) for x in (inv.w, inv.pose, inv.coeff)]


def test_batch_gradients_match_single_image_gradients_and_every_loss_falls():
    """The form and bars of test_reconstruct_batch_gpu's test of this name: 2e-5 of the largest value on the loss and 2e-2
    on the norm of a gradient, the first-iteration gradients of each sample at B = 4 against that image alone at B = 1,
    with the prior on (shape_reg = 1e-3): the rows' prior comes from fit_loss_rows with the effective sigma, its gradient
    from the node's reg.  The coefficients start away from zero, so that the prior and its gradient are not zero."""
    faces = _faces(4)
    start = torch.from_numpy(0.05 * synth.det_normal((4, 156), 71)).to(DEV)

    def grads(target, rows):
        inv = _inverter(target, False)
        with torch.no_grad():
            inv.coeff.copy_(start[rows])
        return _first_gradients(inv), inv

    batched, inv = grads(faces, slice(0, 4))
    fm = inv.face_model
    prior = torch.stack([1e-3 * fm.regulation(start[b:b + 1]) for b in range(4)])
    assert float(prior.min()) > 1e-6                               # the prior is on in every row
    for b in range(4):
        single, _ = grads(faces[b:b + 1], slice(b, b + 1))
        assert float((batched[0][b] - single[0][0]).abs()) <= 2e-5 * float(single[0].abs().max()), b
        for k in (1, 2, 3):
            got, want = batched[k][b], single[k][0]
            err = float((got - want).norm() / want.norm())
            print("sample", b, "term", k, "rel", err)
            assert err <= 2e-2, (b, k, err)
    # the row of the batched loss holds the sample's prior: without it the row is lower by exactly that much
    inv0 = _inverter(faces, False)
    inv0.shape_reg = 0.0
    with torch.no_grad():
        inv0.coeff.copy_(start)
    inv0.loss(inv0.render())
    assert torch.allclose(batched[0] - inv0._rows.detach(), prior.to(batched[0].dtype), rtol=1e-3, atol=1e-7)
    inv = _inverter(faces, True)
    hist = inv.run(50).cpu()
    assert torch.isfinite(hist).all() and bool((hist[-1] < hist[0]).all()), hist[[0, -1]]


def test_reconstruct_cli_with_flame_on_the_device(tmp_path):
    import pickle
    import subprocess
    import sys

    g = model.GeneratorWithMap(256, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_b.npy")
    np.save(img, synth.det_uniform((256, 256, 3), 19))                   # HWC
    flame = str(tmp_path / "flame.pkl")
    with open(flame, "wb") as f:
        pickle.dump(train.synthetic_flame_dict(), f, protocol=2)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "256", "--steps", "8", "--n_mean_latent",
           "256", "--flame", flame, "--shape_reg", "1e-12", "--out", out, ckpt, img]
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(["face_b.obj", "face_b_canonical.obj", "face_b_render.png",
                                              "face_b_normal.png", "face_b.npz"])
    r = np.load(os.path.join(out, "face_b.npz"))
    assert r["loss"].shape == (8,) and np.isfinite(r["loss"]).all() and r["joints"].shape == (4, 3)
    assert float(np.abs(r["coeff"]).max()) > 0 and float(np.abs(r["joints"]).max()) > 0


def test_flame_face_source_samples_inside_a_captured_graph():
    """train --mesh --flame --graphs: sample() (random_input, the native forward, the pose, the normals) is capturable and
    every replay draws a new, finite batch."""
    from stylerenderer_amd import graphs

    src = train.FlameFaceSource(DEV, train.synthetic_flame_dict())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        src.sample(2)                                        # incidence lists and the prepared model before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out = {}

    def body():
        out["v"], out["n"], _ = src.sample(2)

    graph = graphs.capture(body)
    graph.replay()
    torch.cuda.synchronize()
    first = out["v"].clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and torch.isfinite(out["v"]).all() and torch.isfinite(out["n"]).all()
    assert first.shape == (2, src.model.dim[2] // 3, 3) and not torch.equal(first, out["v"])
    assert graph.kernel_nodes <= 16
