"""GPU: the photometric iteration of the latent fit (LatentInverter.run(steps, photometric=True)): eager against captured bit
for bit with all three face models, a camera, landmarks and a shared texture; reset + set_texture against a fresh inverter;
the texture's gradient inside the real step against the host composite; `reconstruct --photo` on the device."""
import os

import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, inversion, lpips, synth
from stylerenderer_amd.op import texture
from test_blendshape_cpu import blendshape_problem
from test_flame_cpu import flame_problem
from test_landmark_cpu import tiny_landmarks
from test_reconstruct_batch_cpu import batch_problem

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


_P = {}


def problem(kind):
    """(g, face, noise, targets) at 16^2 on the device: the tiny generator with the linear, skinned or blendshape stand-in."""
    if kind not in _P:
        if kind == "linear":
            g, _, face, noise, targets = batch_problem(DEV)
        elif kind == "flame":
            g, face, noise, targets = flame_problem(DEV)
        else:
            g, face, noise, targets = blendshape_problem(DEV)
        _P[kind] = (g, face, noise, targets)
    return _P[kind]


def layout_of(face):
    fm, tri = face
    with torch.no_grad():
        v = fm.mesh(torch.zeros(1, fm.n_coeff, device=DEV), torch.zeros(1, 7, device=DEV), tri)[0]
    return face_model.uv_layout(v[0].cpu(), tri)


def start_texture(bt, seed=70):
    return torch.from_numpy(synth.det_uniform((bt, 3, T, T), seed)).to(DEV) * 0.5


def inverter(kind, target, use_graph, **kw):
    g, face, noise, _ = problem(kind)
    torch.manual_seed(3)
    return inversion.LatentInverter(g, lpips.PNetLin().to(DEV), target, None, lr=0.05, pose_lr=0.02, noise=noise,
                                    n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3,
                                    use_graph=use_graph, photometric=layout_of(face), photo_size=T, photo_lr=0.02,
                                    photo_weight=2.0, **kw)


def state(inv, hist):
    out = [hist.cpu()] + [t.detach().cpu().clone() for t in (inv.w, inv.pose, inv.coeff, inv.texture)]
    if inv.camera is not None:
        out.append(inv.camera.detach().cpu().clone())
    return out


def linear_kw(b_n):
    host_face = batch_problem("cpu")[2]
    emb, lmk = tiny_landmarks(host_face)
    return dict(camera=[0.1, 0.25][:b_n], fit_camera=True, camera_lr=0.02, landmarks=np.stack([lmk] * b_n),
                landmark_embedding=emb)


CASES = [("linear", 1, {}), ("linear", 2, {"shared_identity": 10}), ("flame", 1, {}), ("facewarehouse", 1, {})]


@pytest.mark.parametrize("kind,b_n,more", CASES)
def test_photometric_iteration_eager_equals_captured(kind, b_n, more):
    targets = problem(kind)[3][:b_n].contiguous()
    kw = dict(more)
    if kind == "linear":
        kw.update(linear_kw(b_n))
    bt = 1
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = inverter(kind, targets, use_graph, **kw)
        assert tuple(inv.texture.shape) == (bt, 3, T, T)
        inv.set_texture(start_texture(bt))
        runs[key] = state(inv, inv.run(5, photometric=True))
        assert (inv.graph_photo is not None) == use_graph and inv.graph is None
        if use_graph:
            print(kind, "B", b_n, "photometric graph: kernel nodes", inv.graph_photo.kernel_nodes, "nodes",
                  inv.graph_photo.nodes, "memsets replaced", inv.graph_photo.memset_nodes_replaced)
            if kind == "linear":
                # a second picture through the captured graph equals a fresh inverter's run on it
                other = targets.flip(0).contiguous() if b_n > 1 else problem(kind)[3][1:2].contiguous()
                inv.reset(other, landmarks=kw["landmarks"])
                assert float(inv.texture.abs().max()) == 0.0
                inv.set_texture(start_texture(bt, 71))
                got = state(inv, inv.run(5, photometric=True))
                fresh = inverter(kind, other, True, **kw)
                fresh.set_texture(start_texture(bt, 71))
                want = state(fresh, fresh.run(5, photometric=True))
                del fresh
                for a, b in zip(got, want):
                    assert torch.equal(a, b)
        del inv
    for i, (a, b) in enumerate(zip(runs["graph"], runs["eager"])):
        assert torch.equal(a, b), (kind, b_n, i)
    hist, w, pose, coeff, tex = runs["graph"][:5]
    assert torch.isfinite(hist).all()
    assert float((tex - start_texture(bt).cpu()).abs().max()) > 0 and float(pose.abs().max()) > 0
    assert float(coeff.abs().max()) > 0


def test_per_row_textures_eager_equals_captured():
    targets = problem("linear")[3][:2].contiguous()
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = inverter("linear", targets, use_graph)
        assert tuple(inv.texture.shape) == (2, 3, T, T)                      # Bt = B without a shared identity
        inv.set_texture(start_texture(2))
        runs[key] = state(inv, inv.run(5, photometric=True))
        del inv
    for a, b in zip(runs["graph"], runs["eager"]):
        assert torch.equal(a, b)


def test_the_texture_gradient_of_a_step_is_the_host_composites():
    targets = problem("linear")[3][:2].contiguous()
    g, face, noise, _ = problem("linear")
    torch.manual_seed(3)
    inv = inversion.LatentInverter(g, lpips.PNetLin().to(DEV), targets, None, lr=0.05, pose_lr=0.02, noise=noise,
                                   n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3,
                                   use_graph=False, photometric=layout_of(face), photo_size=T, photo_lr=0.0,
                                   photo_weight=2.0, shared_identity=10)
    tex = start_texture(1)
    inv.set_texture(tex)
    texture._PLAN_CACHE.clear()
    inv.run(1, photometric=True)
    assert len(texture._PLAN_CACHE) == 0                                       # the list came from the planner
    assert torch.equal(inv.texture, tex)                                       # photo_lr = 0: the variable stood still
    got = inv.photo.texture.grad.detach().cpu()
    uvmap, cover = inv.photo.uvmap_fit.cpu(), inv.photo.cover_fit.cpu()
    t = tex.cpu().clone().requires_grad_(True)
    out = texture.sample_composite(t, uvmap, cover, 0.0)
    d = out - targets.cpu()
    rows = (cover.unsqueeze(1).to(out.dtype) * (d * d)).sum((1, 2, 3)) * inv.photo.scale
    (want,) = torch.autograd.grad(rows.sum(), t)
    print("texture gradient inside the step: mismatches", int((got != want).sum()), "of", want.numel(), "covered",
          int(cover.sum()))
    assert 0 < int(cover.sum()) < cover.numel() and float(want.abs().max()) > 0
    assert torch.equal(got, want)


# ---- the tool --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,images", [((), 1), (("--batch", "2"), 2), (("--multiview", "2"), 2),
                                          (("--light", "--texture_check"), 1)])
def test_reconstruct_with_photo_on_the_device(tmp_path, flags, images):
    from test_photometric_cpu import run_tool

    res, out = run_tool(tmp_path, "out", ("--photo", "--photo_steps", "6", "--gpu", "0") + flags,
                        {"SR_STRICT_NATIVE": "1"}, images=images)
    assert res.returncode == 0, res.stderr[-3000:]
    for stem in ["face_b", "face_c"][:images]:
        r = np.load(os.path.join(out, stem + ".npz"))
        assert r["photo_loss"].shape == (6,) and np.isfinite(r["photo_loss"]).all()
        assert 0 <= float(r["photo_error_before"]) <= 2 and 0 <= float(r["photo_error_after"]) <= 2
        assert os.path.isfile(os.path.join(out, stem + "_texture.png"))
        if "--texture_check" in flags:
            assert 0 <= float(r["rerender_error"]) <= 2 and "light" in r.files
    if "--multiview" in flags:
        assert os.path.isfile(os.path.join(out, "face_b_merged_texture.png"))
