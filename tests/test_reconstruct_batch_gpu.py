"""GPU: the batched inverter at 256^2 (LatentInverter with a target [B, 3, H, W]) — the per-sample loss kernels and the
batched pose node against float64 / autograd, batch independence, batch against single image, graph against eager,
reset, launch hygiene and `reconstruct --batch` on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import inversion, lpips, model, synth, utils_3d
from stylerenderer_amd.op import lpips_layer, morph
from test_reconstruct_gpu import _big_face, _g256

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 3, 8])
@pytest.mark.parametrize("n", [3 * 256 * 256, 8192 + 4099, 37])       # whole chunks; a scalar tail and odd rows; < 4 x 16
def test_mse_rows_against_float64(b, n):
    a = torch.from_numpy(synth.det_uniform((b, n), 80 + b)).to(DEV).requires_grad_(True)
    t = torch.from_numpy(synth.det_uniform((b, n), 90 + b)).to(DEV)
    out = lpips_layer.mse_rows(a, t)
    want = ((a.detach().double() - t.double()) ** 2).mean(1)
    assert out.shape == (b,)
    assert float((out.double() - want).abs().max() / want.abs().max()) <= 1e-5
    gout = torch.from_numpy(synth.det_normal((b,), 95)).to(DEV)
    (ga,) = torch.autograd.grad(out, a, gout)
    gwant = gout.double().view(b, 1) * 2.0 * (a.detach().double() - t.double()) / n
    assert float((ga.double() - gwant).abs().max() / gwant.abs().max()) <= 1e-6
    # reruns: bit-identical, and row r depends on row r only
    assert torch.equal(out, lpips_layer.mse_rows(a, t))
    assert torch.equal(ga, torch.autograd.grad(lpips_layer.mse_rows(a, t), a, gout)[0])
    if b > 1:
        a2 = a.detach().clone()
        a2[1:] = a2[1:].flip(1)
        assert torch.equal(lpips_layer.mse_rows(a2, t)[0], out[0])


def test_mse_rows_on_unaligned_rows():
    """Base pointers off a 16-byte boundary: the scalar path, same values as the aligned copy."""
    buf = torch.from_numpy(synth.det_uniform((3 * 1001 + 1,), 81)).to(DEV)
    tb = torch.from_numpy(synth.det_uniform((3 * 1001 + 1,), 82)).to(DEV)
    a, t = buf[1:].view(3, 1001), tb[1:].view(3, 1001)
    assert a.data_ptr() % 16 != 0
    got = lpips_layer.mse_rows(a, t)
    want = ((a.double() - t.double()) ** 2).mean(1)
    assert float((got.double() - want).abs().max() / want.abs().max()) <= 1e-5


def test_batched_pose_node_against_the_composite():
    pose = torch.from_numpy(0.3 * synth.det_normal((5, 7), 83)).to(DEV).requires_grad_(True)
    glin = torch.from_numpy(synth.det_normal((5, 3, 3), 84)).to(DEV)
    grot = torch.from_numpy(synth.det_normal((5, 3, 3), 85)).to(DEV)
    lin, rot = utils_3d.pose_matrices(pose)
    gp = torch.autograd.grad((lin * glin).sum() + (rot * grot).sum(), pose)[0]
    p64 = pose.detach().double().requires_grad_(True)
    lw, rw = utils_3d.pose_matrices(p64)                                   # float64: the composite tensor algebra
    gw = torch.autograd.grad((lw * glin.double()).sum() + (rw * grot.double()).sum(), p64)[0]
    assert float((lin.double() - lw).abs().max()) <= 1e-6 * float(lw.abs().max())
    assert float((rot.double() - rw).abs().max()) <= 1e-6
    assert float((gp.double() - gw).abs().max()) <= 1e-5 * float(gw.abs().max())
    assert float(gp[:, 3:6].abs().max()) == 0.0                            # the translation's gradient is affine3's
    lin2, rot2 = utils_3d.pose_matrices(pose)
    gp2 = torch.autograd.grad((lin2 * glin).sum() + (rot2 * grot).sum(), pose)[0]
    assert torch.equal(lin, lin2) and torch.equal(rot, rot2) and torch.equal(gp, gp2)


def test_one_pose_has_one_gradient_whether_given_as_7_or_1x7():
    """A pose given as [7] or as [1, 7] takes the single-pose entry point (sr_pose_bwd: pose_matrices sends seven numbers
    there whatever their shape), so the two gradients are the same bits.  A batch [2, 7] of that pose takes the batched
    kernel (sr_morph_pose_bwd): the same pose_bwd of csrc/pose.h, but built with floating-point contraction on where
    sr_pose_bwd's file has it off, so against it only the float64 bound of the test above is guaranteed, not the bits."""
    p7 = torch.from_numpy(0.3 * synth.det_normal((7,), 86)).to(DEV).requires_grad_(True)
    glin = torch.from_numpy(synth.det_normal((1, 3, 3), 87)).to(DEV)
    grot = torch.from_numpy(synth.det_normal((1, 3, 3), 88)).to(DEV)

    def grad(pose):
        lin, rot = utils_3d.pose_matrices(pose)
        return torch.autograd.grad((lin * glin).sum() + (rot * grot).sum(), pose)[0]

    g7 = grad(p7)
    g17 = grad(p7.detach().view(1, 7).clone().requires_grad_(True))
    g27 = grad(p7.detach().view(1, 7).repeat(2, 1).requires_grad_(True))
    gw = grad(p7.detach().double().requires_grad_(True))                   # float64: the composite tensor algebra
    assert g7.shape == (7,) and g17.shape == (1, 7) and g27.shape == (2, 7)
    print("gradient [7]", g7.tolist(), "[1, 7]", g17.tolist(), "[2, 7]", g27.tolist(), "float64", gw.tolist())
    assert torch.equal(g7[[0, 1, 2, 6]], g17[0, [0, 1, 2, 6]]) and float(g7[[0, 1, 2, 6]].abs().min()) > 0
    assert torch.equal(g7, grad(p7))
    assert torch.equal(g27[0], g27[1])
    for g in (g7, g17[0], g27[0]):
        assert float(g[3:6].abs().max()) == 0.0
        assert float((g.double() - gw).abs().max()) <= 1e-5 * float(gw.abs().max())


def test_fit_loss_rows_against_float64():
    b, d = 6, 144
    layers = [torch.from_numpy(synth.det_uniform((b, 1, 1, 1), 60 + k)).to(DEV).requires_grad_(True) for k in range(5)]
    m = torch.from_numpy(synth.det_uniform((b,), 66)).abs().to(DEV).requires_grad_(True)
    sigma = torch.linspace(0.5, 2.0, d, device=DEV)
    c = torch.from_numpy(synth.det_normal((b, d), 67)).to(DEV).requires_grad_(True)
    reg = (1e-3 * ((c / sigma) ** 2).sum()).detach().requires_grad_(True)       # the morph node's scalar prior
    rows, total = lpips_layer.fit_loss_rows(layers, m, 0.7, coeff=c, sigma=sigma, shape_reg=1e-3, reg=reg)
    want = (sum(x.detach().double().view(b) for x in layers) + 0.7 * m.detach().double()
            + 1e-3 * ((c.detach().double() / sigma.double()) ** 2).sum(1))
    assert float((rows.double() - want).abs().max() / want.abs().max()) <= 1e-6
    assert abs(float(total) - float(want.sum())) <= 1e-6 * float(want.abs().sum())
    assert not rows.requires_grad
    grads = torch.autograd.grad(3.0 * total, layers + [m, reg])
    for gl in grads[:5]:
        assert gl.shape == (b, 1, 1, 1) and bool((gl == 3.0).all())
    assert bool((grads[5] == np.float32(0.7) * 3.0).all()) and float(grads[6]) == 3.0
    rows2, total2 = lpips_layer.fit_loss_rows(layers, m, 0.7, coeff=c, sigma=sigma, shape_reg=1e-3, reg=reg)
    assert torch.equal(rows, rows2) and torch.equal(total, total2)
    with pytest.raises(ValueError):
        lpips_layer.fit_loss_rows(layers, m, 0.7, coeff=c, sigma=sigma, shape_reg=1e-3)


# ---- the inverter at 256^2 ---------------------------------------------------------------------------------------------
_T = {}


def _faces(n):
    """n targets rendered by the 256^2 generator from different latents, shapes and poses (cached)."""
    if n not in _T:
        g = _g256()
        fm, tri = _big_face(DEV)
        noise = _noise()
        ims = []
        with torch.no_grad():
            for k in range(n):
                c = torch.from_numpy(synth.det_normal((1, 144), 8 + k)).to(DEV) * fm.sigma
                p = torch.tensor([[0.2 - 0.1 * k, -0.1 + 0.05 * k, 0.0, 0.02 * k, 0.0, 0.0, 0.0]], device=DEV)
                v, nn_, _ = morph.morph_mesh(fm, c, p, tri)
                w = g.style(torch.from_numpy(synth.det_normal((1, 512), 9 + k)).to(DEV)).unsqueeze(1).repeat(
                    1, g.n_latent, 1)
                ims.append(g([w], (v, nn_, tri), input_is_latent=True, noise=noise)[0])
        _T[n] = torch.cat(ims, 0)
    return _T[n]


def _noise():
    return [torch.from_numpy(synth.det_normal(tuple(n.shape), 300 + i)).to(DEV) for i, n in enumerate(_g256().make_noise())]


def _inverter(target, use_graph):
    fm, tri = _big_face(DEV)
    torch.manual_seed(11)
    return inversion.LatentInverter(_g256(), lpips.PNetLin().to(DEV), target, None, lr=0.05, pose_lr=0.01,
                                    noise=_noise(), n_mean_latent=256, use_graph=use_graph, face=(fm, tri),
                                    fit_shape=True, coeff_lr=0.05, shape_reg=1e-3)


def _state(inv, hist):
    return [hist.cpu()] + [t.detach().cpu().clone() for t in (inv.w, inv.pose, inv.coeff)]


def test_batch_independence_in_graph_mode():
    """Sample 0's fit is bitwise the same whatever images fill slots 1-3: kernel choices depend on shapes, never on
    values, and no kernel mixes samples."""
    faces = _faces(4)
    noise_imgs = torch.from_numpy(synth.det_uniform((3, 3, 256, 256), 97)).to(DEV)
    runs = []
    for others in (faces[1:], noise_imgs, faces[:1].expand(3, -1, -1, -1)):
        inv = _inverter(torch.cat([faces[:1], others], 0).contiguous(), True)
        hist = inv.run(12)
        assert inv.graph is not None and hist.shape == (12, 4)
        runs.append(_state(inv, hist))
        del inv
    for other in runs[1:]:
        assert torch.equal(runs[0][0][:, 0], other[0][:, 0])
        for a, b in zip(runs[0][1:], other[1:]):
            assert torch.equal(a[0], b[0])
    assert not torch.equal(runs[0][0][:, 1], runs[1][0][:, 1])          # the other slots did change


def _first_gradients(inv):
    value = inv.loss(inv.render())
    value.backward()
    loss = inv._rows if inv.batch > 1 else value.detach().view(1)
    return [loss.detach()] + [x.grad.detach().clone().view(inv.batch, -1) for x in (inv.w, inv.pose, inv.coeff)]


def test_batch_gradients_match_single_image_gradients_and_every_loss_falls():
    """Bars of the device-against-CPU inversion tests (test_inversion_gpu): 2e-5 of the largest value on the loss and
    2e-2 on the norm of a gradient, the first-iteration gradients of each sample at B = 4 against that image alone at
    B = 1 (another batch may pick other convolution variants, so the rounding differs, and a ReLU pre-activation near
    zero may change sign)."""
    faces = _faces(4)
    batched = _first_gradients(_inverter(faces, False))
    for b in range(4):
        single = _first_gradients(_inverter(faces[b:b + 1], False))
        assert float((batched[0][b] - single[0][0]).abs()) <= 2e-5 * float(single[0].abs().max()), b
        for k in (1, 2, 3):
            got, want = batched[k][b], single[k][0]
            err = float((got - want).norm() / want.norm())
            assert err <= 2e-2, (b, k, err)
    inv = _inverter(faces, True)
    hist = inv.run(50).cpu()
    assert torch.isfinite(hist).all() and bool((hist[-1] < hist[0]).all()), hist[[0, -1]]


def test_batch_graph_equals_eager_reruns_and_reset():
    faces = _faces(4)
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True), ("graph2", True)):
        inv = _inverter(faces, use_graph)
        runs[key] = _state(inv, inv.run(16))
        if key == "graph":
            # reset to other images, then back: the next run is a fresh inverter's, bit for bit
            other = faces.flip(0).contiguous()
            inv.reset(other)
            got = _state(inv, inv.run(16))
            fresh = _inverter(other, True)
            want = _state(fresh, fresh.run(16))
            del fresh
            for a, b in zip(got, want):
                assert torch.equal(a, b)
        del inv
    for other in ("eager", "graph2"):
        for a, b in zip(runs["graph"], runs[other]):
            assert torch.equal(a, b), other


def test_batch_step_dispatches_no_library_gemm_or_scatter_and_adds_few_launches():
    from torch.utils._python_dispatch import TorchDispatchMode

    faces = _faces(4)
    banned = ("aten::mm", "aten::addmm", "aten::mv", "aten::linear", "aten::matmul", "aten::bmm", "aten::index_add_",
              "aten::index_add", "aten::addmv", "aten::baddbmm", "aten::convolution", "aten::cudnn_convolution",
              "aten::miopen_convolution")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func._schema.name in banned:
                seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    inv = _inverter(faces, False)
    inv._iteration()                                     # lazy preparation outside the spy
    with Spy():
        inv._iteration()
    assert not seen, seen
    nodes = {}
    for b in (1, 4):
        inv = _inverter(faces[:b].contiguous(), True)
        inv.run(6)
        nodes[b] = inv.graph.kernel_nodes
        del inv
    # one captured step for all samples: no per-sample launches.  The batched loss swaps the scalar path's launches
    # (mse, four adds, the pixel weight, the prior's add and their backward) for mse_rows (2 + 1) and fit_loss_rows
    # (1 + 1), and shape-selected kernels may take another variant at B = 4; 16 covers both with room
    print("kernel nodes per captured step:", nodes)
    assert nodes[4] <= nodes[1] + 16, nodes


def test_reconstruct_cli_batch_on_the_device(tmp_path):
    g = model.GeneratorWithMap(256, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    imgs = []
    for k in range(3):
        p = str(tmp_path / ("face_%d.npy" % k))
        np.save(p, synth.det_uniform((256, 256, 3), 19 + k))
        imgs.append(p)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "256", "--steps", "20", "--n_mean_latent",
           "256", "--batch", "2", "--out", out, ckpt] + imgs
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted("face_%d%s" % (k, s) for k in range(3)
                                             for s in (".obj", "_canonical.obj", "_render.png", "_normal.png", ".npz"))
    for k in range(3):
        r = np.load(os.path.join(out, "face_%d.npz" % k))
        assert r["w"].shape == (1, g.n_latent, 512) and r["coeff"].shape == (1, 144) and r["pose"].shape == (7,)
        assert r["loss"].shape == (20,) and np.isfinite(r["loss"]).all() and r["loss"][-1] < r["loss"][0]
