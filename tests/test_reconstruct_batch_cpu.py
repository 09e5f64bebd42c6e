"""CPU: the batched inverter (LatentInverter with a target [B, 3, H, W], B > 1) on the composite path — every sample's
first-iteration gradients are its single-image gradients, reset() re-targets exactly, the batched pose matrices and
per-sample loss terms are their definitions — and `reconstruct --batch` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import inversion, lpips, synth, utils_3d
from stylerenderer_amd.op import lpips_layer, morph
from test_reconstruct_cpu import tiny_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (latent seed, coefficient seed, pose) of the targets: three different faces, poses and images
FACES = ((5, 3, (0.2, -0.1, 0.05, 0.03, -0.02, 0.0, 0.05)), (21, 23, (-0.25, 0.08, 0.0, -0.04, 0.01, 0.0, -0.05)),
         (31, 33, (0.05, 0.15, -0.1, 0.0, 0.03, 0.0, 0.1)))


def batch_problem(device="cpu", faces=FACES):
    """(g, mesh, face, noise, targets [len(faces), 3, 16, 16]) on tiny_problem's generator and 3DMM."""
    g, mesh, face, noise, _ = tiny_problem(device)
    fm, tri = face
    ims = []
    with torch.no_grad():
        for ws, cs, p in faces:
            c = torch.from_numpy(synth.det_normal((1, 14), cs)).to(device) * fm.sigma
            v, n, _ = morph.morph_mesh(fm, c, torch.tensor([p], device=device), tri)
            w = g.style(torch.from_numpy(synth.det_normal((1, 32), ws)).to(device)).unsqueeze(1).repeat(1, g.n_latent, 1)
            img, _, _ = g([w], (v.contiguous(), n.contiguous(), tri), input_is_latent=True, noise=noise)
            ims.append(img)
    return g, mesh, face, noise, torch.cat(ims, 0)


def make_inverter(g, mesh, face, noise, target, fit_shape=True, **kw):
    torch.manual_seed(3)                                      # the mean latent's draws
    if fit_shape:
        kw.update(face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3)
    return inversion.LatentInverter(g, lpips.PNetLin(), target, None if fit_shape else mesh, lr=0.05, pose_lr=0.02,
                                    noise=noise, n_mean_latent=64, **kw)


def first_gradients(inv):
    """(loss, w.grad, pose.grad, coeff.grad) of the first iteration, before any update."""
    value = inv.loss(inv.render())
    value.backward()
    loss = inv._rows if inv.batch > 1 else value.detach().view(1)
    grads = [inv.w.grad, inv.pose.grad.view(-1, 7)] + ([inv.coeff.grad] if inv.coeff is not None else [])
    return [loss.detach()] + [x.detach().clone() for x in grads]


@pytest.mark.parametrize("fit_shape", [True, False])
def test_batch_gradients_are_the_single_image_gradients(fit_shape):
    """The objective is sum_b L_b and L_j does not depend on sample b's variables for j != b, so
    d(sum_j L_j)/d x_b = dL_b/d x_b: at B = 3 every sample's first-iteration gradient is the B = 1 gradient of its own
    image, exactly in real arithmetic.  In fp32 the two differ by the summation order of batched CPU kernels (the
    LPIPS and generator convolutions at another batch, the row means) only.  Measured: at most 1.2e-6 of each
    gradient's largest entry; the bar is 1e-4."""
    prob = batch_problem()
    targets = prob[4]
    batched = first_gradients(make_inverter(*prob[:4], targets, fit_shape=fit_shape))
    assert batched[1].shape == (3, prob[0].n_latent, 32) and batched[2].shape == (3, 7)
    for b in range(3):
        single = first_gradients(make_inverter(*prob[:4], targets[b:b + 1], fit_shape=fit_shape))
        for k, (got, want) in enumerate(zip(batched, single)):
            err = float((got[b:b + 1] - want).abs().max() / want.abs().max())
            assert err <= 1e-4, (b, k, err)
            assert float(want.abs().max()) > 0
    # the samples differ: the test is not three copies of one image
    assert float((batched[1][0] - batched[1][1]).abs().max()) > 1e-3 * float(batched[1].abs().max())


def test_reset_then_run_equals_a_fresh_inverter():
    g, mesh, face, noise, targets = batch_problem()
    other = targets.flip(0).contiguous()
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # the CPU path's threaded reductions are not run-to-run identical
    try:
        inv = make_inverter(g, mesh, face, noise, targets)
        first = inv.run(5)
        assert first.shape == (5, 3) and inv.loss_value.shape == (3,)
        inv.reset(other)
        got = [inv.run(6)] + [t.detach().clone() for t in (inv.w, inv.pose, inv.coeff)]
        fresh = make_inverter(g, mesh, face, noise, other)
        want = [fresh.run(6)] + [t.detach().clone() for t in (fresh.w, fresh.pose, fresh.coeff)]
    finally:
        torch.set_num_threads(threads)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(first[:, 0], got[0][:5, 0])      # the first fit was of other images
    with pytest.raises(ValueError):
        inv.reset(targets[:2])


def test_batched_inverter_shapes_and_single_image_shapes():
    g, mesh, face, noise, targets = batch_problem()
    inv = make_inverter(g, mesh, face, noise, targets)
    assert inv.w.shape == (3, g.n_latent, 32) and inv.pose.shape == (3, 7) and inv.coeff.shape == (3, 14)
    assert torch.equal(inv.w[0], inv.w[2])                    # every row starts at the mean latent
    hist = inv.run(12)
    assert hist.shape == (12, 3) and torch.isfinite(hist).all()
    assert bool((hist[-1] < hist[0]).all())
    one = make_inverter(g, mesh, face, noise, targets[:1])
    assert one.pose.shape == (7,) and one.coeff.shape == (1, 14) and one.loss_value.shape == ()
    assert one.run(3).shape == (3,)
    # the pose-only path at B = 3 too
    plain = make_inverter(g, mesh, face, noise, targets, fit_shape=False)
    assert plain.run(3).shape == (3, 3) and plain.coeff is None


def test_batched_pose_matrices_are_the_per_pose_matrices():
    pose = torch.tensor([[0.3, -0.2, 0.1, 0.5, 0.2, 0.1, 0.2], [-0.1, 0.4, 0.0, 0.0, 0.0, 0.0, -0.3]],
                        dtype=torch.float64)
    lin, rot = utils_3d.pose_matrices(pose)
    assert lin.shape == (2, 3, 3) and rot.shape == (2, 3, 3)
    for b in range(2):
        lb, rb = utils_3d.pose_matrices(pose[b])
        assert torch.allclose(lin[b:b + 1], lb, rtol=0, atol=1e-15) and torch.allclose(rot[b:b + 1], rb, rtol=0, atol=1e-15)


def test_loss_rows_composite_is_the_definition():
    layers = [torch.from_numpy(synth.det_uniform((4, 1, 1, 1), 60 + k)).double() for k in range(5)]
    a = torch.from_numpy(synth.det_uniform((4, 3, 5, 7), 70)).double()
    t = torch.from_numpy(synth.det_uniform((4, 3, 5, 7), 71)).double()
    m = lpips_layer.mse_rows(a, t)
    assert torch.allclose(m, torch.stack([((a[b] - t[b]) ** 2).mean() for b in range(4)]), rtol=1e-14)
    c = torch.from_numpy(synth.det_normal((4, 6), 72)).double().requires_grad_(True)
    sigma = torch.linspace(0.5, 2.0, 6, dtype=torch.float64)
    rows, total = lpips_layer.fit_loss_rows(layers, m, 0.7, coeff=c, sigma=sigma, shape_reg=0.3)
    want = sum(x.view(4) for x in layers) + 0.7 * m + 0.3 * ((c / sigma) ** 2).sum(1)
    assert torch.allclose(rows, want.detach(), rtol=1e-14) and torch.allclose(total, want.sum(), rtol=1e-14)
    (gc,) = torch.autograd.grad(total, c)
    assert torch.allclose(gc, 0.6 * c / sigma ** 2, rtol=1e-14)
    with pytest.raises(ValueError):
        lpips_layer.fit_loss_rows(layers[:4], m, 0.7)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_reconstruct_cli_batch_pads_the_last_group(tmp_path):
    """--batch 2 on three images: two groups through one inverter (the second by reset), the last padded with a copy;
    every image gets the batch-1 files and shapes."""
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    imgs = []
    for k in range(3):
        p = str(tmp_path / ("face_%d.npy" % k))
        np.save(p, synth.det_uniform((16, 16, 3), 40 + k))
        imgs.append(p)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "4", "--n_mean_latent",
           "64", "--batch", "2", "--out", out, ckpt] + imgs
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    names = sorted(os.listdir(out))
    assert names == sorted("face_%d%s" % (k, s) for k in range(3)
                           for s in (".obj", "_canonical.obj", "_render.png", "_normal.png", ".npz"))
    losses = []
    for k in range(3):
        r = np.load(os.path.join(out, "face_%d.npz" % k))
        assert r["w"].shape == (1, g.n_latent, 512) and r["coeff"].shape == (1, 144) and r["pose"].shape == (7,)
        assert r["loss"].shape == (4,) and np.isfinite(r["loss"]).all()
        losses.append(r["loss"])
    assert len({float(x[0]) for x in losses}) == 3                     # three different images were fitted
