"""GPU: several views of one subject — sr_share_rows and sr_texture_merge against the host definitions of op.share and
op.texture, bit for bit; merge under graph capture; LatentInverter(shared_identity=K) on the device (the shared columns,
graph against eager, reset, the tied gradient against the CPU's, launch count, no library GEMM); `reconstruct
--multiview` on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import graphs, inversion, lpips, model, synth
from stylerenderer_amd.op import share, texture
from test_multiview_cpu import check_multiview_outputs, merge_stack, remerge_on_the_host, share_input
from test_reconstruct_batch_cpu import batch_problem
from test_texture_cpu import affine_picture, scene_batch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = [(0.0, 0.0), (0.5, 0.125), (-0.3, -0.6)]                        # test_texture_gpu's three shifted samples


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


# ---- sr_share_rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,d,k", [(1, 5, 5), (3, 14, 10), (8, 300, 257), (8, 300, 1)])   # 257: one past a 256-lane block
def test_share_rows_equals_the_host_bit_for_bit(b, d, k):
    g = torch.from_numpy(share_input(b, d))
    assert bool((g > 0).any()) and bool((g < 0).any())
    want = share.share_rows_(g.clone(), k)
    got = share.share_rows_(g.to(DEV), k)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    assert torch.equal(got.cpu()[:, k:], g[:, k:])
    assert torch.equal(share.share_rows_(g.to(DEV), k), got)                 # reruns give the same bits
    with pytest.raises(RuntimeError):
        share.share_rows_(g.double().to(DEV), k)                             # strict: no float64 on the device


# ---- sr_texture_merge ------------------------------------------------------------------------------------------------
def assert_merge_equals_host(tex, weight, sharpness, what):
    want = texture.merge(tex, weight, sharpness)
    got = texture.merge(tex.to(DEV), weight.to(DEV), sharpness)
    bad = [int((a.cpu() != b).sum()) for a, b in zip(got, want)]
    print("merge", what, "sharpness", sharpness, "mismatches (tex, weight, best)", bad)
    assert got[0].is_cuda and got[2].dtype == torch.uint8
    for a, b in zip(got, want):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(a.cpu(), b), (what, sharpness, bad)
    return want


@pytest.mark.parametrize("size", [(8, 8), (33, 65)])                     # 8: the 16-byte form; 65: scalar, with a tail
@pytest.mark.parametrize("n_v", [1, 2, 5])
def test_merge_equals_the_host_bit_for_bit(size, n_v):
    for c_n in (1, 3):
        tex, weight = merge_stack(n_v, c_n, size)
        kinds = weight.view(n_v, -1)
        assert bool((kinds.max(0).values == 0).any())                        # empty texels
        if n_v > 1:
            assert bool(((kinds == kinds[0]).all(0) & (kinds[0] > 0)).any())  # exact ties of all views
            assert bool(((kinds[-1] == 0.75 * 2.0 ** -20) & (kinds[0] == 0.75)).any())       # the ladder's foot
        for sharpness in (0, 2, 4):
            _, w, best = assert_merge_equals_host(tex, weight, sharpness, (size, n_v, c_n))
            tied = (kinds == kinds[0]).all(0) & (kinds[0] > 0)
            assert bool((best.view(-1)[tied] == 0).all())                    # a tie goes to the first view
    with pytest.raises(RuntimeError):
        texture.merge(tex.double().to(DEV), weight.double().to(DEV), 2)      # strict: no float64 on the device


def scene_bakes(size, on=DEV):
    """The exact two-quad scene of test_texture_cpu baked from its three shifted samples: (tex [3, 3, Th, Tw], weight)."""
    v, n, tri, uv, tri_uv = scene_batch(SHIFTS)
    face, coeff = texture.texel_map(uv, tri_uv, size)
    zbuf = texture.depth_buffer(v, tri, (48, 64))
    img = affine_picture(3, 48, 64, batch=3)
    args = [t.to(on) for t in (v, n, tri, face, coeff, img, zbuf)]
    return texture.bake(*args, facing=(0.0, 0.5), z_bias=1.0 / 64)


@pytest.mark.parametrize("size", [(8, 8), (33, 65)])
def test_merge_of_real_bakes_equals_the_host(size):
    tex, weight = scene_bakes(size)
    host_t, host_w = scene_bakes(size, "cpu")
    assert torch.equal(tex.cpu(), host_t) and torch.equal(weight.cpu(), host_w)
    seen = (host_w > 0).view(3, -1)
    assert int(seen.any(0).sum()) > int(seen.sum(1).min())                   # the views add texels to one another
    for sharpness in (0, 2, 4):
        got = texture.merge(tex, weight, sharpness)
        want = texture.merge(host_t, host_w, sharpness)
        for a, b in zip(got, want):
            assert torch.equal(a.cpu(), b), sharpness
    assert torch.equal(want[1].view(-1) > 0, seen.any(0))                    # the merge sees what any view saw


def test_merge_under_graph_capture():
    tex, weight = (t.to(DEV) for t in merge_stack(5, 3, (33, 65)))
    out = {}

    def body():
        out["tex"], out["weight"], out["best"] = texture.merge(tex, weight, 2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    assert graph.kernel_nodes == 1                                           # one launch, nothing else
    tex2, weight2 = (t.to(DEV) for t in merge_stack(5, 3, (33, 65), seed=90))
    tex.copy_(tex2)                                                          # new inputs, in place
    weight.copy_(weight2.flip(0))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want = texture.merge(tex.cpu(), weight.cpu(), 2)
        for key, b in zip(("tex", "weight", "best"), want):
            assert torch.equal(out[key].cpu(), b), key


# ---- the fit on the device -------------------------------------------------------------------------------------------
_P = {}


def problem(device):
    if str(device) not in _P:
        _P[str(device)] = batch_problem(device)
    return _P[str(device)]


def _inverter(prob, target, **kw):
    """test_reconstruct_batch_cpu.make_inverter's settings with the perceptual network on the problem's device."""
    g, _, face, noise, _ = prob
    torch.manual_seed(3)
    return inversion.LatentInverter(g, lpips.PNetLin().to(target.device), target, None, lr=0.05, pose_lr=0.02, noise=noise,
                                    n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3, **kw)


def _state(inv, hist):
    return [hist.cpu()] + [t.detach().cpu().clone() for t in (inv.w, inv.pose, inv.coeff)]


def test_shared_identity_graph_equals_eager_and_reset():
    prob = problem(DEV)
    targets = prob[4]
    k = prob[2][0].n_identity
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = _inverter(prob, targets, use_graph=use_graph, shared_identity=k)
        runs[key] = _state(inv, inv.run(8))
        assert (inv.graph is not None) == use_graph
        if key == "graph":
            other = targets.flip(0).contiguous()
            inv.reset(other)
            got = _state(inv, inv.run(8))
            fresh = _inverter(prob, other, use_graph=True, shared_identity=k)
            want = _state(fresh, fresh.run(8))
            del fresh
            for a, b in zip(got, want):
                assert torch.equal(a, b)
            for b in (1, 2):
                assert torch.equal(got[3][b, :k], got[3][0, :k])
        del inv
    coeff, pose = runs["graph"][3], runs["graph"][2]
    assert float(coeff[:, :k].abs().max()) > 0
    for b in (1, 2):
        assert torch.equal(coeff[b, :k], coeff[0, :k])                       # bit-identical across the rows
        assert not torch.equal(coeff[b, k:], coeff[0, k:]) and not torch.equal(pose[b], pose[0])
    for a, b in zip(runs["graph"], runs["eager"]):
        assert torch.equal(a, b)


def test_tied_gradient_on_the_device_against_the_cpu():
    """The first iteration's tied gradient, device against CPU, on the same pictures from the same start (the CPU's
    targets, mean latent and coefficients: the two random generators draw different mean latents): the bar of the
    device-against-CPU batch gradients of test_reconstruct_batch_gpu, 2e-2 of the gradient's largest entry.  The tie
    itself adds nothing beyond it: it is the same three-term sum on both sides."""
    host = problem("cpu")
    fm = host[2][0]
    k = fm.n_identity
    start = torch.from_numpy(synth.det_normal((3, fm.n_coeff), 77)).float() * 0.3 * fm.sigma
    start[:, :k] = start[0, :k].clone()
    grads, w0 = {}, None
    for dev in ("cpu", DEV):
        inv = _inverter(problem(dev), host[4].to(dev), use_graph=False, shared_identity=k)
        with torch.no_grad():
            w0 = inv.w.detach().clone() if w0 is None else w0
            inv.w.copy_(w0.to(dev))
            inv.coeff.copy_(start.to(dev))
        inv.loss(inv.render()).backward()
        untied = inv.coeff.grad.detach().cpu().clone()
        grads[str(dev)] = (share.share_rows_(inv.coeff.grad, k).detach().cpu().clone(), untied)
    got, want = grads[str(DEV)][0], grads["cpu"][0]
    err = float((got - want).abs().max() / want.abs().max())
    print("tied gradient, device against CPU: max |diff| / max |want|", err, "norm of the difference / norm",
          float((got - want).norm() / want.norm()), "untied:",
          float((grads[str(DEV)][1] - grads["cpu"][1]).abs().max() / grads["cpu"][1].abs().max()))
    assert err <= 2e-2
    assert torch.equal(got[1, :k], got[0, :k]) and torch.equal(got[2, :k], got[0, :k])
    assert torch.equal(got[:, k:], grads[str(DEV)][1][:, k:])
    assert float(want[0, :k].abs().max()) > 0


def test_shared_identity_adds_at_most_two_kernel_nodes_and_no_library_gemm():
    from torch.utils._python_dispatch import TorchDispatchMode

    prob = problem(DEV)
    targets = prob[4]
    k = prob[2][0].n_identity
    nodes = {}
    for key, kw in (("off", {}), ("on", {"shared_identity": k})):
        inv = _inverter(prob, targets, use_graph=True, **kw)
        inv.run(6)
        nodes[key] = inv.graph.kernel_nodes
        del inv
    print("kernel nodes per captured step:", nodes)
    assert nodes["off"] < nodes["on"] <= nodes["off"] + 2, nodes             # the tie is one launch; one copy is allowed
    banned = ("aten::mm", "aten::addmm", "aten::mv", "aten::linear", "aten::matmul", "aten::bmm", "aten::index_add_",
              "aten::index_add", "aten::addmv", "aten::baddbmm", "aten::convolution", "aten::cudnn_convolution",
              "aten::miopen_convolution")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func._schema.name in banned:
                seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    inv = _inverter(prob, targets, use_graph=False, shared_identity=k)
    inv._iteration()                                     # lazy preparation outside the spy
    with Spy():
        inv._iteration()
    assert not seen, seen


# ---- command line ----------------------------------------------------------------------------------------------------
def test_reconstruct_cli_multiview_on_the_device(tmp_path):
    g = model.GeneratorWithMap(256, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    imgs = []
    for k in range(6):
        p = str(tmp_path / ("view_%d.npy" % k))
        np.save(p, synth.det_uniform((64, 64, 3), 140 + k))                  # resized to 256 on the host; baked at 64
        imgs.append(p)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "256", "--steps", "6", "--n_mean_latent",
           "256", "--multiview", "3", "--texture", "32", "--gpu", "0", "--out", out, ckpt] + imgs
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    groups = [["view_0", "view_1", "view_2"], ["view_3", "view_4", "view_5"]]
    subjects = check_multiview_outputs(out, groups, 6, 32, 80)
    assert subjects[0]["identity"].tobytes() != subjects[1]["identity"].tobytes()
    # the device's merge of the written bakes is the host's, to the byte (the unpadded merge is in the .npz)
    for group, ident in zip(groups, subjects):
        t, w, b = remerge_on_the_host(out, group)
        assert t.tobytes() == ident["merged_texture"].tobytes() and w.tobytes() == ident["merged_weight"].tobytes()
        assert np.array_equal(b, ident["merged_best"])
