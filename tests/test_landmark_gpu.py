"""GPU: the landmark term's kernels (csrc/landmark.hip) against the float64 composite, their accumulate flag and graph
behaviour, pose recovery through the node alone, and the batched inverter with landmarks at 256^2."""
import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, graphs, inversion, lpips, synth, train, utils_3d
from stylerenderer_amd.op import landmark, morph

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HW = (48, 64)                                                            # H != W


def case(b, n_l, nv, beta=1.0, seed=0):
    """Inputs on which the float32 projection is exact, so that residuals sit exactly where they are put and the bars
    below are the sums' own error: vertex coordinates are multiples of 1/128, barycentric weights of 1/4, H / 2 = 24 and
    W / 2 = 32, targets multiples of 1/64.  Landmarks 0, 3, 6, ... are plain vertices, the others genuine three-vertex
    combinations; the last landmark shares landmark 0's vertex (nv = 7 shares many more); sample 0's first residuals
    are exactly (0, beta), (-beta, 1/2) and (-3 beta, 2 beta); the last sample of a batch has confidence 0 throughout."""
    v = np.round(synth.det_uniform((b, nv, 3), 40 + seed) * 112) / 128
    idx = np.zeros((n_l, 3), np.int64)
    bary = np.zeros((n_l, 3), np.float32)
    for l in range(n_l):
        if l % 3 == 0:
            idx[l], bary[l] = (5 * l) % nv, (1, 0, 0)
        else:
            idx[l] = ((7 * l) % nv, (7 * l + 1) % nv, (7 * l + 3) % nv)
            bary[l] = (0.5, 0.25, 0.25) if l % 3 == 1 else (0.25, 0.25, 0.5)
    if n_l > 1:
        idx[-1], bary[-1] = idx[0], (1, 0, 0)
    idx_t, bary_t = torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(bary)
    v64 = torch.from_numpy(v)
    p = landmark.project(landmark.landmark_points(v64, idx_t, bary_t.double()), HW)
    off = torch.from_numpy(np.round(synth.det_uniform((b, n_l, 2), 41 + seed) * 4 * 64) / 64)
    fixed = torch.tensor([[0.0, beta], [-beta, 0.5], [-3 * beta, 2 * beta]], dtype=torch.float64)
    off[0, :min(3, n_l)] = fixed[:n_l]
    target = p - off
    conf = torch.from_numpy(np.abs(synth.det_uniform((b, n_l), 42 + seed)) + 0.125)
    if b > 1:
        conf[-1] = 0.0
    gout = torch.from_numpy(synth.det_normal((b,), 43 + seed)) + 2.0
    f32 = lambda t: t.float().to(DEV)                                     # noqa: E731
    assert torch.equal(target.float().double(), target) and torch.equal(v64.float().double(), v64)
    return f32(v64), idx_t.to(DEV), bary_t.to(DEV), f32(target), f32(conf), f32(gout)


def run(v, idx, bary, target, conf, gout, beta=1.0, weight=1.0):
    v = v.detach().clone().requires_grad_(True)
    rows, p = landmark.landmark_loss(v, idx, bary, target, conf, HW, beta, weight)
    (gv,) = torch.autograd.grad((rows * gout).sum(), v)
    return rows.detach(), p.detach(), gv


@pytest.mark.parametrize("nv", [7, 1000])
@pytest.mark.parametrize("n_l", [1, 5, 64, 70])                          # one wave of landmarks, and just over it
@pytest.mark.parametrize("b", [1, 3])
def test_kernels_against_the_float64_composite(b, n_l, nv):
    beta = 0.75
    args = case(b, n_l, nv, beta)
    rows, p, gv = run(*args, beta=beta, weight=1.5)
    assert rows.shape == (b,) and p.shape == (b, n_l, 2) and gv.shape == (b, nv, 3)
    want_rows, want_p, want_gv = run(*(t.double() if t.is_floating_point() else t for t in args), beta=beta, weight=1.5)
    err_p = float((p.double() - want_p).abs().max())
    err_rows = (rows.double() - want_rows).abs()
    err_gv = float((gv.double() - want_gv).abs().max())
    print("b %d L %d nv %d: rows rel %.3g, gv %.3g of max %.3g, p %.3g px" % (
        b, n_l, nv, float((err_rows / want_rows.abs().clamp_min(1e-30)).max()), err_gv, float(want_gv.abs().max()), err_p))
    assert err_p <= 1e-4
    assert bool((err_rows <= 1e-5 * want_rows.abs()).all()), (rows, want_rows)
    assert float(want_rows[0]) > 0 and err_gv <= 1e-5 * float(want_gv.abs().max())
    # a row without confidence: exactly nothing
    if b > 1:
        assert float(rows[-1]) == 0.0 and float(gv[-1].abs().max()) == 0.0
    # exactly 0 in z and on vertices that carry no landmark
    used = torch.zeros(nv, dtype=torch.bool, device=DEV)
    used[args[1].long()[args[2] != 0]] = True
    assert float(gv[..., 2].abs().max()) == 0.0 and float(gv[:, ~used].abs().max() if (~used).any() else 0.0) == 0.0
    assert float(gv[0, used][:, :2].abs().max()) > 0
    # reruns: the same bits
    rows2, p2, gv2 = run(*args, beta=beta, weight=1.5)
    assert torch.equal(rows, rows2) and torch.equal(p, p2) and torch.equal(gv, gv2)


def test_kernels_on_ordinary_values():
    """Values that are not exactly representable: p to 1e-4 pixel; rho is 1-Lipschitz, so rows moves by no more than
    scale * 2 * (the error of p) plus the sum's own 1e-5."""
    b, n_l, nv = 2, 68, 1000
    v = torch.from_numpy(0.9 * synth.det_uniform((b, nv, 3), 50)).to(DEV)
    idx, bary = face_model.landmark_embedding((np.arange(n_l) * 13 % 1900, np.abs(synth.det_uniform((n_l, 3), 51)) + 0.1),
                                              np.stack([np.arange(1900) % nv, (np.arange(1900) * 3 + 1) % nv,
                                                        (np.arange(1900) * 7 + 2) % nv], 1))
    bary = bary / bary.sum(1, keepdim=True)
    idx, bary = idx.to(DEV), bary.to(DEV)
    target = torch.from_numpy(np.array(HW[::-1]) * (0.5 + 0.45 * synth.det_uniform((b, n_l, 2), 52))).float().to(DEV)
    conf = torch.from_numpy(np.abs(synth.det_uniform((b, n_l), 53))).float().to(DEV)
    gout = torch.ones(b, device=DEV)
    rows, p, gv = run(v, idx, bary, target, conf, gout)
    wr, wp, wgv = run(v.double(), idx, bary.double(), target.double(), conf.double(), gout.double())
    err_p = float((p.double() - wp).abs().max())
    print("p %.3g px, rows %s against %s" % (err_p, rows.tolist(), wr.tolist()))
    assert err_p <= 1e-4
    assert bool(((rows.double() - wr).abs() <= 2.0 / max(HW) * 2 * 1e-4 + 1e-5 * wr.abs()).all())


def test_an_embedding_on_the_host_is_taken_to_the_vertices_device():
    """face_model.landmark_embedding returns host tensors: with device vertices the kernels read device copies of them
    (built once per embedding), and give what the device embedding gives."""
    v, idx, bary, target, conf, gout = case(3, 70, 1000, seed=7)
    want = run(v, idx, bary, target, conf, gout)
    idx_h, bary_h = idx.cpu(), bary.cpu()
    for _ in range(2):                                                   # the second call takes the cached lists
        got = run(v, idx_h, bary_h, target, conf, gout)
        for a, b in zip(got, want):
            assert a.device.type == "cuda" and torch.equal(a, b)
    lists = landmark.vertex_lists(idx_h, bary_h, 1000, v.device)
    assert all(t.device == v.device for t in lists)
    assert landmark.vertex_lists(idx_h, bary_h, 1000, v.device)[0] is lists[0]
    # second order, through the composite, as well
    v2 = v.clone().requires_grad_(True)
    rows, _ = landmark.landmark_loss(v2, idx_h, bary_h, target, conf, HW)
    (gv,) = torch.autograd.grad((rows * gout).sum(), v2, create_graph=True)
    (g2,) = torch.autograd.grad((gv ** 2).sum(), v2)
    assert torch.isfinite(g2).all() and float(g2.abs().max()) > 0


def test_accumulate_flag_adds_to_the_last_bit():
    v, idx, bary, target, conf, gout = case(3, 70, 1000, seed=3)
    rows, p, g, lists = landmark.landmark_forward(v, idx, bary, target, conf, HW, 1.0, 1.0)
    plain = landmark.landmark_backward(g, gout, lists, 1000, HW)
    gv_in = torch.from_numpy(synth.det_normal((3, 1000, 3), 60)).to(DEV)
    out = gv_in.clone()
    assert landmark.landmark_backward(g, gout, lists, 1000, HW, out=out) is out
    assert torch.equal(out, gv_in + plain) and not torch.equal(out, gv_in)
    # a broadcast incoming gradient (the sum over samples) is read through its stride
    one = gout[:1].expand(3)
    assert one.stride(0) == 0
    assert torch.equal(landmark.landmark_backward(g, one, lists, 1000, HW),
                       landmark.landmark_backward(g, one.contiguous(), lists, 1000, HW))


def test_second_order_goes_through_the_composite():
    v, idx, bary, target, conf, gout = case(2, 5, 7, seed=4)
    v = v.requires_grad_(True)
    rows, _ = landmark.landmark_loss(v, idx, bary, target, conf, HW)
    (gv,) = torch.autograd.grad((rows * gout).sum(), v, create_graph=True)
    (g2,) = torch.autograd.grad((gv ** 2).sum(), v)
    v64 = v.detach().double().requires_grad_(True)
    r64, _ = landmark.landmark_composite(v64, idx, bary.double(), target.double(), conf.double(), HW)
    (gv64,) = torch.autograd.grad((r64 * gout.double()).sum(), v64, create_graph=True)
    (w2,) = torch.autograd.grad((gv64 ** 2).sum(), v64)
    assert float((g2.double() - w2).abs().max()) <= 1e-4 * float(w2.abs().max()) and float(w2.abs().max()) > 0


def test_captured_forward_and_backward_equal_eager_and_follow_the_target_buffer():
    v, idx, bary, target, conf, gout = case(3, 70, 1000, seed=5)
    other = case(3, 70, 1000, seed=6)[3]
    v.requires_grad_(True)
    out = {}

    def body():
        rows, p = landmark.landmark_loss(v, idx, bary, target, conf, HW)
        (gv,) = torch.autograd.grad((rows * gout).sum(), v)
        out["rows"], out["p"], out["gv"] = rows.detach(), p, gv

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                                           # the embedding's lists are built here, once
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    print("captured forward + backward: %d kernel nodes of %d" % (graph.kernel_nodes, graph.nodes))
    held = dict(out)
    for tgt in (target.clone(), other, target.clone()):
        target.copy_(tgt)
        graph.replay()
        got = [held[k].clone() for k in ("rows", "p", "gv")]
        want = run(v, idx, bary, tgt, conf, gout)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert not torch.equal(run(v, idx, bary, other, conf, gout)[0], run(v, idx, bary, target, conf, gout)[0])


# ---- pose recovery through the node alone -------------------------------------------------------------------------------
def test_adam_on_the_pose_recovers_it_from_landmarks_alone():
    """Verified first on the float64 composite on the host (same model, pose, size, learning rate): 2e-6 pixel after 300
    steps, below 0.5 pixel from step 44 on."""
    src = train.SyntheticFaceSource(DEV)
    nv = src.model.fc.bias.numel() // 3
    idx, bary = (t.to(DEV) for t in face_model.landmark_embedding(np.linspace(0, nv - 1, 68).round().astype(np.int64)))
    coeff = torch.zeros(1, src.model.n_coeff, device=DEV)
    true = torch.tensor([[0.4, -0.3, 0.2, 0.15, -0.1, 0.0, 0.2]], device=DEV)
    conf = torch.ones(1, 68, device=DEV)
    with torch.no_grad():
        target = landmark.project(landmark.landmark_points(morph.morph_mesh(src.model, coeff, true, src.tri)[0], idx, bary), 256)
    pose = torch.zeros(1, 7, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([pose], lr=0.02)
    for _ in range(300):
        opt.zero_grad()
        rows, p = landmark.landmark_loss(morph.morph_mesh(src.model, coeff, pose, src.tri)[0], idx, bary, target, conf, 256)
        rows.sum().backward()
        opt.step()
    dist = float(((p - target) ** 2).sum(-1).sqrt().mean())
    print("mean landmark distance after 300 steps: %.3g px; pose %s" % (dist, pose.detach()[0].tolist()))
    assert dist < 0.5


# ---- the batched inverter with landmarks at 256^2 -----------------------------------------------------------------------
_FACE = []


def _face():
    """test_reconstruct_gpu's face model, built once."""
    from test_reconstruct_gpu import _big_face

    if not _FACE:
        _FACE.append(_big_face(DEV))
    return _FACE[0]


def _embedding(fm):
    nv = fm.fc.bias.numel() // 3
    return face_model.landmark_embedding(np.linspace(0, nv - 1, 68).round().astype(np.int64))


def _landmarks(n, shift=0.0):
    """Landmarks [n, 68, 2] of the mean shape at the poses of test_reconstruct_batch_gpu._faces (host, float64)."""
    fm, _ = _face()
    idx, bary = _embedding(fm)
    mean = fm.fc.bias.detach().view(1, -1, 3).double().cpu()
    out = []
    for k in range(n):
        p = torch.tensor([0.2 - 0.1 * k, -0.1 + 0.05 * k, 0.0, 0.02 * k, 0.0, 0.0, 0.0], dtype=torch.float64)
        v = mean @ utils_3d.euler_mat(p[:3], "yxz") + p[3:6]
        out.append(landmark.project(landmark.landmark_points(v, idx, bary.double()), 256)[0].numpy() + shift)
    return np.stack(out)


def _inverter(target, use_graph, **kw):
    from test_reconstruct_batch_gpu import _noise
    from test_reconstruct_gpu import _g256

    fm, tri = _face()
    torch.manual_seed(11)
    if kw:
        kw.setdefault("landmark_embedding", _embedding(fm))
    return inversion.LatentInverter(_g256(), lpips.PNetLin().to(DEV), target, None, lr=0.05, pose_lr=0.01,
                                    noise=_noise(), n_mean_latent=256, use_graph=use_graph, face=(fm, tri),
                                    fit_shape=True, coeff_lr=0.05, shape_reg=1e-3, **kw)


def _state(inv, hist):
    return [hist.cpu()] + [t.detach().cpu().clone() for t in (inv.w, inv.pose, inv.coeff, inv.landmarks_fit)]


def test_batched_inverter_with_landmarks_graph_equals_eager_and_reset_equals_fresh():
    from test_reconstruct_batch_gpu import _faces

    faces = _faces(2)
    lmk = _landmarks(2)
    conf = np.ones((2, 68))
    conf[1, :17] = 0.25
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = _inverter(faces, use_graph, landmarks=lmk, landmark_conf=conf, landmark_weight=2.0)
        assert float(inv.pose.detach()[0, 0]) == pytest.approx(0.2, abs=1e-5)       # the closed-form start
        runs[key] = _state(inv, inv.run(8))
        assert (inv.graph is not None) == use_graph
        if use_graph:
            # re-targeted with other pictures and landmarks: a fresh inverter's run, bit for bit
            other, lmk2 = faces.flip(0).contiguous(), _landmarks(2, 1.5)[::-1].copy()
            inv.reset(other, lmk2, conf)
            got = _state(inv, inv.run(8))
            fresh = _inverter(other, True, landmarks=lmk2, landmark_conf=conf, landmark_weight=2.0)
            want = _state(fresh, fresh.run(8))
            del fresh
            for a, b in zip(got, want):
                assert torch.equal(a, b)
            assert not torch.equal(got[0], runs["graph"][0])
        del inv
    for a, b in zip(runs["graph"], runs["eager"]):
        assert torch.equal(a, b)
    hist = runs["graph"][0]
    assert hist.shape == (8, 2) and torch.isfinite(hist).all()


def test_sample_0_does_not_depend_on_the_other_slots_landmarks_or_picture():
    from test_reconstruct_batch_gpu import _faces

    faces = _faces(2)
    lmk = _landmarks(2)
    noise_img = torch.from_numpy(synth.det_uniform((1, 3, 256, 256), 97)).to(DEV)
    lmk_b = np.stack([lmk[0], 0.8 * lmk[1] + 30.0])                      # slot 1: a smaller face elsewhere
    runs = []
    for target, marks, conf in ((faces, lmk, np.ones((2, 68))),
                                (torch.cat([faces[:1], noise_img], 0).contiguous(), lmk_b, np.ones((2, 68))),
                                (faces, lmk, np.stack([np.ones(68), np.zeros(68)]))):
        inv = _inverter(target, True, landmarks=marks, landmark_conf=conf)
        runs.append(_state(inv, inv.run(8)))
        del inv
    for other in runs[1:]:
        assert torch.equal(runs[0][0][:, 0], other[0][:, 0])
        for a, b in zip(runs[0][1:], other[1:]):
            assert torch.equal(a[0], b[0])
    assert not torch.equal(runs[0][0][:, 1], runs[1][0][:, 1]) and not torch.equal(runs[0][0][:, 1], runs[2][0][:, 1])
    assert float(runs[2][2][1].abs().max()) > 0                          # (slot 1 without landmarks started at pose 0 and moved)


def test_step_with_landmarks_stays_native_and_adds_few_launches():
    """SR_STRICT_NATIVE=1 (the GPU suite's setting): no library GEMM, convolution or scatter in a step with landmarks.
    Launches the term adds to the captured step: the forward, the backward, autograd's add of the two vertex gradients
    (rasterizer and landmarks), and the term's way into the loss — one add at B = 1; at B > 1 the per-sample rows' add, a
    sum over the samples and the total's add."""
    import os

    from torch.utils._python_dispatch import TorchDispatchMode

    from test_reconstruct_batch_gpu import _faces

    assert os.environ.get("SR_STRICT_NATIVE") == "1"
    faces = _faces(2)
    lmk = _landmarks(2)
    banned = ("aten::mm", "aten::addmm", "aten::mv", "aten::linear", "aten::matmul", "aten::bmm", "aten::index_add_",
              "aten::index_add", "aten::addmv", "aten::baddbmm", "aten::convolution", "aten::cudnn_convolution",
              "aten::miopen_convolution", "aten::index_put_", "aten::index_put", "aten::scatter_add", "aten::scatter_add_")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func._schema.name in banned:
                seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    inv = _inverter(faces, False, landmarks=lmk)
    inv._iteration()                                     # lazy preparation outside the spy
    with Spy():
        inv._iteration()
    assert not seen, seen
    del inv
    nodes = {}
    for b in (1, 2):
        for with_lmk in (False, True):
            inv = _inverter(faces[:b].contiguous(), True, **({"landmarks": lmk[:b]} if with_lmk else {}))
            inv.run(6)
            nodes[b, with_lmk] = (inv.graph.kernel_nodes, inv.graph.nodes)
            del inv
    print("(kernel nodes, nodes) per captured step by (batch, landmarks):", nodes)
    assert nodes[1, True][0] - nodes[1, False][0] <= 4 and nodes[2, True][0] - nodes[2, False][0] <= 6, nodes
    assert nodes[1, True][1] - nodes[1, True][0] == nodes[1, False][1] - nodes[1, False][0]       # no new memset node
