"""CPU: landmark-guided reconstruction — the closed-form pose start, the landmark scaling, the composite definition of the
landmark term, the embedding loader, load_bfm's landmarks, the inverter with landmarks and `reconstruct --lmk`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import align, face_model, inversion, lpips, reconstruct, synth, train, utils_3d
from stylerenderer_amd.op import landmark
from test_reconstruct_cpu import _env
from test_reconstruct_cpu import tiny_problem as _tiny_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# inside |yaw|, |pitch| <= 0.6, |roll| <= 0.5, |t| <= 0.3, |s| <= 0.3: the corners and an ordinary pose
POSES = [(0.6, -0.6, 0.5, 0.3, -0.3, 0.0, 0.3), (-0.6, 0.6, -0.5, -0.3, 0.3, 0.0, -0.3),
         (0.6, 0.6, 0.5, -0.3, -0.3, 0.0, -0.3), (0.15, -0.1, 0.05, 0.03, -0.02, 0.0, 0.05), (0.0,) * 7]
_SRC = {}


def synthetic_mean_landmarks():
    """(points [L, 3] float64, vertex indices [L]) on the mean shape of train.SyntheticFaceSource: 12 vertices spread over
    the mesh, not coplanar."""
    if not _SRC:
        src = train.SyntheticFaceSource(torch.device("cpu"), face_sized=False)
        v = src.model.fc.bias.detach().view(-1, 3).double().numpy()
        idx = np.linspace(0, len(v) - 1, 12).round().astype(np.int64)
        assert np.linalg.matrix_rank(v[idx] - v[idx].mean(0), tol=1e-3) == 3
        _SRC["v"], _SRC["idx"], _SRC["src"] = v, idx, src
    return _SRC["v"][_SRC["idx"]], _SRC["idx"]


def project_np(pts, pose, hw):
    """Pixel index coordinates [L, 2] of points [L, 3] under a pose [7] in an (H, W) picture, float64."""
    p = torch.tensor(pose, dtype=torch.float64)
    v = torch.from_numpy(pts) @ (torch.exp(p[6]) * utils_3d.euler_mat(p[:3], "yxz")) + p[3:6]
    return landmark.project(v, hw).numpy()


@pytest.mark.parametrize("hw", [(64, 64), (48, 64)])
@pytest.mark.parametrize("pose", POSES)
def test_pose_from_landmarks_recovers_a_known_pose(hw, pose):
    pts, _ = synthetic_mean_landmarks()
    lmk = project_np(pts, pose, hw)
    got = align.pose_from_landmarks(pts, lmk, hw)
    assert got.shape == (7,) and got.dtype == np.float64 and got[5] == 0.0
    assert np.abs(got - np.array(pose)).max() <= 1e-8
    # one pair perturbed and its weight 0: the same pose
    bad = lmk.copy()
    bad[4] += (7.0, -3.0)
    w = np.ones(len(pts))
    w[4] = 0.0
    assert np.abs(align.pose_from_landmarks(pts, bad, hw, w) - np.array(pose)).max() <= 1e-8
    assert np.abs(align.pose_from_landmarks(pts, bad, hw) - np.array(pose)).max() > 1e-3


def test_pose_from_landmarks_refuses_what_does_not_pair_up():
    pts, _ = synthetic_mean_landmarks()
    with pytest.raises(ValueError):
        align.pose_from_landmarks(pts, np.zeros((len(pts) - 1, 2)), 64)
    with pytest.raises(ValueError):
        align.pose_from_landmarks(pts, np.zeros((len(pts), 2)), 64, np.zeros(len(pts)))


def test_solve_ortho_without_weights_is_unchanged_by_unit_weights():
    pts, _ = synthetic_mean_landmarks()
    dst = project_np(pts, POSES[0], (64, 64)) + 0.3 * synth.det_normal((len(pts), 2), 3)
    assert np.abs(align.solve_ortho(pts, dst) - align.solve_ortho(pts, dst, weights=np.ones(len(pts)))).max() <= 1e-9


# (whole-number ratios when shrinking: the taps of the antialiasing filter are then symmetric about the pixel centre and
# a linear picture comes through exactly; at other ratios their discrete centroid is off by some thousandths of a pixel)
@pytest.mark.parametrize("src,dst", [((24, 36), (48, 48)), ((48, 32), (16, 16))])
def test_scale_landmarks_round_trips_and_follows_load_images_pixel_centres(tmp_path, src, dst):
    lmk = np.array([[10.0, 7.0], [3.25, 15.5], [20.0, 11.0]])
    there = align.scale_landmarks(lmk, src, dst)
    assert np.abs(align.scale_landmarks(there, dst, src) - lmk).max() <= 1e-12
    # pixel centres: index -1/2 is the picture's edge in both
    assert np.allclose(align.scale_landmarks([[-0.5, -0.5]], src, dst), [[-0.5, -0.5]])
    assert np.allclose(align.scale_landmarks([[src[1] - 0.5, src[0] - 0.5]], src, dst), [[dst[1] - 0.5, dst[0] - 0.5]])
    # a picture that is linear in x and y stays that function under load_image's resize (away from the border), so its
    # value at a landmark is the resized picture's value at the scaled landmark
    ys, xs = np.meshgrid(np.arange(src[0]), np.arange(src[1]), indexing="ij")
    ramp = lambda x, y: 0.03 * x - 0.02 * y - 0.2                                   # noqa: E731
    path = str(tmp_path / "ramp.npy")
    np.save(path, np.repeat(ramp(xs, ys)[:, :, None], 3, 2).astype(np.float32))
    img, shape = reconstruct.load_image(path, dst[0], with_shape=True)
    assert shape == src and tuple(img.shape) == (1, 3) + dst
    for (x, y), (xs_, ys_) in zip(lmk, there):
        x0, y0 = int(np.floor(xs_)), int(np.floor(ys_))
        fx, fy = xs_ - x0, ys_ - y0
        px = img[0, 0, y0:y0 + 2, x0:x0 + 2].double().numpy()
        got = (px[0, 0] * (1 - fx) + px[0, 1] * fx) * (1 - fy) + (px[1, 0] * (1 - fx) + px[1, 1] * fx) * fy
        assert abs(got - ramp(x, y)) <= 1e-5, (x, y, got, ramp(x, y))


# ---- the composite definition ----------------------------------------------------------------------------------------
def composite_case(b=2, nv=9, dtype=torch.float64, hw=(12, 16), beta=1.0):
    """Vertex landmarks, genuine barycentric ones, two landmarks on one vertex, a zero-confidence row (the last sample)
    and residuals on both sides of beta."""
    v = torch.from_numpy(0.8 * synth.det_uniform((b, nv, 3), 31)).to(dtype)
    idx = torch.tensor([[0, 0, 0], [3, 3, 3], [3, 3, 3], [1, 2, 4], [5, 7, 8], [8, 8, 8]], dtype=torch.int32)
    bary = torch.tensor([[1, 0, 0], [1, 0, 0], [1, 0, 0], [0.5, 0.25, 0.25], [0.2, 0.3, 0.5], [1, 0, 0]], dtype=torch.float32)
    with torch.no_grad():
        p = landmark.project(landmark.landmark_points(v, idx, bary), hw)
    # residuals: inside (-beta, beta) for even landmarks, outside for odd ones
    off = torch.tensor([[0.3, -0.6], [2.5, -1.7], [-0.4, 0.2], [-3.0, 4.0], [0.7, 0.1], [1.5, -2.5]], dtype=dtype) * beta
    target = p - off
    conf = torch.from_numpy(np.abs(synth.det_uniform((b, 6), 32)) + 0.1).to(dtype)
    conf[-1] = 0.0
    return v, idx, bary, target, conf, hw


def test_composite_passes_gradcheck_and_gradgradcheck():
    v, idx, bary, target, conf, hw = composite_case()
    v.requires_grad_(True)
    f = lambda x: landmark.landmark_composite(x, idx, bary, target, conf, hw, 1.0)[0]           # noqa: E731
    assert torch.autograd.gradcheck(f, (v,), eps=1e-6, atol=1e-8)
    assert torch.autograd.gradgradcheck(f, (v,), eps=1e-6, atol=1e-8)
    # landmark_loss on float64 host tensors is that composite
    rows, p = landmark.landmark_loss(v, idx, bary, target, conf, hw)
    want, wp = landmark.landmark_composite(v, idx, bary, target, conf, hw)
    assert torch.equal(rows, want) and torch.equal(p, wp)


def test_composite_is_the_written_definition():
    v, idx, bary, target, conf, hw = composite_case()
    rows, p = landmark.landmark_composite(v, idx, bary, target, conf, hw, beta=0.5, weight=3.0)
    h, w = hw
    for b in range(v.shape[0]):
        num = den = 0.0
        for l in range(idx.shape[0]):
            P = sum(float(bary[l, k]) * v[b, int(idx[l, k])].numpy() for k in range(3))
            px, py = (1 + P[0]) * w / 2 - 0.5, (1 - P[1]) * h / 2 - 0.5
            assert abs(px - float(p[b, l, 0])) <= 1e-12 and abs(py - float(p[b, l, 1])) <= 1e-12
            for e in (px - float(target[b, l, 0]), py - float(target[b, l, 1])):
                num += float(conf[b, l]) * (0.5 * e * e / 0.5 if abs(e) < 0.5 else abs(e) - 0.25)
            den += float(conf[b, l])
        want = 3.0 * 2.0 / max(w, h) * num / max(den, landmark.TINY)
        assert abs(float(rows[b]) - want) <= 1e-12 * max(1.0, abs(want))


def test_all_zero_confidence_gives_zero_loss_and_zero_gradient():
    v, idx, bary, target, conf, hw = composite_case()
    v.requires_grad_(True)
    rows, _ = landmark.landmark_composite(v, idx, bary, target, conf, hw)
    assert float(rows.detach()[-1]) == 0.0 and float(rows.detach()[0]) > 0
    (g,) = torch.autograd.grad(rows.sum(), v)
    assert torch.isfinite(g).all() and float(g[-1].abs().max()) == 0.0 and float(g[0].abs().max()) > 0
    assert float(g[..., 2].abs().max()) == 0.0                              # orthographic: nothing reaches z
    assert float(g[0, 6].abs().max()) == 0.0                                # vertex 6 carries no landmark


def test_vertex_lists_are_the_embeddings_transpose():
    _, idx, bary, _, _, _ = composite_case()
    off, ll, w, idx32, bary32 = landmark.vertex_lists(idx, bary, 9)
    assert off.dtype == torch.int32 and ll.dtype == torch.int32 and w.dtype == torch.float32
    assert off.tolist() == [0, 1, 2, 3, 5, 6, 7, 7, 8, 10]                  # zero weights are not listed
    assert ll.tolist() == [0, 3, 3, 1, 2, 3, 4, 4, 4, 5] 
    assert torch.equal(w, torch.tensor([1, 0.5, 0.25, 1, 1, 0.25, 0.2, 0.3, 0.5, 1]))
    assert torch.equal(idx32, idx) and torch.equal(bary32, bary)
    with pytest.raises(ValueError):
        landmark.vertex_lists(idx.clone(), bary, 8)


# ---- the embedding ---------------------------------------------------------------------------------------------------
def test_landmark_embedding_accepts_each_form(tmp_path):
    tri = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 0]])
    verts = np.array([4, 0, 5])
    idx, bary = face_model.landmark_embedding(verts)
    assert idx.dtype == torch.int32 and bary.dtype == torch.float32
    assert idx.tolist() == [[4] * 3, [0] * 3, [5] * 3] and bary.tolist() == [[1, 0, 0]] * 3
    faces, bw = np.array([1, 2]), np.array([[0.5, 0.25, 0.25], [0.0, 1.0, 0.0]], np.float32)
    fi, fb = face_model.landmark_embedding((faces, bw), tri)
    assert fi.tolist() == [[2, 3, 4], [4, 5, 0]] and np.array_equal(fb.numpy(), bw)
    # tensors and the three file forms
    ti, tb = face_model.landmark_embedding((torch.from_numpy(faces), torch.from_numpy(bw)), torch.from_numpy(tri))
    assert torch.equal(ti, fi) and torch.equal(tb, fb)
    np.save(str(tmp_path / "v.npy"), verts)
    np.savetxt(str(tmp_path / "v.txt"), verts, fmt="%d")
    np.savez(str(tmp_path / "v.npz"), idx=verts)
    np.savez(str(tmp_path / "f.npz"), faces=faces, bary=bw)
    np.savetxt(str(tmp_path / "f.txt"), np.concatenate((faces[:, None], bw), 1))
    for name in ("v.npy", "v.txt", "v.npz"):
        got = face_model.landmark_embedding(str(tmp_path / name), tri)
        assert torch.equal(got[0], idx) and torch.equal(got[1], bary), name
    for name in ("f.npz", "f.txt"):
        got = face_model.landmark_embedding(str(tmp_path / name), tri)
        assert torch.equal(got[0], fi) and torch.equal(got[1], fb), name


def test_landmark_embedding_rejects_what_is_out_of_range():
    tri = np.array([[0, 1, 2], [2, 3, 4]])
    for bad in (np.array([0, -1]), np.array([0.5, 1.0])):
        with pytest.raises(ValueError):
            face_model.landmark_embedding(bad, tri)
    # a vertex no triangle uses is a vertex all the same: its upper bound is the mesh's nv, checked where the embedding
    # meets the vertices
    idx, bary = face_model.landmark_embedding(np.array([0, 5]), tri)
    assert idx[1].tolist() == [5, 5, 5]
    landmark.vertex_lists(idx, bary, 6)
    with pytest.raises(ValueError):
        landmark.vertex_lists(idx, bary, 5)
    bw = np.array([[1.0, 0.0, 0.0]], np.float32)
    for faces in (np.array([2]), np.array([-1])):
        with pytest.raises(ValueError):
            face_model.landmark_embedding((faces, bw), tri)
    with pytest.raises(ValueError):
        face_model.landmark_embedding((np.array([0]), bw))                  # faces need tri
    with pytest.raises(ValueError):
        face_model.landmark_embedding((np.array([0]), np.array([[np.nan, 0, 1]], np.float32)), tri)


def _bfm_dict(with_landmarks):
    v0, tri = synth.uv_ellipsoid(16, 14)
    nv = v0.shape[0]
    cell = np.empty((1, 1), dtype=object)
    cell[0, 0] = (tri + 1).astype(np.float64)                            # MATLAB: 1-based, in a cell
    data = {"v": (v0.T * 1e5).astype(np.float64), "w_shape": 1e3 * synth.det_uniform((3 * nv, 5), 21).astype(np.float64),
            "w_exp": 1e3 * synth.det_uniform((3 * nv, 4), 22).astype(np.float64), "tri": cell}
    if with_landmarks:
        data["landmarks68"] = (np.arange(68) * 3 % nv + 1).reshape(1, -1).astype(np.float64)
    return data, nv, tri


def test_load_bfm_reads_landmarks68_when_the_file_has_it():
    data, nv, tri = _bfm_dict(True)
    model, t = face_model.load_bfm(data)
    assert model.dim == [5, 4, 3 * nv] and np.array_equal(t.numpy(), tri)
    idx, bary = model.landmarks
    assert idx.shape == (68, 3) and idx[:, 0].tolist() == list(np.arange(68) * 3 % nv)
    assert bool((idx == idx[:, :1]).all()) and bary.tolist() == [[1, 0, 0]] * 68
    # the same vertices as the alignment template's
    tpl = align.template_from_bfm(data)
    mean = model.fc.bias.detach().view(-1, 3).double().numpy()
    assert np.abs(mean[idx[:, 0].long().numpy()] - tpl).max() <= 1e-6
    plain, _ = face_model.load_bfm(_bfm_dict(False)[0])
    assert plain.landmarks is None
    assert face_model.BlendShapeModel(4, 1, 1).landmarks is None
    assert face_model.LinearBlendSkinningModel(4, 2, 1).landmarks is None


# ---- the inverter ----------------------------------------------------------------------------------------------------
_PROBLEM = []


def tiny_problem():
    """test_reconstruct_cpu's 16 x 16 problem, built once (the inverter freezes the generator and changes nothing else)."""
    if not _PROBLEM:
        _PROBLEM.append(_tiny_problem())
    return _PROBLEM[0]


TRUE_POSE = (0.2, -0.1, 0.05, 0.03, -0.02, 0.0, 0.05)                    # tiny_problem's target pose


def tiny_landmarks(face, pose=TRUE_POSE, hw=(16, 16), coeff=None):
    """An embedding of 10 vertices of the tiny face (one barycentric) and their projection at `pose` on the mean shape
    (or on the shape of `coeff` [1, d])."""
    fm, tri = face
    nv = fm.fc.bias.numel() // 3
    verts = np.linspace(0, nv - 1, 10).round().astype(np.int64)
    idx, bary = face_model.landmark_embedding(verts)
    idx[3] = tri[7].to(torch.int32)
    bary[3] = torch.tensor([0.25, 0.5, 0.25])
    with torch.no_grad():
        shape = fm(torch.zeros(1, fm.n_coeff) if coeff is None else coeff).double()
    pts = landmark.landmark_points(shape, idx, bary.double())[0].numpy()
    return (idx, bary), project_np(pts, pose, hw)


def _inverter(problem, **kw):
    g, _, face, noise, target = problem
    torch.manual_seed(3)
    return inversion.LatentInverter(g, lpips.PNetLin(), target, None, lr=0.05, pose_lr=0.02, noise=noise,
                                    n_mean_latent=64, face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3, **kw)


def test_inverter_starts_at_the_pose_of_the_landmarks():
    problem = tiny_problem()
    emb, lmk = tiny_landmarks(problem[2])
    inv = _inverter(problem, landmarks=lmk, landmark_embedding=emb)
    assert inv.pose.shape == (7,) and inv.pose.requires_grad
    # float32 storage of a float64 closed form on exact data (float32 mean shape)
    assert float((inv.pose.detach().double() - torch.tensor(TRUE_POSE, dtype=torch.float64)).abs().max()) <= 1e-6
    # every confidence 0: the pose stays at zero, the term is 0
    off = _inverter(problem, landmarks=lmk, landmark_conf=np.zeros((1, 10)), landmark_embedding=emb)
    assert float(off.pose.detach().abs().max()) == 0.0
    off.run(1)
    assert float(off.landmark.rows.detach().abs().max()) == 0.0


def test_inverter_refuses_landmarks_it_cannot_use():
    problem = tiny_problem()
    g, mesh, face, noise, target = problem
    emb, lmk = tiny_landmarks(face)
    with pytest.raises(ValueError, match="landmark_embedding"):
        _inverter(problem, landmarks=lmk)                                 # the model names no landmarks
    with pytest.raises(ValueError, match="fit_shape"):
        inversion.LatentInverter(g, lpips.PNetLin(), target, mesh, noise=noise, n_mean_latent=8, landmarks=lmk,
                                 landmark_embedding=emb)
    with pytest.raises(ValueError):
        _inverter(problem, landmarks=lmk[:-1], landmark_embedding=emb)
    plain = _inverter(problem)
    with pytest.raises(ValueError):
        plain.reset(target, landmarks=lmk)


def _mean_distance(inv, lmk):
    return float(np.sqrt(((inv.landmarks_fit[0].double().numpy() - lmk) ** 2).sum(1)).mean())


def test_a_large_landmark_weight_keeps_the_mesh_on_the_landmarks():
    """The landmarks of the face the target shows (tiny_problem's coefficients and pose): the closed-form start on the
    mean shape leaves the distance that the difference in shape makes, and the fit must not lose it."""
    problem = tiny_problem()
    fm = problem[2][0]
    c_true = torch.from_numpy(synth.det_normal((1, 14), 3)) * fm.sigma.detach()
    emb, lmk = tiny_landmarks(problem[2], coeff=c_true)
    inv = _inverter(problem, landmarks=lmk, landmark_embedding=emb, landmark_weight=100.0)
    first = inv.run(1).numpy()
    start = _mean_distance(inv, lmk)                                     # landmarks_fit of the first forward: the start
    hist = inv.run(29).numpy()
    print("mean landmark distance: start %.4f px, after 30 steps %.4f px" % (start, _mean_distance(inv, lmk)))
    assert np.isfinite(first).all() and np.isfinite(hist).all()
    assert _mean_distance(inv, lmk) <= start
    # loss_value and the history include the term
    assert float(inv.loss_value) == float(hist[-1]) and float(first[0]) > 100.0 * 2 / 16 * 0.01


def test_without_landmarks_the_inverter_is_bit_identical():
    problem = tiny_problem()
    runs = []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                  # the CPU path's threaded reductions are not run-to-run identical
    try:
        for extra in ({}, {"landmarks": None, "landmark_weight": 7.0, "landmark_beta": 0.5,
                           "landmark_embedding": tiny_landmarks(problem[2])[0]}):
            inv = _inverter(problem, **extra)
            runs.append((inv.run(6).numpy(), inv.w.detach().clone(), inv.pose.detach().clone(), inv.coeff.detach().clone()))
            assert inv.landmarks_fit is None and not inv.with_landmarks
    finally:
        torch.set_num_threads(threads)
    assert np.array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)


def test_batched_reset_with_landmarks_equals_a_fresh_inverter():
    g, mesh, face, noise, target = tiny_problem()
    emb, lmk_a = tiny_landmarks(face)
    _, lmk_b = tiny_landmarks(face, pose=(-0.1, 0.2, 0.0, -0.05, 0.04, 0.0, -0.1))
    targets = torch.cat([target, target.flip(3)], 0).contiguous()
    first = dict(landmarks=np.stack([lmk_a, lmk_b]), landmark_conf=np.ones((2, 10)))
    second = dict(landmarks=np.stack([lmk_b, lmk_a]), landmark_conf=np.stack([np.ones(10), np.zeros(10)]))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        inv = _inverter((g, mesh, face, noise, targets), landmark_embedding=emb, **first)
        assert inv.pose.shape == (2, 7) and inv.run(3).shape == (3, 2) and inv.landmarks_fit.shape == (2, 10, 2)
        inv.reset(targets.flip(0).contiguous(), **second)
        assert float(inv.pose.detach()[1].abs().max()) == 0.0 and float(inv.pose.detach()[0].abs().max()) > 0
        got = [inv.run(3)] + [t.detach().clone() for t in (inv.w, inv.pose, inv.coeff)]
        fresh = _inverter((g, mesh, face, noise, targets.flip(0).contiguous()), landmark_embedding=emb, **second)
        want = [fresh.run(3)] + [t.detach().clone() for t in (fresh.w, fresh.pose, fresh.coeff)]
    finally:
        torch.set_num_threads(threads)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


# ---- command line ----------------------------------------------------------------------------------------------------
def test_reconstruct_cli_with_landmarks(tmp_path):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    imgs = []
    for k, name in enumerate(("face_a", "face_b", "face_c")):
        from PIL import Image

        path = str(tmp_path / (name + ".png"))                           # (the reader knows pictures by .png / .jpg / .bmp)
        pix = (127.5 * (synth.det_uniform((24, 32, 3), 9 + k) + 1)).clip(0, 255).astype(np.uint8)
        Image.fromarray(pix).save(path)                                  # 24 x 32, resized to 16 on the host
        imgs.append(path)
    v0, _ = synth.face_sized_mesh()                                      # train.SyntheticFaceSource's mesh
    verts = np.linspace(0, len(v0) - 1, 9).round().astype(np.int64)
    index = str(tmp_path / "index.txt")
    np.savetxt(index, verts, fmt="%d")
    # landmarks in the pictures' own pixels (24 x 32): the mean shape at a pose, scaled from the 16 x 16 target
    pose = (0.2, -0.1, 0.05, 0.05, -0.04, 0.0, -0.1)
    lmk = {name: align.scale_landmarks(project_np(v0[verts].astype(np.float64), pose, (16, 16)) + shift, (16, 16), (24, 32))
           for name, shift in (("face_a", 0.0), ("face_c", 0.5))}
    lmk_file = str(tmp_path / "lmk.txt")
    with open(lmk_file, "w") as f:
        for name, pts in lmk.items():                                    # face_b is not listed
            f.write(name + ".png " + " ".join("%.6f" % x for x in pts.reshape(-1)) + "\n")
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "4", "--n_mean_latent",
           "64", "--batch", "2", "--lmk", lmk_file, "--lmk_index", index, "--lmk_weight", "2.0", "--out", out, ckpt] + imgs
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "landmarks: 1 of 3 images are not listed" in res.stdout, res.stdout
    assert sorted(os.listdir(out)) == sorted(n + s for n in ("face_a", "face_b", "face_c")
                                             for s in (".obj", "_canonical.obj", "_render.png", "_normal.png", ".npz"))
    for name in ("face_a", "face_b", "face_c"):
        r = np.load(os.path.join(out, name + ".npz"))
        assert r["w"].shape == (1, g.n_latent, 512) and r["coeff"].shape == (1, 144) and r["pose"].shape == (7,)
        assert r["loss"].shape == (4,) and np.isfinite(r["loss"]).all()
        assert r["landmarks"].shape == (9, 2) and np.isfinite(r["landmarks"]).all()
        assert r["landmarks_target"].shape == (9, 2) and r["lmk_error"].shape == ()
        if name == "face_b":
            assert np.isnan(r["landmarks_target"]).all() and np.isnan(r["lmk_error"])
        else:
            assert np.abs(r["landmarks_target"] - lmk[name]).max() <= 1e-5
            want = np.sqrt(((r["landmarks"] - r["landmarks_target"]) ** 2).sum(1)).mean()
            assert abs(float(r["lmk_error"]) - want) <= 1e-9
            # four steps from the closed-form start: still within a few pixels of the 24 x 32 picture's landmarks
            assert float(r["lmk_error"]) < 3.0, float(r["lmk_error"])
            assert abs(r["pose"][0] - pose[0]) < 0.1
    # a model without landmarks and no --lmk_index: the error names the option
    res = subprocess.run([a for a in cmd if a not in ("--lmk_index", index)], env=_env(), cwd=str(tmp_path),
                         capture_output=True, text=True, timeout=900)
    assert res.returncode != 0 and "--lmk_index" in res.stderr
