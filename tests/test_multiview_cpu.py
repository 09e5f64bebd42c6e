"""CPU: several views of one subject — op.share's tied gradient against its definition and against an explicit shared
leaf, LatentInverter(shared_identity=K) on the three face models (the shared columns stay equal bit for bit, reset, the
option off), op.texture.merge on hand-computed cases and against float64, and `reconstruct --multiview` end to end."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_blendshape_cpu as blended
import test_flame_cpu as skinned
from stylerenderer_amd import face_model, synth
from stylerenderer_amd.op import share, texture
from test_reconstruct_batch_cpu import batch_problem, first_gradients, make_inverter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- share_rows_ -----------------------------------------------------------------------------------------------------
def share_by_hand(g, k):
    """The definition in scalar float32 arithmetic: s = ((g[0, j] + g[1, j]) + g[2, j]) + ..., then every row gets s."""
    out = g.copy()
    for j in range(k):
        s = np.float32(g[0, j])
        for b in range(1, g.shape[0]):
            s = np.float32(s + np.float32(g[b, j]))
        out[:, j] = s
    return out


def share_input(b, d, seed=50):
    """Seeded float32 with mixed signs and mixed magnitudes (so that the order of the additions shows)."""
    return (synth.det_normal((b, d), seed + b) * 10.0 ** synth.det_uniform((b, d), seed + 1 + b)).astype(np.float32)


@pytest.mark.parametrize("b,d,k", [(1, 5, 5), (2, 7, 3), (3, 14, 10)])
def test_share_rows_is_its_definition(b, d, k):
    g = share_input(b, d)
    assert (g > 0).any() and (g < 0).any()
    t = torch.from_numpy(g.copy())
    assert share.share_rows_(t, k) is t                                      # in place
    want = share_by_hand(g, k)
    assert np.array_equal(t.numpy(), want)
    assert np.array_equal(t.numpy()[:, k:], g[:, k:])                        # columns >= k are untouched
    for row in range(b):
        assert np.array_equal(t.numpy()[row, :k], want[0, :k])
    t64 = torch.from_numpy(g.astype(np.float64))
    share.share_rows_(t64, k)
    assert float((t64[0, :k] - torch.from_numpy(g.astype(np.float64))[:, :k].sum(0)).abs().max()) <= 1e-12


def test_share_rows_refuses_bad_arguments():
    g = torch.zeros(3, 5)
    for k in (0, -1, 6):
        with pytest.raises(ValueError):
            share.share_rows_(g, k)
    with pytest.raises(ValueError):
        share.share_rows_(torch.zeros(5), 1)
    with pytest.raises(ValueError):
        share.share_rows_(torch.zeros(5, 3).t(), 1)                          # not contiguous
    with pytest.raises(ValueError):
        share.share_rows_(torch.zeros(3, 5, dtype=torch.int32), 1)


def test_share_rows_argument_validation_of_the_c_abi():
    from stylerenderer_amd import _lib

    L = _lib.lib()
    assert L.sr_share_rows(None, 3, 5, 2, None) == -1                        # NULL
    assert L.sr_share_rows(None, 3, 5, 0, None) == -1 and L.sr_share_rows(None, 3, 5, 6, None) == -1
    assert L.sr_share_rows(None, 0, 5, 2, None) == -1
    assert L.sr_texture_merge(None, None, None, None, None, 2, 3, 8, 8, 2, None) == -1
    assert L.sr_texture_merge(None, None, None, None, None, 0, 3, 8, 8, 2, None) == -1
    assert L.sr_texture_merge(None, None, None, None, None, 65, 3, 8, 8, 2, None) == -1
    assert L.sr_texture_merge(None, None, None, None, None, 2, 3, 8, 8, 5, None) == -1
    assert L.sr_texture_merge(None, None, None, None, None, 2, 3, 0, 8, 2, None) == 0


# ---- the tied gradient -------------------------------------------------------------------------------------------------
def single_threaded(fn):
    @functools.wraps(fn)
    def run(*args, **kw):
        threads = torch.get_num_threads()
        torch.set_num_threads(1)              # the CPU path's threaded reductions are not run-to-run identical
        try:
            return fn(*args, **kw)
        finally:
            torch.set_num_threads(threads)
    return run


@single_threaded
def test_the_tied_gradient_is_the_gradient_of_the_shared_variable():
    """The B = 3 objective with an explicit leaf theta [K] expanded into the rows: autograd's theta.grad[j] is the sum of
    the three rows' gradients g_b[j], and so is the tied coeff.grad[:, j]; the graphs up to there are the same, so the two
    differ only by the order of a three-term float32 sum.  Each order rounds twice, each rounding by at most 2^-24 of a
    partial sum that is at most sum_b |g_b[j]|: |diff| <= 4 * 2^-24 * sum_b |g_b[j]| per column."""
    prob = batch_problem()
    fm = prob[2][0]
    k, d = fm.n_identity, fm.n_coeff
    assert (k, d) == (8, 14)
    start = torch.from_numpy(synth.det_normal((3, d), 77)).float() * 0.3 * fm.sigma
    start[:, :k] = start[0, :k]                                              # the rows agree on the shared columns
    # the tied inverter: every row's own gradient, then the tie
    inv = make_inverter(*prob[:4], prob[4], shared_identity=k)
    with torch.no_grad():
        inv.coeff.copy_(start)
    rows = first_gradients(inv)[3]                                           # [3, d], untied
    tied = share.share_rows_(rows.clone(), k)
    assert torch.equal(tied[:, k:], rows[:, k:])
    for b in (1, 2):
        assert torch.equal(tied[b, :k], tied[0, :k])
    # the three rows' own gradients differ: the test is not three copies of one view
    scale = float(rows[:, :k].abs().max())
    assert scale > 0
    assert float((rows[0, :k] - rows[1, :k]).abs().max()) > 1e-3 * scale
    assert float((rows[1, :k] - rows[2, :k]).abs().max()) > 1e-3 * scale
    # the explicit leaf
    ref = make_inverter(*prob[:4], prob[4])
    theta = start[0, :k].clone().requires_grad_(True)
    rest = start[:, k:].clone().requires_grad_(True)
    ref.coeff = torch.cat([theta.unsqueeze(0).expand(3, k), rest], 1)
    ref.loss(ref.render()).backward()
    bound = 4 * 2.0 ** -24 * rows[:, :k].abs().sum(0).double()
    diff = (theta.grad.double() - tied[0, :k].double()).abs()
    print("tied against the explicit leaf: |diff| / bound per column", (diff / bound).tolist())
    assert bool((diff <= bound).all()), (diff / bound).tolist()
    assert torch.equal(rest.grad, rows[:, k:])                               # the per-view columns are untouched


# ---- the inverter ------------------------------------------------------------------------------------------------------
def linear_case():
    g, mesh, face, noise, targets = batch_problem()
    return (lambda target, **kw: make_inverter(g, mesh, face, noise, target, **kw)), face[0], targets


def skinned_case():
    g, face, noise, targets = skinned.flame_problem()
    return (lambda target, **kw: skinned.make_inverter(g, face, noise, target, **kw)), face[0], targets


def blended_case():
    g, face, noise, targets = blended.blendshape_problem()
    return (lambda target, **kw: blended.make_inverter(g, face, noise, target, **kw)), face[0], targets


def state(inv, hist):
    return [hist.detach().clone()] + [t.detach().clone() for t in (inv.w, inv.pose, inv.coeff)]


@pytest.mark.parametrize("case,k,d", [(linear_case, 8, 14), (skinned_case, 8, 20), (blended_case, 5, 9)])
@single_threaded
def test_shared_identity_on_every_face_model(case, k, d):
    build, fm, targets = case()
    assert (fm.n_identity, fm.n_coeff) == (k, d)
    other = targets.flip(0).contiguous()
    rows = targets.shape[0]
    inv = build(targets, shared_identity=k)
    assert inv.shared_identity == k
    first = state(inv, inv.run(6))
    coeff, pose = first[3], first[2]
    assert float(coeff[:, :k].abs().max()) > 0
    for b in range(1, rows):
        assert torch.equal(coeff[b, :k], coeff[0, :k])                       # bit-identical across the rows
        assert not torch.equal(coeff[b, k:], coeff[0, k:]) and not torch.equal(pose[b], pose[0])
    # reset, then run: a fresh shared-identity inverter on the other pictures
    inv.reset(other)
    got = state(inv, inv.run(6))
    fresh = build(other, shared_identity=k)
    want = state(fresh, fresh.run(6))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert not torch.equal(first[0], got[0])
    # the option off is the inverter without the keyword
    off = build(targets, shared_identity=None)
    assert off.shared_identity is None
    plain = build(targets)
    for a, b in zip(state(off, off.run(6)), state(plain, plain.run(6))):
        assert torch.equal(a, b)
    assert not torch.equal(plain.coeff.detach()[0, :k], plain.coeff.detach()[1, :k])     # untied rows go their own way
    assert not torch.equal(plain.coeff.detach(), coeff)


def test_shared_identity_refuses_bad_arguments():
    from stylerenderer_amd import inversion, lpips

    g, mesh, face, noise, targets = batch_problem()
    percept = lpips.PNetLin()
    for bad in (0, 15, -1, 2.0, True):
        with pytest.raises(ValueError):
            inversion.LatentInverter(g, percept, targets, None, noise=noise, n_mean_latent=64, face=face, fit_shape=True,
                                     shared_identity=bad)
    with pytest.raises(ValueError):
        inversion.LatentInverter(g, percept, targets, mesh, noise=noise, n_mean_latent=64, shared_identity=3)
    one = make_inverter(g, mesh, face, noise, targets[:1], shared_identity=14)           # a single view, every column
    assert one.shared_identity == 14 and one.run(2).shape == (2,)


def test_every_model_names_its_identity_columns():
    assert linear_case()[1].n_identity == 8 and blended_case()[1].n_identity == 5
    from stylerenderer_amd import train

    small, _ = face_model.load_flame(train.synthetic_flame_dict(8, mesh=synth.uv_ellipsoid(6, 6)))
    assert small.n_identity == small.dim[0] == 8
    # a published FLAME file's layout: 400 columns of shapedirs, 300 of identity and then 100 of expression
    big, _ = face_model.load_flame(train.synthetic_flame_dict(400, mesh=synth.uv_ellipsoid(6, 6)))
    assert big.dim[0] == 400 and big.n_identity == 300 == face_model.FLAME_IDENTITY_DIMS
    edge, _ = face_model.load_flame(train.synthetic_flame_dict(300, mesh=synth.uv_ellipsoid(6, 6)))
    assert edge.n_identity == 300


# ---- merge -------------------------------------------------------------------------------------------------------------
def merge_stack(n_v, c_n, size, seed=70, dtype=torch.float32):
    """tex [V, C, Th, Tw] and weight [V, 1, Th, Tw] whose texels contain, in this order along the flattened plane and then
    repeating: an empty texel, an exact tie of all views, a power-of-two ladder (the first view at 3/4, the others at 3/4 of
    2^-4, 2^-8, ... 2^-20 from one ladder texel to the next), and ordinary smoothstep values with single views switched off
    here and there."""
    th, tw = size
    tex = torch.from_numpy(synth.det_uniform((n_v, c_n, th, tw), seed).astype(np.float32))
    t = torch.from_numpy(synth.det_uniform((n_v, 1, th, tw), seed + 1).astype(np.float32)).abs().clamp(0, 1)
    smooth = t * t * (3.0 - 2.0 * t)
    off = torch.from_numpy(synth.det_uniform((n_v, 1, th, tw), seed + 2)) > 0.6
    smooth = torch.where(off, torch.zeros_like(smooth), smooth)
    kind = (torch.arange(th * tw) % 4).view(1, 1, th, tw)
    step = (torch.arange(th * tw) // 4 % 5 + 1).view(1, 1, th, tw).float()
    later = (torch.arange(n_v) > 0).view(n_v, 1, 1, 1).float()
    ladder = 0.75 * 2.0 ** (-4.0 * step * later)
    tie = torch.full((n_v, 1, th, tw), 0.625)
    weight = torch.where(kind == 0, torch.zeros_like(smooth),
                         torch.where(kind == 1, tie, torch.where(kind == 2, ladder, smooth)))
    return tex.to(dtype), weight.to(dtype)


def test_merge_of_one_view_is_the_view():
    tex, weight = merge_stack(1, 3, (5, 7))
    out, w, best = texture.merge(tex, weight, 2)
    assert out.shape == (1, 3, 5, 7) and w.shape == (1, 1, 5, 7) and best.shape == (5, 7) and best.dtype == torch.uint8
    seen = weight[0, 0] > 0
    assert 0 < int(seen.sum()) < seen.numel()
    assert torch.equal(out[0][:, seen], tex[0][:, seen]) and bool((out[0][:, ~seen] == 0).all())
    assert torch.equal(w, weight) and torch.equal(best, torch.where(seen, 0, 255).to(torch.uint8))
    assert torch.equal(tex, merge_stack(1, 3, (5, 7))[0])                    # the input is not changed


def test_merge_hand_computed_texels():
    # texel 0: equal weights; 1: weights (1, 2^-4); 2: nobody saw it; 3: NaN colour in a view that did not see it
    nan = float("nan")
    tex = torch.tensor([[0.3, 0.5, nan, 0.25], [0.7000001, -0.5, 0.5, nan]]).view(2, 1, 1, 4)
    weight = torch.tensor([[0.4, 1.0, 0.0, 0.5], [0.4, 2.0 ** -4, 0.0, 0.0]]).view(2, 1, 1, 4)
    for sharpness in range(5):
        out, w, best = texture.merge(tex, weight, sharpness)
        assert best.tolist() == [[0, 0, 255, 0]]
        assert torch.equal(w.view(-1), torch.tensor([0.4, 1.0, 0.0, 0.5]))
        mean = (np.float32(0.3) + np.float32(0.7000001)) / np.float32(2)     # the rounded sum, halved
        assert float(out[0, 0, 0, 0]) == float(mean)
        assert float(out[0, 0, 0, 2]) == 0.0 and float(out[0, 0, 0, 3]) == 0.25
        r = np.float32(2.0 ** -(4 * 2 ** sharpness))                         # (2^-4)^(2^sharpness)
        if sharpness == 4:
            assert float(out[0, 0, 0, 1]) == 0.5                             # 2^-64 is flushed: exactly the first view
        else:
            num = np.float32(np.float32(0.5) + np.float32(r * np.float32(-0.5)))
            want = np.float32(np.float64(num) / np.float64(np.float32(np.float32(1) + r)))
            assert float(out[0, 0, 0, 1]) == float(want)
    assert not bool(torch.isnan(out).any())
    # a tie goes to the first view that attains the maximum
    weight3 = torch.tensor([0.25, 0.5, 0.5]).view(3, 1, 1, 1)
    assert int(texture.merge(torch.zeros(3, 1, 1, 1), weight3, 0)[2]) == 1


def test_merge_refuses_bad_arguments():
    tex, weight = merge_stack(2, 3, (4, 4))
    for bad in (-1, 5, 1.5, True):
        with pytest.raises(ValueError):
            texture.merge(tex, weight, bad)
    with pytest.raises(ValueError):
        texture.merge(tex, weight[:1], 2)
    with pytest.raises(ValueError):
        texture.merge(tex, weight.expand(2, 3, 4, 4), 2)
    with pytest.raises(ValueError):
        texture.merge(torch.zeros(65, 1, 2, 2), torch.zeros(65, 1, 2, 2), 2)
    with pytest.raises(ValueError):
        texture.merge(tex, weight.double(), 2)


def merge_bound(n_v, sharpness, scale):
    """|float32 - float64| of a merged colour, to first order in u = 2^-24, relative to scale = max |tex|.  A ratio r_v
    carries the division's u; every squaring doubles the relative error and adds u: (2^(s + 1) - 1) u after s.  The result
    is a weighted mean of the t_v, so relative errors e of the weights move it by at most 2 e scale.  The products add u,
    the V - 1 additions of the numerator and of the denominator (V - 1) u each, the final division u.  A ratio flushed in
    one type and not in the other is below 2^-63 of a denominator >= 1 and does not show."""
    return (2 * (2 ** (sharpness + 1) - 1) + 1 + 2 * (n_v - 1) + 1) * 2.0 ** -24 * scale


@pytest.mark.parametrize("n_v,sharpness", [(2, 0), (5, 2), (5, 4), (8, 3)])
def test_merge_in_float32_against_float64(n_v, sharpness):
    tex, weight = merge_stack(n_v, 3, (9, 11))
    out, w, best = texture.merge(tex, weight, sharpness)
    out64, w64, best64 = texture.merge(tex.double(), weight.double(), sharpness)
    assert torch.equal(best, best64) and torch.equal(w.double(), w64)
    kinds = {int(x) for x in best.unique()}
    assert 255 in kinds and 0 in kinds and len(kinds) > 2                    # empty texels, and more than one winner
    err = float((out.double() - out64).abs().max())
    bound = merge_bound(n_v, sharpness, float(tex.abs().max()))
    print("merge float32 against float64: V", n_v, "sharpness", sharpness, "error", err, "bound", bound)
    assert err <= bound


# ---- command line ----------------------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


SUBJECT_FILES = ("_identity.obj", "_identity.npz", "_merged_texture.png", "_merged_texture_weight.png",
                 "_merged_texture_views.png", "_merged.obj", "_merged.mtl")
VIEW_FILES = (".obj", "_canonical.obj", "_render.png", "_normal.png", ".npz", "_texture.png", "_texture_weight.png",
              "_textured.obj", "_textured.mtl")


def check_multiview_outputs(out, groups, steps, size, k):
    """The files and entries `reconstruct --multiview --texture` leaves for `groups` (lists of stems); returns the
    subjects' .npz entries."""
    from PIL import Image

    want = [stem + s for group in groups for stem in group for s in VIEW_FILES]
    want += [group[0] + s for group in groups for s in SUBJECT_FILES]
    assert sorted(os.listdir(out)) == sorted(want)
    subjects = []
    for group in groups:
        name = group[0]
        ident = np.load(os.path.join(out, name + "_identity.npz"))
        assert ident["identity"].shape == (k,) and ident["identity"].dtype == np.float32
        assert np.abs(ident["identity"]).max() > 0
        assert [str(x) for x in ident["views"]] == list(group)
        assert ident["loss"].shape == (steps,) and np.isfinite(ident["loss"]).all()
        assert ident["texture_coverage"].shape == (len(group),)
        total = 0.0
        for i, stem in enumerate(group):
            r = np.load(os.path.join(out, stem + ".npz"))
            assert str(r["subject"]) == name and int(r["view"]) == i
            assert r["coeff"][0, :k].tobytes() == ident["identity"].tobytes()            # bit for bit
            assert float(ident["merged_coverage"]) >= float(r["texture_coverage"]) == float(ident["texture_coverage"][i])
            assert r["texture"].shape == (3, size, size) and r["texture_weight"].shape == (size, size)
            total = total + r["loss"].astype(np.float64)
        assert np.allclose(ident["loss"], total, rtol=1e-5)
        assert 0 < float(ident["merged_coverage"]) <= 1
        for s, mode in (("_merged_texture.png", "RGB"), ("_merged_texture_weight.png", "L"),
                        ("_merged_texture_views.png", "L")):
            pic = Image.open(os.path.join(out, name + s))
            assert pic.size == (size, size) and pic.mode == mode
        views = np.asarray(Image.open(os.path.join(out, name + "_merged_texture_views.png")))
        assert np.array_equal(views, ident["merged_best"]) and set(np.unique(views)) <= set(range(len(group))) | {255}
        assert np.array_equal(views == 255, ident["merged_weight"] == 0)
        assert open(os.path.join(out, name + "_merged.mtl")).read().endswith("map_Kd %s_merged_texture.png\n" % name)
        lines = open(os.path.join(out, name + "_identity.obj")).read().splitlines()
        plain = open(os.path.join(out, group[0] + ".obj")).read().splitlines()
        for kind in ("v ", "vn ", "f "):
            assert sum(l.startswith(kind) for l in lines) == sum(l.startswith(kind) for l in plain) > 0
        merged = [l for l in open(os.path.join(out, name + "_merged.obj")) if l.startswith("v ")]
        assert merged == [l + "\n" for l in lines if l.startswith("v ")]                # the identity mesh carries it
        subjects.append(ident)
    return subjects


def remerge_on_the_host(out, group, sharpness=2):
    """op.texture.merge of the views' written bakes on the host: (tex [C, T, T], weight [T, T], best [T, T]) as numpy."""
    views = [np.load(os.path.join(out, stem + ".npz")) for stem in group]
    tex = torch.from_numpy(np.stack([r["texture"] for r in views]))
    weight = torch.from_numpy(np.stack([r["texture_weight"] for r in views]))[:, None]
    t, w, b = texture.merge(tex, weight, sharpness)
    return t[0].numpy(), w[0, 0].numpy(), b.numpy()


def test_reconstruct_cli_multiview(tmp_path):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    imgs = []
    for k in range(6):
        p = str(tmp_path / ("view_%d.npy" % k))
        np.save(p, synth.det_uniform((16, 16, 3), 140 + k))
        imgs.append(p)
    base = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "6", "--n_mean_latent", "64"]
    out = str(tmp_path / "out")
    res = subprocess.run(base + ["--multiview", "3", "--texture", "16", "--out", out, ckpt] + imgs, env=_env(),
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    groups = [["view_0", "view_1", "view_2"], ["view_3", "view_4", "view_5"]]
    first, second = check_multiview_outputs(out, groups, 6, 16, 80)                       # the synthetic 3DMM: 80 + 64
    assert first["identity"].tobytes() != second["identity"].tobytes()                   # two subjects, two identities
    for group, ident in zip(groups, (first, second)):
        t, w, b = remerge_on_the_host(out, group)
        assert t.tobytes() == ident["merged_texture"].tobytes() and w.tobytes() == ident["merged_weight"].tobytes()
        assert np.array_equal(b, ident["merged_best"])
    # five pictures are not groups of three
    bad = subprocess.run(base + ["--multiview", "3", "--out", str(tmp_path / "bad"), ckpt] + imgs[:5], env=_env(),
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert bad.returncode != 0 and "groups of 3 views, got 5 images" in bad.stderr
    assert not os.path.exists(str(tmp_path / "bad"))
    clash = subprocess.run(base + ["--multiview", "3", "--batch", "2", ckpt] + imgs, env=_env(), cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=900)
    assert clash.returncode == 2 and "conflicts with --batch 2" in clash.stderr
    # without --multiview nothing of it is written
    plain = str(tmp_path / "plain")
    res = subprocess.run(base + ["--batch", "3", "--texture", "16", "--out", plain, ckpt] + imgs[:3], env=_env(),
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(plain)) == sorted(stem + s for stem in groups[0] for s in VIEW_FILES)
    r = np.load(os.path.join(plain, "view_0.npz"))
    assert "subject" not in r.files and "view" not in r.files and "texture" not in r.files
    assert not any("_identity" in n or "_merged" in n for n in os.listdir(plain))
