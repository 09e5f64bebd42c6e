"""CPU: op.edge (the definition of the edge antialiasing node), fit_parts.Silhouette, photo_edges and the tool's options.
The hand-computed pictures are written from the formula in op/edge.py's note, not from the code: an image of small whole
numbers and edges a quarter of a pixel off a centre make every blend exact."""
import os

import numpy as np
import pytest
import torch

import edge_cases as ec
from stylerenderer_amd import fit_parts, synth
from stylerenderer_amd.op import edge, texture
from test_photometric_cpu import ROOT, one_thread, planted, run_tool  # noqa: F401  (one_thread: a fixture)


# ---- adjacency -------------------------------------------------------------------------------------------------------------
def brute_adjacency(tri):
    users = {}
    for f, t in enumerate(tri):
        for k in range(3):
            users.setdefault(frozenset((int(t[k]), int(t[(k + 1) % 3]))), []).append((f, k))
    out = np.full((len(tri), 3), -1, np.int32)
    for f, t in enumerate(tri):
        for k in range(3):
            key = frozenset((int(t[k]), int(t[(k + 1) % 3])))
            bad = len(users[key]) > 2 or any(len(set(int(x) for x in tri[g])) < 3 for g, _ in users[key])
            if bad:
                out[f, k] = -2
            elif len(users[key]) == 2:
                g, j = [u for u in users[key] if u != (f, k)][0]
                out[f, k] = tri[g][(j + 2) % 3]
    return out


@pytest.mark.parametrize("name", ["triangle", "quad", "ellipsoid", "fan", "degenerate"])
def test_adjacency_against_a_brute_force_dictionary(name):
    tri = {"triangle": [[0, 1, 2]], "quad": [[0, 1, 2], [0, 2, 3]], "ellipsoid": synth.uv_ellipsoid(10, 12)[1],
           "fan": [[0, 1, 2], [1, 0, 3], [0, 1, 4]], "degenerate": [[0, 1, 2], [2, 1, 1], [0, 2, 3]]}[name]
    tri = np.asarray(tri, np.int64)
    nv = int(tri.max()) + 1
    got = edge.adjacency(torch.from_numpy(tri), nv)
    want = brute_adjacency(tri)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    if name == "triangle":
        assert want.tolist() == [[-1, -1, -1]]
    if name == "quad":
        assert want.tolist() == [[-1, -1, 3], [1, -1, -1]]
    if name == "ellipsoid":
        assert (want >= 0).all()                                                 # closed
    if name == "fan":
        assert want[:, 0].tolist() == [-2, -2, -2] and (want[:, 1:] == -1).all()
    if name == "degenerate":
        assert want[1].tolist() == [-2, -2, -2] and want[0].tolist() == [-1, -2, 3]
    with pytest.raises(ValueError):
        edge.adjacency(torch.from_numpy(tri.copy()), nv - 1)
    t = torch.from_numpy(tri)
    assert edge.adjacency(t, nv) is edge.adjacency(t, nv)                        # cached per topology tensor


# ---- hand-computed pictures at 8 x 8 -----------------------------------------------------------------------------------
# the image: value 4 (8 y + x), so neighbours differ by 4 along a row and by 32 along a column
def image8():
    return ec.ramp()


@pytest.mark.parametrize("offset", [0.25, 0.5, 0.75])
def test_one_triangle_with_a_vertical_edge_between_two_columns(offset):
    """Columns 0..3 are covered, the edge lies at X = 3 + offset.  The pair (column 3, column 4): a = column 3, d = offset.
    offset 0.25: a receives (0.5 - 0.25) (image[4] - image[3]) = 0.25 * 4 = +1.  offset 0.5: d >= 0.5, o receives
    (0.5 - 0.5) (...) = 0.  offset 0.75: o = column 4 receives (0.75 - 0.5) (image[3] - image[4]) = -1."""
    sc, img = ec.vertical_edge(offset), image8()
    face, zbuf = edge.face_map(sc.v, sc.tri, sc.size)
    assert (face[0, :, :4] == 0).all() and (face[0, :, 4:] == -1).all()
    want = img.clone()
    if offset == 0.25:
        want[0, 0, :, 3] += 1.0
    if offset == 0.75:
        want[0, 0, :, 4] -= 1.0
    out = edge.antialias(img, sc.v, sc.tri, face, zbuf)
    assert torch.equal(out, want)
    # the coverage: the hard cover is 1 | 0 across the pair, so the receiver gets -/+ its weight
    alpha = edge.coverage(sc.v, sc.tri, sc.size)
    hard = (face >= 0).float()
    if offset == 0.25:
        hard[0, :, 3] = 0.75
    if offset == 0.75:
        hard[0, :, 4] = 0.25
    assert torch.equal(alpha, hard)


def test_the_diagonal_of_a_quad_is_no_silhouette():
    """The square [1.25, 6.25]^2 in two triangles.  Its outline blends: the row above (Y = 1, d = 0.75) receives
    0.25 * 32 = 8, the bottom row of face 1 (Y = 6, d = 0.25) receives 8, the column left of it (X = 1) receives 0.25 * 4 = 1
    and its last column (X = 6) receives 1.  The pixels on either side of the diagonal keep the image's bits."""
    sc, img = ec.quad(), image8()
    face, zbuf = edge.face_map(sc.v, sc.tri, sc.size)
    inner = face[0, 2:7, 2:7]
    assert (inner >= 0).all() and int((inner == 0).sum()) > 5 and int((inner == 1).sum()) > 5
    out = edge.antialias(img, sc.v, sc.tri, face, zbuf)
    assert torch.equal(out[0, 0, 2:6, 2:6], img[0, 0, 2:6, 2:6])
    diff = (out - img)[0, 0]
    assert diff[1, 2:7].tolist() == [8.0] * 5                                    # above the top edge: o receives
    assert diff[3:7, 1].tolist() == [1.0] * 4                                    # left of face 1's vertical edge
    assert diff[2:6, 6].tolist() == [1.0] * 4                                    # face 0's last column: a receives
    assert diff[6, 2:6].tolist() == [8.0] * 4                                    # face 1's bottom row: a receives
    assert float(diff[0].abs().max()) == 0 and float(diff[7].abs().max()) == 0


def test_two_triangles_at_different_depth_blend_inside_the_cover():
    """A far face over the whole picture and a near one left of X = 3.25: every pixel is covered, the pair (3, 4) shows
    two faces, the nearer one (column 3) is the foreground and its edge decides: column 3 receives 0.25 * 4 = +1."""
    sc, img = ec.overlap(), image8()
    face, zbuf = edge.face_map(sc.v, sc.tri, sc.size)
    assert (face[0, :, :4] == 1).all() and (face[0, :, 4:] == 0).all() and bool((zbuf[0, :, 3] > zbuf[0, :, 4]).all())
    want = img.clone()
    want[0, 0, :, 3] += 1.0
    assert torch.equal(edge.antialias(img, sc.v, sc.tri, face, zbuf), want)
    assert torch.equal(edge.coverage(sc.v, sc.tri, sc.size), torch.ones(1, 8, 8))        # 1 blended with 1


def test_a_folded_neighbour_makes_the_edge_a_silhouette():
    img = image8()
    folded, flat = ec.fold(True), ec.fold(False)
    assert edge.adjacency(folded.tri, 4).tolist() == edge.adjacency(flat.tri, 4).tolist()
    assert int((edge.adjacency(folded.tri, 4) >= 0).sum()) == 2                   # the shared edge, seen from both faces
    want = img.clone()
    want[0, 0, :, 3] += 1.0                                                       # as the single triangle at offset 0.25
    assert torch.equal(edge.antialias(img, folded.v, folded.tri), want)
    # unfolded, the second face continues the surface: two faces across the pair, but no silhouette
    face, _ = edge.face_map(flat.v, flat.tri, flat.size)
    assert (face[0, :, :4] == 0).all() and (face[0, :, 4:] == 1).all()
    assert torch.equal(edge.antialias(img, flat.v, flat.tri), img)


def test_an_edge_that_ends_on_a_centre_line():
    """The vertical edge X = 3.25 ends at Y = 4 exactly: in row 4 its s are (0, 7), neither is below 0, so it does not
    cross; the upper edge, which ends in the same vertex with s = (-14, 0), does, at c = 3.25 exactly (t = 1 or t = 0).
    Row 4's pair (3, 4) therefore has d = 0.25 as rows 5..7 have, through another edge.  Rows 5..7: column 3 receives
    0.25 * 4 = +1.  In row 4 column 3 also receives from the pair with the empty pixel above it, so there the pair is
    read from the analysis: an edge, k the upper edge's, d = 0.25 and w = 0.25 exactly."""
    sc, img = ec.through_centre(), image8()
    face, zbuf = edge.face_map(sc.v, sc.tri, sc.size)
    assert (face[0, 4:, 3] == 0).all() and (face[0, 4:, 4] == -1).all() and (face[0, 3, 2:] == -1).all()
    diff = (edge.antialias(img, sc.v, sc.tri, face, zbuf) - img)[0, 0]
    assert diff[5:, 3].tolist() == [1.0] * 3 and float(diff[4:, 4:].abs().max()) == 0
    P = edge.pixel_coordinates(sc.v, sc.size)
    r = edge.analyse(P, sc.tri, edge.adjacency(sc.tri, 3), face, zbuf, True)
    X = P[0, sc.tri[0], 0]
    vertical = [k for k in range(3) if float(X[k]) == 3.25 and float(X[(k + 1) % 3]) == 3.25]
    assert len(vertical) == 1
    assert r["hit"][0, 4:, 3].all() and r["d"][0, 4:, 3].tolist() == [0.25] * 4 and r["w"][0, 4:, 3].tolist() == [0.25] * 4
    assert int(r["k"][0, 4, 3]) != vertical[0] and r["k"][0, 5:, 3].tolist() == vertical * 3


def test_a_tie_in_z_takes_the_left_pixel():
    """Face 0 left of X = 3.25 and face 1 right of X = 3.75 at the same depth: the foreground of the pair (3, 4) is p =
    column 3, its edge at d = 0.25 lets column 3 receive +1; with q in front column 4 would receive instead."""
    sc, img = ec.z_tie(), image8()
    face, zbuf = edge.face_map(sc.v, sc.tri, sc.size)
    assert torch.equal(zbuf[0, :, 3], zbuf[0, :, 4]) and (face[0, :, 3] == 0).all() and (face[0, :, 4] == 1).all()
    want = img.clone()
    want[0, 0, :, 3] += 1.0
    assert torch.equal(edge.antialias(img, sc.v, sc.tri, face, zbuf), want)
    nearer = zbuf.clone()
    nearer[0, :, 4] += 1.0
    other = img.clone()
    other[0, 0, :, 4] -= 1.0
    assert torch.equal(edge.antialias(img, sc.v, sc.tri, face, nearer), other)


# ---- degenerate inputs and shapes ----------------------------------------------------------------------------------------
def test_nothing_and_everything_covered_return_the_image():
    sc = ec.vertical_edge(0.25)
    img = torch.from_numpy(synth.det_normal((1, 3, 8, 8), 3))
    img[0, 0, 0, 0] = -0.0
    off = sc.v + torch.tensor([0.0, 5.0, 0.0])
    out = edge.antialias(img, off, sc.tri)
    assert int(edge.face_map(off, sc.tri, 8)[0].max()) == -1 and torch.equal(out.view(torch.int32), img.view(torch.int32))
    full = ec._soup([((-40.0, -20.0, -0.5), (40.0, -20.0, -0.5), (4.0, 60.0, -0.5))])
    assert int(edge.face_map(full.v, full.tri, 8)[0].min()) == 0
    out = edge.antialias(img, full.v, full.tri)
    assert torch.equal(out.view(torch.int32), img.view(torch.int32))


def test_nan_and_far_vertices():
    v, tri = ec.ellipsoid(4, 6)
    img = torch.from_numpy(synth.det_normal((1, 2, 16, 16), 4))
    face, zbuf = edge.face_map(v, tri, 16)
    base = edge.antialias(img, v, tri, face, zbuf)
    assert int((base != img).sum()) > 8
    for value in (float("nan"), 1e6, -1e6):
        for vertex in range(0, v.shape[1], 3):
            w = v.clone()
            w[0, vertex, :2] = value
            w.requires_grad_(True)
            out = edge.antialias(img, w, tri, face, zbuf)                        # (the face map of the sound mesh)
            assert bool(torch.isfinite(out).all())
            gv, = torch.autograd.grad(out.sum() + (out * out).sum(), w)
            assert bool(torch.isfinite(gv).all())
            if value != value:
                # a NaN corner switches off the pairs whose foreground face holds it; no other pair changes
                uses = (tri == vertex).any(1)
                own = uses[face.clamp_min(0).long()] & (face >= 0)
                near = own.clone()
                near[:, :, 1:] |= own[:, :, :-1]
                near[:, :, :-1] |= own[:, :, 1:]
                near[:, 1:] |= own[:, :-1]
                near[:, :-1] |= own[:, 1:]
                assert torch.equal(torch.where(near.unsqueeze(1), base, out), base)
    w = v.clone()
    w[0, :, 0] = float("nan")
    assert torch.equal(edge.antialias(img, w, tri, face, zbuf), img)


@pytest.mark.parametrize("size,b,c", [((5, 7), 3, 1), ((16, 12), 3, 4), ((16, 16), 1, 3)])
def test_shapes_batches_and_channels(size, b, c):
    v, tri = ec.ellipsoid(4, 6, b=b)
    img = torch.from_numpy(synth.det_normal((b, c) + size, 6))
    out = edge.antialias(img, v, tri)
    assert tuple(out.shape) == (b, c) + size and int((out != img).sum()) > 0
    face, zbuf = edge.face_map(v, tri, size)
    assert tuple(face.shape) == (b,) + size and face.dtype == torch.int32
    assert torch.equal(zbuf, texture.depth_buffer(v, tri, size))
    assert torch.equal(face >= 0, zbuf > -3e38)
    for r in range(b):
        # every row on its own gives the same bits, and every channel is blended by the same weights
        one = edge.antialias(img[r:r + 1], v[r:r + 1], tri)
        assert torch.equal(one, out[r:r + 1])
        for ch in range(c):
            assert torch.equal(edge.antialias(img[r:r + 1, ch:ch + 1], v[r:r + 1], tri), one[:, ch:ch + 1])
    if b > 1:
        assert not torch.equal(face[0], face[1])


# ---- gradients -----------------------------------------------------------------------------------------------------------
def test_gradcheck_on_the_ellipsoid():
    v, tri = ec.ellipsoid(10, 12)
    size = (16, 16)
    face, zbuf = edge.face_map(v, tri, size)
    opp = edge.adjacency(tri, int(v.shape[1]))
    vd = v.double()
    P = edge.pixel_coordinates(vd, size)
    active = hits = 0
    margin = 1.0
    for horiz in (True, False):
        r = edge.analyse(P, tri, opp, face, zbuf.double(), horiz)
        fp, fq = (face[:, :, :-1], face[:, :, 1:]) if horiz else (face[:, :-1], face[:, 1:])
        active += int((fp != fq).sum())
        hit = r["hit"]
        hits += int(hit.sum())
        d = r["d"][hit]
        margin = min(margin, float((d - 0.5).abs().min()), float(d.min()), float((1 - d).min()),
                     float(r["si"][hit].abs().min()), float(r["sj"][hit].abs().min()))
    print("gradcheck: %d active pairs, %d with an edge, margin %.4f" % (active, hits, margin))
    assert active >= 20 and hits >= 8 and margin > 1e-3
    img = torch.from_numpy(synth.det_normal((1, 2, 16, 16), 9)).double()

    def f(im, vv):
        return edge.antialias(im, vv, tri, face, zbuf.double(), opp)

    assert torch.autograd.gradcheck(f, (img.requires_grad_(True), vd.clone().requires_grad_(True)), eps=1e-6, atol=1e-6,
                                    rtol=1e-4)
    # z gets exactly 0, in either float type
    for dt in (torch.float32, torch.float64):
        w = v.to(dt).requires_grad_(True)
        out = edge.antialias(img.detach().to(dt), w, tri, face, zbuf.to(dt), opp)
        gv, = torch.autograd.grad((out * out).sum(), w)
        assert float(gv[..., 2].abs().max()) == 0.0 and float(gv[..., :2].abs().max()) > 0


def test_float32_gradient_within_the_summation_bound_of_float64():
    """The host float32 definition sums in the kernel's order; against the float64 terms it stays within the float32
    summation bound (n + 8) 2^-24 sum |t| per corner coordinate, n the number of its terms, plus the error the float32
    terms themselves carry from the pixel coordinates (their absolute error 2^-24 max|X| enters s and den relatively)."""
    v, tri = ec.ellipsoid(4, 6, b=2)
    size = (24, 24)
    img = torch.from_numpy(synth.det_normal((2, 3) + size, 12))
    g = torch.from_numpy(synth.det_normal((2, 3) + size, 13))
    face, zbuf = edge.face_map(v, tri, size)
    opp = edge.adjacency(tri, int(v.shape[1]))
    nf = int(tri.shape[0])
    got = edge._backward_corners(g, img, edge.pixel_coordinates(v, size), tri, opp, face, zbuf).view(2, nf, 3, 3)
    bi, F, k, _, _, vals = edge.corner_terms(g.double(), img.double(), edge.pixel_coordinates(v.double(), size), tri, opp, face,
                                             zbuf.double())
    exact = torch.zeros(2, nf, 3, 2, dtype=torch.float64)
    mass = torch.zeros(2, nf, 3, 2, dtype=torch.float64)
    count = torch.zeros(2, nf, 3, 2, dtype=torch.float64)
    for corner, cols in (((k), slice(0, 2)), (((k + 1) % 3), slice(2, 4))):
        exact.index_put_((bi, F, corner), vals[:, cols], accumulate=True)
        mass.index_put_((bi, F, corner), vals[:, cols].abs(), accumulate=True)
        count.index_put_((bi, F, corner), torch.ones_like(vals[:, cols]), accumulate=True)
    u = 2.0 ** -24
    # a term is gd (C products and sums) times a ratio of differences of pixel coordinates: each coordinate carries
    # 3 u |X| <= 3 u 24 absolute, the differences here exceed 1e-3 (asserted by the margin of the terms' d and s below)
    bound = (count + 8) * u * mass + 64 * 24 * u * mass
    err = (got[..., :2].double() - exact).abs()
    print("corner gradient: max error %.3g, bound there %.3g, terms up to %d per sum"
          % (float(err.max()), float(bound.flatten()[err.argmax()]), int(count.max())))
    assert int(count.max()) >= 4 and bool((err <= bound).all())
    assert float(got[..., 2].abs().max()) == 0.0


# ---- rigid shifts ----------------------------------------------------------------------------------------------------------
def test_a_rigid_shift_moves_the_coverage_smoothly():
    """The disc shifted by 0.1 .. 0.9 pixel: a rigid shift keeps the area, so sum(alpha) has no reason to move; what
    moves is where the coverage lies.  Its first moment sum(alpha X) / sum(alpha) moves monotonically; and the hard cover's gradient to v is exactly 0, the antialiased coverage's is not: the property
    the node adds."""
    size = (24, 24)
    xs = torch.arange(24, dtype=torch.float64).view(1, 1, 24)
    soft, hard, total = [], [], []
    for k in range(0, 10):
        v, tri = ec.facing_disc(size, shift=(0.1 * k, 0.0))
        alpha = edge.coverage(v, tri, size).double()
        cover = (edge.face_map(v, tri, size)[0] >= 0).double()
        soft.append(float((alpha * xs).sum() / alpha.sum()))
        hard.append(float((cover * xs).sum() / cover.sum()))
        total.append(float(alpha.sum()))
    print("centroid, antialiased:", np.round(soft, 3), "hard:", np.round(hard, 3), "sum(alpha):", np.round(total, 2))
    steps = np.diff(soft)
    assert (steps > 0).all() and abs(soft[-1] - soft[0] - 0.9) < 0.15
    v, tri = ec.facing_disc(size, shift=(0.3, 0.2))
    w = v.clone().requires_grad_(True)
    face, zbuf = edge.face_map(w, tri, size)
    assert not face.requires_grad and not zbuf.requires_grad
    # the hard cover is a step function of v: it comes without a graph (as texture.uv_map's cover does), so whatever is
    # computed from it has the gradient 0 to v, exactly
    hard = (face >= 0).float()
    gh, = torch.autograd.grad((hard * xs.float()).sum() + 0.0 * w.sum(), w)
    assert not hard.requires_grad and float(gh.abs().max()) == 0.0
    gs, = torch.autograd.grad((edge.coverage(w, tri, size) * xs.float()).sum(), w)
    assert float(gs[..., 0].abs().max()) > 0 and float(gs[..., 0].sum()) > 0    # moving right moves the moment right


def planted_translation(steps, size=(24, 24), lr=0.008):
    v0, tri = ec.facing_disc(size)
    off = torch.tensor([1.2, -0.9])                                              # pixels, |off| = 1.5
    mask = edge.coverage(v0 + torch.tensor([2 * 1.2 / size[1], 2 * 0.9 / size[0], 0.0]), tri, size).detach()
    target = torch.zeros((1, 3) + size)
    term = fit_parts.Silhouette(tri, target, mask, 1.0, "cpu")
    t = torch.zeros(2, requires_grad=True)
    opt = torch.optim.Adam([t], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = term(v0 + torch.cat((t, torch.zeros(1)))).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    px = torch.stack((t[0] * size[1] / 2, -t[1] * size[0] / 2)).detach()
    return losses, float((px - off).norm())


def test_planted_scene_the_silhouette_term_pulls_a_translation_back():
    """The mask is the disc's coverage 1.5 pixels away; Adam on the translation alone, the silhouette term alone.  The
    composite was measured at 60 steps before the count was fixed: final offset 0.090 px (profiles/edge_notes.md)."""
    losses, offset = planted_translation(60)
    print("planted: loss %.5f -> %.5f, offset 1.5 -> %.3f px" % (losses[0], losses[-1], offset))
    assert offset < 0.75 and losses[-1] < losses[0]


# ---- the terms and the inverter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_n", [1, 2])
def test_silhouette_rows_equal_the_formula(b_n):
    v0, tri0 = synth.uv_ellipsoid(4, 6)
    tri = torch.from_numpy(tri0)
    v = torch.from_numpy(synth.random_poses(v0, b_n, seed=3)).double()
    size, weight = (12, 16), 0.7
    mask = torch.from_numpy(synth.det_uniform((b_n,) + size, 5)).double() * 0.5 + 0.5
    term = fit_parts.Silhouette(tri, torch.zeros((b_n, 3) + size), mask, weight, "cpu")
    term.mask = term.mask.double()
    term.set(mask.unsqueeze(1))                                                  # [B, 1, H, W] as well
    rows = term(v)
    alpha = edge.coverage(v, tri, size).numpy()
    want = np.array([weight * ((alpha[b] - mask.numpy()[b]) ** 2).sum() / (size[0] * size[1]) for b in range(b_n)])
    np.testing.assert_allclose(rows.numpy(), want, rtol=1e-12, atol=0)
    assert torch.equal(term.coverage_fit, torch.from_numpy(alpha)) and 0 < alpha.sum() < alpha.size
    with pytest.raises(ValueError):
        term.set(torch.zeros((b_n, 3) + size))
    with pytest.raises(ValueError):
        term.set(mask + 1.0)


@pytest.mark.parametrize("with_mask", [False, True])
def test_photo_edges_rows_equal_the_formula(with_mask):
    from test_photometric_cpu import scene

    v0, tri, uv, tri_uv, keep = scene()
    size, t_size, c_n, weight, b_n = 12, 8, 3, 0.7, 2
    v = torch.from_numpy(synth.random_poses(v0, b_n, seed=3)).double()
    target = torch.from_numpy(synth.det_uniform((b_n, c_n, size, size), 11)).double()
    mask = (torch.from_numpy(synth.det_uniform((b_n, 1, size, size), 12)).double() * 0.5 + 0.5) if with_mask else None
    term = fit_parts.Photometric((uv, tri_uv, keep), tri, target, t_size, weight, False, "cpu", edges=True)
    tex = torch.from_numpy(synth.det_uniform((b_n, c_n, t_size, t_size), 15)).double()
    term.texture = tex.clone().requires_grad_(True)
    rows = term(v, target, mask)
    render, cover = texture.render(v, tri, uv, tri_uv, tex, size, 0.0, keep)
    c = torch.where(cover.unsqueeze(1), render, target)
    aa = edge.antialias(c, v, tri).numpy()
    m = mask.numpy() if with_mask else np.ones((b_n, 1, size, size))
    want = np.array([weight * (m[b] * (aa[b] - target.numpy()[b]) ** 2).sum() / (c_n * size * size) for b in range(b_n)])
    np.testing.assert_allclose(rows.detach().numpy(), want, rtol=1e-12, atol=0)
    # an uncovered pixel that no edge touched differs from the picture by exactly 0; the outline takes part
    untouched = torch.from_numpy(aa) == c
    assert bool(((torch.from_numpy(aa) - target)[(~cover).unsqueeze(1).expand_as(c) & untouched] == 0).all())
    assert int((~untouched).sum()) > 0
    gv, = torch.autograd.grad(rows.sum(), term.texture)
    assert float(gv.abs().max()) > 0


def test_without_the_new_arguments_the_iteration_is_untouched(one_thread):
    a, _, _ = planted(False, lr=0.05, pose_lr=0.02)
    sil = torch.from_numpy(synth.det_uniform((1, 16, 16), 31)) * 0.5 + 0.5
    b, _, _ = planted(False, lr=0.05, pose_lr=0.02, silhouette=sil, silhouette_weight=0.0)
    assert a.sil is None and not a.with_silhouette and a.coverage_fit is None and b.with_silhouette
    ha = a.run(5)
    plain = (ha.clone(), a.w.detach().clone(), a.pose.detach().clone())
    # an inverter built as today gives what it gave: the same five steps from a second plain inverter, bit for bit
    c, _, _ = planted(False, lr=0.05, pose_lr=0.02)
    hc = c.run(5)
    assert torch.equal(hc, plain[0]) and torch.equal(c.w.detach(), plain[1]) and torch.equal(c.pose.detach(), plain[2])
    # with the term at weight 0 the mesh path runs and adds exactly 0
    hb = b.run(5)
    assert torch.equal(hb, plain[0]) and torch.equal(b.w.detach(), plain[1])
    assert tuple(b.coverage_fit.shape) == (1, 16, 16)
    with pytest.raises(ValueError):
        a.reset(a.target, silhouette=sil)
    with pytest.raises(ValueError):
        b.reset(b.target)
    with pytest.raises(ValueError):
        planted(False, photo_edges=True)


def test_the_silhouette_term_in_the_inverter_and_reset(one_thread):
    sil = torch.from_numpy(synth.det_uniform((1, 1, 16, 16), 31)) * 0.5 + 0.5
    inv, _, _ = planted(False, lr=0.05, pose_lr=0.02, silhouette=sil, silhouette_weight=2.0)
    h = inv.run(4)
    # the last step's value holds the term of that step's forward: the numpy float64 formula on the kept coverage
    alpha = inv.coverage_fit.double().numpy()
    want = 2.0 * ((alpha[0] - sil[0, 0].double().numpy()) ** 2).sum() / 256.0
    np.testing.assert_allclose(float(inv.sil.rows.detach()), want, rtol=1e-5)
    other, _, _ = planted(False, lr=0.05, pose_lr=0.02)
    assert not torch.equal(other.run(4), h)                                       # the term is in the loss
    moved = inv.pose.detach().clone()
    # re-targeted in place: a fresh inverter on the new silhouette gives the same steps
    sil2 = torch.from_numpy(synth.det_uniform((1, 16, 16), 32)) * 0.5 + 0.5
    inv.reset(inv.target, silhouette=sil2)
    assert torch.equal(inv.sil.mask, sil2)
    again = inv.run(4)
    fresh, _, _ = planted(False, lr=0.05, pose_lr=0.02, silhouette=sil2, silhouette_weight=2.0)
    assert torch.equal(fresh.run(4), again) and torch.equal(fresh.pose.detach(), inv.pose.detach())
    assert not torch.equal(moved, inv.pose.detach())


def test_photo_edges_in_the_inverter(one_thread):
    inv, _, tex = planted(True, lr=0.01, pose_lr=0.01, photo_lr=0.01, photo_edges=True)
    ref, _, _ = planted(True, lr=0.01, pose_lr=0.01, photo_lr=0.01)
    assert inv.photo.edges and not ref.photo.edges
    inv.set_texture(tex)
    ref.set_texture(tex)
    assert torch.equal(inv.run(3), ref.run(3))                                     # the plain iteration: no term at all
    ha, hb = inv.run(3, photometric=True), ref.run(3, photometric=True)
    assert np.isfinite(ha.numpy()).all() and not torch.equal(ha, hb)
    # batch of two: the rows are added where the landmark rows are
    assert tuple(inv.photo.rows.shape) == (1,)


# ---- the tool --------------------------------------------------------------------------------------------------------------
def silhouette_dir(tmp_path, size=16, stems=("face_b", "face_c")):
    d = tmp_path / "sil"
    d.mkdir(exist_ok=True)
    yy, xx = np.mgrid[0:size, 0:size]
    for k, stem in enumerate(stems):
        disc = ((xx - size / 2 + k) ** 2 + (yy - size / 2) ** 2 < (0.3 * size) ** 2).astype(np.float32)
        np.save(str(d / (stem + ".npy")), disc)
    return str(d)


def check_tool_outputs(out, stems, steps=3):
    for stem in stems:
        r = np.load(os.path.join(out, stem + ".npz"))
        assert r["loss"].shape == (steps,) and np.isfinite(r["loss"]).all()
        assert np.isfinite(r["silhouette_loss"]) and float(r["silhouette_loss"]) >= 0
        assert 0.0 <= float(r["silhouette_iou"]) <= 1.0
        assert os.path.isfile(os.path.join(out, stem + "_coverage.png"))


def test_reconstruct_with_a_silhouette_writes_its_entries_and_without_it_nothing_changes(tmp_path):
    d = silhouette_dir(tmp_path)
    res, out = run_tool(tmp_path, "sil", ["--silhouette_dir", d, "--silhouette_weight", "2"])
    assert res.returncode == 0, res.stderr[-3000:]
    check_tool_outputs(out, ["face_b"])
    plain, out_a = run_tool(tmp_path, "plain", [])
    assert plain.returncode == 0, plain.stderr[-2000:]
    a = np.load(os.path.join(out_a, "face_b.npz"))
    assert not any(k.startswith("silhouette") for k in a.files)
    assert not os.path.exists(os.path.join(out_a, "face_b_coverage.png"))
    # a run that cannot import the new code gives the same arrays
    guard = tmp_path / "guard"
    guard.mkdir()
    (guard / "sitecustomize.py").write_text(
        "import stylerenderer_amd.fit_parts as f, stylerenderer_amd.op.edge as e\n"
        "def _no(*a, **k):\n    raise RuntimeError('the new code ran without its flags')\n"
        "f.Silhouette = _no\ne.antialias = _no\ne.face_map = _no\ne.adjacency = _no\ne.coverage = _no\n")
    other, out_b = run_tool(tmp_path, "guarded", [], {"PYTHONPATH": str(guard) + os.pathsep + ROOT})
    assert other.returncode == 0, other.stderr[-2000:]
    b = np.load(os.path.join(out_b, "face_b.npz"))
    assert sorted(os.listdir(out_a)) == sorted(os.listdir(out_b)) and sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    bad, _ = run_tool(tmp_path, "bad", ["--silhouette_weight", "2"])
    assert bad.returncode != 0 and "--silhouette_dir" in bad.stderr
    bad, _ = run_tool(tmp_path, "bad2", ["--photo_edges"])
    assert bad.returncode != 0 and "--photo" in bad.stderr


def test_reconstruct_silhouette_in_a_batch_with_photo_edges(tmp_path):
    d = silhouette_dir(tmp_path)
    res, out = run_tool(tmp_path, "both", ["--silhouette_dir", d, "--batch", "2", "--photo", "--photo_steps", "2",
                                           "--photo_edges"], images=2)
    assert res.returncode == 0, res.stderr[-3000:]
    check_tool_outputs(out, ["face_b", "face_c"])
    r = np.load(os.path.join(out, "face_c.npz"))
    assert r["photo_loss"].shape == (2,) and np.isfinite(r["photo_loss"]).all()


def test_render_antialias_is_the_node_after_the_sampler():
    from test_photometric_cpu import scene

    v0, tri, uv, tri_uv, keep = scene()
    v = torch.from_numpy(synth.random_poses(v0, 2, seed=3)).float()
    tex = torch.from_numpy(synth.det_uniform((1, 3, 8, 8), 15))
    plain, cover = texture.render(v, tri, uv, tri_uv, tex, 12, -1.0, keep)
    again, _ = texture.render(v, tri, uv, tri_uv, tex, 12, -1.0, keep, antialias=False)
    aa, cover_aa = texture.render(v, tri, uv, tri_uv, tex, 12, -1.0, keep, antialias=True)
    assert torch.equal(plain, again) and torch.equal(cover, cover_aa)
    assert torch.equal(aa, edge.antialias(plain, v, tri)) and not torch.equal(aa, plain)
