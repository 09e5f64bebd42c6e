"""CPU: op.light — the composites of shade / unshade / texel_attribute against literal per-pixel loops bit for bit, the
gradient checks, the kinks and exclusions, the closed-form fit against numpy's least squares, the round trip, and a planted
scene: bake -> fit -> unshade brings the texture nearer to the planted albedo than the plain bake is."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import synth
from stylerenderer_amd.op import light, texture
from test_texture_cpu import _env, ordinary_case, scene_batch

NP = {torch.float32: np.float32, torch.float64: np.float64}


# ---- the literal loops -------------------------------------------------------------------------------------------------
def pixel_basis(n, t):
    """(Y[9], (x, y, z), r, len) of one normal, every step one operation of type t."""
    nx, ny, nz = (t(c) for c in n)
    r = np.sqrt((nx * nx + ny * ny) + nz * nz)
    length = r if r > t(light.TINY) else t(light.TINY)
    x, y, z = nx / length, ny / length, nz / length
    return [t(1), x, y, z, x * y, x * z, y * z, x * x - y * y, t(3) * (z * z) - t(1)], (x, y, z), r, length


def pixel_shading(ys, gam):
    s = gam[0] + gam[1] * ys[1]
    for k in range(2, 9):
        s = s + gam[k] * ys[k]
    return s


def loops(a, normals, on, gamma, g, black, background, floor):
    """out, unshaded, ga, gn and the terms [B, Cl, 9, H, W] of ggamma, pixel by pixel in numpy scalars of a's type."""
    t = NP[a.dtype]
    a_, n_, on_, gam_, g_ = (x.numpy() for x in (a, normals, on, gamma, g))
    b_n, c_n, h, w = a_.shape
    cl = gam_.shape[1]
    black, background, floor = t(black), t(background), t(floor)
    out, un, ga = np.zeros_like(a_), np.zeros_like(a_), np.zeros_like(a_)
    gn = np.zeros_like(n_)
    terms = np.zeros((b_n, cl, 9, h, w), a_.dtype)
    with np.errstate(all="ignore"):
        for b in range(b_n):
            for y in range(h):
                for x in range(w):
                    n = n_[b, :, y, x]
                    if not (on_[b, y, x] and np.isfinite(n).all()):
                        out[b, :, y, x] = background
                        un[b, :, y, x] = a_[b, :, y, x]
                        continue
                    ys, (nx, ny, nz), r, length = pixel_basis(n, t)
                    s = [pixel_shading(ys, gam_[b, l]) for l in range(cl)]
                    e = [t(0)] * cl
                    for c in range(c_n):
                        l = c if cl > 1 else 0
                        sp = s[l] if s[l] > 0 else t(0)
                        m = s[l] if s[l] > floor else floor
                        d = a_[b, c, y, x] - black
                        out[b, c, y, x] = d * sp + black
                        un[b, c, y, x] = d / m + black
                        ga[b, c, y, x] = g_[b, c, y, x] * sp
                        e[l] = e[l] + g_[b, c, y, x] * d
                    e = [e[l] if s[l] > 0 else t(0) for l in range(cl)]
                    for l in range(cl):
                        terms[b, l, 0, y, x] = e[l]
                        for k in range(1, 9):
                            terms[b, l, k, y, x] = e[l] * ys[k]
                    gy_ = [None]
                    for k in range(1, 9):
                        acc = t(0)
                        for l in range(cl):
                            acc = acc + e[l] * gam_[b, l, k]
                        gy_.append(acc)
                    gx = ((gy_[1] + gy_[4] * ny) + gy_[5] * nz) + (t(2) * gy_[7]) * nx
                    gy = ((gy_[2] + gy_[4] * nx) + gy_[6] * nz) - (t(2) * gy_[7]) * ny
                    gz = ((gy_[3] + gy_[5] * nx) + gy_[6] * ny) + (t(6) * gy_[8]) * nz
                    d = (nx * gx + ny * gy) + nz * gz
                    if not r < t(light.TINY):
                        gn[b, :, y, x] = [(gx - nx * d) / length, (gy - ny * d) / length, (gz - nz * d) / length]
    return out, un, ga, gn, terms


def bits(x):
    x = x.detach().cpu().contiguous() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def planted_case(b_n, c_n, h, w, cl, dtype=torch.float32, seed=0):
    """(a, normals, on, gamma, g, counts) on the host.  Planted where the picture has room: a pixel with s <= 0 (its normal
    points away from a light that is made directional enough), a zero normal, a NaN and an infinite normal, and an
    `on = False` pixel; counts names how many of each there are."""
    a = torch.from_numpy(synth.det_uniform((b_n, c_n, h, w), 300 + seed)).to(dtype)
    normals = torch.from_numpy(synth.det_normal((b_n, 3, h, w), 301 + seed)).to(dtype)
    g = torch.from_numpy(synth.det_normal((b_n, c_n, h, w), 302 + seed)).to(dtype)
    gamma = 0.2 * torch.from_numpy(synth.det_normal((b_n, cl, 9), 303 + seed)).to(dtype)
    gamma[:, :, 0] = 0.7
    gamma[:, :, 3] = 0.9                                                       # mostly from +z
    gamma[:, :, 8] *= 0.25                                                     # (so that -z is dark whatever the draw)
    on = torch.ones((b_n, h, w), dtype=torch.bool)
    counts = dict(dark=0, zero=0, nan=0, inf=0, off=0)
    flat = [(y, x) for y in range(h) for x in range(w)]
    if len(flat) >= 6:
        for b in range(b_n):
            (y0, x0), (y1, x1), (y2, x2), (y3, x3), (y4, x4) = flat[1], flat[len(flat) // 2], flat[-1], flat[2], flat[-2]
            normals[b, :, y0, x0] = torch.tensor([0.0, 0.0, -2.0], dtype=dtype)
            normals[b, :, y1, x1] = 0.0
            normals[b, 1, y2, x2] = float("nan")
            normals[b, 0, y3, x3] = float("inf")
            on[b, y4, x4] = False
            for k in counts:
                counts[k] += 1
    return a, normals, on, gamma, g, counts


def run_composite(a, normals, on, gamma, g, black=-1.0, background=-1.0):
    a, normals, gamma = (x.detach().clone().requires_grad_(True) for x in (a, normals, gamma))
    out = light.shade(a, normals, on, gamma, black, background)
    return (out.detach(),) + torch.autograd.grad(out, (a, normals, gamma), grad_outputs=g)


CASES = [(1, 1, 1, 1), (1, 3, 5, 7), (2, 3, 4, 6)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("shape", CASES)
def test_composites_equal_the_literal_loops(shape, white, dtype):
    b_n, c_n, h, w = shape
    cl = 1 if white else c_n
    a, normals, on, gamma, g, counts = planted_case(b_n, c_n, h, w, cl, dtype)
    black, background, floor = -1.0, 0.25, 0.3
    want_out, want_un, want_ga, want_gn, terms = loops(a, normals, on, gamma, g, black, background, floor)
    out, ga, gn, ggamma = run_composite(a, normals, on, gamma, g, black, background)
    un = light.unshade(a, normals, on, gamma, black, floor)
    assert not un.requires_grad
    for got, want in ((out, want_out), (un, want_un), (ga, want_ga), (gn, want_gn)):
        assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(light.light_terms(a, normals, on, gamma, g, black)), bits(terms))
    # ggamma is the host sum of the loop's terms: against their exact sum, within the bound of a sum of n terms
    t64 = terms.astype(np.float64).reshape(b_n, cl, 9, -1)
    exact = np.array([[[math.fsum(t64[b, l, k]) for k in range(9)] for l in range(cl)] for b in range(b_n)])
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    bound = h * w * u * np.abs(t64).sum(-1)
    assert (np.abs(ggamma.double().numpy() - exact) <= bound).all()
    if h * w >= 6:
        live = on & torch.isfinite(normals).all(1)
        assert int((~on).sum()) == counts["off"] and int((~live).sum()) == counts["off"] + counts["nan"] + counts["inf"]


def test_kinks_and_exclusions():
    a, normals, on, gamma, g, counts = planted_case(2, 3, 5, 7, 1)
    assert counts == dict(dark=2, zero=2, nan=2, inf=2, off=2)
    out, ga, gn, ggamma = run_composite(a, normals, on, gamma, g, -1.0, 0.5)
    live = on & torch.isfinite(normals).all(1)
    ys = light.basis(light._clean(normals, live))[0]
    s = light._shading(ys, gamma)[:, 0]
    dark = live & (s <= 0)
    assert int(dark.sum()) >= counts["dark"] and bool(dark[:, 0, 1].all())
    d3 = dark.unsqueeze(1).expand(-1, 3, -1, -1)
    assert bool((out[d3] == -1.0).all()) and bool((ga[d3] == 0).all()) and bool((gn[d3] == 0).all())
    zero = (normals == 0).all(1)
    assert int(zero.sum()) == counts["zero"]
    z3 = zero.unsqueeze(1).expand(-1, 3, -1, -1)
    assert bool(torch.isfinite(out[z3]).all()) and bool((gn[z3] == 0).all())
    dead = ~live
    assert int(dead.sum()) == counts["nan"] + counts["inf"] + counts["off"]
    k3 = dead.unsqueeze(1).expand(-1, 3, -1, -1)
    assert bool((out[k3] == 0.5).all()) and bool((ga[k3] == 0).all()) and bool((gn[k3] == 0).all())
    assert bool(torch.isfinite(ggamma).all()) and bool(torch.isfinite(gn).all())
    # nothing of the dead pixels reaches the light's gradient: other values there, the same sums
    a2, g2 = a.clone(), g.clone()
    a2[k3], g2[k3] = 123.0, -77.0
    again = run_composite(a2, normals, on, gamma, g2, -1.0, 0.5)
    assert torch.equal(bits(again[3]), bits(ggamma))


def smooth_case(cl, seed=0):
    """float64 inputs away from both kinks: unit-ish normals around +z under a light from +z."""
    a = torch.from_numpy(synth.det_uniform((2, 3, 3, 4), 310 + seed)).double()
    normals = 0.3 * torch.from_numpy(synth.det_normal((2, 3, 3, 4), 311 + seed)).double()
    normals[:, 2] = normals[:, 2].abs() + 1.0
    gamma = 0.1 * torch.from_numpy(synth.det_normal((2, cl, 9), 312 + seed)).double()
    gamma[:, :, 0] = 1.0
    gamma[:, :, 3] = 0.5
    on = torch.ones((2, 3, 4), dtype=torch.bool)
    on[1, 2, 3] = False
    return a, normals, on, gamma


@pytest.mark.parametrize("cl", [1, 3])
def test_gradcheck_and_gradgradcheck_in_float64(cl):
    a, normals, on, gamma = smooth_case(cl)
    s = light._shading(light.basis(normals)[0], gamma)
    r = light.basis(normals)[2]
    assert float(s.min()) > 0.2 and float(r.min()) > 0.5                       # away from s = 0 and from r = TINY
    a, normals, gamma = (x.requires_grad_(True) for x in (a, normals, gamma))

    def f(a_, n_, g_):
        return light.shade(a_, n_, on, g_, -1.0, 0.0)

    assert torch.autograd.gradcheck(f, (a, normals, gamma), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradgradcheck(f, (a, normals, gamma), eps=1e-6, atol=1e-6, rtol=1e-5)


# ---- texel attributes ----------------------------------------------------------------------------------------------------
def attribute_loops(attr, tri, face, coeff):
    t = NP[attr.dtype]
    at, tr, fc, cf = attr.numpy(), tri.numpy(), face.numpy(), coeff.numpy().astype(t)
    b_n, nv, n_a = at.shape
    th, tw = fc.shape
    out = np.zeros((b_n, n_a, th, tw), at.dtype)
    for ty in range(th):
        for tx in range(tw):
            f = fc[ty, tx]
            if f < 0 or f >= tr.shape[0] or (tr[f] < 0).any() or (tr[f] >= nv).any():
                continue
            i0, i1, i2 = tr[f]
            c0, c1, c2 = cf[ty, tx]
            for b in range(b_n):
                for q in range(n_a):
                    out[b, q, ty, tx] = (c0 * at[b, i0, q] + c1 * at[b, i1, q]) + c2 * at[b, i2, q]
    return out


def attribute_case(size, n_a, b_n, dtype=torch.float32):
    """The two-quad scene's map with a per-vertex attribute, one face index planted out of range."""
    shifts = [(0.0, 0.0), (0.5, 0.125), (-0.3, -0.6)][:b_n]
    v, _, tri, uv, tri_uv = scene_batch(shifts, dtype)
    face, coeff = texture.texel_map(uv, tri_uv, size)
    face = face.clone()
    live = torch.nonzero(face >= 0)
    assert live.shape[0] > 2
    ty, tx = (int(x) for x in live[len(live) // 2])
    face[ty, tx] = 1000                                                        # outside the mesh: counts as empty
    attr = torch.from_numpy(synth.det_normal((b_n, v.shape[1], n_a), 320 + n_a)).to(dtype)
    return attr, tri, face, coeff, (ty, tx)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("size,n_a,b_n", [((8, 8), 1, 1), ((8, 8), 3, 3), ((33, 65), 4, 1)])
def test_texel_attribute_equals_the_literal_loops(size, n_a, b_n, dtype):
    attr, tri, face, coeff, (ty, tx) = attribute_case(size, n_a, b_n, dtype)
    got = light.texel_attribute(attr, tri, face, coeff)
    assert tuple(got.shape) == (b_n, n_a) + tuple(size)
    assert torch.equal(bits(got), bits(attribute_loops(attr, tri, face, coeff)))
    assert bool((got[:, :, face < 0] == 0).all()) and bool((got[:, :, ty, tx] == 0).all())
    # a vertex of the mesh carried to its own texels: with the normals (0, 0, 1) everywhere the map gives (0, 0, 1)
    if n_a == 3:
        ones = torch.zeros_like(attr)
        ones[..., 2] = 1.0
        flat = light.texel_attribute(ones, tri, face, coeff)
        live = (face >= 0) & (face < tri.shape[0])
        assert float((flat[:, 2][:, live] - 1).abs().max()) < 1e-5 and bool((flat[:, :2] == 0).all())


def test_normal_map_draws_the_normals():
    v, n, tri, _, _ = scene_batch([(0.0, 0.0)])
    for size in (16, (12, 16)):
        nm = light.normal_map(v, n, tri, size)
        h, w = (size, size) if isinstance(size, int) else size
        assert tuple(nm.shape) == (1, 3, h, w)
        drawn = nm[:, 2] != 0
        assert int(drawn.sum()) > h * w // 4 and bool((nm[:, :2] == 0).all())
        assert float((nm[:, 2][drawn] - 1).abs().max()) < 1e-5


# ---- the fit ---------------------------------------------------------------------------------------------------------
def sphere_cap(n=65):
    """normals [1, 3, n, n] float64 of the unit sphere over a grid on [-1, 1]^2 and the mask z > 0.1."""
    t = torch.linspace(-1, 1, n, dtype=torch.float64)
    y, x = torch.meshgrid(t, t, indexing="ij")
    zz = 1 - x * x - y * y
    z = torch.sqrt(zz.clamp_min(0))
    mask = (zz > 0) & (z > 0.1)
    normals = torch.stack((x, y, torch.where(mask, z, torch.ones_like(z))))[None]
    return normals, mask[None, None]


def design(normals, mask):
    ys = light.basis(normals)[0]
    return torch.stack([y[0][mask[0, 0]] for y in ys], 1).numpy()              # [P, 9]


def test_fit_equals_least_squares_and_recovers_a_planted_light():
    normals, mask = sphere_cap()
    weight = mask.double()
    A = design(normals, mask)
    cond = np.linalg.cond(A.T @ A)
    print("Gram matrix of the nine functions on the cap z > 0.1, 65 x 65: condition number %.4g" % cond)
    assert 1.0e3 < cond < 2.5e3
    planted = torch.tensor([[[0.9, 0.2, -0.15, 0.4, 0.05, -0.1, 0.08, 0.03, -0.06],
                             [0.8, -0.1, 0.1, 0.5, 0.0, 0.1, -0.05, 0.02, 0.04],
                             [1.0, 0.0, 0.2, 0.3, -0.04, 0.0, 0.03, -0.07, 0.02]]], dtype=torch.float64)
    albedo = torch.tensor([-0.2, 0.1, 0.4], dtype=torch.float64).view(1, 3, 1, 1).expand(1, 3, 65, 65).contiguous()
    on = mask[:, 0]
    s = light._shading(light.basis(normals)[0], planted)
    assert float(s[:, :, on[0]].min()) > 0.05
    picture = light.shade(albedo, normals, on, planted, -1.0, -1.0)
    got = light.fit(picture, normals, weight, ridge=0.0).numpy()[0]
    for c in range(3):
        rhs = (picture[0, c][mask[0, 0]] + 1).numpy()
        lsq = np.linalg.lstsq(A, rhs, rcond=None)[0]
        want = lsq / rhs.mean()
        tol = 64 * cond * 2.0 ** -53 * np.abs(want).max()
        print("channel %d: |fit - lstsq| %.3g, tolerance %.3g" % (c, np.abs(got[c] - want).max(), tol))
        assert np.abs(got[c] - want).max() <= tol
        mean_s = float(s[0, c][on[0]].mean())
        assert np.abs(got[c] - planted[0, c].numpy() / mean_s).max() <= 64 * cond * 2.0 ** -53 * np.abs(want).max() + 1e-12
    mono = light.fit(picture, normals, weight, ridge=0.0, mono=True)
    assert tuple(mono.shape) == (1, 1, 9)


def test_fitted_shading_has_weighted_mean_one():
    normals, mask = sphere_cap()
    weight = mask.double() * torch.from_numpy(synth.det_uniform((1, 1, 65, 65), 330)).double().abs()
    noise = 0.2 * torch.from_numpy(synth.det_normal((1, 3, 65, 65), 331)).double()
    planted = torch.tensor([[[0.9, 0.2, -0.15, 0.4, 0.05, -0.1, 0.08, 0.03, -0.06]]], dtype=torch.float64)
    on = mask[:, 0]
    picture = light.shade(noise, normals, on, planted, -1.0, -1.0)
    A = design(normals, mask)
    cond = np.linalg.cond(A.T @ A)
    for mono in (False, True):
        gamma = light.fit(picture, normals, weight, mono=mono, ridge=1e-3)
        s = light._shading(light.basis(normals)[0], gamma)
        for l in range(gamma.shape[1]):
            mean = float((weight[0, 0] * s[0, l]).sum() / weight.sum())
            tol = 64 * cond * 2.0 ** -53 * float(gamma.abs().max())
            print("mono %s light %d: weighted mean shading - 1 = %.3g (tolerance %.3g)" % (mono, l, mean - 1, tol))
            assert abs(mean - 1) <= tol


def test_fit_stays_finite_on_degenerate_input():
    a = torch.from_numpy(synth.det_uniform((1, 3, 6, 6), 332))
    flat = torch.zeros((1, 3, 6, 6))
    flat[:, 2] = 1.0                                                           # equal normals: a system of rank 1
    w = torch.ones((1, 1, 6, 6))
    for ridge in (0.0, 1e-3):
        gamma = light.fit(a, flat, w, ridge=ridge)
        assert tuple(gamma.shape) == (1, 3, 9) and gamma.dtype == a.dtype and bool(torch.isfinite(gamma).all())
    nothing = light.fit(a, flat, torch.zeros_like(w))
    want = torch.zeros((1, 3, 9))
    want[:, :, 0] = 1.0
    assert torch.equal(nothing, want)
    assert torch.equal(light.fit(a, flat, torch.zeros_like(w), mono=True), want[:, :1])


def test_moments_composite_sums_its_terms():
    a, normals, on, _, _, _ = planted_case(2, 3, 5, 7, 1)
    weight = torch.from_numpy(synth.det_uniform((2, 1, 5, 7), 333)) * on.unsqueeze(1)      # some weights not positive
    terms = light.moment_terms(a, normals, weight, -1.0)
    assert tuple(terms.shape) == (2, 45 + 27, 5, 7) and terms.dtype == torch.float64
    got = light.moments(a, normals, weight, -1.0)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 72) and bool(torch.isfinite(got).all())
    used = (weight[:, 0] > 0) & torch.isfinite(normals).all(1)
    assert 0 < int(used.sum()) < used.numel() - 4                              # the planted pixels are left out
    assert bool((terms.permute(0, 2, 3, 1)[~used] == 0).all())
    flat = terms.reshape(2, 72, -1).numpy()
    exact = np.array([[math.fsum(flat[b, i]) for i in range(72)] for b in range(2)])
    assert (np.abs(got.numpy() - exact) <= 35 * 2.0 ** -53 * np.abs(flat).sum(-1)).all()
    # M_00 is the sum of the weights, M_0k = sum w Y_k and R_c[0] = sum w (a_c + 1)
    for b in range(2):
        wsum = math.fsum(weight[b, 0][used[b]].double().tolist())
        assert abs(float(got[b, 0]) - wsum) <= 35 * 2.0 ** -53 * wsum
        d = (a[b, 1] + 1.0)[used[b]].double() * weight[b, 0][used[b]].double()
        assert abs(float(got[b, 45 + 9]) - math.fsum(d.tolist())) <= 35 * 2.0 ** -53 * float(d.abs().sum())


# ---- round trip --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_unshade_inverts_shade(dtype):
    """With d = a - black, s >= floor > 0 and u the unit roundoff, shade computes fl(fl(d s) + black) and unshade
    fl(fl(fl(out - black) / s) + black): four roundings on the way back to d (the product, the first sum, the difference,
    the quotient; d = fl(a - black) itself is the same number both times), each relative to a magnitude of at most
    |d| s + |black| before the division by s, and two more of a's own magnitude for the final sum and the first sum seen
    from a.  So |a' - a| <= u (4 (|d| s + |black|) / s + 2 (|d| + |black|)) to first order; the test allows 1.01 of it."""
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    a, normals, on, gamma, _, _ = planted_case(2, 3, 9, 11, 3, dtype, seed=4)
    floor = 0.05
    live = on & torch.isfinite(normals).all(1)
    s = light._shading(light.basis(light._clean(normals, live))[0], gamma)
    ok = live.unsqueeze(1) & (s >= floor)
    assert int(ok.sum()) > ok.numel() // 2
    back = light.unshade(light.shade(a, normals, on, gamma, -1.0, -1.0), normals, on, gamma, -1.0, floor)
    d = (a + 1).abs().double()
    bound = 1.01 * u * (4 * (d * s.double() + 1) / s.double().clamp_min(floor) + 2 * (d + 1))
    err = (back.double() - a.double()).abs()
    print("%s: largest |unshade(shade(a)) - a| / bound %.3f" % (dtype, float((err / bound)[ok].max())))
    assert bool((err <= bound)[ok].all())


# ---- a planted scene -----------------------------------------------------------------------------------------------------
def planted_scene(device="cpu", tsize=(32, 32), psize=64):
    """A posed ellipsoid with an albedo texture affine in uv under a planted directional light: the picture is
    shade(render(albedo)); then bake -> texel normals -> fit -> unshade.  Returns a dict of everything."""
    args, _, (uv, tri_uv, keep) = ordinary_case(torch.float32, device, size=tsize, batch=1)
    v, n, tri = args["v"], args["n"], args["tri"]
    face, coeff = args["face"], args["coeff"]
    cen = texture.texel_centres(tsize, torch.float32).to(device)
    albedo = torch.stack((-0.4 + 0.5 * cen[..., 0], 0.1 + 0.4 * cen[..., 1], 0.3 - 0.3 * cen[..., 0] + 0.2 * cen[..., 1]))[None]
    gamma = torch.tensor([[[0.75, 0.35, 0.0, 0.45, 0.0, 0.0, 0.0, 0.0, 0.0]]], device=device)
    flat, cover = texture.render(v, tri, uv.to(device), tri_uv.to(device), albedo.contiguous(), psize, -1.0, keep)
    nmap = light.normal_map(v, n, tri, psize)
    picture = light.shade(flat, nmap, cover, gamma, -1.0, -1.0)
    zbuf = texture.depth_buffer(v, tri, psize)
    tex, weight = texture.bake(v, n, tri, face, coeff, picture, zbuf)
    tn = light.texel_attribute(n, tri, face, coeff)
    fitted = light.fit(tex, tn, weight, mono=True)
    clean = light.unshade(tex, tn, weight[:, 0] > 0, fitted)
    return dict(albedo=albedo, tex=tex, weight=weight, normals=tn, planted=gamma, fitted=fitted, clean=clean)


def test_planted_scene_the_delit_texture_is_nearer_to_the_albedo():
    """Measured here: mean |texture - albedo| over the baked texels 0.1252 for the de-lit texture against 0.2384 for the
    plain bake (32 x 32 texels, a 64 x 64 picture).  No ratio is asserted, only the order."""
    sc = planted_scene()
    counted = sc["weight"][0, 0] > 0
    assert int(counted.sum()) > 100
    for gam in (sc["planted"], sc["fitted"]):
        s = light._shading(light.basis(sc["normals"])[0], gam)[0, 0]
        assert float(s[counted].min()) > 0.05                                   # the floor is never reached
    m3 = counted.expand(3, -1, -1)
    lit = float((sc["tex"][0] - sc["albedo"][0]).abs()[m3].mean())
    clean = float((sc["clean"][0] - sc["albedo"][0]).abs()[m3].mean())
    print("planted scene: mean |texture - albedo| de-lit %.4f, plain bake %.4f" % (clean, lit))
    assert clean < lit


# ---- arguments -------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    a, normals, on, gamma, _, _ = planted_case(1, 3, 4, 4, 1)
    with pytest.raises(ValueError):
        light.shade(a, normals[:, :2], on, gamma)
    with pytest.raises(ValueError):
        light.shade(a, normals, on.float(), gamma)
    with pytest.raises(ValueError):
        light.shade(a, normals, on, gamma.expand(-1, 2, -1))
    with pytest.raises(ValueError):
        light.shade(a, normals, on, gamma, ggamma_out=torch.zeros(9))            # the buffer is for the kernels
    with pytest.raises(ValueError):
        light.unshade(a, normals, on, gamma, floor=0.0)
    with pytest.raises(ValueError):
        light.fit(a, normals, torch.ones((1, 1, 4, 4)), ridge=-1.0)
    with pytest.raises(ValueError):
        light.texel_attribute(torch.zeros((1, 4, 5)), torch.zeros((1, 3), dtype=torch.int64),
                              torch.zeros((2, 2), dtype=torch.int32), torch.zeros((2, 2, 3)))
    assert light.partial_rows(16, 256) == 1 and light.partial_rows(17, 256) == 2
    assert light.terms_per_lane(1, 1) == 1 and light.terms_per_lane(16, 256) == 16 and light.terms_per_lane(2, 512) == 4
    assert len(light.D3DFR) == 9 and sorted(light.D3DFR_ORDER) == list(range(9))
    from stylerenderer_amd import _lib

    L = _lib.lib()                                                             # size and NULL checks precede any launch
    assert L.sr_light_shade_fwd(None, None, None, None, None, 1, 3, 2, 4, 4, -1.0, 0.0, -1.0, 0, None) == -1
    assert L.sr_light_shade_fwd(None, None, None, None, None, 0, 3, 1, 4, 4, -1.0, 0.0, -1.0, 0, None) == 0
    assert L.sr_light_shade_bwd(None, None, None, None, None, None, None, None, 1, 5, 5, 4, 4, -1.0, None) == -1
    assert L.sr_light_reduce(None, None, 1, 0, 9, 0, None) == -1
    assert L.sr_light_moments(None, None, None, None, 1, 5, 4, 4, -1.0, None) == -1
    assert L.sr_light_texel_attr(None, None, None, None, None, 1, 5, 4, 2, 4, 4, None) == -1


# ---- command line ----------------------------------------------------------------------------------------------------
LIGHT_FILES = ["face_a_texture_lit.png", "face_a_shading.png", "face_a_relit.png"]
LIGHT_ENTRIES = {"light", "light_fit", "light_residual", "rerender_error_lit"}


def _checkpoint(tmp_path, size):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    return ckpt


def run_light_cli(tmp_path, env, size=16, steps=4, more=(), without=True):
    """`reconstruct --texture 32 --light --texture_check --turntable 2 --texture_refine 3 --relight FILE` on the synthetic
    checkpoint and, with `without`, the same without the light's flags; checks the files and entries (shared with the GPU
    suite)."""
    ckpt = _checkpoint(tmp_path, size)
    img = str(tmp_path / "face_a.npy")
    np.save(img, synth.det_uniform((3, 24, 24), 9))
    other = str(tmp_path / "other.txt")
    np.savetxt(other, np.array([1.0, -0.4, 0.0, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0]))
    base = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", str(size), "--steps", str(steps),
            "--n_mean_latent", "64", "--texture", "32", "--texture_check", "--turntable", "2", "--texture_refine", "3"]
    base += list(more)
    lit, plain = str(tmp_path / "lit"), str(tmp_path / "plain")
    res = subprocess.run(base + ["--light", "--light_floor", "0.1", "--light_ridge", "0.01", "--light_lr", "0.01",
                                 "--relight", other, "--out", lit, ckpt, img],
                         env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    names = sorted(os.listdir(lit))
    assert set(LIGHT_FILES) <= set(names)
    r = np.load(os.path.join(lit, "face_a.npz"))
    assert LIGHT_ENTRIES <= set(r.files)
    assert r["light"].shape == (3, 9) and r["light_fit"].shape == (3, 9) and np.isfinite(r["light"]).all()
    assert np.isfinite(r["light_fit"]).all() and r["light_residual"].shape == () and np.isfinite(r["light_residual"])
    assert r["texture_refine_loss"].shape == (3,) and np.isfinite(r["texture_refine_loss"]).all()
    assert np.isfinite(float(r["rerender_error"])) and np.isfinite(float(r["rerender_error_lit"]))
    from PIL import Image

    for name in LIGHT_FILES[1:] + ["face_a_rerender.png", "face_a_turn_00.png", "face_a_turn_01.png"]:
        pic = Image.open(os.path.join(lit, name))
        assert pic.size == (size, size) and pic.mode == "RGB", name
    assert Image.open(os.path.join(lit, "face_a_texture_lit.png")).size == (32, 32)
    if without:
        res = subprocess.run(base + ["--out", plain, ckpt, img], env=env, cwd=str(tmp_path), capture_output=True,
                             text=True, timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        assert sorted(os.listdir(plain)) == sorted(set(names) - set(LIGHT_FILES))       # none of the new files
        r0 = np.load(os.path.join(plain, "face_a.npz"))
        assert set(r.files) - set(r0.files) == LIGHT_ENTRIES and set(r0.files) <= set(r.files)
    return res, ckpt, img


def run_light_cli_multiview(tmp_path, env, size=16, steps=4, more=()):
    """Two views of one subject with --light --light_mono: every view has its own light, the merged albedo is checked
    under each."""
    ckpt = _checkpoint(tmp_path, size)
    imgs = []
    for k in range(2):
        p = str(tmp_path / ("view_%d.npy" % k))
        np.save(p, synth.det_uniform((16, 16, 3), 140 + k))
        imgs.append(p)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", str(size), "--steps", str(steps),
           "--n_mean_latent", "64", "--multiview", "2", "--subject", "anna", "--texture", "32", "--light", "--light_mono",
           "--texture_check", "--turntable", "2", "--texture_refine", "3", "--out", out, ckpt] + list(more) + imgs
    res = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    names = set(os.listdir(out))
    assert {"anna_merged_turn_00.png", "anna_merged_turn_01.png", "anna_merged_texture.png", "view_0_texture_lit.png",
            "view_1_texture_lit.png", "view_0_shading.png", "view_1_shading.png", "view_0_rerender.png"} <= names
    ident = np.load(os.path.join(out, "anna_identity.npz"))
    assert ident["lights"].shape == (2, 1, 9) and np.isfinite(ident["lights"]).all()
    assert ident["merged_rerender_error"].shape == (2,) and np.isfinite(ident["merged_rerender_error"]).all()
    assert ident["merged_texture_refine_loss"].shape == (3,) and np.isfinite(ident["merged_texture_refine_loss"]).all()
    for k in range(2):
        view = np.load(os.path.join(out, "view_%d.npz" % k))
        assert view["light"].shape == (1, 9) and view["light_fit"].shape == (1, 9)
        assert view["texture_lit"].shape == view["texture"].shape == (3, 32, 32)
        assert np.isfinite(float(view["rerender_error"])) and np.isfinite(float(view["rerender_error_lit"]))
        assert view["texture_refine_loss"].shape == (3,) and np.isfinite(view["texture_refine_loss"]).all()
    return res


def test_reconstruct_cli_with_a_light(tmp_path):
    _, ckpt, img = run_light_cli(tmp_path, _env())
    for flags, word in ((["--light"], "need --texture"), (["--relight", "x.txt"], "need --texture"),
                        (["--texture", "16", "--light_mono"], "need --light"),
                        (["--texture", "16", "--light_floor", "0.1"], "need --light"),
                        (["--texture", "16", "--light", "--light_lr", "0.01"], "needs --texture_refine")):
        bad = subprocess.run([sys.executable, "-m", "stylerenderer_amd.reconstruct"] + flags + [ckpt, img], env=_env(),
                             cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
        assert bad.returncode == 2 and word in bad.stderr, (flags, bad.stderr[-500:])


def test_reconstruct_cli_multiview_with_a_light(tmp_path):
    run_light_cli_multiview(tmp_path, _env())
