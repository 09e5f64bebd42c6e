"""CPU: the mip-mapped texture look-up — the host definitions `mip_build`, `mip_lod`, `mip_sample` of op.texture against
literal per-texel / per-pixel loops (bit for bit, the ordered sum included), their gradients, the level layout, the cases
whose answer is known exactly (a checkerboard's area mean, a chart seam, uncovered neighbours, coordinates out of range),
the argument checks of the C ABI and refinement with the mip look-up."""
import numpy as np
import pytest
import torch

from stylerenderer_amd import synth
from stylerenderer_amd.op import texture
from test_texture_sample_cpu import ABC, affine_texture, random_case, two_views


# ---- the definitions, as loops ---------------------------------------------------------------------------------------
def build_loops(tex, layout, gpyr):
    """(pyr, grad_tex) of numpy arrays: level by level and texel by texel, every step one operation of tex's type."""
    ft = tex.dtype.type
    bt, c_n, th, tw = tex.shape
    p = layout[-1][0] + layout[-1][1] * layout[-1][2]
    pyr = np.zeros((bt, c_n, p), tex.dtype)
    gtex = np.zeros_like(tex)
    for b in range(bt):
        for c in range(c_n):
            cur = tex[b, c]
            pyr[b, c, :th * tw] = cur.reshape(-1)
            for off, h, w in layout[1:]:
                nxt = np.zeros((h, w), tex.dtype)
                for y in range(h):
                    for x in range(w):
                        nxt[y, x] = ft(ft(ft(cur[2 * y, 2 * x] + cur[2 * y, 2 * x + 1])
                                          + ft(cur[2 * y + 1, 2 * x] + cur[2 * y + 1, 2 * x + 1])) * ft(0.25))
                pyr[b, c, off:off + h * w] = nxt.reshape(-1)
                cur = nxt
            for y in range(th):
                for x in range(tw):
                    t = None
                    for l in range(len(layout) - 1, -1, -1):
                        off, h, w = layout[l]
                        gl = gpyr[b, c, off + (y >> l) * w + (x >> l)]
                        t = gl if t is None else ft(gl + ft(ft(0.25) * t))
                    gtex[b, c, y, x] = t
    return pyr, gtex


def lod_loops(uvmap, cover, size, n_l, bias):
    ft = uvmap.dtype.type
    th, tw = size
    b_n, h, w = cover.shape
    lod = np.zeros((b_n, h, w), uvmap.dtype)

    def live(b, y, x):
        return (0 <= y < h and 0 <= x < w and bool(cover[b, y, x]) and bool(np.isfinite(uvmap[b, y, x, 0]))
                and bool(np.isfinite(uvmap[b, y, x, 1])))

    with np.errstate(over="ignore"):
        for b in range(b_n):
            for y in range(h):
                for x in range(w):
                    if not live(b, y, x):
                        continue
                    u, v = uvmap[b, y, x]
                    q = []
                    for pair in (((y, x + 1), (y, x - 1)), ((y + 1, x), (y - 1, x))):
                        ds = []
                        for ny, nx in pair:
                            if live(b, ny, nx):
                                du = ft(ft(uvmap[b, ny, nx, 0] - u) * ft(tw))
                                dv = ft(ft(uvmap[b, ny, nx, 1] - v) * ft(th))
                                ds.append(ft(ft(du * du) + ft(dv * dv)))
                        q.append(min(ds) if ds else ft(0))
                    rho = ft(np.sqrt(max(q)))
                    l = 0
                    while l < n_l - 1 and rho >= ft(2 ** (l + 1)):
                        l += 1
                    if rho < 1:
                        lam = ft(0)
                    elif l == n_l - 1:
                        lam = ft(n_l - 1)
                    else:
                        lam = ft(ft(l) + ft(ft(rho * ft(2.0 ** -l)) - ft(1)))
                    lod[b, y, x] = min(max(ft(lam + ft(bias)), ft(0)), ft(n_l - 1))
    return lod


def level_blend(ft, t, off, th, tw, u, v, gs):
    """One level of one pixel: (colours [C], gx, gy, inx, iny, the four plane indices, the four weights)."""
    one, half = ft(1), ft(0.5)
    sx, sy = ft(ft(u * ft(tw)) - half), ft(ft(ft(one - v) * ft(th)) - half)
    inx, iny = -1 <= sx <= tw, -1 <= sy <= th
    sxc, syc = ft(min(max(sx, ft(-1)), ft(tw))), ft(min(max(sy, ft(-1)), ft(th)))
    x0, y0 = int(np.floor(sxc)), int(np.floor(syc))
    fx, fy = ft(sxc - ft(x0)), ft(syc - ft(y0))
    xa, xb = min(max(x0, 0), tw - 1), min(max(x0 + 1, 0), tw - 1)
    ya, yb = min(max(y0, 0), th - 1), min(max(y0 + 1, 0), th - 1)
    idx = (off + ya * tw + xa, off + ya * tw + xb, off + yb * tw + xa, off + yb * tw + xb)
    wk = (ft(ft(one - fx) * ft(one - fy)), ft(fx * ft(one - fy)), ft(ft(one - fx) * fy), ft(fx * fy))
    col, gx, gy = [], ft(0), ft(0)
    for c in range(t.shape[0]):
        t00, t01, t10, t11 = (t[c, i] for i in idx)
        top = ft(ft(ft(one - fx) * t00) + ft(fx * t01))
        bot = ft(ft(ft(one - fx) * t10) + ft(fx * t11))
        col.append(ft(ft(top * ft(one - fy)) + ft(bot * fy)))
        gx = ft(gx + ft(gs[c] * ft(ft(ft(t01 - t00) * ft(one - fy)) + ft(ft(t11 - t10) * fy))))
        gy = ft(gy + ft(gs[c] * ft(bot - top)))
    return col, (ft(gx * ft(tw)) if inx else ft(0)), (-ft(gy * ft(th)) if iny else ft(0)), idx, wk


def sample_loops(pyr, layout, uvmap, cover, lod, background, g):
    """(out, grad_uv, grad_pyr): pixel by pixel and tap by tap in ascending (b, y, x, k) order, the definition literally."""
    ft = pyr.dtype.type
    bt, c_n, _ = pyr.shape
    b_n, h, w = cover.shape
    n_l = len(layout)
    out = np.full((b_n, c_n, h, w), ft(background), pyr.dtype)
    guv = np.zeros((b_n, h, w, 2), pyr.dtype)
    gpyr = np.zeros_like(pyr)
    one = ft(1)
    for b in range(b_n):
        t, gt = pyr[b if bt > 1 else 0], gpyr[b if bt > 1 else 0]
        for y in range(h):
            for x in range(w):
                u, v = uvmap[b, y, x]
                if not (cover[b, y, x] and np.isfinite(u) and np.isfinite(v)):
                    continue
                lc = lod[b, y, x]
                lc = ft(min(lc, ft(n_l - 1))) if lc >= 0 else ft(0)
                l0 = int(np.floor(lc))
                f = ft(lc - ft(l0))
                gs = g[b, :, y, x]
                c0, ux0, vy0, idx0, w0 = level_blend(ft, t, *layout[l0], u, v, gs)
                if f == 0:
                    out[b, :, y, x] = c0
                    guv[b, y, x] = (ux0, vy0)
                else:
                    c1, ux1, vy1, idx1, w1 = level_blend(ft, t, *layout[l0 + 1], u, v, gs)
                    for c in range(c_n):
                        out[b, c, y, x] = ft(ft(ft(one - f) * c0[c]) + ft(f * c1[c]))
                    guv[b, y, x, 0] = ft(ft(ft(one - f) * ux0) + ft(f * ux1))
                    guv[b, y, x, 1] = ft(ft(ft(one - f) * vy0) + ft(f * vy1))
                for c in range(c_n):
                    for k in range(4):
                        gt[c, idx0[k]] = ft(gt[c, idx0[k]] + ft(ft(ft(one - f) * w0[k]) * gs[c]))
                    if f != 0:
                        for k in range(4):
                            gt[c, idx1[k]] = ft(gt[c, idx1[k]] + ft(ft(f * w1[k]) * gs[c]))
    return out, guv, gpyr


# ---- the layout ------------------------------------------------------------------------------------------------------
def test_mip_layout():
    full = texture.mip_layout((512, 512))
    assert len(full) == 10 and full[0] == (0, 512, 512) and full[1] == (512 * 512, 256, 256) and full[-1][1:] == (1, 1)
    assert texture.mip_layout(512) == full
    assert texture.mip_layout((12, 20)) == ((0, 12, 20), (240, 6, 10), (300, 3, 5))
    assert texture.mip_layout((33, 65)) == ((0, 33, 65),)
    seven = texture.mip_layout((128, 64))
    assert len(seven) == 7 and seven[-1][1:] == (2, 1)
    assert texture.mip_layout((8, 8), levels=2) == ((0, 8, 8), (64, 4, 4))
    assert texture.mip_layout((8, 8), levels=9) == texture.mip_layout((8, 8)) and len(texture.mip_layout((8, 8))) == 4
    assert texture.mip_layout((1, 1)) == ((0, 1, 1),)
    for size in ((512, 512), (12, 20), (128, 64), (72, 40)):
        lay = texture.mip_layout(size)
        for (o0, h0, w0), (o1, h1, w1) in zip(lay, lay[1:]):
            assert o1 == o0 + h0 * w0 and (h1, w1) == (h0 // 2, w0 // 2) and h0 % 2 == 0 and w0 % 2 == 0
        for l, (off, h, w) in enumerate(lay):                                   # the closed form the kernels use
            assert (h, w) == (size[0] >> l, size[1] >> l) and off == (size[0] * size[1] - h * w) // 3 * 4
    with pytest.raises(ValueError):
        texture.mip_layout((8, 8), levels=0)
    with pytest.raises(ValueError):
        texture.mip_layout((0, 8))


# ---- bit for bit against the loops -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tsize,levels", [((12, 20), None), ((8, 16), None), ((8, 8), 2), ((5, 7), None)])
def test_mip_build_equals_the_literal_loops(dtype, tsize, levels):
    layout = texture.mip_layout(tsize, levels)
    tex = torch.from_numpy(synth.det_uniform((2, 2) + tsize, 31)).to(dtype).requires_grad_(True)
    p = layout[-1][0] + layout[-1][1] * layout[-1][2]
    g = torch.from_numpy(synth.det_uniform((2, 2, p), 32)).to(dtype)
    pyr = texture.mip_build(tex, levels)
    (gtex,) = torch.autograd.grad(pyr, tex, g)
    want, want_g = build_loops(tex.detach().numpy(), layout, g.numpy())
    assert pyr.dtype == dtype and tuple(pyr.shape) == (2, 2, p)
    assert np.array_equal(pyr.detach().numpy(), want)
    assert np.array_equal(gtex.numpy(), want_g)
    assert torch.equal(pyr[..., :tsize[0] * tsize[1]].reshape(tex.shape), tex)   # level 0 is the texture


def lod_case(dtype, seed=41):
    """A uv map that mixes magnification and minification by up to 16, with holes in the cover and special values."""
    b_n, h, w = 2, 7, 9
    r = torch.from_numpy(synth.det_uniform((b_n, h, w, 2), seed)).double()
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    step = torch.tensor([0.004, 0.11]).view(2, 1, 1)                             # sample 0 magnifies, sample 1 minifies
    uvmap = torch.stack((0.1 + step * xs + 0.01 * r[..., 0], 0.9 - step * ys * 0.7 + 0.01 * r[..., 1]), -1).to(dtype)
    cover = torch.from_numpy(synth.det_uniform((b_n, h, w), seed + 1)) > -0.6
    cover[1, 3, 3:6] = True
    uvmap[1, 3, 4] = torch.tensor([float("nan"), 0.5])
    uvmap[1, 3, 5] = torch.tensor([0.5, float("inf")])
    uvmap[1, 0, 0] = torch.tensor([3e38, -3e38])
    cover[1, 0, :2] = True
    return uvmap, cover


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("size,levels,bias", [((64, 64), None, 0.0), ((12, 20), None, 0.37), ((64, 32), 3, -0.5)])
def test_mip_lod_equals_the_literal_loops(dtype, size, levels, bias):
    uvmap, cover = lod_case(dtype)
    n_l = len(texture.mip_layout(size, levels))
    lod = texture.mip_lod(uvmap, cover, size, levels, bias)
    want = lod_loops(uvmap.numpy(), cover.numpy(), size, n_l, float(np.float32(bias)) if dtype == torch.float32 else bias)
    assert lod.dtype == dtype and not lod.requires_grad
    assert np.array_equal(lod.numpy(), want)
    assert bool(torch.isfinite(lod).all()) and float(lod.min()) >= 0 and float(lod.max()) <= n_l - 1
    if levels is None and size == (64, 64) and dtype == torch.float32:
        assert len(np.unique(np.floor(want))) >= 3                               # several levels are in play


def mip_case(dtype, bt, tsize=(12, 20), seed=51):
    """`random_case` of the sampler's test on a pyramid, with a lod that holds whole and fractional values of every
    level, values out of range and a NaN."""
    tex, uvmap, cover, g = random_case(dtype, bt, tsize=tsize, seed=seed)
    layout = texture.mip_layout(tsize)
    n_l = len(layout)
    r = torch.from_numpy(synth.det_uniform(tuple(cover.shape), seed + 9)).double()
    lod = ((r * 0.5 + 0.5) * (n_l - 1)).to(dtype)
    lod[0, 1, :] = torch.tensor([0.0, 1.0, 2.0, 0.5, 1.5, -1.0, 7.0, float("nan"), 2.0][:lod.shape[2]]).to(dtype)
    return tex, layout, uvmap, cover, lod, g


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("bt", [1, 2])
def test_mip_sample_equals_the_literal_loops(dtype, bt):
    tex, layout, uvmap, cover, lod, g = mip_case(dtype, bt)
    pyr = texture.mip_build(tex).detach().requires_grad_(True)
    uvmap.requires_grad_(True)
    out = texture.mip_sample(pyr, (12, 20), uvmap, cover, lod, 0.25)
    gpyr, guv = torch.autograd.grad(out, (pyr, uvmap), g)
    want = sample_loops(pyr.detach().numpy(), layout, uvmap.detach().numpy(), cover.numpy(), lod.numpy(), 0.25, g.numpy())
    assert out.dtype == dtype and tuple(out.shape) == (2, 3, 6, 9)
    assert np.array_equal(out.detach().numpy(), want[0])
    assert np.array_equal(guv.numpy(), want[1])
    assert np.array_equal(gpyr.numpy(), want[2])
    for off, h, w in layout:                                                    # every level takes a gradient somewhere
        assert int((want[2][..., off:off + h * w] != 0).sum()) > 0
    assert int((want[2] == 0).sum()) > 0
    assert torch.equal(texture.mip_sample_composite(pyr, (12, 20), uvmap, cover, lod, 0.25), out)
    o = out.detach()
    assert bool((o[~cover.unsqueeze(1).expand_as(o)] == 0.25).all()) and bool((guv[~cover] == 0).all())
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(guv).all()) and bool(torch.isfinite(gpyr).all())


def test_mip_tap_plan():
    tex, layout, uvmap, cover, lod, _ = mip_case(torch.float32, 1)
    p = layout[-1][0] + layout[-1][1] * layout[-1][2]
    off, entries = texture.mip_tap_plan(uvmap, cover, lod, (12, 20), None, 1)
    assert off.dtype == torch.int32 and entries.dtype == torch.int32
    assert tuple(off.shape) == (p + 2,) and tuple(entries.shape) == (8 * cover.numel(),)
    assert int(off[0]) == 0 and int(off[-1]) == entries.numel() and bool((off[1:] >= off[:-1]).all())
    assert sorted(entries.tolist()) == list(range(entries.numel()))                  # every tap is filed once
    for key in range(p + 1):
        part = entries[int(off[key]):int(off[key + 1])].tolist()
        assert part == sorted(part)
    live = cover & torch.isfinite(uvmap).all(-1)
    lc = torch.where(lod >= 0, lod.clamp_max(len(layout) - 1.0), torch.zeros_like(lod))
    whole = live & (lc == torch.floor(lc))
    assert int(whole.sum()) > 0
    assert int(off[-1]) - int(off[-2]) == 8 * int((~live).sum()) + 4 * int(whole.sum())
    assert texture.mip_tap_plan(uvmap, cover, lod, (12, 20), None, 1)[1] is entries  # cached
    lod[1, 2, 3] += 0.25                                                              # a changed lod is another list
    assert texture.mip_tap_plan(uvmap, cover, lod, (12, 20), None, 1)[1] is not entries
    assert tuple(texture.mip_tap_plan(uvmap, cover, lod, (12, 20), None, 2)[0].shape) == (2 * p + 2,)
    with pytest.raises(ValueError):
        texture.mip_tap_plan(uvmap, cover, lod, (12, 20), None, 3)


# ---- gradients -------------------------------------------------------------------------------------------------------
def gradcheck_case(bt, tsize=(4, 8)):
    """Texture 4 x 8 (levels 4 x 8, 2 x 4, 1 x 2), image 3 x 3, B = 2.  With u = (s + 1/2) / Tw the look-up of level l
    has its kinks where (s + 1/2) / 2^l - 1/2 is whole: s = n at level 0, 2 n + 1/2 at level 1, 4 n + 3/2 at level 2.
    The positions s = 4 cell + e, e in [0.6, 0.9], [1.6, 1.9] or [2.6, 2.9], keep 0.1 away from all of them, and the
    lod's fraction lies in [0.2, 0.8] or is whole: finite differences cross neither a kink nor a level."""
    th, tw = tsize
    r = torch.from_numpy(synth.det_uniform((2, 3, 3, 5), 61)).double() * 0.5 + 0.5             # [0, 1]
    tx = torch.floor(r[..., 0] * 2).clamp(0, 1) * 4 + 0.5 + torch.floor(r[..., 1] * 3).clamp(0, 2) + 0.1 + 0.3 * r[..., 1]
    ty = 0.5 + torch.floor(r[..., 3] * 3).clamp(0, 2) + 0.1 + 0.3 * r[..., 3]
    uvmap = torch.stack(((tx + 0.5) / tw, 1 - (ty + 0.5) / th), -1)
    cover = torch.from_numpy(synth.det_uniform((2, 3, 3), 62)) > -0.7
    lod = torch.floor(r[..., 4] * 2).clamp(0, 1) + 0.2 + 0.6 * r[..., 0]
    lod[0, 0, :3] = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)
    tex = torch.from_numpy(synth.det_uniform((bt, 2, th, tw), 63)).double()
    return tex, uvmap, cover, lod


def test_gradcheck_of_mip_build():
    tex = torch.from_numpy(synth.det_uniform((2, 2, 4, 12), 64)).double().requires_grad_(True)
    assert torch.autograd.gradcheck(texture.mip_build, (tex,))
    assert torch.autograd.gradgradcheck(texture.mip_build, (tex,))
    assert torch.autograd.gradcheck(lambda t: texture.mip_build(t, 2), (tex,))


@pytest.mark.parametrize("bt", [1, 2])
def test_gradcheck_of_mip_sample_and_of_the_chain(bt):
    tex, uvmap, cover, lod = gradcheck_case(bt)
    assert 0 < int((~cover).sum()) < 9
    frac = lod - torch.floor(lod)
    assert bool(((frac == 0) | ((frac >= 0.2) & (frac <= 0.8))).all()) and int((frac == 0).sum()) >= 3
    pyr = texture.mip_build(tex).detach().requires_grad_(True)
    uvmap.requires_grad_(True)

    def look(p, m):
        return texture.mip_sample(p, (4, 8), m, cover, lod, 0.3)

    assert torch.autograd.gradcheck(look, (pyr, uvmap))
    assert torch.autograd.gradgradcheck(look, (pyr, uvmap))
    tex.requires_grad_(True)

    def chain(t, m):
        return texture.sample_mip(t, m, cover, lod=lod, background=0.3)

    assert torch.autograd.gradcheck(chain, (tex, uvmap))
    assert torch.autograd.gradgradcheck(chain, (tex, uvmap))


# ---- lod 0 and one level are `sample` --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("bt", [1, 2])
def test_lod_zero_is_sample_bit_for_bit(dtype, bt):
    tex, uvmap, cover, g = random_case(dtype, bt, tsize=(12, 20), seed=71)
    tex.requires_grad_(True)
    uvmap.requires_grad_(True)
    want = texture.sample(tex, uvmap, cover, 0.25)
    want_t, want_uv = torch.autograd.grad(want, (tex, uvmap), g)
    got = texture.sample_mip(tex, uvmap, cover, lod=torch.zeros(cover.shape, dtype=dtype), background=0.25)
    got_t, got_uv = torch.autograd.grad(got, (tex, uvmap), g)
    assert torch.equal(got, want) and torch.equal(got_uv, want_uv) and torch.equal(got_t, want_t)
    # levels=1 is `sample`, whatever the uv map's level of detail would be
    one = texture.sample_mip(tex, uvmap, cover, levels=1, background=0.25)
    one_t, one_uv = torch.autograd.grad(one, (tex, uvmap), g)
    assert torch.equal(one, want) and torch.equal(one_uv, want_uv) and torch.equal(one_t, want_t)


def test_a_texture_of_one_level_is_sample_at_any_uv_map():
    tex, uvmap, cover, g = random_case(torch.float32, 1, tsize=(33, 65), seed=72)
    tex.requires_grad_(True)
    uvmap.requires_grad_(True)
    assert len(texture.mip_layout((33, 65))) == 1
    want = texture.sample(tex, uvmap, cover, -1.0)
    got = texture.sample_mip(tex, uvmap, cover, background=-1.0)
    assert torch.equal(got, want)
    for a, b in zip(torch.autograd.grad(got, (tex, uvmap), g), torch.autograd.grad(want, (tex, uvmap), g)):
        assert torch.equal(a, b)
    assert bool((texture.mip_lod(uvmap, cover, (33, 65)) == 0).all())


# ---- aliasing, exact -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("per,lod_want", [(8, 3.0), (4, 2.0)])
def test_a_checkerboard_drawn_small_is_its_area_mean(dtype, per, lod_want):
    """64 x 64 checkerboard (x + y) & 1 under a picture with `per` texels per pixel, the samples half a texel off the
    pixel's block: every number is exact in float32.  The plain look-up lands on texel centres of one parity and
    returns 0 everywhere; the mip look-up returns the area mean."""
    n = 64 // per
    y, x = torch.meshgrid(torch.arange(64), torch.arange(64), indexing="ij")
    tex = ((x + y) & 1).to(dtype).view(1, 1, 64, 64)
    py, px = torch.meshgrid(torch.arange(n, dtype=dtype), torch.arange(n, dtype=dtype), indexing="ij")
    uvmap = torch.stack(((per * px + per / 2 + 0.5) / 64, 1 - (per * py + per / 2 + 0.5) / 64), -1)[None].contiguous()
    cover = torch.ones(1, n, n, dtype=torch.bool)
    assert bool((texture.sample(tex, uvmap, cover) == 0).all())
    lod = texture.mip_lod(uvmap, cover, (64, 64))
    assert bool((lod == lod_want).all())
    assert bool((texture.sample_mip(tex, uvmap, cover) == 0.5).all())


# ---- the seam rule ---------------------------------------------------------------------------------------------------
def test_a_chart_seam_does_not_force_the_coarse_level():
    """Columns 0..5 lie in one affine chart, columns 6..11 in a chart 32 texels away with the same slope of 2 texels per
    pixel, column 12 alone in a third chart.  Every column of the two wide charts, the two at the seam included, has a
    neighbour of its own chart on one side along x, so the minimum over the two sides gives the chart's own lod 1.  The
    one-pixel column has no such neighbour: along x it sees 30 texels, rho = 30, l = 4, lod = 4 + (30 / 16 - 1)."""
    h, w = 4, 13
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    u = torch.where(xs < 6, (2 * xs + 4) / 64, (2 * xs + 36) / 64)
    u = torch.where(xs == 12, torch.full_like(u, 28.0 / 64), u)
    uvmap = torch.stack((u, (40 - 2 * ys) / 64), -1)[None].contiguous()
    cover = torch.ones(1, h, w, dtype=torch.bool)
    lod = texture.mip_lod(uvmap, cover, (64, 64))
    assert bool((lod[0, :, :12] == 1.0).all())
    assert bool((lod[0, :, 12] == 4.875).all())
    # the plain maximum over both sides would have sent the seam's columns to level 5
    assert float(torch.log2(torch.tensor(34.0))) > 5


def test_uncovered_neighbours():
    """2 texels per pixel along x, 4 along y: with both axes usable the lod is 2 (rho = 4), with x alone 1, with none 0.
    The border rows and columns have one neighbour per axis at most."""
    ys, xs = torch.meshgrid(torch.arange(5, dtype=torch.float32), torch.arange(5, dtype=torch.float32), indexing="ij")
    uvmap = torch.stack(((2 * xs + 8) / 64, (40 - 4 * ys) / 64), -1)[None].contiguous()
    full = torch.ones(1, 5, 5, dtype=torch.bool)
    assert bool((texture.mip_lod(uvmap, full, (64, 64)) == 2.0).all())
    cover = torch.tensor([[1, 1, 1, 0, 1],
                          [0, 0, 0, 0, 0],
                          [1, 0, 1, 0, 0],
                          [1, 0, 0, 0, 1],
                          [1, 0, 0, 0, 1]], dtype=torch.bool)[None]
    want = torch.tensor([[1, 1, 1, 0, 0],
                         [0, 0, 0, 0, 0],
                         [2, 0, 0, 0, 0],
                         [2, 0, 0, 0, 2],
                         [2, 0, 0, 0, 2]], dtype=torch.float32)[None]
    assert torch.equal(texture.mip_lod(uvmap, cover, (64, 64)), want)
    # a neighbour with a non-finite coordinate is as good as uncovered
    broken = uvmap.clone()
    broken[0, 0, 1, 0] = float("nan")
    got = texture.mip_lod(broken, cover, (64, 64))
    assert float(got[0, 0, 0]) == 0 and float(got[0, 0, 1]) == 0 and float(got[0, 0, 2]) == 0


# ---- coordinates out of range ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_coordinates_out_of_range(dtype):
    big = 3e38 if dtype == torch.float32 else 1.5e308
    tex = torch.from_numpy(synth.det_uniform((1, 2, 8, 8), 81)).to(dtype).requires_grad_(True)
    uvmap = torch.full((1, 3, 4, 2), 0.5, dtype=dtype)
    uvmap[0, 0, 0] = torch.tensor([big, -big], dtype=dtype)
    uvmap[0, 0, 1] = torch.tensor([-big, big], dtype=dtype)
    uvmap[0, 0, 2] = torch.tensor([big, big], dtype=dtype)
    assert bool(torch.isfinite(uvmap[0, 0, :3]).all())
    uvmap[0, 1, 1] = torch.tensor([float("inf"), 0.5])
    uvmap[0, 2, 2] = torch.tensor([0.5, float("nan")])
    uvmap.requires_grad_(True)
    cover = torch.ones(1, 3, 4, dtype=torch.bool)
    lod = texture.mip_lod(uvmap, cover, (8, 8))
    top = len(texture.mip_layout((8, 8))) - 1
    assert bool(torch.isfinite(lod).all())
    assert float(lod[0, 0, 0]) == top and float(lod[0, 0, 1]) == top and float(lod[0, 0, 2]) == top     # the overflow
    assert float(lod[0, 1, 1]) == 0 and float(lod[0, 2, 2]) == 0                                        # not live
    out = texture.sample_mip(tex, uvmap, cover, background=-2.0)
    assert bool(torch.isfinite(out).all())
    assert bool((out[0, :, 1, 1] == -2.0).all()) and bool((out[0, :, 2, 2] == -2.0).all())
    gtex, guv = torch.autograd.grad(out.sum(), (tex, uvmap))
    assert bool(torch.isfinite(gtex).all()) and bool(torch.isfinite(guv).all())
    assert bool((guv[0, 1, 1] == 0).all()) and bool((guv[0, 2, 2] == 0).all()) and bool((guv[0, 0, :3] == 0).all())


# ---- bias, constants, affine textures --------------------------------------------------------------------------------
def test_bias_shifts_and_clamps():
    uvmap, cover = lod_case(torch.float32)
    base = texture.mip_lod(uvmap, cover, (64, 64))
    live = cover & torch.isfinite(uvmap).all(-1)
    up = texture.mip_lod(uvmap, cover, (64, 64), bias=0.5)
    inner = live & (base + 0.5 <= 6)
    assert int(inner.sum()) > 20 and torch.equal(up[inner], base[inner] + 0.5)
    assert bool((up[live & ~inner] == 6).all()) and bool((up[~live] == 0).all())
    assert bool((texture.mip_lod(uvmap, cover, (64, 64), bias=-10.0) == 0).all())
    assert bool((texture.mip_lod(uvmap, cover, (64, 64), bias=100.0)[live] == 6).all())
    assert bool((texture.mip_lod(uvmap, cover, (64, 64), levels=3, bias=100.0)[live] == 2).all())


def test_a_constant_texture_stays_constant_and_an_affine_one_is_reproduced():
    """A constant c: every level holds c exactly (((c + c) + (c + c)) 0.25), and the look-up is three nested convex
    blends of c, each two products and a sum, within 1.5 ulp each: 8 eps |c| bounds the result.  An affine texture: the
    2 x 2 mean of an affine function is its value at the block's centre, the texel centre of the next level, so every
    level holds the same affine function and the bilinear look-up reproduces it between a level's outermost texel
    centres; float64 on values below 2 with some twenty operations: 1e-13."""
    _, uvmap, cover, _ = random_case(torch.float64, 1, tsize=(32, 32), seed=91)
    r = torch.from_numpy(synth.det_uniform(tuple(cover.shape), 92)).double()
    lod = (r * 0.5 + 0.5) * 5
    const = torch.full((1, 2, 32, 32), 0.3, dtype=torch.float64)
    pyr = texture.mip_build(const)
    assert bool((pyr == 0.3).all())
    out = texture.mip_sample(pyr, (32, 32), uvmap, cover, lod, 0.3)
    assert float((out - 0.3).abs().max()) <= 8 * 2.0 ** -52 * 0.3
    tex = affine_texture((32, 32), torch.float64)
    u = 0.15 + 0.7 * (torch.from_numpy(synth.det_uniform((1, 6, 9, 2), 93)).double() * 0.5 + 0.5)
    want = torch.einsum("byxk,ck->bcyx", u, ABC[:, :2]) + ABC[:, 2].view(1, 3, 1, 1)
    every = torch.ones(1, 6, 9, dtype=torch.bool)
    for level in range(4):                                                      # level 3 is 4 x 4: centres at 1/8 .. 7/8
        got = texture.sample_mip(tex, u, every, lod=torch.full((1, 6, 9), float(level), dtype=torch.float64))
        assert float((got - want).abs().max()) <= 1e-13, level


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    from stylerenderer_amd import _lib

    L = _lib.lib()
    assert L.sr_mip_build_fwd(None, None, 2, 8, 8, 4, None) == -1              # NULL pointers
    assert L.sr_mip_build_fwd(None, None, 0, 8, 8, 4, None) == 0               # no planes: nothing to do
    assert L.sr_mip_build_fwd(None, None, 2, 8, 8, 5, None) == -1              # 8 x 8 has four levels
    assert L.sr_mip_build_fwd(None, None, 2, 33, 65, 2, None) == -1            # an odd side: one level
    assert L.sr_mip_build_fwd(None, None, 2, 0, 8, 1, None) == -1
    assert L.sr_mip_build_bwd(None, None, 1, 3, 8, 8, 4, None) == -1
    assert L.sr_mip_build_bwd(None, None, 1, 0, 8, 8, 4, None) == -1
    assert L.sr_mip_lod(None, None, None, 2, 8, 8, 8, 8, 4, 0.0, None) == -1
    assert L.sr_mip_lod(None, None, None, 2, 0, 8, 8, 8, 4, 0.0, None) == 0
    assert L.sr_mip_lod(None, None, None, 2, 8, 8, 8, 8, 0, 0.0, None) == -1
    sizes = dict(B=2, Bt=1, C=3, H=8, W=8, Th=8, Tw=8, L=4)
    order = ("B", "Bt", "C", "H", "W", "Th", "Tw", "L")

    def fwd(**over):
        s = dict(sizes, **over)
        return L.sr_mip_sample_fwd(None, None, None, None, None, *[s[k] for k in order], 0.0, None)

    def bwd_uv(**over):
        s = dict(sizes, **over)
        return L.sr_mip_sample_bwd_uv(None, None, None, None, None, None, *[s[k] for k in order], None)

    def bwd_pyr(**over):
        s = dict(sizes, **over)
        return L.sr_mip_sample_bwd_pyr(None, None, None, None, None, None, None, *[s[k] for k in order], None)

    for call in (fwd, bwd_uv, bwd_pyr):
        assert call() == -1
        assert call(Bt=3) == -1
        for name in ("C", "Th", "Tw", "L"):
            assert call(**{name: 0}) == -1, name
        assert call(L=5) == -1 and call(B=-1) == -1 and call(H=-1) == -1
    for call in (fwd, bwd_uv):
        assert call(B=0, Bt=0) == 0 and call(H=0) == 0 and call(W=0) == 0
    assert bwd_pyr(H=0) == -1                                                  # (it still writes zeros: the pointers count)


# ---- the tool --------------------------------------------------------------------------------------------------------
def refine_as_before(tex, views, steps, lr):
    """The refinement loop as it stood before the mip look-up, step for step."""
    from stylerenderer_amd import optim

    uvmap = torch.cat([u for u, _, _ in views], 0).contiguous()
    cover = torch.cat([c for _, c, _ in views], 0).contiguous()
    target = torch.cat([t for _, _, t in views], 0)
    p = tex.detach().clone().contiguous().requires_grad_(True)
    offs, total = optim.flat_layout([p])
    flat_g = torch.zeros(total, dtype=p.dtype, device=p.device)
    opt = optim.FlatAdam([p], flat_g, lr=float(lr))
    slot = optim.flat_views(flat_g, [p], offs)[0]
    on = cover.unsqueeze(1).to(p.dtype)
    losses = []
    for _ in range(steps):
        diff = (texture.sample(p, uvmap, cover, 0.0) - target) * on
        loss = (diff * diff).sum()
        (g,) = torch.autograd.grad(loss, p)
        slot.copy_(g)
        opt.step()
        losses.append(float(loss.detach()))
    return p.detach().clone(), np.asarray(losses, np.float64)


def test_refinement_with_the_mip_look_up():
    from stylerenderer_amd import reconstruct

    views, start = two_views((64, 64), 24)                                    # 64^2 texels under 24^2 pixels: minified
    weight = torch.ones(1, 1, 64, 64)
    refined, loss = reconstruct.texture_refine(start, views, 12, lr=0.02, mip=0.0)
    assert loss.shape == (12,) and np.isfinite(loss).all() and loss[-1] < loss[0]
    assert tuple(refined.shape) == tuple(start.shape) and not start.requires_grad
    after = reconstruct.texture_rerender(refined, weight, views, mip=0.0)
    before = reconstruct.texture_rerender(start, weight, views, mip=0.0)
    for a, b in zip(after, before):
        assert a[1] <= b[1] and a[2] == b[2] and a[3] > 0
    # step 0's gradient reaches more texels through the pyramid
    uvmap = torch.cat([u for u, _, _ in views], 0).contiguous()
    cover = torch.cat([c for _, c, _ in views], 0).contiguous()
    target = torch.cat([t for _, _, t in views], 0)
    on = cover.unsqueeze(1).float()
    shares = []
    for mip in (None, 0.0):
        p = start.clone().requires_grad_(True)
        img = texture.sample(p, uvmap, cover) if mip is None else texture.sample_mip(p, uvmap, cover, bias=mip)
        (g,) = torch.autograd.grad((((img - target) * on) ** 2).sum(), p)
        shares.append(float((g != 0).any(1).float().mean()))
    print("share of texels with a gradient in step 0: plain %.3f, mip %.3f" % tuple(shares))
    assert 0 < shares[0] < shares[1]
    # without `mip` the outputs are the earlier ones bit for bit
    plain, plain_loss = reconstruct.texture_refine(start, views, 5, lr=0.02)
    old, old_loss = refine_as_before(start, views, 5, 0.02)
    assert torch.equal(plain, old) and np.array_equal(plain_loss, old_loss)
    for (img, err, n_c, n_o), (uvm, cov, tgt) in zip(reconstruct.texture_rerender(start, weight, views), views):
        assert torch.equal(img, texture.sample(start, uvm, cov, -1.0)) and n_c == int(cov.sum()) and n_o == n_c
