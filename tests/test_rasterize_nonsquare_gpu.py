"""The device rasterizer on non-square images with geometry over the whole x = -1 .. 1 span, against the C oracle:
samples that alias into later rows (h > w), dropped rows (w > h), one-pixel-wide images.  Inputs, references and the
per-element gradient tolerance: tests/raster_nonsquare_cases.py; what the inputs exercise: the CPU companion
tests/test_rasterize_nonsquare_cpu.py."""
import importlib

import numpy as np
import pytest
import torch

import raster_nonsquare_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRAD_SWITCHES = [("SR_RASTER_GRAD_SLOTS", "0"), ("SR_RASTER_GRAD_EAGER", "0"), ("SR_RASTER_GRAD_EAGER", "1")]
CLEAR = ["SR_RASTER_TILED", "SR_RASTER_GRAD_SLOTS", "SR_RASTER_GRAD_EAGER", "SR_RASTER_LEVELS", "SR_RASTER_PYRAMID"]


def T(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None or a.dtype.kind != "f" else a.astype(dtype))
    return torch.from_numpy(a).to(DEV)


@pytest.fixture
def clean(monkeypatch):
    for name in CLEAR:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _differ(a, b, rows):
    """pixels (rows of the flattened image stack) at which two arrays differ in any bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    kind = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return int((a.view(kind) != b.view(kind)).reshape(rows, -1).any(1).sum())


@pytest.mark.parametrize("p", C.all_cases(), ids=C.case_id)
def test_forward_equals_the_oracle_bit_for_bit(p, clean):
    """ids, weights, depth, dcoeff and the interpolated attributes in both layouts; fp32 and fp64; SR_RASTER_TILED unset
    and = 1 (the forced tiled path declines a non-square image and the global-key path draws it)."""
    import stylerenderer_amd.op as op
    R = importlib.import_module("stylerenderer_amd.op.rasterize")

    cs = C.case(*p)
    n = 2 * cs.h * cs.w
    bad = []
    for dtype in (np.float32, np.float64):
        o = cs.oracle(dtype)
        v, tex, tri = T(cs.v, dtype), T(cs.tex, dtype), T(cs.tri)
        for tiled in (None, "1"):
            if tiled is None:
                clean.delenv("SR_RASTER_TILED", raising=False)
            else:
                clean.setenv("SR_RASTER_TILED", tiled)
            idx, coeff, zbuf = R.forward_with_depth(v, tri, cs.h, cs.w, cs.persp, C.EPS)
            out = op.rasterize(v, tex, tri, cs.h, cs.w, cs.persp)
            chw = op.rasterize(v, tex, tri, cs.h, cs.w, cs.persp, channel_major=True)
            dco = R.backward(v, idx, cs.persp, C.EPS)
            counts = dict(ids=int((idx.cpu().numpy() != o["index"]).reshape(n, 3).any(1).sum()),
                          weights=_differ(coeff.cpu().numpy(), o["coeff"], n), depth=_differ(zbuf.cpu().numpy(), o["zbuf"], n),
                          attributes=_differ(out.cpu().numpy(), o["attr"], n),
                          channel_major=_differ(chw.permute(0, 2, 3, 1).contiguous().cpu().numpy(), o["attr"], n),
                          dcoeff=_differ(dco.cpu().numpy(), o["dcoeff"], n))
            print("%s tiled=%s: pixels of %d that differ from the oracle: %s" % (np.dtype(dtype).name, tiled, n, counts))
            bad += ["%s tiled=%s %s: %d pixels" % (np.dtype(dtype).name, tiled, k, c) for k, c in counts.items() if c]
    assert not bad, bad


def _grads(cs, dtype):
    import stylerenderer_amd.op as op

    v, tx = T(cs.v, dtype).requires_grad_(), T(cs.tex, dtype).requires_grad_()
    out = op.rasterize(v, tx, T(cs.tri), cs.h, cs.w, cs.persp)
    return torch.autograd.grad(out, [v, tx], T(cs.go, dtype))


@pytest.mark.parametrize("p", C.all_cases(), ids=C.case_id)
def test_gradients_equal_the_oracle_per_element(p, clean):
    """Both gradients of op.rasterize, fp32 and fp64: every element within tol * S_i of the oracle's float64-accumulated
    gradient (raster_nonsquare_cases: S_i is the sum of the magnitudes of the terms of element i, tol four times the
    reference's own float32 accumulation error), the suite's whole-tensor bound as well, no non-finite value, byte
    identical from run to run and under SR_RASTER_GRAD_SLOTS=0 and SR_RASTER_GRAD_EAGER=0 / 1."""
    cs = C.case(*p)
    bad = []
    for dtype, tol in ((np.float32, C.TOL_F32), (np.float64, C.TOL_F64)):
        o = cs.oracle(dtype)
        name = np.dtype(dtype).name
        gv, gt = _grads(cs, dtype)
        again = _grads(cs, dtype)
        if not (torch.equal(gv, again[0]) and torch.equal(gt, again[1])):
            bad.append(name + ": differs from run to run")
        for setting in GRAD_SWITCHES:
            for sw, _ in GRAD_SWITCHES:
                clean.delenv(sw, raising=False)
            clean.setenv(*setting)
            other = _grads(cs, dtype)
            if not (torch.equal(gv, other[0]) and torch.equal(gt, other[1])):
                bad.append("%s: %s=%s changes the gradient" % ((name,) + setting))
        for sw, _ in GRAD_SWITCHES:
            clean.delenv(sw, raising=False)
        gv, gt = gv.cpu().numpy(), gt.cpu().numpy()
        ev, et = C.in_units(gv, o["grad_v"], o["s_v"]), C.in_units(gt, o["grad_tex"], o["s_tex"])
        mv, mt = np.abs(o["grad_v"]).max(), np.abs(o["grad_tex"]).max()
        wv = np.abs(gv - o["grad_v"]).max() / mv if mv > 0 else np.abs(gv).max()
        wt = np.abs(gt - o["grad_tex"]).max() / mt if mt > 0 else np.abs(gt).max()
        print("%s: grad_v %.3g, grad_tex %.3g in units of S_i (tol %.3g); of the largest element %.3g, %.3g; max|grad_v| %.3g"
              % (name, ev, et, tol, wv, wt, mv))
        if not (np.isfinite(gv).all() and np.isfinite(gt).all()):
            bad.append(name + ": non-finite gradient")
        if not (ev <= tol and et <= tol):
            bad.append("%s: per-element error %.3g / %.3g above %.3g" % (name, ev, et, tol))
        if not (wv <= 5e-5 and wt <= 5e-6):
            bad.append("%s: whole-tensor error %.3g / %.3g" % (name, wv, wt))
    assert not bad, bad


@pytest.mark.parametrize("persp", [False, True], ids=["ortho", "persp"])
def test_pyramid_with_non_square_levels_equals_the_single_calls(persp, clean):
    """rasterize_pyramid over [(20, 12), (12, 20), (16, 16)]: maps and gradients equal the per-level op.rasterize calls
    bit for bit (the gradients added in list order), with the levels entry points taken (sr_rasterize_forward_levels_f32,
    sr_rasterize_grad_levels_f32: the level with h > w gets k_resolve_alias / k_grad_*_alias launches of its own inside
    them) and with SR_RASTER_LEVELS=0.  The list without that level is compared the same way."""
    from stylerenderer_amd.op.rasterize import rasterize, rasterize_pyramid
    R = importlib.import_module("stylerenderer_amd.op.rasterize")

    vh, trih = C.ab_mesh(20, 12, persp, on_image=False)
    tex = C.det_normal((2, vh.shape[1], 3), 91)
    for sizes in ([(20, 12), (12, 20), (16, 16)], [(12, 20), (16, 16)], [(16, 16), (40, 12), (20, 12)]):
        ups = [T(C.det_normal((2, 3, h, w), 93 + k)) for k, (h, w) in enumerate(sizes)]
        tri = T(trih)
        single_maps, gv_want, gt_want = [], None, None
        for (h, w), up in zip(sizes, ups):
            v, tx = T(vh).requires_grad_(), T(tex).requires_grad_()
            m = rasterize(v, tx, tri, h, w, persp, channel_major=True)
            gv, gt = torch.autograd.grad(m, [v, tx], up)
            single_maps.append(m.detach())
            gv_want = gv if gv_want is None else gv_want + gv
            gt_want = gt if gt_want is None else gt_want + gt
        got = R._forward_levels(T(vh), T(tex), tri, sizes, persp, 1e-6, True, True)
        assert got[0] is not None                                  # the entry point takes the list
        for levels in (None, "0"):
            if levels is None:
                clean.delenv("SR_RASTER_LEVELS", raising=False)
            else:
                clean.setenv("SR_RASTER_LEVELS", levels)
            v, tx = T(vh).requires_grad_(), T(tex).requires_grad_()
            maps = rasterize_pyramid(v, tx, tri, sizes, persp, channel_major=True)
            gv, gt = torch.autograd.grad(maps, [v, tx], ups)
            for a, b in zip(maps, single_maps):
                assert torch.equal(a.detach(), b)
            assert torch.equal(gv, gv_want) and torch.equal(gt, gt_want)
            assert bool(torch.isfinite(gv).all()) and bool(torch.isfinite(gt).all())
        clean.delenv("SR_RASTER_LEVELS", raising=False)
