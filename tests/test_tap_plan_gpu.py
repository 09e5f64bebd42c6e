"""GPU: the native tap-list builder (csrc/tap_plan.hip, op.texture.TapPlanner) against the host definition op.texture.tap_plan,
integer for integer; both sides of every pass-count threshold; no stale scratch under poisoned buffers; reruns; the sampler's
gradients with a planner against the host float32 composite bit for bit, eagerly and under graph capture with a uv map that
moves between replays; the corner explode's ordered adjoint (csrc/explode.hip)."""
import functools

import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, graphs, synth
from stylerenderer_amd.op import texture
from test_texture_sample_gpu import host_case, host_map

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


# ---- uv maps ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ellipsoid():
    v0, tri0 = synth.uv_ellipsoid(16, 14)
    uv0, tri_uv0, keep = face_model.uv_layout(v0, tri0)
    return v0, torch.from_numpy(tri0), uv0, tri_uv0, keep


@functools.lru_cache(maxsize=None)
def ellipsoid_map(isize, b_n, seed=1234, shrink=1.0, shift=0.0):
    """The uv map of the posed ellipsoid of test_texture_sample_gpu.py (host); shrink and shift move it out of the picture."""
    v0, tri, uv0, tri_uv0, keep = ellipsoid()
    vp = torch.from_numpy(synth.random_poses(v0, b_n, seed=seed)).float() * shrink
    vp[..., 0] += shift
    uvmap, cover = texture.uv_map(vp, tri, uv0, tri_uv0, isize, keep)
    return uvmap.contiguous(), cover.contiguous()


def synthetic_maps(isize, b_n):
    """name -> (uvmap, cover): the values the definition treats specially, and the extremes of coverage."""
    shape = (b_n, isize, isize)
    rnd = torch.from_numpy(synth.det_uniform(shape + (2,), 40 + isize + b_n)) * 0.7 + 0.5          # in [-0.2, 1.2)
    special = rnd.clone()
    vals = [(0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (-0.3, 1.4), (1.7, -0.2), (float("nan"), 0.5),
            (0.5, float("nan")), (float("inf"), 0.5), (0.5, float("-inf")), (float("-inf"), float("inf")), (7.0, -3.0)]
    for j, (a, b) in enumerate(vals):
        special[b_n - 1, j % isize, (3 * j) % isize] = torch.tensor([a, b])
    some = torch.from_numpy(synth.det_uniform(shape, 41 + isize)) > -0.5
    for j in range(len(vals)):
        some[b_n - 1, j % isize, (3 * j) % isize] = True
    return {
        "special": (special, some),
        "uncovered": (rnd, torch.zeros(shape, dtype=torch.bool)),
        "covered": (rnd, torch.ones(shape, dtype=torch.bool)),
        # all 4 B H W taps on one key: both coordinates clamp onto texel (0, 0)
        "constant": (torch.tensor([-5.0, 9.0]).expand(shape + (2,)).contiguous(), torch.ones(shape, dtype=torch.bool)),
    }


def host_plan(uvmap, cover, tsize, bt):
    texture._PLAN_CACHE.clear()
    off, entries = texture.tap_plan(uvmap, cover, tsize, bt)
    return off.clone(), entries.clone()


def check_equal(planner, uvmap, cover, tsize, bt, what):
    want_off, want_e = host_plan(uvmap, cover, tsize, bt)
    off, entries = planner.build(uvmap.to(DEV), cover.to(DEV))
    torch.cuda.synchronize()
    bad = (int((off.cpu() != want_off).sum()), int((entries.cpu() != want_e).sum()))
    print("tap plan", what, tsize, tuple(cover.shape), "Bt", bt, "passes", planner.passes, "mismatches (off, entries)", bad)
    assert off.dtype == torch.int32 and entries.dtype == torch.int32
    assert tuple(off.shape) == tuple(want_off.shape) and tuple(entries.shape) == tuple(want_e.shape)
    assert torch.equal(off.cpu(), want_off), (what, bad)
    assert torch.equal(entries.cpu(), want_e), (what, bad)


# ---- equality with tap_plan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tsize", [(8, 8), (33, 65), (4, 4), (1, 1)])
@pytest.mark.parametrize("isize", [16, 33])
def test_build_equals_tap_plan(tsize, isize):
    for b_n in (1, 3):
        maps = {"ellipsoid": ellipsoid_map(isize, b_n), "scene": host_map(isize, b_n)}
        maps.update(synthetic_maps(isize, b_n))
        for bt in sorted({1, b_n}):
            planner = texture.TapPlanner(b_n, isize, isize, tsize, bt, DEV)
            for name, (uvmap, cover) in maps.items():
                check_equal(planner, uvmap, cover, tsize, bt, name)
    # what the maps are there for
    uvmap, cover = ellipsoid_map(isize, 3)
    assert 0 < int(cover.sum()) < cover.numel()
    off, _ = host_plan(*synthetic_maps(isize, 3)["constant"], tsize, 1)
    assert int(off[0]) == 0 and int(off[1]) == 4 * 3 * isize * isize         # the pile-up: one list holds every tap
    off, _ = host_plan(*synthetic_maps(isize, 3)["uncovered"], tsize, 1)
    assert int(off[-2]) == 0 and int(off[-1]) == 4 * 3 * isize * isize


def _sides(n):
    a = int(np.sqrt(n))
    while n % a:
        a -= 1
    return a, n // a


def test_both_sides_of_every_pass_threshold():
    d = texture.TAP_RADIX_BITS
    want_passes = {2 ** d - 1: 1, 2 ** d: 2, 2 ** (2 * d) - 1: 2, 2 ** (2 * d): 3}
    uvmap, cover = ellipsoid_map(16, 1)
    spread = synthetic_maps(16, 1)["covered"]
    for n_keys, passes in want_passes.items():
        tsize = _sides(n_keys)
        assert tsize[0] * tsize[1] == n_keys
        planner = texture.TapPlanner(1, 16, 16, tsize, 1, DEV)
        assert planner.passes == passes, (n_keys, planner.passes)
        assert planner.launches == 2 + 3 * passes
        check_equal(planner, uvmap, cover, tsize, 1, "threshold %d" % n_keys)
        check_equal(planner, *spread, tsize, 1, "threshold %d spread" % n_keys)
    # Bt Th Tw counts, not Th Tw: three textures of 2^d / 4 ... the batch moves the threshold
    planner = texture.TapPlanner(3, 16, 16, (8, 16), 3, DEV)                  # 3 * 128 = 384 >= 2^8
    if d == 8:
        assert planner.passes == 2 and texture.TapPlanner(3, 16, 16, (8, 16), 1, DEV).passes == 1
    check_equal(planner, *ellipsoid_map(16, 3), (8, 16), 3, "threshold Bt")


# ---- no stale scratch, reruns ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tsize,isize", [((33, 65), 33), ((4, 4), 16)])
def test_no_stale_scratch_and_reruns(tsize, isize):
    b_n = 3
    a = ellipsoid_map(isize, b_n)
    b = synthetic_maps(isize, b_n)["special"]
    for bt in (1, b_n):
        fresh = texture.TapPlanner(b_n, isize, isize, tsize, bt, DEV)
        want = tuple(x.clone() for x in fresh.build(b[0].to(DEV), b[1].to(DEV)))
        again = tuple(x.clone() for x in fresh.build(b[0].to(DEV), b[1].to(DEV)))
        assert torch.equal(want[0], again[0]) and torch.equal(want[1], again[1])                    # reruns
        host = host_plan(b[0], b[1], tsize, bt)
        assert torch.equal(want[0].cpu(), host[0]) and torch.equal(want[1].cpu(), host[1])
        used = texture.TapPlanner(b_n, isize, isize, tsize, bt, DEV)
        for poison in (None, 0x7f, -1):
            used.build(a[0].to(DEV), a[1].to(DEV))
            if poison is not None:
                for buf in used.buffers():
                    buf.view(torch.uint8).fill_(poison & 0xff)
                assert int(used.off[0]) == (0x7f7f7f7f if poison == 0x7f else -1)
            got = used.build(b[0].to(DEV), b[1].to(DEV))
            torch.cuda.synchronize()
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (bt, poison)


def test_a_planner_refuses_what_it_was_not_made_for():
    with pytest.raises(ValueError):
        texture.TapPlanner(2, 16, 16, 8, 1, "cpu")
    with pytest.raises(ValueError):
        texture.TapPlanner(3, 16, 16, 8, 2, DEV)
    planner = texture.TapPlanner(1, 16, 16, 8, 1, DEV)
    uvmap, cover = ellipsoid_map(16, 1)
    tex = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError):
        texture.sample(tex, uvmap, cover, planner=planner)                   # host tensors
    with pytest.raises(ValueError):
        texture.sample(torch.zeros(1, 1, 4, 4, device=DEV), uvmap.to(DEV), cover.to(DEV), planner=planner)
    with pytest.raises(ValueError):
        planner.build(uvmap.to(DEV)[:, :8], cover.to(DEV)[:, :8])


# ---- the sampler's gradients with a planner --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tsize,isize", [((33, 65), 16), ((33, 65), 33), ((4, 4), 16), ((4, 4), 33)])
def test_gradients_with_a_planner_equal_the_host_bit_for_bit(tsize, isize):
    for b_n in (1, 3):
        for c_n in (1, 3):
            for bt in sorted({1, b_n}):
                tex, uvmap, cover, g, want, want_t, want_uv = host_case(tsize, isize, b_n, c_n, bt)
                planner = texture.TapPlanner(b_n, isize, isize, tsize, bt, DEV)
                t, m = tex.to(DEV).requires_grad_(True), uvmap.to(DEV).requires_grad_(True)
                out = texture.sample(t, m, cover.to(DEV), 0.25, planner=planner)
                texture._PLAN_CACHE.clear()
                before = len(texture._PLAN_CACHE)
                gtex, guv = torch.autograd.grad(out, (t, m), g.to(DEV))
                assert len(texture._PLAN_CACHE) == before                     # the list came from the planner
                bad = (int((out.cpu() != want).sum()), int((guv.cpu() != want_uv).sum()), int((gtex.cpu() != want_t).sum()))
                print("planner", tsize, isize, "B", b_n, "C", c_n, "Bt", bt, "mismatches (out, grad_uv, grad_tex)", bad)
                assert torch.equal(out.detach().cpu(), want), bad
                assert torch.equal(guv.cpu(), want_uv), bad
                assert torch.equal(gtex.cpu(), want_t), bad


def test_capture_with_a_moving_uv_map():
    tsize, isize, b_n, c_n = (33, 65), 16, 3, 3
    poses = [ellipsoid_map(isize, b_n, 1234), ellipsoid_map(isize, b_n, 77), ellipsoid_map(isize, b_n, 5, 0.3, 0.9)]
    assert int(poses[2][1].sum()) < 0.1 * poses[2][1].numel()                 # most pixels uncovered
    assert int(poses[2][1].sum()) > 0
    gd = torch.from_numpy(synth.det_uniform((b_n, c_n, isize, isize), 9)).to(DEV)
    for bt in (1, b_n):
        planner = texture.TapPlanner(b_n, isize, isize, tsize, bt, DEV)
        t = torch.zeros((bt, c_n) + tsize, device=DEV, requires_grad=True)
        m = poses[1][0].to(DEV).clone().requires_grad_(True)
        c = poses[1][1].to(DEV).clone()
        out = {}

        def body():
            y = texture.sample(t, m, c, 0.25, planner=planner)
            out["gtex"], out["guv"] = torch.autograd.grad(y, (t, m), gd)
            out["y"] = y.detach()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = graphs.capture(body)
        assert graph.memset_nodes_replaced == 0
        for k, (uvmap, cover) in enumerate(poses):
            tex = torch.from_numpy(synth.det_uniform((bt, c_n) + tsize, 300 + k))
            with torch.no_grad():
                t.copy_(tex)
                m.copy_(uvmap)
                c.copy_(cover)
            graph.replay()
            torch.cuda.synchronize()
            th, mh = tex.clone().requires_grad_(True), uvmap.clone().requires_grad_(True)
            y = texture.sample_composite(th, mh, cover, 0.25)
            want_t, want_uv = torch.autograd.grad(y, (th, mh), gd.cpu())
            bad = (int((out["y"].cpu() != y.detach()).sum()), int((out["guv"].cpu() != want_uv).sum()),
                   int((out["gtex"].cpu() != want_t).sum()))
            print("capture Bt", bt, "replay", k, "covered", int(cover.sum()), "mismatches (out, grad_uv, grad_tex)", bad)
            assert torch.equal(out["y"].cpu(), y.detach()), bad
            assert torch.equal(out["guv"].cpu(), want_uv), bad
            assert torch.equal(out["gtex"].cpu(), want_t), bad
            if k < 2:
                assert float(want_t.abs().max()) > 0 and float(want_uv.abs().max()) > 0


# ---- the corner explode -------------------------------------------------------------------------------------------------------
def explode_mesh():
    """A fan of 12 faces around vertex 0 (valence 12), one more face whose corners 14 and 15 have valence 1, vertex 16
    unused."""
    faces = [(0, 1 + j, 2 + j) for j in range(12)] + [(13, 14, 15)]
    return torch.tensor(faces, dtype=torch.int64), 17


def literal_adjoint(g, tri, nv):
    """The ordered sum, element by element in float32: the corners of a vertex in ascending k nf + f."""
    g = g.numpy()
    nf = tri.shape[0]
    flat = tri.t().reshape(-1).numpy()                                       # position k nf + f holds tri[f, k]
    out = np.zeros((g.shape[0], nv, 3), np.float32)
    for a, i in enumerate(flat):
        k, f = divmod(a, nf)
        out[:, i] = out[:, i] + g[:, 3 * f + k]
    return torch.from_numpy(out)


def test_explode_forward_and_ordered_adjoint():
    tri, nv = explode_mesh()
    b_n = 2
    v = torch.from_numpy(synth.det_uniform((b_n, nv, 3), 3))
    g = torch.from_numpy(synth.det_uniform((b_n, 3 * tri.shape[0], 3), 4)) * 1e3
    vh = v.clone().requires_grad_(True)
    ch = texture.explode(vh, tri)
    assert torch.equal(ch.detach(), v[:, tri.reshape(-1)])
    (want,) = torch.autograd.grad(ch, vh, g)
    assert torch.equal(want, literal_adjoint(g, tri, nv))                     # the host path is the stated order
    assert bool((want[:, 16] == 0).all()) and torch.equal(want[:, 14], g[:, 3 * 12 + 1])
    tri_d = tri.to(DEV)
    vd = v.to(DEV).requires_grad_(True)
    cd = texture.explode(vd, tri_d)
    assert cd.is_cuda and torch.equal(cd.detach().cpu(), ch.detach())
    (got,) = torch.autograd.grad(cd, vd, g.to(DEV), retain_graph=True)
    (again,) = torch.autograd.grad(cd, vd, g.to(DEV))
    print("explode mismatches", int((got.cpu() != want).sum()))
    assert torch.equal(got.cpu(), want) and torch.equal(again, got)
    # the sum is not the library's: the order matters at this magnitude, and the index path may differ
    (lib,) = torch.autograd.grad(vh[:, tri.reshape(-1)], vh, g)
    assert torch.allclose(lib, want, rtol=1e-4, atol=1e-2)
    # through uv_map: the same values, the same gradient up to the order of the sum
    v0, tri0, uv0, tri_uv0, keep = ellipsoid()
    vp = torch.from_numpy(synth.random_poses(v0, 2)).float()
    gm = torch.from_numpy(synth.det_uniform((2, 16, 16, 2), 6))
    res = []
    for flag in (False, True):
        vq = vp.to(DEV).requires_grad_(True)
        uvmap, cover = texture.uv_map(vq, tri0.to(DEV) if flag else tri0, uv0.to(DEV), tri_uv0, 16, keep.to(DEV), explode=flag)
        res.append((uvmap.detach(), cover, torch.autograd.grad(uvmap, vq, gm.to(DEV))[0]))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.allclose(res[0][2], res[1][2], rtol=1e-4, atol=1e-5) and float(res[1][2].abs().max()) > 0


def test_explode_under_graph_capture():
    tri, nv = explode_mesh()
    tri_d = tri.to(DEV)
    vd = torch.zeros(2, nv, 3, device=DEV, requires_grad=True)
    gd = torch.zeros(2, 3 * tri.shape[0], 3, device=DEV)
    out = {}

    def body():
        c = texture.explode(vd, tri_d)
        out["c"] = c.detach()
        (out["gv"],) = torch.autograd.grad(c, vd, gd)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    for k in range(2):
        v = torch.from_numpy(synth.det_uniform((2, nv, 3), 50 + k))
        g = torch.from_numpy(synth.det_uniform((2, 3 * tri.shape[0], 3), 60 + k))
        with torch.no_grad():
            vd.copy_(v)
            gd.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["c"].cpu(), v[:, tri.reshape(-1)])
        assert torch.equal(out["gv"].cpu(), literal_adjoint(g, tri, nv))
