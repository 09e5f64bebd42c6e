"""GPU: the region kernels (csrc/region.hip) against the host definitions of op.region, byte for byte and bit for bit; the
blend under graph capture; the inverter with mask= / mask_mesh= at 256^2 (exact stationarity, reset, graph against eager)."""
import os

import numpy as np
import pytest
import torch

from stylerenderer_amd import graphs, inversion, lpips, synth
from stylerenderer_amd.op import region
from test_reconstruct_batch_gpu import _faces, _noise
from test_reconstruct_gpu import _big_face, _g256
from test_region_cpu import stationarity

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


# ---- fill ------------------------------------------------------------------------------------------------------------
def fill_case(b, t, h, w, seed):
    """(points float32 [B, 3 T, 2] with fractions on both sides of zero, some outside the picture; tris [T, 3]): small
    triangles scattered over the picture so that many of them leave pixels clear; triangle 0 is a segment, triangle 2 (if
    any) a point, triangle 1 (if any) large with every vertex outside."""
    base = synth.det_uniform((b, t, 1, 2), seed) * np.array([w / 2 + 4, h / 2 + 4]) + np.array([w / 2, h / 2])
    base[:, 0] = (w / 2, h / 2)                                             # triangle 0 lies in the picture
    pts = (base + 3.5 * synth.det_uniform((b, t, 3, 2), seed + 1)).astype(np.float32)
    pts[:, 0, 2] = pts[:, 0, 1]
    if t > 2:
        pts[:, 1] = np.array([[-3.5, -2.5], [w + 4.25, h / 3], [w / 4, h + 6.75]], np.float32)
        pts[:, 2, 1] = pts[:, 2, 2] = pts[:, 2, 0]
    return torch.from_numpy(pts.reshape(b, 3 * t, 2)), torch.arange(3 * t).view(t, 3)


@pytest.mark.parametrize("t", [1, 3, 300])                               # 300: more than one LDS chunk of 256
@pytest.mark.parametrize("hw", [(5, 7), (16, 16), (33, 65)])             # 33 x 65: no multiple of a wave or of 4
def test_fill_equals_the_host_to_the_byte(hw, t):
    for b in (1, 3):
        pts, tris = fill_case(b, t, hw[0], hw[1], 100 + t)
        per = torch.stack([tris.roll(k, 0)[:, [0, 2, 1] if k % 2 else [0, 1, 2]] for k in range(b)])
        for tr in (tris, per):                                              # shared and per-sample
            want = region.fill_triangles(pts, tr, hw)
            got = region.fill_triangles(pts.to(DEV), tr.to(DEV), hw)
            assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (b, 1) + hw
            assert torch.equal(got.cpu(), want), (hw, t, b, tr.dim())
        assert 0 < int(want.sum()) and (t != 1 or int(want.sum()) < want.numel())
    # in a late chunk only: the first 299 triangles miss the picture
    pts, tris = fill_case(1, 300, hw[0], hw[1], 7)
    far = pts.clone()
    far[:, :3 * 299] += 4096.0
    want = region.fill_triangles(far, tris, hw)
    assert torch.equal(region.fill_triangles(far.to(DEV), tris, hw).cpu(), want)
    assert torch.equal(want, region.fill_triangles(pts[:, 3 * 299:], torch.tensor([[0, 1, 2]]), hw))


def test_landmark_region_on_the_device_is_the_hosts():
    lmk = torch.from_numpy(synth.det_uniform((3, 68, 2), 5) * 20 + 32).float()
    conf = torch.ones(3, 68)
    conf[1, :30] = 0
    conf[2] = 0
    for margin in (0, 3, -2):
        want = region.landmark_region(lmk, conf, (64, 72), margin=margin)
        got = region.landmark_region(lmk.to(DEV), conf.to(DEV), (64, 72), margin=margin)
        assert got.is_cuda and torch.equal(got.cpu(), want)
    assert float(want[2].min()) == 1.0 and 0 < float(want[0].mean()) < 1


# ---- grow ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, -1, 3, -3, 32, -32])
def test_grow_equals_the_host_to_the_byte(r):
    h, w = 33, 65
    m = np.zeros((4, 1, h, w), np.uint8)
    m[0, 0] = synth.det_uniform((h, w), 71) > 0.8                           # sparse
    m[1, 0] = synth.det_uniform((h, w), 72) > -0.97                         # nearly full
    m[2, 0, 2, 3] = 1                                                       # one pixel: a dilation by 32 leaves columns clear
    m[3, 0] = 1
    m[3, 0, 30, 62] = 0                                                     # one hole: an erosion by 32 leaves columns set
    want = region.grow(torch.from_numpy(m), r)
    got = region.grow(torch.from_numpy(m).to(DEV), r)
    assert got.is_cuda and torch.equal(got.cpu(), want)
    assert 0 < int(want.sum()) < want.numel()


# ---- blend -----------------------------------------------------------------------------------------------------------
def blend_inputs(shape, seed=0, soft=True):
    b, c, h, w = shape
    t = lambda s, key: torch.from_numpy(synth.det_normal(s, key + seed))   # noqa: E731
    img, target, gy = t(shape, 81), t(shape, 82), t(shape, 83)
    mask = (torch.from_numpy(synth.det_uniform((b, 1, h, w), 84 + seed)) + 1) / 2
    if not soft:
        mask = (mask > 0.5).float()
    mask[:, :, 0, :2] = 0.0
    mask[:, :, -1, -2:] = 1.0
    n = t((b, 3, h, w), 85) * 0.03                                          # n . n on both sides of 1e-3
    n[:, :, :, 0] = 0.0
    return img, target, mask, n, gy


def offset_by_4_bytes(x):
    """The same values in device memory 4 bytes off a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(x.shape)
    out.copy_(x)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def run_blend(img, target, mask, n, gy):
    x = img.detach().requires_grad_(True)
    y, m_eff = region.region_blend(x, target, mask, n)
    if x.is_cuda:
        assert "RegionBlend" in type(y.grad_fn).__name__ and not m_eff.requires_grad
    (gi,) = torch.autograd.grad(y, x, gy)
    return y.detach().cpu(), m_eff.detach().cpu(), gi.cpu()


@pytest.mark.parametrize("shape", [(1, 3, 4, 4), (2, 3, 17, 19), (3, 3, 64, 64), (2, 1, 8, 12)])
def test_blend_equals_the_host_composite_bit_for_bit(shape):
    img, target, mask, n, gy = blend_inputs(shape)
    d = lambda x: x.to(DEV)                                                 # noqa: E731
    view = n.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # the rasterizer's permuted view
    view_d = d(n.permute(0, 2, 3, 1).contiguous()).permute(0, 3, 1, 2)
    assert not view_d.is_contiguous()
    cases = {"no map": (mask, None, None), "map": (mask, n, d(n)), "view": (mask, view, view_d),
             "hard": ((mask > 0.5).float(), n, d(n)), "zero": (torch.zeros_like(mask), n, d(n))}
    for name, (m, n_host, n_dev) in cases.items():
        want = run_blend(img, target, m, n_host, gy)
        got = run_blend(d(img), d(target), d(m), n_dev, d(gy))
        for a, b, what in zip(got, want, ("y", "m_eff", "g_img")):
            assert torch.equal(a, b), (shape, name, what, float((a - b).abs().max()))
        if name == "zero":
            assert torch.equal(got[0], target) and float(got[2].abs().max()) == 0.0
        if name == "map":
            assert 0 < float(want[1].sum()) < float(mask.sum())             # the gate closes some pixels, not all
    # 4 bytes off a 16-byte boundary: the one-pixel-per-lane path, the same bits
    want = run_blend(img, target, mask, n, gy)
    got = run_blend(*(offset_by_4_bytes(d(x)) for x in (img, target, mask, n, gy)))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # one operand misaligned is enough to leave the float4 path
    got = run_blend(d(img), offset_by_4_bytes(d(target)), d(mask), offset_by_4_bytes(d(n)), d(gy))
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_blend_captured_once_follows_its_buffers():
    shape = (2, 3, 32, 32)
    img, target, mask, n, gy = (x.to(DEV) for x in blend_inputs(shape))
    img.requires_grad_(True)
    out = {}

    def body():
        y, m_eff = region.region_blend(img, target, mask, n)
        (gi,) = torch.autograd.grad(y, img, gy)
        out["y"], out["m"], out["g"] = y.detach(), m_eff, gi

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    assert graph.kernel_nodes == 2, graph.kernel_nodes                      # one launch each way
    _, target2, mask2, _, _ = blend_inputs(shape, seed=50, soft=False)
    target.copy_(target2)
    mask.copy_(mask2)
    graph.replay()
    torch.cuda.synchronize()
    first = [out[k].cpu().clone() for k in ("y", "m", "g")]
    want = run_blend(img.detach().cpu(), target2, mask2, n.cpu(), gy.cpu())
    for a, b in zip(first, want):
        assert torch.equal(a, b)
    graph.replay()
    torch.cuda.synchronize()
    for a, k in zip(first, ("y", "m", "g")):
        assert torch.equal(a, out[k].cpu())


def test_float64_on_the_device_takes_the_composite():
    img, target, mask, n, gy = (x.double().to(DEV) for x in blend_inputs((1, 3, 6, 6)))
    y, m = region.region_blend(img, target, mask, n)
    wy, wm = region.region_blend_composite(img.cpu(), target.cpu(), mask.cpu(), n.cpu())
    assert y.dtype == torch.float64 and torch.equal(y.cpu(), wy) and torch.equal(m.cpu(), wm)


@pytest.mark.parametrize("c", [64, 72, 512])
def test_target_features_in_the_layer_kernels_order_give_distance_exactly_zero(c):
    """What exact stationarity on the device rests on: the fused LPIPS layer normalises the render's features in its own
    summation order, so the target's are normalised in that order too when a region is fitted."""
    from stylerenderer_amd.op import lpips_layer

    f = torch.from_numpy(synth.det_normal((2, c, 9, 11), 77 + c)).to(DEV).requires_grad_(True)
    lin = torch.from_numpy(np.abs(synth.det_normal((c,), 78))).to(DEV)
    with torch.no_grad():
        t = lpips_layer.normalize_in_kernel_order(f)
        plain = lpips.normalize_tensor(f)
    assert float((t - plain).abs().max()) <= 2e-7 * float(plain.abs().max())
    d = lpips_layer.lpips_layer(f, t, lin)
    (g,) = torch.autograd.grad(d.sum(), f)
    assert float(d.abs().max()) == 0.0 and float(g.abs().max()) == 0.0


# ---- the inverter at 256^2 -------------------------------------------------------------------------------------------
def _inverter(target, use_graph, shape_reg=1e-3, **kw):
    fm, tri = _big_face(DEV)
    torch.manual_seed(11)
    return inversion.LatentInverter(_g256(), lpips.PNetLin().to(DEV), target, None, lr=0.05, pose_lr=0.01,
                                    noise=_noise(), n_mean_latent=256, use_graph=use_graph, face=(fm, tri),
                                    fit_shape=True, coeff_lr=0.05, shape_reg=shape_reg, **kw)


def _state(inv, hist):
    return [hist.cpu()] + [t.detach().cpu().clone() for t in (inv.w, inv.pose, inv.coeff)] + [inv.mask_fit.cpu().clone()]


def _masks(b):
    m = (torch.from_numpy(synth.det_uniform((b, 1, 256, 256), 91)) + 1) / 2             # soft
    m[:, :, 40:200, 60:190] = 1.0
    m[:, :, :, :30] = 0.0
    return m.to(DEV)


def test_exact_stationarity_on_the_device():
    g = _g256()
    fm, _ = _big_face(DEV)
    with torch.no_grad():
        c = torch.from_numpy(synth.det_normal((1, 144), 8)).to(DEV) * fm.sigma
        w = g.style(torch.from_numpy(synth.det_normal((1, 512), 9)).to(DEV)).unsqueeze(1).repeat(1, g.n_latent, 1)
    state = (w, torch.tensor([0.2, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0], device=DEV), c)
    base = _faces(1)
    make = lambda t, **kw: _inverter(base if t is None else t, False, shape_reg=0.0, **kw)   # noqa: E731
    occluder = (slice(60, 120), slice(130, 200))
    for mask_mesh in (False, True):
        loss_m, grads_m, loss_u, grads_u = stationarity(make, state, occluder, mask_mesh)
        assert loss_m == 0.0 and all(float(x.abs().max()) == 0.0 for x in grads_m), (mask_mesh, loss_m)
        assert loss_u > 0.0 and all(float(x.abs().max()) > 0.0 for x in grads_u)


def test_reset_with_a_mask_equals_a_fresh_inverter_at_batch_2():
    faces = _faces(2)
    other = faces.flip(0).contiguous()
    m_a, m_b = _masks(2), _masks(2).flip(0).flip(3).contiguous()
    inv = _inverter(faces, True, mask=m_a, mask_mesh=True)
    inv.run(8)
    assert inv.graph is not None
    inv.reset(other, mask=m_b)
    got = _state(inv, inv.run(8))
    del inv
    fresh = _inverter(other, True, mask=m_b, mask_mesh=True)
    want = _state(fresh, fresh.run(8))
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert 0 < float(want[4].sum()) < float(m_b.sum())                      # the mesh gate closed part of the mask


@pytest.mark.parametrize("how", ["mask", "mask_mesh", "both"])
def test_captured_run_equals_the_eager_iteration(how):
    faces = _faces(1)
    kw = {"mask": dict(mask=_masks(1)), "mask_mesh": dict(mask_mesh=True), "both": dict(mask=_masks(1), mask_mesh=True)}[how]
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = _inverter(faces, use_graph, **kw)
        runs[key] = _state(inv, inv.run(8))
        assert (inv.graph is not None) == use_graph
        assert torch.equal(inv.image, inv.image) and inv.image.shape == faces.shape
        nodes = inv.graph.kernel_nodes if use_graph else None
        del inv
    assert torch.isfinite(runs["graph"][0]).all()
    for a, b in zip(runs["graph"], runs["eager"]):
        assert torch.equal(a, b), how
    # against the plain step: two launches more, whichever way the region is given
    plain = _inverter(faces, True)
    plain.run(8)
    assert nodes - plain.graph.kernel_nodes == 2, (nodes, plain.graph.kernel_nodes)
    assert os.environ.get("SR_STRICT_NATIVE") == "1"
