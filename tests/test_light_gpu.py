"""GPU: op.light — sr_light_shade_fwd / _bwd against the host float32 composite bit for bit, the light's gradient and the
moments within the bound of the kernels' own summation order on both sides of every boundary of the reduction's layout,
texel attributes bit for bit, the fit, graph capture and strict mode."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from stylerenderer_amd import graphs
from stylerenderer_amd.op import light
from stylerenderer_amd.op._dispatch import native
from test_light_cpu import (attribute_case, bits, design, planted_case, run_composite, run_light_cli,
                            run_light_cli_multiview, sphere_cap)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(1, 1, 1, 1), (1, 3, 5, 7), (3, 3, 16, 16), (2, 1, 33, 65), (1, 3, 8, 260)]
# the reduction's layout: a workgroup takes WG items of GROUP pixels, a lane up to ITEMS of them.  One row of pixels, so
# that items = ceil(W / GROUP): a lane short of one item each, exactly one, one more (the second item of lane 0); one item
# fewer than a workgroup, exactly one, one pixel more (the second partial row holds a single pixel), two full rows; and
# H > 1 with a tail in every row
WG = light.BLOCK * light.ITEMS
LAYOUT = [(1, light.GROUP * (light.BLOCK - 1)), (1, light.GROUP * light.BLOCK), (1, light.GROUP * light.BLOCK + 1),
          (1, light.GROUP * (WG - 1)), (1, light.GROUP * WG), (1, light.GROUP * WG + 1), (1, 2 * light.GROUP * WG),
          (5, light.GROUP * (WG // 4) - 1)]


@pytest.fixture(autouse=True)
def strict(monkeypatch):
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")


def unaligned(t):
    """A contiguous device copy of t that starts past a 16-byte boundary (floats: 4 bytes past; the mask: 1 byte)."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=t.dtype)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    return out


def on_device(tensors, aligned):
    return [t.to(DEV) if aligned else unaligned(t) for t in tensors]


@functools.lru_cache(maxsize=None)
def host(shape, cl, seed=0):
    """The case and the host composite's results, computed once."""
    b_n, c_n, h, w = shape
    a, normals, on, gamma, g, counts = planted_case(b_n, c_n, h, w, cl, seed=seed)
    out, ga, gn, ggamma = run_composite(a, normals, on, gamma, g, -1.0, 0.25)
    un = light.unshade(a, normals, on, gamma, -1.0, 0.3)
    return dict(a=a, normals=normals, on=on, gamma=gamma, g=g, counts=counts, out=out, ga=ga, gn=gn, ggamma=ggamma, un=un)


def exact_sums(terms):
    """(the exact sums over the last axis as float64, sum |term|) of an array [..., n]."""
    t = np.asarray(terms, np.float64)
    flat = t.reshape(-1, t.shape[-1])
    exact = np.array([math.fsum(row) for row in flat]).reshape(t.shape[:-1])
    return exact, np.abs(t).sum(-1)


# ---- 1: bit equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_shade_and_unshade_equal_the_host_composite_bit_for_bit(shape, white, aligned):
    b_n, c_n, h, w = shape
    cl = 1 if white else c_n
    ref = host(shape, cl)
    if h * w >= 6:
        live = ref["on"] & torch.isfinite(ref["normals"]).all(1)
        assert int((~live).sum()) == 3 * b_n and int((ref["normals"] == 0).all(1).sum()) == b_n
    a, normals, on, g = on_device((ref["a"], ref["normals"], ref["on"], ref["g"]), aligned)
    gamma = ref["gamma"].to(DEV)
    out, ga, gn, ggamma = run_composite(a, normals, on, gamma, g, -1.0, 0.25)
    assert out.is_cuda
    for key, got in (("out", out), ("ga", ga), ("gn", gn)):
        assert torch.equal(bits(got), bits(ref[key])), key
    un = light.unshade(a, normals, on, gamma, -1.0, 0.3)
    assert not un.requires_grad and torch.equal(bits(un), bits(ref["un"]))
    dead = ~(ref["on"] & torch.isfinite(ref["normals"]).all(1))
    k = dead.unsqueeze(1).expand(-1, c_n, -1, -1)
    assert torch.equal(bits(un.cpu()[k]), bits(ref["a"][k]))                    # passed through
    # the light's gradient: here only its bound against the host's terms (the layout's boundaries are tested below)
    terms = light.light_terms(ref["a"], ref["normals"], ref["on"], ref["gamma"], ref["g"], -1.0)
    exact, scale = exact_sums(terms.reshape(b_n, cl, 9, -1).numpy())
    n = light.terms_per_lane(h, w) + light.TREE_DEPTH + light.partial_rows(h, w)
    assert (np.abs(ggamma.double().cpu().numpy() - exact) <= n * 2.0 ** -24 * scale).all()
    # the normal's gradient alone and the albedo's alone: the same bits, nothing else computed
    aa = a.detach().requires_grad_(True)
    (only_a,) = torch.autograd.grad(light.shade(aa, normals, on, gamma, -1.0, 0.25), aa, grad_outputs=g)
    assert torch.equal(bits(only_a), bits(ref["ga"]))


def test_strict_refuses_what_the_kernels_do_not_take():
    ref = host((1, 3, 5, 7), 1)
    a, normals, gamma = (ref[k].double().to(DEV) for k in ("a", "normals", "gamma"))
    on = ref["on"].to(DEV)
    with pytest.raises(RuntimeError):
        light.shade(a, normals, on, gamma)
    with pytest.raises(RuntimeError):
        light.unshade(a, normals, on, gamma)
    with pytest.raises(RuntimeError):
        light.moments(a, normals, torch.ones((1, 1, 5, 7), dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError):
        light.texel_attribute(torch.zeros((1, 4, 3), dtype=torch.float64, device=DEV),
                              torch.zeros((1, 3), dtype=torch.int64, device=DEV),
                              torch.zeros((2, 2), dtype=torch.int32, device=DEV), torch.zeros((2, 2, 3), device=DEV))
    with pytest.raises(ValueError):
        light.shade(a.float(), normals.float(), on, ref["gamma"])              # gamma on the host


# ---- 2: the light's gradient and the moments ---------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("cl", [1, 3])
@pytest.mark.parametrize("h,w", LAYOUT)
def test_light_gradient_on_both_sides_of_the_layout_boundaries(h, w, cl, aligned):
    """ggamma against the float64 sum S of the host's float32 terms (the kernel's bit for bit, as ga and gn are).  A lane
    adds its n <= terms_per_lane terms from 0 (n - 1 roundings of partial sums of at most sum_lane |x|), the tree adds the
    lanes in TREE_DEPTH levels and sr_light_reduce the P = partial_rows rows one after the other (P - 1 roundings), every
    level and every row rounding sums that together hold each term once:
    |ggamma - S| <= (terms_per_lane + TREE_DEPTH + P) 2^-24 sum |x| to first order."""
    shape = (2, 3, h, w)
    ref = host(shape, cl, seed=7)
    a, normals, on, g = on_device((ref["a"], ref["normals"], ref["on"], ref["g"]), aligned)
    gamma = ref["gamma"].to(DEV)
    out, ga, gn, ggamma = run_composite(a, normals, on, gamma, g, -1.0, 0.25)
    for key, got in (("out", out), ("ga", ga), ("gn", gn)):
        assert torch.equal(bits(got), bits(ref[key])), key
    terms = light.light_terms(ref["a"], ref["normals"], ref["on"], ref["gamma"], ref["g"], -1.0)
    exact, scale = exact_sums(terms.reshape(2, cl, 9, -1).numpy())
    rows, per_lane = light.partial_rows(h, w), light.terms_per_lane(h, w)
    bound = (per_lane + light.TREE_DEPTH + rows) * 2.0 ** -24 * scale
    err = np.abs(ggamma.double().cpu().numpy() - exact)
    print("H %d W %d Cl %d: %d terms per lane, %d partial rows, largest |ggamma - S| / bound %.3f"
          % (h, w, cl, per_lane, rows, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all() and float(scale.min()) > 0
    again = run_composite(a, normals, on, gamma, g, -1.0, 0.25)
    assert torch.equal(bits(again[3]), bits(ggamma))                            # reruns are bit-identical
    # written into a buffer of the caller's: the same bits, and no gradient through autograd
    buf = torch.full((ggamma.numel() + 3,), float("nan"), device=DEV)
    aa, gg = a.detach().requires_grad_(True), gamma.detach().requires_grad_(True)
    direct = torch.autograd.grad(light.shade(aa, normals, on, gg, -1.0, 0.25, ggamma_out=buf), (aa, gg), grad_outputs=g,
                                 allow_unused=True)
    assert direct[1] is None and torch.equal(bits(direct[0]), bits(ref["ga"]))
    assert torch.equal(bits(buf[:-3]), bits(ggamma.reshape(-1))) and bool(torch.isnan(buf[-3:]).all())
    # an all-off mask gives exactly 0
    off = torch.zeros_like(on)
    dark = run_composite(a, normals, off, gamma, g, -1.0, 0.25)
    assert bool((dark[3] == 0).all()) and bool((dark[1] == 0).all()) and bool((dark[2] == 0).all())
    assert bool((dark[0] == 0.25).all())


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("h,w", LAYOUT)
def test_raw_entries_write_every_element_and_read_nothing_stale(h, w, aligned):
    """Outputs and scratch pre-filled with NaN: every element of out, ga, gn, the scratch's partial rows and ggamma is
    written (the results are the Function's bit for bit and hold no NaN)."""
    cl = 3
    ref = host((2, 3, h, w), cl, seed=7)
    a, normals, on, g = on_device((ref["a"], ref["normals"], ref["on"], ref["g"]), aligned)
    gamma = ref["gamma"].to(DEV)
    nan = float("nan")
    filled = (lambda t: torch.full_like(t, nan)) if aligned else (lambda t: unaligned(torch.full_like(t, nan)))
    out, ga, gn = filled(a), filled(a), filled(normals)
    rows = light.partial_rows(h, w)
    scratch = torch.full((light.scratch_floats(2, cl, h, w),), nan, device=DEV)
    ggamma = torch.full((2, cl, 9), nan, device=DEV)
    run = native(a)
    run.sr_light_shade_fwd(out, a, normals, on, gamma, 2, 3, cl, h, w, -1.0, 0.0, 0.25, 0)
    run.sr_light_shade_bwd(ga, gn, scratch, g, a, normals, on, gamma, 2, 3, cl, h, w, -1.0)
    run.sr_light_reduce(ggamma, scratch, 2, rows, cl * 9, 0)
    assert scratch.numel() == 2 * rows * cl * 9 and not bool(torch.isnan(scratch).any())
    for key, got in (("out", out), ("ga", ga), ("gn", gn)):
        assert torch.equal(bits(got), bits(ref[key])), key
    want = run_composite(a, normals, on, gamma, g, -1.0, 0.25)[3]
    assert torch.equal(bits(ggamma), bits(want))
    mom_scratch = torch.full((2 * rows * 72,), nan, dtype=torch.float64, device=DEV)
    mom = torch.full((2, 72), nan, dtype=torch.float64, device=DEV)
    weight = on.unsqueeze(1).float().contiguous()
    run.sr_light_moments(mom_scratch, a, normals, weight, 2, 3, h, w, -1.0)
    run.sr_light_reduce(mom, mom_scratch, 2, rows, 72, 1)
    assert not bool(torch.isnan(mom_scratch).any())
    assert torch.equal(mom.cpu().view(torch.int64), light.moments(a, normals, weight).cpu().view(torch.int64))


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("c_n", [1, 3])
@pytest.mark.parametrize("h,w", LAYOUT + [(5, 7), (33, 65)])
def test_moments_within_the_bound_of_the_summation_order(h, w, c_n, aligned):
    """The same expression as the light's gradient at u = 2^-53, against the exact sums of the host's float64 terms."""
    ref = host((2, c_n, h, w), 1, seed=7)
    weight = ref["g"][:, :1].contiguous()                                       # about half of the weights not positive
    terms = light.moment_terms(ref["a"], ref["normals"], weight, -1.0)
    exact, scale = exact_sums(terms.reshape(2, 45 + 9 * c_n, -1).numpy())
    a, normals, wd = on_device((ref["a"], ref["normals"], weight), aligned)
    got = light.moments(a, normals, wd, -1.0)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (2, 45 + 9 * c_n)
    n = light.terms_per_lane(h, w) + light.TREE_DEPTH + light.partial_rows(h, w)
    err = np.abs(got.cpu().numpy() - exact)
    bound = n * 2.0 ** -53 * scale
    print("H %d W %d C %d: largest |moments - S| / bound %.3f" % (h, w, c_n, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    assert torch.equal(light.moments(a, normals, wd, -1.0).cpu().view(torch.int64), got.cpu().view(torch.int64))
    assert bool((light.moments(a, normals, torch.zeros_like(wd)) == 0).all())


# ---- 3: texel attributes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b_n", [1, 3])
@pytest.mark.parametrize("n_a", [1, 3, 4])
@pytest.mark.parametrize("size", [(8, 8), (33, 65)])
def test_texel_attribute_equals_the_host(size, n_a, b_n):
    attr, tri, face, coeff, (ty, tx) = attribute_case(size, n_a, b_n)
    want = light.texel_attribute(attr, tri, face, coeff)
    da, dt, df, dc = attr.to(DEV), tri.to(DEV), face.to(DEV), coeff.to(DEV)
    got = light.texel_attribute(da, dt, df, dc)
    assert got.is_cuda and torch.equal(bits(got), bits(want))
    for aligned in (True, False):
        out = torch.full_like(got, float("nan"))
        if not aligned:
            out = unaligned(out)
        native(da).sr_light_texel_attr(out, da, dt, df, dc, b_n, n_a, int(attr.shape[1]), int(tri.shape[0]), *size)
        assert torch.equal(bits(out), bits(want))
        assert bool((out[:, :, df < 0] == 0).all()) and bool((out[:, :, ty, tx] == 0).all())


# ---- 4: the fit ------------------------------------------------------------------------------------------------------
def test_fit_on_the_device_equals_the_host_fit():
    normals, mask = sphere_cap()
    planted = torch.tensor([[[0.9, 0.2, -0.15, 0.4, 0.05, -0.1, 0.08, 0.03, -0.06]]])
    albedo = torch.tensor([-0.2, 0.1, 0.4]).view(1, 3, 1, 1).expand(1, 3, 65, 65).contiguous()
    normals, weight, on = normals.float(), mask.float(), mask[:, 0]
    picture = light.shade(albedo, normals, on, planted, -1.0, -1.0)
    a_design = design(normals.double(), mask)
    cond = np.linalg.cond(a_design.T @ a_design)
    for mono, ridge in ((False, 0.0), (False, 1e-3), (True, 1e-3)):
        # both solve in float64 on the host, from moments that differ by their summation order only: the two float64
        # lights are compared (fit returns them rounded to the picture's float32)
        want = light.solve_light(light.moments(picture, normals, weight).numpy(), 3, mono, ridge)
        got = light.solve_light(light.moments(picture.to(DEV), normals.to(DEV), weight.to(DEV)).cpu().numpy(), 3, mono, ridge)
        tol = 64 * cond * 2.0 ** -53 * float(np.abs(want).max())
        err = float(np.abs(got - want).max())
        print("mono %s ridge %g: |device fit - host fit| %.3g, tolerance %.3g" % (mono, ridge, err, tol))
        assert err <= tol
        fitted = light.fit(picture.to(DEV), normals.to(DEV), weight.to(DEV), mono=mono, ridge=ridge)
        assert fitted.is_cuda and fitted.dtype == torch.float32 and tuple(fitted.shape) == (1, 1 if mono else 3, 9)
        assert torch.equal(fitted.cpu(), torch.from_numpy(got).float())


# ---- 6: command line -------------------------------------------------------------------------------------------------
def _strict_env():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return dict(os.environ, PYTHONPATH=root, SR_STRICT_NATIVE="1")


def test_reconstruct_cli_with_a_light_on_the_device(tmp_path):
    run_light_cli(tmp_path, _strict_env(), size=64, steps=3, more=("--gpu", "0"), without=False)


def test_reconstruct_cli_multiview_with_a_light_on_the_device(tmp_path):
    run_light_cli_multiview(tmp_path, _strict_env(), size=64, steps=3, more=("--gpu", "0"))


# ---- 5: capture ------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward_replay_on_changed_values():
    ref = host((2, 3, 33, 65), 3)
    a, normals, on, gamma, g = (ref[k].to(DEV) for k in ("a", "normals", "on", "gamma", "g"))
    a.requires_grad_(True)
    normals.requires_grad_(True)
    buf = torch.zeros(gamma.numel(), device=DEV)
    out = {}

    def body():
        res = light.shade(a, normals, on, gamma, -1.0, 0.25, ggamma_out=buf)
        ga, gn = torch.autograd.grad(res, (a, normals), grad_outputs=g)
        out.update(res=res.detach(), ga=ga, gn=gn, ggamma=buf)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    print("captured forward + backward: %d kernel nodes of %d" % (graph.kernel_nodes, graph.nodes))
    assert graph.kernel_nodes == 3 and graph.nodes == 3                         # forward, backward, the reduction
    held = dict(out)
    for step in (1, 2):
        with torch.no_grad():
            a.mul_(0.5).add_(0.1 * step)
            gamma.mul_(0.9)
            gamma[:, :, 1] += 0.05 * step
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.clone() for k, t in held.items()}
        body()
        torch.cuda.synchronize()
        for k in got:
            assert torch.equal(bits(got[k]), bits(out[k])), (step, k)
        want = run_composite(a.detach().cpu(), normals.detach().cpu(), on.cpu(), gamma.cpu(), g.cpu(), -1.0, 0.25)
        for k, w in (("res", want[0]), ("ga", want[1]), ("gn", want[2])):
            assert torch.equal(bits(got[k]), bits(w)), (step, k)
