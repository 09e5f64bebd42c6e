"""The fused backward of a styled layer's tail that forks into ToRGB (csrc/fused_elem.hip k_fork_nba_bwd, op.fork_tail):
bit for bit what the three entries it replaces compute, at the entry and through the generator; which kernels run with
SR_FORK_TAIL unset and 0; and its memory behaviour under poisoned buffers."""
import itertools
import re

import pytest
import torch

import poison
from util import launched_kernels

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_RGB = 3
SLOPE, GAIN = 0.2, 2 ** 0.5
# (B, C, hw): one chunk; two chunks with a ragged second one (the finish kernels run); three samples, two channel tiles
SHAPES = [(2, 64, 8 * 32), (1, 64, 72 * 64), (3, 128, 16 * 32)]
NOISE = ["sample", "shared", "none"]


def _inputs(b, c, hw, noise_kind, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + 1000 * b + c + hw)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                                                 # noqa: E731
    t = dict(y=r(b, c, hw), g_above=r(b, c, hw), g_rgb=r(b, N_RGB, hw), ws=r(b, N_RGB, c) * 0.1, bias=r(c) * 0.1,
             noise_w=r(1) * 0.3, noise=None)
    if noise_kind != "none":
        t["noise"] = r(b if noise_kind == "sample" else 1, 1, hw)
    return t


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _three_entries(t, b, c, hw, addend, params, rgb_bias):
    """sr_smallconv_dx_add -> sr_smallconv_dw_bias -> sr_noise_bias_act_bwd_dot."""
    from stylerenderer_amd import _lib
    from stylerenderer_amd.op._dispatch import native
    from stylerenderer_amd.op.fused_elem import noise_stride

    L, run = _lib.lib(), native(t["y"])
    gy, gpre, rdot, dws = _nan(b, c, hw), _nan(b, c, hw), _nan(b, c), _nan(b, N_RGB, c)
    gb, gnw = (_nan(c), _nan(1)) if params else (None, None)
    gb_rgb = _nan(N_RGB) if rgb_bias else None
    run.sr_smallconv_dx_add(gy, t["g_rgb"], t["ws"], t["g_above"] if addend else None, b, c, N_RGB, hw)
    run.sr_smallconv_dw_bias(dws, gb_rgb, t["g_rgb"], t["y"], b, c, N_RGB, hw,
                             _nan(L.sr_smallconv_dw_scratch_floats(b, c, N_RGB, hw)))
    run.sr_noise_bias_act_bwd_dot(gpre, gb, gnw, rdot, gy, t["y"], t["noise"], t["noise_w"], t["bias"], SLOPE, GAIN, b, c, hw,
                                  noise_stride(t["noise"], hw), _nan(L.sr_noise_bias_act_bwd_dot_scratch_floats(b, c, hw)))
    return dict(gpre=gpre, gbias=gb, gnoise_w=gnw if t["noise"] is not None else None, rowdot=rdot, dws=dws, gb_rgb=gb_rgb)


def _fused_entry(t, b, c, hw, addend, params, rgb_bias, scratch_fill=float("nan")):
    from stylerenderer_amd import _lib
    from stylerenderer_amd.op._dispatch import native
    from stylerenderer_amd.op.fused_elem import noise_stride

    gpre, rdot, dws = _nan(b, c, hw), _nan(b, c), _nan(b, N_RGB, c)
    gb, gnw = (_nan(c), _nan(1)) if params else (None, None)
    gb_rgb = _nan(N_RGB) if rgb_bias else None
    scratch = torch.full((_lib.lib().sr_fork_nba_bwd_scratch_floats(b, c, N_RGB, hw),), scratch_fill, device=DEV)
    native(t["y"]).sr_fork_nba_bwd(gpre, gb, gnw, rdot, dws, gb_rgb, t["g_above"] if addend else None, t["y"], t["g_rgb"],
                                   t["ws"], t["noise"], t["noise_w"], t["bias"], SLOPE, GAIN, b, c, N_RGB, hw,
                                   noise_stride(t["noise"], hw), scratch)
    return dict(gpre=gpre, gbias=gb, gnoise_w=gnw if t["noise"] is not None else None, rowdot=rdot, dws=dws, gb_rgb=gb_rgb)


@pytest.mark.parametrize("noise_kind", NOISE)
@pytest.mark.parametrize("addend", [True, False], ids=["addend", "no-addend"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entry_equals_the_three_entries_bit_for_bit(shape, addend, noise_kind):
    b, c, hw = shape
    t = _inputs(b, c, hw, noise_kind)
    for params, rgb_bias in itertools.product([True, False], [True, False]):
        want = _three_entries(t, b, c, hw, addend, params, rgb_bias)
        got = _fused_entry(t, b, c, hw, addend, params, rgb_bias)
        again = _fused_entry(t, b, c, hw, addend, params, rgb_bias, scratch_fill=1e30)
        torch.cuda.synchronize()
        for name, w in want.items():
            what = "%s (params %s, rgb bias %s)" % (name, params, rgb_bias)
            assert (w is None) == (got[name] is None), what
            if w is None:
                continue
            assert bool(torch.isfinite(w).all()), "the reference left part of %s unwritten" % what
            assert torch.equal(got[name], w), "%s: %d element(s) differ" % (what, int((got[name] != w).sum()))
            assert torch.equal(again[name], w), "%s: the second run (stale scratch) differs" % what


# ---- through the generator ---------------------------------------------------------------------------------------------
_PAT = {}


def _count(names, base):
    pat = _PAT.setdefault(base, re.compile(r"(?<![A-Za-z0-9_])%s(?![A-Za-z0-9_])" % re.escape(base)))
    return sum(1 for n in names if pat.search(n))


@pytest.fixture(scope="module")
def gen():
    from stylerenderer_amd.model import Generator

    torch.manual_seed(7)
    g = Generator(64, 32, 2, channel_multiplier=1).to(DEV)
    with torch.no_grad():                     # biases, noise strengths start at zero: give every gradient something to do
        for name, p in g.named_parameters():
            if name.endswith("noise.weight") or name.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
    z = torch.randn(2, 32, device=DEV)
    probe = torch.randn(2, 3, 64, 64, device=DEV)
    return g, z, probe


def _nba_layers(g, batch):
    """How many of the stride-1 layers that are followed by a ToRGB head take the conv-NBA path, by the library's query."""
    from stylerenderer_amd import _lib

    x = torch.empty(16, device=DEV)
    count = 0
    for i, conv in enumerate(g.convs[1::2]):
        c, n = conv.conv.in_channel, conv.conv.out_channel
        res = 8 << i
        path = _lib.lib().sr_conv2d_path(batch, c, n, res, res, res, res, 3, 1, 1, 0, _lib.ptr(x), None, None, 0, 1)
        count += int(path == _lib.CONV_PATH_WINO)
    return count


def _first_order(g, z, probe):
    g.zero_grad(set_to_none=True)
    img, _ = g([z], randomize_noise=False)
    (img * probe).sum().backward()
    return img.detach(), {n: (p.grad.clone() if p.grad is not None else None) for n, p in g.named_parameters()}


def _recorded(g, z, probe):
    g.zero_grad(set_to_none=True)
    w = g.get_latent(z).detach().requires_grad_()
    img, _ = g([w], input_is_latent=True, randomize_noise=False)
    gw, = torch.autograd.grad((img * probe).sum(), w, create_graph=True)
    gw.square().sum().backward()
    return img.detach(), {n: (p.grad.clone() if p.grad is not None else None) for n, p in g.named_parameters()}


def _same(a, b):
    img_a, grads_a = a
    img_b, grads_b = b
    assert torch.equal(img_a, img_b), "the image differs"
    assert grads_a.keys() == grads_b.keys()
    some = 0
    for name in grads_a:
        ga, gb = grads_a[name], grads_b[name]
        assert (ga is None) == (gb is None), name
        if ga is not None:
            some += 1
            assert torch.equal(ga, gb), "%s: %d element(s) differ" % (name, int((ga != gb).sum()))
    assert some > 10


def test_generator_gradients_equal_with_and_without_the_combined_node(gen, monkeypatch):
    g, z, probe = gen
    layers = _nba_layers(g, z.shape[0])
    assert layers >= 1, "no layer of this generator takes the conv-NBA path: the test would compare nothing"
    heads = len(g.convs) // 2 + 1
    monkeypatch.delenv("SR_FORK_TAIL", raising=False)
    on, names_on = launched_kernels(lambda: _first_order(g, z, probe))
    monkeypatch.setenv("SR_FORK_TAIL", "0")
    off, names_off = launched_kernels(lambda: _first_order(g, z, probe))
    _same(on, off)
    # switch on: the fused kernel once per conv-NBA layer, whose three kernels are gone; the other heads keep theirs
    assert _count(names_on, "k_fork_nba_bwd") == layers
    assert _count(names_on, "k_smallconv_dw") == heads - layers
    assert _count(names_on, "k_smallconv_dx") == heads - layers
    # switch off: the three kernels of every head and every conv-NBA layer
    assert _count(names_off, "k_fork_nba_bwd") == 0
    assert _count(names_off, "k_smallconv_dw") == heads
    assert _count(names_off, "k_smallconv_dx") == heads
    assert _count(names_off, "k_nba_bwd") - _count(names_on, "k_nba_bwd") == layers
    assert _count(names_off, "k_nba_bwd") >= layers


def test_recorded_backward_takes_the_separate_kernels_under_both_settings(gen, monkeypatch):
    g, z, probe = gen
    assert _nba_layers(g, z.shape[0]) >= 1
    monkeypatch.delenv("SR_FORK_TAIL", raising=False)
    on, names_on = launched_kernels(lambda: _recorded(g, z, probe))
    monkeypatch.setenv("SR_FORK_TAIL", "0")
    off, names_off = launched_kernels(lambda: _recorded(g, z, probe))
    _same(on, off)
    assert _count(names_on, "k_fork_nba_bwd") == 0 and _count(names_off, "k_fork_nba_bwd") == 0
    for base in ("k_smallconv_dx", "k_smallconv_dw", "k_smallconv_fwd", "k_nba_bwd", "k_nba_fwd"):
        assert _count(names_on, base) == _count(names_off, base), base


# ---- poisoned buffers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("addend", [True, False], ids=["addend", "no-addend"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "x".join(map(str, s)))
def test_fused_backward_under_poisoned_buffers(shape, addend, monkeypatch):
    """Every output element written, nothing outside the outputs and the scratch touched, no input modified, and NaN in
    every byte the wrapper allocates (scratch included) changes nothing."""
    from stylerenderer_amd.op.fork_tail import _fused_backward

    b, c, hw = shape
    h = hw // 32
    t = _inputs(b, c, hw, "sample", seed=3)
    view = lambda x: x.view(b, -1, h, 32)                                                                # noqa: E731

    def run(t):
        return _fused_backward(view(t["g_above"]) if addend else None, view(t["g_rgb"]), view(t["y"]), t["ws"],
                               view(t["noise"]), t["noise_w"], t["bias"], SLOPE, GAIN, True, True)

    want = run(t)
    with poison.poisoned(monkeypatch) as log:
        emb = {k: (poison.embed(v) if v is not None else None) for k, v in t.items()}
        got = run(emb)
    assert len(log.entries) >= 7               # six outputs and the scratch
    poison.check(log, list(got), [v for v in emb.values() if v is not None])
    for i, (a, w) in enumerate(zip(got, want)):
        assert torch.equal(a, w), "output %d differs from the plain run" % i
