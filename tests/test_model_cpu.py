"""CPU: the drop-in model classes against the golden vectors generated from the reference
(BASELINE config 0: the reference's CPU-runnable plumbing case)."""
import numpy as np
import pytest
import torch

from stylerenderer_amd import model, synth
from util import check_grad_samples, rel_err

T = torch.from_numpy


def noise_list(g, key):
    return [T(synth.det_normal((1, 1, 2 ** ((i + 5) // 2), 2 ** ((i + 5) // 2)), key + i))
            for i in range(g.num_layers)]


def test_parameter_counts_and_state_dict_keys():
    # probed on the reference
    g256 = model.Generator(256, 512, 8)
    assert sum(p.numel() for p in g256.parameters()) == 31289268
    assert len(g256.state_dict()) == 165
    assert sum(p.numel() for p in model.Generator(64, 512, 8).parameters()) == 28089380
    assert sum(p.numel() for p in model.GeneratorWithMap(256, 512, 8).parameters()) == 31290709
    assert sum(p.numel() for p in model.Discriminator(256).parameters()) == 28870017
    assert sum(p.numel() for p in model.Discriminator(64).parameters()) == 26493953
    keys = set(g256.state_dict())
    for k in ("style.1.weight", "input.input", "conv1.conv.weight", "conv1.conv.modulation.bias",
              "conv1.noise.weight", "conv1.activate.bias", "to_rgb1.bias", "convs.0.conv.blur.kernel",
              "to_rgbs.0.upsample.kernel", "to_rgbs.11.conv.weight", "noises.noise_12"):
        assert k in keys, k
    blur = g256.state_dict()["convs.0.conv.blur.kernel"]
    assert torch.allclose(blur[0], torch.tensor([.0625, .1875, .1875, .0625]))


def test_state_dict_contract_names_shapes_and_order(golden):
    """tests/golden/state_dict_contract.npz: ordered (name, shape) of the reference's Generator / GeneratorWithMap /
    Discriminator at 256^2 (reference model.py:86-123 with the duplicated to_rgbs tail, :188-223, :296-336) — what a
    checkpoint written by reference train.py:411-420 contains, in the order `load_state_dict(strict=True)` and
    optimizer-state indexing rely on."""
    gold = golden("state_dict_contract")
    for tag, net in (("g", model.Generator(256, 512, 8, channel_multiplier=2)),
                     ("gm", model.GeneratorWithMap(256, 512, 8, channel_multiplier=2)),
                     ("d", model.Discriminator(256, channel_multiplier=2))):
        got = list(net.state_dict().items())
        names = [str(n) for n in gold[tag + "_names"]]
        assert [k for k, _ in got] == names, tag
        for (k, t), row in zip(got, gold[tag + "_shapes"]):
            assert list(t.shape) == [int(x) for x in row[1:1 + int(row[0])]], (tag, k)
        assert [n for n, _ in net.named_parameters()] == [str(n) for n in gold[tag + "_param_names"]], tag
    assert len(gold["g_names"]) == 165


@pytest.fixture(scope="module")
def g8():
    g = model.Generator(8, 64, 2)
    synth.fill_state_dict(g.state_dict(), salt=41)
    return g


def test_generator_s8_forward_variants(golden, g8):
    gold = golden("generator_s8")
    assert int(gold["n_keys"]) == len(g8.state_dict())
    z = T(synth.det_normal((2, 64), 42))
    noise = noise_list(g8, 4300)
    img, lat = g8([z], return_latents=True, noise=noise)
    assert rel_err(lat.detach().numpy(), gold["latent"]) < 1e-5
    assert rel_err(img.detach().numpy(), gold["image"]) < 2e-5
    img2, none = g8([z, T(synth.det_normal((2, 64), 44))], inject_index=1, noise=noise)
    assert none is None and rel_err(img2.detach().numpy(), gold["image_mix"]) < 2e-5
    img3, _ = g8([z], randomize_noise=False)
    assert rel_err(img3.detach().numpy(), gold["image_bufnoise"]) < 2e-5
    img4, _ = g8([z], truncation=0.7, truncation_latent=T(gold["trunc_latent"]), noise=noise)
    assert rel_err(img4.detach().numpy(), gold["image_trunc"]) < 2e-5
    # input_is_latent round trip
    img5, _ = g8([lat.detach()], input_is_latent=True, noise=noise)
    assert rel_err(img5.detach().numpy(), gold["image"]) < 2e-5


def check_grad_digest(named_grads, names, norms, heads, tol):
    assert sorted(named_grads) == list(names)
    for n, want_norm, want_head in zip(names, norms, heads):
        g = named_grads[n]
        got_norm = float(g.double().norm())
        assert abs(got_norm - want_norm) <= tol * max(want_norm, 1e-6), (n, got_norm, want_norm)
        head = g.reshape(-1)[:8].detach().cpu().numpy()
        scale = max(float(np.abs(want_head).max()), want_norm / np.sqrt(g.numel()), 1e-8)
        assert np.abs(head - want_head[:head.size]).max() <= 10 * tol * scale, n


def test_generator_s8_gradients_and_unused_tail(golden, g8):
    gold = golden("generator_s8")
    z = T(synth.det_normal((2, 64), 42))
    img, _ = g8([z], noise=noise_list(g8, 4300))
    proj = T(synth.det_normal(tuple(img.shape), 46))
    params = dict(g8.named_parameters())
    grads = torch.autograd.grad((img * proj).sum(), list(params.values()), allow_unused=True)
    got = {n: g for n, g in zip(params, grads) if g is not None}
    unused = sorted(n for n, g in zip(params, grads) if g is None)
    assert unused == list(gold["unused"])                 # the dead half of to_rgbs
    check_grad_digest(got, gold["grad_names"], gold["grad_norms"], gold["grad_heads"], 1e-4)
    # 256 evenly spaced entries of every gradient tensor (measured 5e-7 of the tensor's scale)
    check_grad_samples(got, gold["grad_names"], gold["grad_samples"], gold["grad_sample_offsets"], 4e-6)


def test_path_length_regulariser_double_backward(golden, g8):
    """Double backward through every layer (reference train.py:118-134 semantics)."""
    gold = golden("generator_s8")
    z = T(synth.det_normal((2, 64), 42))
    img, lat = g8([z], return_latents=True, noise=noise_list(g8, 4300))
    pl_noise = T(synth.det_normal(tuple(img.shape), 47)) / np.sqrt(img.shape[2] * img.shape[3])
    (gl,) = torch.autograd.grad((img * pl_noise).sum(), lat, create_graph=True)
    flat = gl.reshape(gl.shape[0], -1)
    lengths = torch.sqrt((flat * flat).sum(1))
    assert rel_err(lengths.detach().numpy(), gold["pl_lengths"]) < 1e-4
    mean = 0.01 * lengths.mean()
    penalty = (lengths - mean).pow(2).mean()
    assert abs(float(penalty) - float(gold["pl_penalty"])) < 1e-4 * float(gold["pl_penalty"])
    g8.zero_grad()
    penalty.backward()
    got = {n: p.grad for n, p in g8.named_parameters() if p.grad is not None}
    check_grad_digest(got, gold["pl_grad_names"], gold["pl_grad_norms"], gold["pl_grad_heads"], 1e-3)
    check_grad_samples(got, gold["pl_grad_names"], gold["pl_grad_samples"], gold["pl_grad_sample_offsets"], 4e-5)
    g8.zero_grad()


def test_generator_s64_plumbing(golden):
    """BASELINE config 0: 64x64 generator on CPU; image equals the reference's."""
    gold = golden("generator_s64")
    g = model.Generator(64, 512, 8)
    assert sum(p.numel() for p in g.parameters()) == int(gold["n_params"])
    assert len(g.state_dict()) == int(gold["n_keys"])
    synth.fill_state_dict(g.state_dict(), salt=41)
    with torch.no_grad():
        img, lat = g([T(synth.det_normal((1, 512), 42))], return_latents=True, noise=noise_list(g, 4300))
    assert rel_err(lat.numpy(), gold["latent"]) < 1e-5
    assert rel_err(img.numpy(), gold["image"]) < 5e-5


def test_discriminator_s16(golden):
    gold = golden("discriminator_s16")
    d = model.Discriminator(16)
    assert sum(p.numel() for p in d.parameters()) == int(gold["n_params"])
    synth.fill_state_dict(d.state_dict(), salt=61)
    x = T(gold["x"]).requires_grad_()
    y = d(x)
    assert rel_err(y.detach().numpy(), gold["y"]) < 2e-5
    (gx,) = torch.autograd.grad(y.sum(), x, create_graph=True)
    assert rel_err(gx.detach().numpy(), gold["gx"]) < 5e-5
    r1 = (gx * gx).reshape(4, -1).sum(1).mean()
    assert abs(float(r1) - float(gold["r1"])) < 1e-4 * float(gold["r1"])
    d.zero_grad()
    r1.backward()
    got = {n: p.grad for n, p in d.named_parameters() if p.grad is not None}
    check_grad_digest(got, gold["r1_grad_names"], gold["r1_grad_norms"], gold["r1_grad_heads"], 1e-3)
    # measured against the exact (float64) values: the R1 bias gradients cancel, and a float32 CPU build other than
    # the fixture's (another convolution ISA or thread count) lands as far from the exact value as the reference does
    check_grad_samples(got, gold["r1_grad_names"], gold["r1_grad_samples"], gold["r1_grad_sample_offsets"], 4e-6,
                       truth=gold["r1_grad_samples_f64"])
    # the same formulation in float64 is the exact value itself
    d64 = d.double()
    x64 = T(gold["x"]).double().requires_grad_()
    (gx64,) = torch.autograd.grad(d64(x64).sum(), x64, create_graph=True)
    d64.zero_grad()
    (gx64 * gx64).reshape(4, -1).sum(1).mean().backward()
    got64 = {n: p.grad for n, p in d64.named_parameters() if p.grad is not None}
    check_grad_samples(got64, gold["r1_grad_names"], gold["r1_grad_samples_f64"], gold["r1_grad_sample_offsets"], 1e-9)


def test_discriminator_s64_vs_reference(golden):
    """N1 on CPU tensors at 64^2 (tests/golden/discriminator_s64.npz): logits, first-order gradients, weighted R1 double
    backward, and the kink records themselves (per-channel positive counts of every LeakyReLU equal the
    reference's)."""
    from util import run_discriminator_case

    meas = run_discriminator_case(golden("discriminator_s64"), 64, "cpu", 2e-5, 2e-5, 5e-5)
    print(meas)
    assert meas["forced"] == 0, meas


def test_generator_with_map_s16_gradients_vs_reference(golden):
    """M7 on CPU tensors: image, normal maps, parameter / mesh gradients and the path-length regulariser over
    [latents] + normal maps (reference model.py:224-295, train.py:118-134, 340-347)."""
    from util import run_generator_with_map_case

    meas = run_generator_with_map_case(golden("generator_map_s16"), 16, "cpu", 5e-5, 1e-5, 1e-4, 2e-5, 2e-4)
    print(meas)


def test_generic_geometry_layers_cpu_vs_reference(golden):
    """The CPU formulation of ModulatedConv2d (kernel_size 5 / 7; plain, up-sampling incl. the cropping blur,
    down-sampling, no demodulation) and EqualConv2d at geometries outside the matrix-core set against the reference's
    layers (tests/golden/conv_generic.npz, oracle/make_golden.gold_conv_generic)."""
    from stylerenderer_amd import layers

    T = torch.from_numpy
    gold = golden("conv_generic")
    for tag, kw in [("m5", dict(kernel_size=5)), ("m5up", dict(kernel_size=5, upsample=True)),
                    ("m5down", dict(kernel_size=5, downsample=True)), ("m7up", dict(kernel_size=7, upsample=True)),
                    ("m5nodemod", dict(kernel_size=5, demodulate=False))]:
        m = layers.ModulatedConv2d(in_channel=8, out_channel=12, style_dim=16, **kw)
        synth.fill_state_dict(m.state_dict(), salt=35)
        x, s = T(synth.det_normal((2, 8, 10, 10), 36)).requires_grad_(), T(synth.det_normal((2, 16), 37)).requires_grad_()
        y = m(x, s)
        assert rel_err(y.detach().numpy(), gold[tag + "_y"]) < 2e-6, tag
        grads = torch.autograd.grad(y, [x, s, m.weight, m.modulation.weight, m.modulation.bias],
                                    T(synth.det_normal(tuple(y.shape), 38)))
        for a, k in zip(grads, ("gx", "gs", "gw", "gmw", "gmb")):
            assert rel_err(a.numpy(), gold[tag + "_" + k]) < 5e-6, (tag, k)
    for tag, (k, st, pd) in [("e5", (5, 1, 2)), ("e4s2", (4, 2, 1)), ("e3p0", (3, 1, 0)), ("e2s3", (2, 3, 0))]:
        m = layers.EqualConv2d(6, 10, k, stride=st, padding=pd)
        synth.fill_state_dict(m.state_dict(), salt=39)
        x = T(synth.det_normal((3, 6, 11, 13), 40)).requires_grad_()
        y = m(x)
        assert rel_err(y.detach().numpy(), gold[tag + "_y"]) < 2e-6, tag
        grads = torch.autograd.grad(y, [x, m.weight, m.bias], T(synth.det_normal(tuple(y.shape), 41)))
        for a, kk in zip(grads, ("gx", "gw", "gb")):
            assert rel_err(a.numpy(), gold[tag + "_" + kk]) < 2e-6, (tag, kk)
