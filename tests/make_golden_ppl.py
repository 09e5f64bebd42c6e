"""TEST INFRASTRUCTURE — writes tests/golden/ppl_interp.npz and tests/golden/ppl_paths.npz by RUNNING THE REFERENCE's
perceptual path length (ppl.py) where the reference sources lie.  Never imported by a test (the reference does not exist
on the GPU machine).  Re-run:  python tests/make_golden_ppl.py

* `lerp` and `slerp` are the reference's own definitions (ppl.py), `normalize` the reference's (utils_3d.py over
  layers.Normalize), extracted from the files and exec'ed.  ppl.py does not parse as shipped, so two syntax repairs are
  applied in memory first: the comma before `for` in SLerp.forward's list comprehension (line 29) and the space + tab
  indentation of slerp's last line (line 118).  Neither touches lerp / two-input slerp.
* The generator is the reference's model.Generator (oracle/ref_shim.py) with the deterministic fill, the distance the
  reference's PNetLin (oracle/make_golden._load_reference_lpips) with the real v0.1 heads and the synthetic trunk, called
  the way PerceptualLoss.forward(pred, target) calls it: model.forward(target, pred).
* The per-batch body restates ppl.py:140-168 (it lives under `if __name__ == "__main__"` and cannot be imported), fed
  with the draws of tests/ppl_cases.det_draw instead of torch's RNG.
* Every path case also runs in float64 (generator, trunk, heads and the interpolation), so the tests can measure the
  reference's own float32 error and set their bars from it (capped at 10x the nominal bar; printed below).
"""
import os
import re
import sys

import numpy as np
import torch
from torch.nn import functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import make_golden  # noqa: E402
import ppl_cases  # noqa: E402
import ref_shim  # noqa: E402
from stylerenderer_amd import lpips as sr_lpips  # noqa: E402

OUT = os.path.join(HERE, "golden")


def reference_ppl_functions(ns):
    """lerp / slerp from the reference's ppl.py, normalize from its utils_3d.py, exec'ed (not restated)."""
    text = open(os.path.join(ref_shim.REF, "ppl.py")).read()
    bad_comma = "min = -1, max = 1)).unsqueeze(-1), \\\n"
    assert bad_comma in text
    text = text.replace(bad_comma, "min = -1, max = 1)).unsqueeze(-1) \\\n")
    bad_indent = "\n \treturn SLerp.apply(w, *args)"
    assert bad_indent in text
    text = text.replace(bad_indent, "\n\t\treturn SLerp.apply(w, *args)")
    text = text.replace("\t", "    ")
    compile(text, "ppl.py", "exec")                  # the repaired file parses
    u3d = open(os.path.join(ref_shim.REF, "utils_3d.py")).read().replace("\t", "    ")
    env = {"torch": torch, "np": np, "F": F, "Normalize": ns.layers.Normalize}
    for name, src in (("normalize", u3d), ("lerp", text), ("slerp", text)):
        m = re.search(r"^def %s\(.*?(?=^def |^class |^if __name__)" % name, src, flags=re.S | re.M)
        exec(m.group(0), env)
    return env


def reference_lpips():
    """The reference's PNetLin: real v0.1 heads, the product's synthetic trunk (the pattern of make_golden.gold_lpips)."""
    ref_lpips, ref_nb = make_golden._load_reference_lpips()
    net = ref_nb.PNetLin(pnet_type="vgg", pnet_rand=True, use_dropout=True, spatial=False, version="0.1", lpips=True)
    heads = torch.load(os.path.join(ref_shim.REF, "lpips", "weights", "v0.1", "vgg.pth"), map_location="cpu")
    missing = net.load_state_dict(heads, strict=False)
    assert not missing.unexpected_keys, missing
    feat = sr_lpips.synthetic_trunk_state()
    for sl in (net.net.slice1, net.net.slice2, net.net.slice3, net.net.slice4, net.net.slice5):
        for idx, layer in sl.named_children():
            if hasattr(layer, "weight"):
                layer.weight.data.copy_(feat[idx + ".weight"])
                layer.bias.data.copy_(feat[idx + ".bias"])
    return net.eval()


def reference_batch(fn, g, net, noise, inputs, t, space, eps, crop):
    """ppl.py:140-168 for one batch (the reference's expressions, in its order)."""
    if space == "w":
        latent = g.get_latent(inputs)
        latent_t0, latent_t1 = latent[::2], latent[1::2]
        latent_e0 = fn["lerp"](t[:, None], latent_t0, latent_t1)
        latent_e1 = fn["lerp"](t[:, None] + eps, latent_t0, latent_t1)
        latent_e = torch.stack([latent_e0, latent_e1], 1).view(*latent.shape)
    else:
        inputs_t0, inputs_t1 = inputs[::2], inputs[1::2]
        latent_t0 = g.get_latent(fn["slerp"](t[:, None], inputs_t0, inputs_t1))
        latent_t1 = g.get_latent(fn["slerp"](t[:, None] + eps, inputs_t0, inputs_t1))
        latent_e = torch.stack([latent_t0, latent_t1], 1).view(*inputs.shape[:1], latent_t0.shape[-1])
    image, _ = g([latent_e], input_is_latent=True, noise=noise)
    if crop:
        c = image.shape[2] // 8
        image = image[:, :, c * 3:c * 7, c * 2:c * 6]
    factor = image.shape[2] // 256
    if factor > 1:
        image = F.interpolate(image, size=(256, 256), mode="bilinear", align_corners=False)
    # PerceptualLoss.forward(pred=image[::2], target=image[1::2]) -> model.forward(target, pred)
    return net(image[1::2], image[::2]).view(image.shape[0] // 2) / (eps * eps)


def reference_path_lengths(fn, g, net, case, dtype):
    size, space, crop, eps, sampling, key = case
    draw = ppl_cases.det_draw(key)
    out = []
    with torch.no_grad():
        for b in ppl_cases.batch_sizes(ppl_cases.N_SAMPLE, ppl_cases.BATCH):
            noise, inputs, t = draw(g, b, sampling, "cpu")
            noise = [n.to(dtype) for n in noise]
            out.append(reference_batch(fn, g, net, noise, inputs.to(dtype), t.to(dtype), space, eps, crop).numpy())
    return np.concatenate(out, 0)


def gold_interp(fn):
    a, b, ts = ppl_cases.interp_inputs()
    arrays = {}
    for tag, t in ts.items():
        arrays["lerp_" + tag] = fn["lerp"](torch.from_numpy(t), torch.from_numpy(a), torch.from_numpy(b)).numpy()
        arrays["slerp_" + tag] = fn["slerp"](torch.from_numpy(t), torch.from_numpy(a), torch.from_numpy(b)).numpy()
    make_golden.save("ppl_interp", **arrays)


def gold_paths(fn, ns):
    net32 = reference_lpips()
    net64 = reference_lpips().double()
    arrays = {}
    for name, case in ppl_cases.PATH_CASES.items():
        g = ppl_cases.make_generator(ns.model.Generator, case[0])
        d32 = reference_path_lengths(fn, g, net32, case, torch.float32)
        d64 = reference_path_lengths(fn, g.double(), net64, case, torch.float64)
        arrays[name + "_f32"], arrays[name + "_f64"] = d32.astype(np.float32), d64
        ref_err = float(np.abs(d32 - d64).max() / np.abs(d64).max())
        nominal = ppl_cases.NOMINAL_BAR[case[3]]
        bar = min(max(nominal, 2 * ref_err), 10 * nominal)
        print("  %-18s reference float32 error %.2e of scale; bar %.1e%s" % (
            name, ref_err, bar, " (widened from %.0e)" % nominal if bar > nominal else ""))
        if 2 * ref_err > 10 * nominal:
            print("  %-18s WARNING: the reference's own float32 error exceeds the 10x cap" % name)
    make_golden.save("ppl_paths", **arrays)


def main():
    torch.manual_seed(0)
    ns = ref_shim.load()
    fn = reference_ppl_functions(ns)
    gold_interp(fn)
    gold_paths(fn, ns)


if __name__ == "__main__":
    main()
