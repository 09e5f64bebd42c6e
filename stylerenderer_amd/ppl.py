"""Perceptual path length of a trained generator — the reference's ppl.py on this package:

    python -m stylerenderer_amd.ppl --space w [--batch 64] [--n_sample 5000] [--size 256] [--eps 1e-4] [--crop]
                                    [--sampling end|full] [--gpu 0] [--seed S] [--lpips-trunk VGG16.pth] CHECKPOINT

Same flags, same checkpoint keys ('g_ema', else 'g'), same draws in the same order per batch (`g.make_noise()`,
`randn(2B, 512)`, `rand(B)` for --sampling full), same 1st-99th percentile filter, `ppl: <value>` on stdout.

On device tensors the heavy parts are the package's kernels (mapping network, generator, LPIPS VGG16 trunk) and the
glue is csrc/ppl.hip (op/ppl.py): the endpoints of every pair in one launch, the mapping network ONCE on all 2B
endpoints in z space (the reference maps each half separately; the rows are independent), the image crop / resize /
LPIPS scaling in one launch, the trunk ONCE on all 2B images and the per-pair distance from the raw features.  CPU
tensors take the composite torch form of the reference's expressions.

Differences from the reference, on purpose:
  * --space is required (the reference's default None crashes);
  * when n_sample is a multiple of batch the empty trailing batch is skipped (the reference runs a zero-size batch);
  * the N-input iterative `SLerp` Function (reference ppl.py:20-91) is not provided: PPL never calls it;
  * the LPIPS trunk is the deterministic synthetic VGG16 fill unless --lpips-trunk names a torchvision vgg16 (or
    vgg16().features) state dict: without it the value is NOT comparable with published PPL (stderr says so).
"""
import argparse
import contextlib
import sys
import time

import numpy as np
import torch

from . import checkpoint
from . import lpips as _lpips
from .op import ppl as _ppl


def normalize(v, eps=1e-8):
    """The reference's normalize(v, -1, 'L2') forward (layers.py:13-24): v / clamp(|v|, min=eps)."""
    return v / torch.clamp(torch.sqrt(torch.sum(v * v, -1, keepdim=True)), min=eps)


def _native(w, args):
    return (all(x.device.type == "cuda" and x.dtype == torch.float32 for x in (w,) + tuple(args))
            and not (torch.is_grad_enabled() and any(x.requires_grad for x in (w,) + tuple(args))))


def _pair_kernel_ok(w, a, b):
    return a.dim() == 2 and a.shape == b.shape and w.shape == (a.shape[0], 1)


def lerp(w, *args):
    """Reference ppl.py:14-19: w [..., N-1] holds the weights of args[1:] (args[0] gets 1 - sum); w [..., N] is
    L1-normalised.  Device tensors with no gradient (two [B, D] inputs, w [B, 1]) take k_ppl_endpoints, bit-identical."""
    if len(args) == 2 and _native(w, args) and _pair_kernel_ok(w, *args):
        return _ppl.endpoints(args[0].contiguous(), args[1].contiguous(), w, "w", n_ends=1)
    if w.shape[-1] == len(args) - 1:
        w = torch.cat((1 - torch.sum(w, -1, keepdim=True), w), -1)
    else:
        w = w / torch.clamp(torch.sum(w, -1, keepdim=True), min=1e-8)
    return sum([args[i] * w[..., i:i + 1] for i in range(len(args))])


def slerp(w, *args):
    """Reference ppl.py:93-112 for two inputs: spherical interpolation of the L2-normalised inputs at w [..., 1] (or
    w[..., 1:2] / sum(w) for w [..., 2]), no clamp before acos, renormalised."""
    if len(args) != 2:
        raise NotImplementedError("slerp of %d inputs needs the reference's iterative SLerp Function (ppl.py:20-91), "
                                  "which is not provided: perceptual path length only interpolates two" % len(args))
    if w.shape[-1] > 1:
        w = w[..., 1:2] / torch.sum(w, -1, keepdim=True)
    if _native(w, args) and _pair_kernel_ok(w, *args):
        return _ppl.endpoints(args[0].contiguous(), args[1].contiguous(), w, "z", n_ends=1)
    a, b = normalize(args[0]), normalize(args[1])
    ang = torch.acos((a * b).sum(-1, keepdim=True))
    c = torch.sin(ang * (1 - w)) * a + torch.sin(ang * w) * b
    return normalize(c)


def pair_latents(g, inputs, t, space, eps):
    """[2B, D] samples -> [2B, D] latents of the pairs (inputs[::2], inputs[1::2]): row 2i at t[i], row 2i+1 at
    t[i] + eps (reference ppl.py:146-156)."""
    if inputs.device.type == "cuda" and inputs.dtype == torch.float32:
        if space == "w":
            return _ppl.pair_endpoints(g.get_latent(inputs), t, "w", eps)
        return g.get_latent(_ppl.pair_endpoints(inputs, t, "z", eps))
    tc = t[:, None]
    if space == "w":
        latent = g.get_latent(inputs)
        e0 = lerp(tc, latent[::2], latent[1::2])
        e1 = lerp(tc + eps, latent[::2], latent[1::2])
    else:
        e0 = g.get_latent(slerp(tc, inputs[::2], inputs[1::2]))
        e1 = g.get_latent(slerp(tc + eps, inputs[::2], inputs[1::2]))
    return torch.stack([e0, e1], 1).view(*inputs.shape[:1], e0.shape[-1])


def reference_draw(g, batch, sampling, device):
    """One batch of the reference's draws, in its order: noise, the 2B latents, then t."""
    noise = g.make_noise()
    inputs = torch.randn([batch * 2, g.style_dim], device=device)
    t = torch.rand(batch, device=device) if sampling == "full" else torch.zeros(batch, device=device)
    return noise, inputs, t


def batch_sizes(n_sample, batch):
    n_batch = n_sample // batch
    resid = n_sample - n_batch * batch
    return [batch] * n_batch + ([resid] if resid else [])


def path_lengths(g, percept, n_sample, batch, space, eps=1e-4, crop=False, sampling="end", device=None, draw=None,
                 timer=None):
    """Per-pair perceptual path lengths (numpy [n_sample]) of generator `g` under LPIPS `percept` (lpips.PNetLin).
    `draw(g, batch, sampling, device) -> (noise, inputs [2B, D], t [B])` replaces the reference's random draws
    (tests feed fixed inputs); `timer(phase)` is a context-manager factory called around 'latent', 'generator' and
    'distance' (scripts/bench_ppl.py)."""
    if space not in ("z", "w"):
        raise ValueError("space must be 'z' or 'w', got %r" % (space,))
    if device is None:
        device = g.input.input.device
    draw = draw or reference_draw
    phase = timer or (lambda name: contextlib.nullcontext())
    g.eval()
    percept.eval()
    out = []
    with torch.no_grad():
        for b in batch_sizes(n_sample, batch):
            noise, inputs, t = draw(g, b, sampling, device)
            noise = [n.to(device) for n in noise]
            inputs, t = inputs.to(device), t.to(device)
            with phase("latent"):
                latent_e = pair_latents(g, inputs, t, space, eps)
            with phase("generator"):
                image, _ = g([latent_e], input_is_latent=True, noise=noise)
            with phase("distance"):
                dist = percept.pair_distance(image, eps, crop=crop)
            out.append(dist.cpu().numpy())
    return np.concatenate(out, 0) if out else np.zeros(0, np.float32)


def filtered_mean(distances):
    """Reference ppl.py:174-178: the mean of the distances between the 1st (lower) and 99th (higher) percentiles."""
    d = np.asarray(distances)
    lo = np.percentile(d, 1, method="lower")
    hi = np.percentile(d, 99, method="higher")
    return np.extract(np.logical_and(lo <= d, d <= hi), d).mean()


def main(argv=None):
    ap = argparse.ArgumentParser(description="Perceptual Path Length calculator")
    ap.add_argument("--space", choices=["z", "w"], required=True, help="space that PPL calculated with")
    ap.add_argument("--batch", type=int, default=64, help="batch size for the models [%(default)d]")
    ap.add_argument("--n_sample", type=int, default=5000, help="number of the samples for calculating PPL [%(default)d]")
    ap.add_argument("--size", type=int, default=256, help="output image sizes of the generator [%(default)d]")
    ap.add_argument("--eps", type=float, default=1e-4, help="epsilon for numerical stability [%(default)f]")
    ap.add_argument("--crop", action="store_true", help="apply center crop to the images")
    ap.add_argument("--sampling", default="end", choices=["end", "full"], help="set endpoint sampling method")
    ap.add_argument("--gpu", type=int, default=0, help="use gpu id to test")
    ap.add_argument("--seed", type=int, default=-1, help="random seed for sample")
    ap.add_argument("--lpips-trunk", default=None, metavar="PATH",
                    help="torchvision vgg16 (or vgg16().features) state dict for the LPIPS trunk")
    ap.add_argument("ckpt", metavar="CHECKPOINT", help="path to the model checkpoints")
    args = ap.parse_args(argv)
    if args.seed < 0:
        args.seed = int(time.time())
    torch.manual_seed(args.seed)
    if torch.cuda.is_available() and 0 <= args.gpu < torch.cuda.device_count():
        torch.cuda.manual_seed(args.seed)
        device = "cuda:%d" % args.gpu
    else:
        device = "cpu"
    g = checkpoint.load_generator(args.ckpt, args.size, 512, 8, device=device)
    percept = _lpips.PNetLin()
    if args.lpips_trunk:
        percept.net.load_trunk_state_dict(torch.load(args.lpips_trunk, map_location="cpu", weights_only=False))
    else:
        sys.stderr.write("warning: no --lpips-trunk given: the LPIPS VGG16 trunk is the deterministic synthetic fill, "
                         "so this value is not comparable with published PPL\n")
    percept = percept.to(device)
    distances = path_lengths(g, percept, args.n_sample, args.batch, args.space, args.eps, args.crop, args.sampling,
                             device)
    value = filtered_mean(distances)
    print("ppl:", value)
    return value


if __name__ == "__main__":
    main()
