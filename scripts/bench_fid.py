"""Fréchet Inception distance throughput on one GPU: the native FID Inception trunk (stylerenderer_amd.inception) alone,
and the full sampling loop of stylerenderer_amd.fid (Generator(256, 512, 8) with the deterministic fill + Inception +
the fp64 feature statistics).

    python scripts/bench_fid.py [--batch 64] [--batches 8] [--warmup 2] [--size 256]

One JSON line per configuration:
  * inception_b64_s256: images/s of the trunk on [64, 3, 256, 256] inputs (resize to 299^2 included), ms per batch, and
    the share of the fp32-MFMA peak (157.3 TFLOPS) in ALGORITHMIC FLOPs (2 * multiply-adds of every convolution,
    counted from the network's geometry; pools and resize not counted);
  * fid_loop_g256_b64: images/s of extract_feature_from_samples and the device time per batch of its phases
    (generator, inception, stats) from CUDA events.
torch.cuda.synchronize before and after every timed region; warm-up batches excluded.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SR_STRICT_NATIVE", "1")
from stylerenderer_amd import fid, inception, model, synth  # noqa: E402

PEAK_FP32_MFMA = 157.3e12


class EventTimer:
    def __init__(self):
        self.events = {}

    def __call__(self, name):
        timer = self

        class _Ctx:
            def __enter__(self):
                self.a = torch.cuda.Event(enable_timing=True)
                self.a.record()

            def __exit__(self, *exc):
                b = torch.cuda.Event(enable_timing=True)
                b.record()
                timer.events.setdefault(name, []).append((self.a, b))
                return False

        return _Ctx()

    def ms(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.events.items()}


def conv_flops_per_image():
    """2 * sum over convolutions of M * C * kh * kw * OH * OW at a 299^2 input (CPU forward with hooks)."""
    net = inception.InceptionV3FID()
    total, hooks = [0], []
    for mod in net.modules():
        if isinstance(mod, inception.BasicConv2d):
            def hook(m, inp, out):
                w = m.conv.weight
                total[0] += 2 * w.numel() * out.shape[2] * out.shape[3]
            hooks.append(mod.register_forward_hook(hook))
    with torch.no_grad():
        net(torch.zeros(1, 3, 299, 299))
    for h in hooks:
        h.remove()
    return total[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    dev = "cuda:0"
    flops = conv_flops_per_image()
    net = inception.load_inception(None, dev)
    torch.manual_seed(0)
    x = torch.rand(args.batch, 3, args.size, args.size, device=dev) * 2 - 1
    with torch.no_grad():
        for _ in range(args.warmup):
            net(x)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.batches):
            feat = net(x)
        b.record()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    ms = a.elapsed_time(b) / args.batches
    print(json.dumps({
        "config": "inception_b%d_s%d" % (args.batch, args.size),
        "images_per_s": round(args.batch * args.batches / wall, 1), "batch_ms": round(ms, 3),
        "gflop_per_image": round(flops / 1e9, 3),
        "tflops": round(flops * args.batch / (ms * 1e-3) / 1e12, 2),
        "share_of_fp32_mfma_peak": round(flops * args.batch / (ms * 1e-3) / PEAK_FP32_MFMA, 4),
        "finite": bool(torch.isfinite(feat).all())}), flush=True)

    g = model.Generator(args.size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(dev).eval()
    fid.extract_feature_from_samples(g, net, 1, None, args.batch, args.batch * args.warmup, dev)
    timer = EventTimer()
    n = args.batch * args.batches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = fid.extract_feature_from_samples(g, net, 1, None, args.batch, n, dev, timer=timer)
    mean, cov = stats.finalize()
    wall = time.perf_counter() - t0
    phases = {k: round(v / args.batches, 3) for k, v in timer.ms().items()}
    print(json.dumps({
        "config": "fid_loop_g%d_b%d" % (args.size, args.batch),
        "images_per_s": round(n / wall, 1), "wall_s": round(wall, 3), "batch_ms": phases,
        "finite": bool(torch.isfinite(torch.from_numpy(cov)).all())}), flush=True)


if __name__ == "__main__":
    main()
