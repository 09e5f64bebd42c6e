"""Perceptual path length throughput on one GPU: stylerenderer_amd.ppl.path_lengths with Generator(256, 512, 8)
(deterministic fill) and the LPIPS VGG16 path, batch 64 pairs, --space w / z, with and without --crop.

    python scripts/bench_ppl.py [--batch 64] [--batches 4] [--warmup 1] [--size 256]

Per configuration: pairs/s over `--batches` timed batches (warm-up batches excluded, torch.cuda.synchronize before and
after), the device time of the phases of a batch from CUDA events (latents = mapping network + k_ppl_endpoints,
generator, distance = k_ppl_prep + trunk + k_lpips_pair), and the distance split into its parts, each timed alone on
the same shapes.  One JSON line per configuration.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("SR_STRICT_NATIVE", "1")
from stylerenderer_amd import lpips, model, ppl, synth  # noqa: E402
from stylerenderer_amd.op import ppl as ppl_op  # noqa: E402


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


def time_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--eps", type=float, default=1e-4)
    args = ap.parse_args()
    dev = "cuda:0"
    g = model.Generator(args.size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(dev).eval()
    percept = lpips.PNetLin().to(dev)
    torch.manual_seed(0)
    for space in ("w", "z"):
        for crop in (False, True):
            ppl.path_lengths(g, percept, args.batch * args.warmup, args.batch, space, args.eps, crop, "end", dev)
            timer = EventTimer()
            n = args.batch * args.batches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = ppl.path_lengths(g, percept, n, args.batch, space, args.eps, crop, "end", dev, timer=timer)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            phases = {k: v / args.batches for k, v in timer.ms().items()}
            # the distance split, each part alone on one batch of this configuration's shapes
            with torch.no_grad():
                x = torch.randn(2 * args.batch, 512, device=dev)
                t = torch.zeros(args.batch, device=dev)
                img, _ = g([g.get_latent(x)], input_is_latent=True)
                h = img.shape[2]
                window = ppl_op.crop_window(h, h, crop)
                size = (256, 256) if window[2] // 256 > 1 else (window[2], window[3])
                sl = percept.scaling_layer
                xin = ppl_op.prep(img, sl.shift, sl.scale, window, size)
                feats = percept.net(xin)
                parts = {
                    "endpoints": time_ms(lambda: ppl_op.pair_endpoints(x, t, space, args.eps)),
                    "prep": time_ms(lambda: ppl_op.prep(img, sl.shift, sl.scale, window, size)),
                    "trunk": time_ms(lambda: percept.net(xin)),
                    "lpips_pair": time_ms(lambda: ppl_op.lpips_pair(feats, percept.lins, args.eps ** 2)),
                }
            batch_ms = sum(phases.values())
            new_ms = parts["endpoints"] + parts["prep"] + parts["lpips_pair"]
            print(json.dumps({
                "config": "ppl_g%d_b%d_%s%s" % (args.size, args.batch, space, "_crop" if crop else ""),
                "pairs_per_s": round(n / wall, 1), "wall_s": round(wall, 3), "finite": bool(torch.isfinite(
                    torch.from_numpy(d)).all()),
                "batch_ms": {k: round(v, 3) for k, v in phases.items()},
                "parts_ms": {k: round(v, 3) for k, v in parts.items()},
                "new_kernels_share": round(new_ms / batch_ms, 4)}), flush=True)


if __name__ == "__main__":
    main()
