#!/usr/bin/env python3
"""GPU box: stride-2 weight-gradient kernels at the generator's up-convolution and the discriminator's down-convolution
shapes: the polyphase 25-product kernel (SR_WGRAD_S2_WINO=force) against k_wgrad_s2_dma (SR_WGRAD_S2_WINO=0), and the
dword staging (SR_WGRAD_DMA=0).  Means of 20 launches, the modes alternating, `--reps` rounds; TF = direct flops / time.

  bench_wgrad_s2.py [--reps 3] [--dword]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from stylerenderer_amd.op.conv import conv2d_wgrad_mfma  # noqa: E402

dev = "cuda"
MODES = {  # name -> switches
    "s2p": {"SR_WGRAD_S2_WINO": "force", "SR_WGRAD_DMA": "1"},
    "dma": {"SR_WGRAD_S2_WINO": "0", "SR_WGRAD_DMA": "1"},
    "dword": {"SR_WGRAD_S2_WINO": "0", "SR_WGRAD_DMA": "0"},
}


def run(b, c, n, g, tr, modes, reps, iters=20):
    out = 2 * g + 1 if tr else (g - 3) // 2 + 1
    x = torch.randn(b, c, g, g, device=dev)
    gy = torch.randn(b, n, out, out, device=dev)
    xs, gs = torch.randn(b, c, device=dev), torch.randn(b, n, device=dev)
    grid = g if tr else out
    fl = 2.0 * b * grid * grid * c * n * 9
    best = {m: [] for m in modes}
    for _ in range(reps):
        for mode in modes:
            os.environ.update(MODES[mode])
            for _ in range(3):
                conv2d_wgrad_mfma(x, gy, xs, gs, 3, 2, 0, tr)
            torch.cuda.synchronize()
            t = time.time()
            for _ in range(iters):
                conv2d_wgrad_mfma(x, gy, xs, gs, 3, 2, 0, tr)
            torch.cuda.synchronize()
            best[mode].append((time.time() - t) / iters)
    res = ["%s %s ms (%.1f TF)" % (m, "/".join("%.3f" % (dt * 1e3) for dt in best[m]), fl / min(best[m]) / 1e12)
           for m in modes]
    print("B%d C%d N%d grid%d %s work %.2e: %s" % (b, c, n, grid, "convT" if tr else "conv", fl, " | ".join(res)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dword", action="store_true", help="also time the dword staging")
    a = ap.parse_args()
    modes = ["s2p", "dma"] + (["dword"] if a.dword else [])
    shapes = [
        # the headline step's four (batch 16) and their batch-4 forms
        (16, 256, 128, 128, True), (16, 512, 256, 64, True), (16, 512, 512, 32, True), (16, 512, 512, 16, True),
        (4, 256, 128, 128, True), (4, 512, 256, 64, True), (4, 512, 512, 32, True), (4, 512, 512, 16, True),
        # the discriminator's 257^2 -> 128^2 and 129^2 -> 64^2 convolutions
        (4, 128, 256, 257, False), (8, 128, 256, 257, False), (4, 256, 512, 129, False), (8, 256, 512, 129, False),
        # either side of the work bar 6.0e9 (work = 18 B CU CV GH GW = the direct flops)
        (3, 64, 256, 129, False), (2, 512, 512, 16, True), (6, 512, 512, 16, True), (3, 512, 256, 32, True),
        (4, 512, 256, 32, True), (5, 512, 256, 32, True),
    ]
    for s in shapes:
        run(*s, modes, a.reps)


if __name__ == "__main__":
    main()
