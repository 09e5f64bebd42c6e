"""Transposed (up-sampling) 3x3 stride-2 convolution, launch by launch: the 25-product kernel k_convt_wino
(SR_CONVT_WINO=force) against the 36-product k_convt_fused (SR_CONVT_WINO=0), alternating in ONE session — means of 20
launches (interior + strips), --reps rounds, all shown.  --phases adds the per-phase launches (SR_CONVT_FUSED=0).
work = 18 B C N IH IW, the direct flops: the 25-product kernel's executed rate is its TF x 25/36.

    python scripts/bench_convt.py [--reps 2] [--phases]
    python scripts/bench_convt.py child      # the three headline launches, switches as they stand (for a profiler)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [
    # the generator's three launches at batch 16 (the headline step)
    (16, 256, 128, 128), (16, 512, 256, 64), (16, 512, 512, 32),
    # config[2]: batch 4
    (4, 256, 128, 128), (4, 512, 256, 64), (4, 512, 512, 32),
    # around the bar of the dispatch plan (4.0e10)
    (8, 512, 512, 32), (12, 512, 512, 32), (6, 512, 256, 64), (8, 512, 256, 64), (6, 256, 128, 128), (8, 256, 128, 128),
]


def child():
    """The three launches of the headline step with the switches as they stand (scripts/pmc_sq.sh profiles this)."""
    import time

    import torch
    from stylerenderer_amd.op.conv import conv2d_mfma

    for (b, c, n, res) in SHAPES[:3]:
        x = torch.randn(b, c, res, res, device="cuda")
        wt = torch.randn(9, c, n, device="cuda")
        isc, osc = torch.randn(b, c, device="cuda"), torch.randn(b, n, device="cuda")
        for _ in range(2):
            conv2d_mfma(x, wt, isc, osc, None, 3, 2, 0, True)
        torch.cuda.synchronize()
        t = time.time()
        for _ in range(20):
            conv2d_mfma(x, wt, isc, osc, None, 3, 2, 0, True)
        torch.cuda.synchronize()
        dt = (time.time() - t) / 20
        print("convT B%d C%d N%d res%d: %.3f ms  %.1f TFLOP/s" % (b, c, n, res, dt * 1e3, 18.0 * b * res * res * c * n / dt / 1e12),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--phases", action="store_true")
    args = ap.parse_args()

    import torch
    from stylerenderer_amd import _lib
    from stylerenderer_amd.op.conv import conv2d_mfma

    os.environ["SR_CONVT_TAPS"] = "0"
    modes = [("wino", {"SR_CONVT_WINO": "force", "SR_CONVT_FUSED": "1"}), ("fused", {"SR_CONVT_WINO": "0", "SR_CONVT_FUSED": "1"})]
    if args.phases:
        modes.append(("phases", {"SR_CONVT_WINO": "0", "SR_CONVT_FUSED": "0"}))
    print("| shape (B, C -> N, res) | work | default path | " + " | ".join("%s ms" % m for m, _ in modes) + " | wino / fused |")
    print("|---|---|---|" + "---|" * (len(modes) + 1))
    for (b, c, n, res) in SHAPES:
        x = torch.randn(b, c, res, res, device="cuda")
        wt = torch.randn(9, c, n, device="cuda")
        isc = torch.randn(b, c, device="cuda")
        osc = torch.randn(b, n, device="cuda")
        work = 18.0 * b * c * n * res * res
        for k in ("SR_CONVT_WINO", "SR_CONVT_FUSED"):
            os.environ.pop(k, None)
        path = _lib.lib().sr_conv2d_path(b, c, n, res, res, 2 * res + 1, 2 * res + 1, 3, 2, 0, 1, None, None, None, 0, 1) & 0xFF
        times = {m: [] for m, _ in modes}
        for _ in range(args.reps):
            for m, env in modes:
                os.environ.update(env)
                for _ in range(3):
                    conv2d_mfma(x, wt, isc, osc, None, 3, 2, 0, True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    conv2d_mfma(x, wt, isc, osc, None, 3, 2, 0, True)
                e1.record()
                torch.cuda.synchronize()
                times[m].append(e0.elapsed_time(e1) / 20)
        best = {m: min(v) for m, v in times.items()}
        print("| %d, %d -> %d, %d^2 | %.2e | %d | %s | %.3f |" % (
            b, c, n, res, work, path,
            " | ".join("%s (%.1f TF)" % (" / ".join("%.3f" % t for t in times[m]), work / best[m] / 1e9) for m, _ in modes),
            best["wino"] / best["fused"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    else:
        main()
