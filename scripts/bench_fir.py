"""Blur (4x4 FIR, up = down = 1) after the up-sampling convolutions: time and HBM GB/s per shape (algorithmic bytes).

  bench_fir.py             the plain blur and the tail backward (two kernels against one pass), this process
  bench_fir.py --tail      blur + noise + bias + LeakyReLU and its one-pass backward on the six up-sampling layers of
                           Generator(256) at batch 16, this process (band or tiled kernels as SR_FIR_BAND says), one JSON line
  bench_fir.py --ab [N]    --tail in child processes, SR_FIR_BAND=0 and 1 alternating, N of each (default 2); a table of
                           the per-shape kernel times (the switch is read once per process, hence processes)"""
import json, os, subprocess, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEP_SHAPES = ((16, 128, 256), (16, 256, 128), (16, 512, 64), (16, 512, 32), (16, 512, 16), (16, 512, 8))   # b, c, 2^k side


def kernel_us(fn, reps=20, warm=3):
    """Device time of the kernels one fn() launches, in microseconds: the profiler's kernel durations summed over `reps`
    calls, per call (the host's gaps between short kernels are not in it, as they are in an event pair around a call)."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(e.time_range.elapsed_us() for e in dev) / reps


def tail():
    from stylerenderer_amd.op import conv as cv
    from stylerenderer_amd.op.fused_elem import blur_noise_bias_act
    from stylerenderer_amd.op.upfirdn2d import flipped
    k1 = torch.tensor([1., 3., 3., 1.])
    k = (k1[:, None] * k1[None, :]); k = (k / k.sum() * 4).to("cuda")
    kf = flipped(k)
    res = {}
    for (b, c, oh) in STEP_SHAPES:
        x = torch.randn(b, c, oh + 1, oh + 1, device="cuda")
        gy = torch.randn(b, c, oh, oh, device="cuda")
        noise, nw, ab = torch.randn(b, 1, oh, oh, device="cuda"), torch.randn(1, device="cuda"), torch.randn(c, device="cuda")
        with torch.no_grad():
            y = blur_noise_bias_act(x, k, (1, 1), noise, nw, ab)
            fwd = kernel_us(lambda: blur_noise_bias_act(x, k, (1, 1), noise, nw, ab))
            bwd = kernel_us(lambda: cv._blur_nba_bwd(gy, y, kf, 1, tuple(x.shape), noise, nw, ab, 0.2, 2 ** 0.5, True))
        res[str(oh)] = {"fwd_us": fwd, "bwd_us": bwd, "fwd_bytes": (x.numel() + y.numel()) * 4,
                        "bwd_bytes": (2 * y.numel() + x.numel()) * 4}
        del x, gy, y
    print("FIR_TAIL " + json.dumps({"band": os.environ.get("SR_FIR_BAND", "1") != "0", "shapes": res}), flush=True)


def ab(n):
    runs = {False: [], True: []}
    for i in range(2 * n):
        on = bool(i % 2)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--tail"], env=dict(os.environ, SR_FIR_BAND=str(int(on))),
                             capture_output=True, text=True, timeout=600)
        line = [l for l in out.stdout.splitlines() if l.startswith("FIR_TAIL ")]
        if out.returncode != 0 or not line:
            sys.exit("bench_fir --tail failed (exit %d): %s" % (out.returncode, out.stderr[-2000:]))
        runs[on].append(json.loads(line[0][9:])["shapes"])
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    print("| 2^k side | pass | tiled us (runs) | band us (runs) | tiled TB/s | band TB/s | x |")
    print("|---|---|---|---|---|---|---|")
    for (_, _, oh) in STEP_SHAPES:
        for p in ("fwd", "bwd"):
            t = [r[str(oh)][p + "_us"] for r in runs[False]]
            u = [r[str(oh)][p + "_us"] for r in runs[True]]
            byt = runs[False][0][str(oh)][p + "_bytes"]
            print("| %d | %s | %.1f (%s) | %.1f (%s) | %.2f | %.2f | %.2f |" % (
                oh, p, med(t), " ".join("%.1f" % v for v in t), med(u), " ".join("%.1f" % v for v in u),
                byt / med(t) / 1e6, byt / med(u) / 1e6, med(t) / med(u)), flush=True)


if "--tail" in sys.argv:
    tail()
    sys.exit(0)
if "--ab" in sys.argv:
    i = sys.argv.index("--ab")
    ab(int(sys.argv[i + 1]) if len(sys.argv) > i + 1 else 2)
    sys.exit(0)

from stylerenderer_amd.op.upfirdn2d import upfirdn2d
dev = "cuda"
k1 = torch.tensor([1., 3., 3., 1.])
k = (k1[:, None] * k1[None, :]); k = (k / k.sum() * 4).to(dev)
for (b, c, res) in ((16, 128, 257), (16, 256, 129), (16, 512, 65), (16, 128, 255)):
    x = torch.randn(b, c, res, res, device=dev)
    pad = (1, 1) if res % 2 else (2, 2)
    for _ in range(3): y = upfirdn2d(x, k, pad=pad)
    torch.cuda.synchronize(); t = time.time()
    for _ in range(20): y = upfirdn2d(x, k, pad=pad)
    torch.cuda.synchronize(); dt = (time.time() - t) / 20
    byt = (x.numel() + y.numel()) * 4
    print("fir4 B%d C%d %d^2 -> %d^2: %.1f us  %.0f GB/s  checksum %.6e" % (b, c, res, y.shape[-1], dt * 1e6, byt / dt / 1e9, y.double().sum().item()), flush=True)

# ---- backward of the up-sampling layer's tail: two kernels (k_nba_bwd<true> + k_fir4_tile<false>) vs k_fir4_nba_bwd
from stylerenderer_amd.op import conv as cv  # noqa: E402
from stylerenderer_amd.op.upfirdn2d import flipped, upfirdn2d_op  # noqa: E402


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(); t = time.time()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.time() - t) / reps


for (b, c, oh) in ((16, 128, 256), (16, 256, 128), (16, 512, 64), (4, 128, 256)):
    gy, out = torch.randn(b, c, oh, oh, device=dev), torch.randn(b, c, oh, oh, device=dev)
    noise, nw, ab = torch.randn(b, 1, oh, oh, device=dev), torch.randn(1, device=dev), torch.randn(c, device=dev)
    shape257 = (b, c, oh + 1, oh + 1)
    kf = flipped(k)

    def two():
        gm, gb, gnw, rd = cv._nba_bwd_dot(gy, out, noise, nw, ab, 0.2, 2 ** 0.5, True)
        return upfirdn2d_op(gm.reshape(-1, oh, oh, 1), kf, 1, 1, 1, 1, 2, 2, 2, 2)

    def one():
        return cv._blur_nba_bwd(gy, out, kf, 1, shape257, noise, nw, ab, 0.2, 2 ** 0.5, True)[0]

    t2, t1 = timeit(two), timeit(one)
    alg = (2 * gy.numel() + (oh + 1) ** 2 * b * c) * 4
    print("tail bwd B%d C%d %d^2: two kernels %.1f us, one pass %.1f us (%.0f GB/s of its 3 tensors)  x%.2f" % (
        b, c, oh, t2 * 1e6, t1 * 1e6, alg / t1 / 1e9, t2 / t1), flush=True)
