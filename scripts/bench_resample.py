"""Measurements behind profiles/prepare_data_notes.md (MI355X host).

    python scripts/bench_resample.py kernels [--batch 16] [--reps 20]     the pyramid of a batch, device events
    python scripts/bench_resample.py pillow  [--batch 16]                 the same work in Pillow, 1 and 16 threads
    python scripts/bench_resample.py cli     [--images 96] [--dir DIR]    prepare_data end to end, --gpu 0 against
                                                                          --gpu -1 with Pillow as the host resampler
`kernels` is also the program to put behind `rocprofv3 --kernel-trace --stats --` for per-kernel times.
"""
import argparse
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylerenderer_amd import dataset, prepare_data  # noqa: E402
from stylerenderer_amd.op import resample  # noqa: E402

SIZES = (128, 256, 512, 1024)


def source(batch, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(batch, 1024, 1024, 3)).astype(np.uint8)


def kernels(args):
    import torch

    x = torch.from_numpy(source(args.batch)).to("cuda:0")
    for _ in range(3):
        resample.resize_pyramid(x, SIZES, "lanczos")
    torch.cuda.synchronize()
    for sizes in [SIZES] + [(s,) for s in SIZES]:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            resample.resize_pyramid(x, sizes, "lanczos")
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.reps
        print("device  batch %d  1024^2 -> %-20s %8.3f ms per batch  %9.0f images/s" % (
            args.batch, ",".join(str(s) for s in sizes), ms, args.batch / ms * 1e3), flush=True)


def pillow(args):
    imgs = list(source(args.batch))
    for threads in (1, 16):
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(lambda a: prepare_data._pillow_pyramid(a, SIZES, "lanczos"), imgs[:threads]))
            t0 = time.perf_counter()
            for _ in range(args.pillow_reps):
                list(pool.map(lambda a: prepare_data._pillow_pyramid(a, SIZES, "lanczos"), imgs))
            ms = (time.perf_counter() - t0) / args.pillow_reps * 1e3
        print("pillow  batch %d  %2d thread(s)  1024^2 -> %s  %8.1f ms per batch  %7.0f images/s" % (
            args.batch, threads, ",".join(str(s) for s in SIZES), ms, args.batch / ms * 1e3), flush=True)


def cli(args):
    from PIL import Image

    root = args.dir or tempfile.mkdtemp(prefix="prepare_bench_")
    src = os.path.join(root, "src")
    os.makedirs(src, exist_ok=True)
    rs = np.random.RandomState(1)
    y, x = np.mgrid[0:1024, 0:1024]
    for i in range(args.images):         # smooth picture plus mild noise: JPEG sizes in the range of photographs
        img = np.stack([(x + 3 * i) % 256, (y * 2 + i) % 256, ((x * y) >> 6) % 256], 2) + rs.randint(-12, 13, (1024, 1024, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(src, "%05d.jpg" % i), quality=92)
    files = sorted(f for f, _ in dataset.ImgDataset(src).imgs)
    for label, gpu, host in [("--gpu 0", 0, "numpy"), ("--gpu -1 (Pillow resampler)", -1, "pillow"),
                             ("--gpu 0", 0, "numpy"), ("--gpu -1 (Pillow resampler)", -1, "pillow")]:
        out = os.path.join(root, "store_%s" % ("dev" if gpu >= 0 else "host"))
        stored, skipped, spent = prepare_data.prepare(prepare_data._DirStore(out), files, SIZES, "lanczos", 16, 100,
                                                      "jpeg", gpu, host)
        busy = spent["decode"] + spent["encode"] + spent["resample"]
        print("cli  %-28s %d images  %6.2f s  %6.1f images/s   thread seconds: decode %.2f encode %.2f resample %.2f "
              "(decode + encode = %.0f %% of them)" % (label, stored, spent["wall"], stored / spent["wall"], spent["decode"],
                                                      spent["encode"], spent["resample"],
                                                      100 * (spent["decode"] + spent["encode"]) / busy), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "pillow", "cli"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pillow_reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--dir", type=str, default=None)
    a = ap.parse_args()
    {"kernels": kernels, "pillow": pillow, "cli": cli}[a.what](a)
