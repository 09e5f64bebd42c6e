"""Measurements behind profiles/align_notes.md (MI355X host).

    python scripts/bench_align.py kernels [--batch 16] [--reps 200]      warp_affine of a batch, device events
    python scripts/bench_align.py pillow  [--batch 16]                   the same work in Pillow's transform, 16 threads
    python scripts/bench_align.py cli     [--images 64] [--dir DIR]      align_faces to PNG then prepare_data, against
                                                                         prepare_data --align, both with --gpu 0
`kernels` is also the program to put behind `rocprofv3 --kernel-trace --stats --` for the kernel's own time.
"""
import argparse
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylerenderer_amd import align, align_faces, dataset, prepare_data  # noqa: E402
from stylerenderer_amd.op import warp  # noqa: E402

SIZES = (128, 256, 512, 1024)
S = 1024


def rotation(deg, scale=1.0, size=S):
    """Pillow matrix of a rotation about the centre of a size x size picture."""
    c, s = np.cos(np.deg2rad(deg)) * scale, np.sin(np.deg2rad(deg)) * scale
    h = size / 2.0
    return np.array([c, -s, h - c * h + s * h, s, c, h - s * h - c * h])


def source(batch, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(batch, S, S, 3)).astype(np.uint8)


def kernels(args):
    import torch

    x = torch.from_numpy(source(args.batch)).to("cuda:0")
    mats = torch.from_numpy(np.stack([rotation(10.0 + 0.1 * i) for i in range(args.batch)])).to("cuda:0")
    # bytes the algorithm needs: every source byte once (a rotation by 10 degrees reads nearly all of it), every output
    # byte once
    for out, out_bytes in (("u8_hwc", 1), ("f32_chw", 4)):
        for border in ("reflect", "constant"):
            for _ in range(5):
                warp.warp_affine(x, mats, (S, S), border, out=out)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.reps):
                warp.warp_affine(x, mats, (S, S), border, out=out)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / args.reps
            need = args.batch * S * S * 3 * (1 + out_bytes)
            print("device  batch %d  1024^2 -> 1024^2 rot 10  %-8s %-8s %8.4f ms per call (events, allocation included)  "
                  "%7.1f GB/s of %d needed bytes  %8.0f images/s" % (args.batch, border, out, ms, need / ms / 1e6, need,
                                                                     args.batch / ms * 1e3), flush=True)


def pillow(args):
    from PIL import Image

    imgs = [Image.fromarray(a) for a in source(args.batch)]
    mats = [tuple(rotation(10.0 + 0.1 * i)) for i in range(args.batch)]

    def one(i):
        return np.asarray(imgs[i].transform((S, S), Image.AFFINE, mats[i], resample=Image.BILINEAR))

    for threads in (1, 16):
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(one, range(min(threads, args.batch))))
            t0 = time.perf_counter()
            for _ in range(args.pillow_reps):
                list(pool.map(one, range(args.batch)))
            ms = (time.perf_counter() - t0) / args.pillow_reps * 1e3
        print("pillow  batch %d  %2d thread(s)  1024^2 -> 1024^2 rot 10  %8.1f ms per batch  %7.0f images/s" % (
            args.batch, threads, ms, args.batch / ms * 1e3), flush=True)


def cli(args):
    from PIL import Image

    root = args.dir or tempfile.mkdtemp(prefix="align_bench_")
    src = os.path.join(root, "src")
    os.makedirs(src, exist_ok=True)
    rs = np.random.RandomState(1)
    y, x = np.mgrid[0:S, 0:S]
    shape = np.array([[380.0, 400.0], [640.0, 400.0], [512.0, 560.0], [420.0, 700.0], [600.0, 700.0]])
    rows = []
    for i in range(args.images):         # smooth picture plus mild noise: JPEG sizes in the range of photographs
        img = np.stack([(x + 3 * i) % 256, (y * 2 + i) % 256, ((x * y) >> 6) % 256], 2) + rs.randint(-12, 13, (S, S, 3))
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(src, "%05d.jpg" % i), quality=92)
        th, s = rs.uniform(-0.3, 0.3), rs.uniform(0.8, 1.1)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) * s
        pts = (shape - 512.0).dot(R.T) + 512.0 + rs.uniform(-30.0, 30.0, 2)
        rows.append("%05d.jpg " % i + " ".join("%.3f" % v for v in pts.reshape(-1)))
    lmk, tpl = os.path.join(root, "landmarks.txt"), os.path.join(root, "template.txt")
    with open(lmk, "w") as f:
        f.write("\n".join(rows) + "\n")
    with open(tpl, "w") as f:
        f.write("template.png " + " ".join("%.1f" % v for v in shape.reshape(-1)) + "\n")
    files = sorted(f for f, _ in dataset.ImgDataset(src).imgs)

    def report(label, stored, wall, spent):
        busy = spent["decode"] + spent["encode"] + spent["resample"]
        print("cli  %-34s %d images  %6.2f s  %6.1f images/s   thread seconds: decode %.2f resample %.2f encode %.2f "
              "(decode + encode = %.0f %% of them)" % (label, stored, wall, stored / wall, spent["decode"],
                                                      spent["resample"], spent["encode"],
                                                      100 * (spent["decode"] + spent["encode"]) / busy), flush=True)

    for rep in range(2):                 # alternating, twice: the second pass is the warm one
        aligner = align.aligner_from_args(lmk, "", tpl, S, "reflect", files, dataset.read_image)
        aligned = os.path.join(root, "aligned_%d" % rep)
        first = {}
        t0 = time.perf_counter()
        written, _, _ = align_faces.align_files(aligner, files, aligned, 16, 0, ext=".png", spent=first)
        t_align = time.perf_counter() - t0
        stored, _, spent = prepare_data.prepare(prepare_data._DirStore(os.path.join(root, "two_%d" % rep)),
                                                sorted(os.path.join(aligned, n) for n in os.listdir(aligned)), SIZES,
                                                "lanczos", 16, 100, "jpeg", 0)
        print("cli  align_faces --ext .png: %d pictures in %.2f s (thread seconds: decode %.2f warp %.2f encode %.2f); "
              "prepare_data over them: %.2f s" % (written, t_align, first["decode"], first["warp"], first["encode"],
                                                  spent["wall"]), flush=True)
        spent["decode"] += first["decode"]
        spent["resample"] += first["warp"]
        spent["encode"] += first["encode"]
        report("align_faces + prepare_data", stored, t_align + spent["wall"], spent)
        stored, _, spent = prepare_data.prepare(prepare_data._DirStore(os.path.join(root, "one_%d" % rep)), files, SIZES,
                                                "lanczos", 16, 100, "jpeg", 0, aligner=aligner)
        report("prepare_data --align", stored, spent["wall"], spent)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "pillow", "cli"])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--pillow_reps", type=int, default=3)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--dir", type=str, default=None)
    a = ap.parse_args()
    {"kernels": kernels, "pillow": pillow, "cli": cli}[a.what](a)
