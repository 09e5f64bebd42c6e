"""Aligns every picture of a folder by its landmarks (the reference's `utils_face.py --output`, for a landmark file):

    python -m stylerenderer_amd.align_faces --lmk LANDMARKS.txt [--bfm BFM.mat | --template FILE]
        [--size S] [--border reflect] [--gpu 0] [--n_worker 8] [--ext .png] --output DIR PATH

Every image found by dataset.ImgDataset under PATH (sorted by path) for which LANDMARKS.txt lists landmarks
(align.LandmarksReader) is warped onto the canvas so that its landmarks meet the template's (align.alignment_matrix,
op.warp_affine: bilinear, cv2's BORDER_REFLECT by default) and written to DIR under its own basename, in the format its
extension names (--ext .png: under its basename with that extension instead, e.g. lossless output from JPEG sources).  The template is
  * --bfm: the landmark vertices of a Basel Face Model on its mean shape (3-D: scale, roll and translation are fitted),
  * --template: a one-row landmark file in pixels of the S x S canvas,
  * neither: the landmarks of the first readable picture that has any, on a canvas of that picture's shape;
the canvas is S x S with --size, else the shape of that first picture.

--lmk dlib / exec / torch (the reference's detectors) exit with a message: their libraries and weights are not here.
Work split as in prepare_data: a thread pool (at most 16 threads) decodes and encodes, the parent thread warps on
--gpu N, one upload and one launch per run of pictures of one shape; with --gpu -1 the workers warp on the host.  Both
write the same bytes.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import align, dataset
from .prepare_data import MAX_THREADS

SAVE_FORMATS = {".png": "PNG", ".jpg": "JPEG", ".jpeg": "JPEG", ".bmp": "BMP"}


def _save(path, img, quality):
    from PIL import Image

    fmt = SAVE_FORMATS.get(os.path.splitext(path)[1].lower(), "PNG")
    Image.fromarray(img).save(path, format=fmt, **({"quality": quality} if fmt == "JPEG" else {}))


def align_files(aligner, files, output, n_worker=8, gpu=-1, quality=95, ext=None, spent=None):
    """Writes the aligned picture of every file of `files` that has landmarks into `output`.
    Returns (written, without_landmarks, unreadable); a dict given as `spent` receives the seconds of "decode", "warp"
    and "encode", the first and last summed over the worker threads (as is "warp" on the host path)."""
    from .op import warp

    os.makedirs(output, exist_ok=True)
    workers = max(1, min(int(n_worker), MAX_THREADS))
    device = None
    if gpu >= 0:
        import torch

        device = torch.device("cuda", gpu)
    todo = [(f, aligner.matrix(f)) for f in files]
    missing = sum(1 for _, m in todo if m is None)
    todo = [(f, m) for f, m in todo if m is not None]

    spent = {} if spent is None else spent
    spent.update({"decode": 0.0, "warp": 0.0, "encode": 0.0})

    def timed(what, fn, *args):
        t0 = time.perf_counter()
        res = fn(*args)
        spent[what] += time.perf_counter() - t0
        return res

    def load(item):
        path, m = item
        img = timed("decode", dataset.read_image, path)
        if img is None or device is not None:
            return img
        return timed("warp", warp.warp_affine, img, m, aligner.canvas, aligner.border)

    def target(path):
        name = os.path.basename(path)
        return os.path.join(output, name if ext is None else os.path.splitext(name)[0] + ext)

    def device_warp(imgs, mats):
        import torch

        out = [None] * len(imgs)
        groups = {}
        for i, im in enumerate(imgs):
            groups.setdefault(im.shape, []).append(i)
        for idx in groups.values():
            x = torch.from_numpy(np.stack([imgs[i] for i in idx])).to(device)
            y = warp.warp_affine(x, np.stack([mats[i] for i in idx]), aligner.canvas, aligner.border).cpu().numpy()
            for j, i in enumerate(idx):
                out[i] = y[j]
        return out

    written = unreadable = 0
    chunk = 4 * workers
    with ThreadPoolExecutor(workers) as pool:
        for c0 in range(0, len(todo), chunk):
            part = todo[c0:c0 + chunk]
            loaded = list(pool.map(load, part))
            good = [(p, m, r) for (p, m), r in zip(part, loaded) if r is not None]
            unreadable += len(part) - len(good)
            imgs = [r for _, _, r in good]
            if device is not None and good:
                imgs = timed("warp", device_warp, imgs, [m for _, m, _ in good])
            paths = [target(p) for p, _, _ in good]
            list(pool.map(lambda a: timed("encode", _save, a[0], a[1], quality), zip(paths, imgs)))
            written += len(good)
    return written, missing, unreadable


def main(argv=None):
    ap = argparse.ArgumentParser(description="Align faces by landmarks")
    ap.add_argument("--lmk", type=str, required=True, help="landmark .txt file (one picture per line)")
    align.add_arguments(ap, "--size")
    ap.add_argument("--output", type=str, required=True, help="folder for the aligned pictures")
    ap.add_argument("--n_worker", type=int, default=8, help="decode / encode threads (at most %d)" % MAX_THREADS)
    ap.add_argument("--quality", type=int, default=95, help="JPEG quality of .jpg outputs")
    ap.add_argument("--gpu", type=int, default=0, help="device that warps; -1: the host")
    ap.add_argument("--ext", type=str, default="", choices=[""] + sorted(SAVE_FORMATS),
                    help="write every picture under this extension instead of its own")
    ap.add_argument("path", type=str, help="path to image / images folder")
    args = ap.parse_args(argv)
    files = sorted(f for f, _ in dataset.ImgDataset(args.path).imgs)
    aligner = align.aligner_from_args(args.lmk, args.bfm, args.template, args.size, args.border, files,
                                      dataset.read_image)
    written, missing, unreadable = align_files(aligner, files, args.output, args.n_worker, args.gpu, args.quality,
                                                args.ext or None)
    print("aligned %d pictures to %d x %d in %s; %d without landmarks, %d unreadable"
          % (written, aligner.canvas[0], aligner.canvas[1], args.output, missing, unreadable))
    return 0


if __name__ == "__main__":
    sys.exit(main())
