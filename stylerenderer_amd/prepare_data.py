"""Builds the multi-resolution image store that `train --data`, `calc_inception` and `fid` read, from a folder of
pictures (reference prepare_data.py):

    python -m stylerenderer_amd.prepare_data --out STORE [--size 128,256,512,1024] [--resample lanczos]
        [--n_worker 8] [--quality 100] [--format jpeg|png|npy] [--gpu 0]
        [--align LANDMARKS.txt [--bfm BFM.mat | --template FILE] [--align_size S] [--border reflect]] PATH

Every image found by dataset.ImgDataset under PATH (sorted by path) is resized so that its shorter side is the target
size, centre cropped to size x size (op.resample.resize_center_crop: torchvision's geometry, Pillow's resampler to the
byte) and stored once per size under dataset.make_key, JPEG quality 100 as in the reference.  The store is an LMDB
environment when `lmdb` imports, else a directory of <key> files; dataset.MultiResolutionDataset reads both.

Work split: a thread pool (at most 16 threads; Pillow releases the GIL while it decodes and encodes) reads and encodes,
the parent thread resamples.  --gpu N resamples on that device with the sr_resample_u8 kernels, one upload per image
(or per run of images of one source shape) for all sizes; --gpu -1 resamples on the host inside the worker threads.
Only this process opens the GPU: there are no worker processes and nothing forks.  Both paths write identical stores.

--align LANDMARKS.txt first warps every picture onto an S x S canvas (S = --align_size, by default the largest --size;
without --bfm / --template and without --align_size: the shape of the first picture, whose landmarks are the template)
on which its landmarks meet the template's, exactly as align_faces does (align.py; template selection as there), and
resamples that canvas: on the device upload -> op.warp_affine -> resize_pyramid on the canvas tensor with nothing read
back in between, on the host the same two steps inside the workers.  It stores what prepare_data stores from
align_faces' lossless output, but decodes every picture once and never writes the aligned intermediates.  Pictures the
landmark file does not list are skipped and counted; the indices stay compact.

Where the reference's tool does something else than it says, this one does what it says:
  * resize_img tests `elif 'area' or 'box' in resample.lower()`, which is always true: whatever --resample names, the
    reference resamples with BOX (NEAREST when the name contains 'near').  Here every name selects its own filter
    (box, bilinear, hamming, bicubic, lanczos); `--resample box` gives what the reference actually computes.
  * `txn.put(key, img)` stands after the loop over sizes: only the LAST size of every image reaches the reference's
    store.  Here every size is stored.
  * an unreadable file leaves a hole in the reference's indices while `length` counts the readable ones only, so the
    last images are never read and a hole raises.  Here the indices are compact over the readable files, in sorted
    order, and the number of skipped files is printed.
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import align, dataset
from .op import resample, warp

MAX_THREADS = 16
FORMATS = {"jpeg": "JPEG", "png": "PNG", "npy": "NPY"}


class _DirStore:
    def __init__(self, path):
        self.path = path
        os.makedirs(path, exist_ok=True)

    def put(self, key, value):
        with open(os.path.join(self.path, key.decode("utf-8")), "wb") as f:
            f.write(value)

    def rename(self, old, new):
        os.replace(os.path.join(self.path, old.decode("utf-8")), os.path.join(self.path, new.decode("utf-8")))

    def close(self):
        pass


class _LmdbStore:
    def __init__(self, path, lmdb):
        self.env = lmdb.open(path, map_size=1024 ** 4, readahead=False)

    def put(self, key, value):
        with self.env.begin(write=True) as txn:
            txn.put(key, value)

    def rename(self, old, new):
        with self.env.begin(write=True) as txn:
            txn.put(new, txn.get(old))
            txn.delete(old)

    def close(self):
        self.env.close()


def open_writer(path):
    try:
        import lmdb
    except ImportError:
        return _DirStore(path)
    return _LmdbStore(path, lmdb)


def _pillow_pyramid(img, sizes, name):
    from PIL import Image

    flt = {"box": Image.BOX, "bilinear": Image.BILINEAR, "hamming": Image.HAMMING, "bicubic": Image.BICUBIC,
           "lanczos": Image.LANCZOS}[name]
    im, out = Image.fromarray(img), {}
    for s in sizes:
        (oh, ow), (top, left, _, _) = resample.center_crop_geometry(img.shape[0], img.shape[1], s)
        out[s] = np.asarray(im.resize((ow, oh), flt).crop((left, top, left + s, top + s)))
    return out


def prepare(writer, files, sizes=(128, 256, 512, 1024), filter="lanczos", n_worker=8, quality=100, fmt="jpeg",
            gpu=-1, host_resampler="numpy", log=None, aligner=None):
    """Writes every size of every readable file of `files` (paths, in the order given) into `writer`; with an
    align.Aligner every file (all of which it must have landmarks for) is first warped onto its canvas.
    Returns (stored, skipped, seconds) with seconds = {"decode", "resample", "encode", "wall"}: decode / encode are
    summed over the worker threads."""
    sizes = [int(s) for s in sizes]
    name = resample._filter(filter)
    workers = max(1, min(int(n_worker), MAX_THREADS))
    enc_fmt = FORMATS[fmt.lower()]
    q = quality if enc_fmt == "JPEG" else None
    device = None
    if gpu >= 0:
        import torch

        device = torch.device("cuda", gpu)
    spent = {"decode": 0.0, "resample": 0.0, "encode": 0.0}

    def timed(what, fn, *args):
        t0 = time.perf_counter()
        res = fn(*args)
        spent[what] += time.perf_counter() - t0       # float += under the GIL: good enough for a share of wall time
        return res

    def host_levels(img):
        if host_resampler == "pillow":
            return _pillow_pyramid(img, sizes, name)
        return resample.resize_pyramid(img, sizes, name)

    def load(path):
        img = timed("decode", dataset.read_image, path)
        if img is None:
            return None
        if aligner is None:
            return img if device is not None else timed("resample", host_levels, img)
        m = aligner.matrix(path)
        if device is not None:
            return img, m
        return timed("resample", lambda: host_levels(warp.warp_affine(img, m, aligner.canvas, aligner.border)))

    def encode(levels):
        return timed("encode", lambda: [dataset.encode_image(np.ascontiguousarray(levels[s]), enc_fmt, q) for s in sizes])

    def device_levels(imgs):
        """[H, W, 3] arrays -> one {size: array} per image; images of one shape share the upload and the launches.
        With an aligner: (array, matrix) pairs, warped to the canvas on the device before the pyramid."""
        import torch

        t0 = time.perf_counter()
        mats = None
        if aligner is not None:
            imgs, mats = [im for im, _ in imgs], [m for _, m in imgs]
        out = [None] * len(imgs)
        groups = {}
        for i, im in enumerate(imgs):
            groups.setdefault(im.shape, []).append(i)
        for idx in groups.values():
            x = torch.from_numpy(np.stack([imgs[i] for i in idx])).to(device)
            if mats is not None:
                x = warp.warp_affine(x, np.stack([mats[i] for i in idx]), aligner.canvas, aligner.border)
            levels = {s: v.cpu().numpy() for s, v in resample.resize_pyramid(x, sizes, name).items()}
            for j, i in enumerate(idx):
                out[i] = {s: levels[s][j] for s in sizes}
        spent["resample"] += time.perf_counter() - t0
        return out

    t_start = time.perf_counter()
    bits_len = len(files)                   # provisional zero padding; fixed up below when the readable count needs less
    stored = skipped = 0
    chunk = 4 * workers
    with ThreadPoolExecutor(workers) as pool:
        for c0 in range(0, len(files), chunk):
            loaded = [r for r in pool.map(load, files[c0:c0 + chunk])]
            good = [r for r in loaded if r is not None]
            skipped += len(loaded) - len(good)
            if device is not None and good:
                good = device_levels(good)
            for payloads in pool.map(encode, good):
                for s, blob in zip(sizes, payloads):
                    writer.put(dataset.make_key(s, stored, bits_len), blob)
                stored += 1
            if log:
                log("%d / %d files" % (min(c0 + chunk, len(files)), len(files)))
    if dataset.index_bits(stored) != dataset.index_bits(bits_len):
        for i in range(stored):
            for s in sizes:
                writer.rename(dataset.make_key(s, i, bits_len), dataset.make_key(s, i, stored))
    writer.put(b"length", str(stored).encode("utf-8"))
    spent["wall"] = time.perf_counter() - t_start
    return stored, skipped, spent


def main(argv=None):
    ap = argparse.ArgumentParser(description="Preprocess images for model training")
    ap.add_argument("--out", type=str, required=True, help="the store to write (LMDB when lmdb imports, else a directory)")
    ap.add_argument("--size", type=str, default="128,256,512,1024", help="resolutions of images for the dataset")
    ap.add_argument("--n_worker", type=int, default=8, help="decode / encode threads (at most %d)" % MAX_THREADS)
    ap.add_argument("--resample", type=str, default="lanczos", help="|".join(sorted(resample.FILTERS)))
    ap.add_argument("--quality", type=int, default=100, help="JPEG quality")
    ap.add_argument("--format", type=str, default="jpeg", choices=sorted(FORMATS))
    ap.add_argument("--gpu", type=int, default=0, help="device that resamples; -1: the host")
    ap.add_argument("--host_resampler", type=str, default="numpy", choices=["numpy", "pillow"],
                    help="with --gpu -1: the integer restatement of this package, or Pillow itself (the same bytes)")
    ap.add_argument("--align", type=str, default="", help="landmark .txt file: align every picture before resampling")
    align.add_arguments(ap, "--align_size")
    ap.add_argument("path", type=str, help="path to the image dataset")
    args = ap.parse_args(argv)
    sizes = []
    for s in args.size.split(","):
        try:
            sizes.append(int(s.strip()))
        except ValueError:
            pass
    if not sizes:
        ap.error("--size names no resolution")
    resample._filter(args.resample)
    print("Make dataset of image sizes:" + ",".join("%d" % s for s in sizes))
    files = sorted(f for f, _ in dataset.ImgDataset(args.path).imgs)
    aligner = None
    if args.align:
        # without a template the first picture gives template AND canvas (its own shape), as in align_faces
        size = args.align_size or (max(sizes) if args.bfm or args.template else 0)
        aligner = align.aligner_from_args(args.align, args.bfm, args.template, size, args.border, files, dataset.read_image)
        listed = [f for f in files if aligner.has(f)]
        print("aligning to %d x %d by %s: %d of %d pictures have landmarks, %d skipped"
              % (aligner.canvas[0], aligner.canvas[1], args.align, len(listed), len(files), len(files) - len(listed)))
        files = listed
    elif args.bfm or args.template or args.align_size:
        ap.error("--bfm, --template and --align_size go with --align")
    writer = open_writer(args.out)
    try:
        stored, skipped, spent = prepare(writer, files, sizes, args.resample, args.n_worker, args.quality, args.format,
                                         args.gpu, args.host_resampler, aligner=aligner)
    finally:
        writer.close()
    wall = spent["wall"]
    print("stored %d images x %d sizes in %s, skipped %d unreadable files; %.1f s (%.1f images/s; thread time: decode "
          "%.1f s, resample %.1f s, encode %.1f s)" % (stored, len(sizes), args.out, skipped, wall,
                                                       stored / wall if wall > 0 else 0.0, spent["decode"],
                                                       spent["resample"], spent["encode"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
