"""Inception feature statistics of a dataset — the reference's calc_inception.py on this package:

    python -m stylerenderer_amd.calc_inception [--size 256] [--batch 64] [--n_sample 50000] [--flip] [--gpu 0]
                                               [--inception-weights FILE] [--out FILE] PATH

PATH is a store of prepare_data (LMDB directory, or a directory of key files) read through dataset.py.  Images go
through the reference's transform (optional horizontal flip with p = 0.5, ToTensor, Normalize to [-1, 1]) and the FID
Inception trunk (inception.InceptionV3FID, resized to 299^2 inside).  The output is the reference's pickle
{'mean', 'cov', 'size', 'path'} with float64 mean [2048] and cov [2048, 2048], so the reference's fid.py reads it,
plus 'inception': the trunk that made it ('synthetic' or the SHA-256 of --inception-weights).  Default file name
as the reference: inception_<name of PATH>.pkl in the working directory.

Differences from the reference, on purpose:
  * no DataParallel and no worker processes: one device (--gpu);
  * the first n_sample images are read, not every image followed by a cut to n_sample; the statistics are the same;
  * the features accumulate in inception.FeatureStats (fp64 sum and Gram matrix, on the device for a GPU run)
    instead of being gathered on the host;
  * the flip draws torch.rand(1) per image, not torchvision's RandomHorizontalFlip;
  * the Inception trunk is the deterministic synthetic fill unless --inception-weights names pytorch-fid's weight
    file (stderr says so): such statistics are only comparable with FIDs computed on the same synthetic trunk.
"""
import argparse
import os
import pickle

import numpy as np
import torch

from . import dataset
from . import inception as _inception
from .fid import pick_device, warn_trunk


def flip_transform(flip):
    def apply(img_u8):
        if flip and torch.rand(1).item() < 0.5:
            img_u8 = img_u8[:, ::-1]
        return dataset.to_unit_tensor(img_u8)

    return apply


@torch.no_grad()
def extract_stats(dset, inception, batch, n_sample, device):
    stats = _inception.FeatureStats()
    n = min(n_sample, len(dset))
    for start in range(0, n, batch):
        img = torch.stack([dset[i] for i in range(start, min(start + batch, n))]).to(device)
        stats.update(inception(img).view(img.shape[0], -1))
    return stats


def main(argv=None):
    ap = argparse.ArgumentParser(description="Calculate Inception v3 features for datasets")
    ap.add_argument("--size", type=int, default=256, help="image sizes used for embedding calculation [%(default)d]")
    ap.add_argument("--batch", type=int, default=64, help="batch size for inception networks [%(default)d]")
    ap.add_argument("--n_sample", type=int, default=50000,
                    help="number of samples used for embedding calculation [%(default)d]")
    ap.add_argument("--flip", action="store_true", help="apply random flipping to real images")
    ap.add_argument("--gpu", type=int, default=0, help="use gpu id to test")
    ap.add_argument("--inception-weights", default=None, metavar="FILE",
                    help="pytorch-fid pt_inception-2015-12-05-6726825d.pth for the Inception trunk")
    ap.add_argument("--out", default=None, help="output pickle [inception_<name>.pkl]")
    ap.add_argument("path", metavar="PATH", help="path to datset lmdb file")
    args = ap.parse_args(argv)
    device = pick_device(args.gpu)
    inception = _inception.load_inception(args.inception_weights, device)
    warn_trunk(inception.trunk_name, bool(args.inception_weights))
    dset = dataset.MultiResolutionDataset(args.path, transform=flip_transform(args.flip), resolution=args.size)
    stats = extract_stats(dset, inception, args.batch, args.n_sample, device)
    print("extracted %d features" % stats.count)
    mean, cov = stats.finalize()
    name = os.path.splitext(os.path.basename(os.path.normpath(str(args.path))))[0]
    out = args.out or "inception_%s.pkl" % name
    data = {"mean": np.asarray(mean, np.float64), "cov": np.asarray(cov, np.float64), "size": args.size,
            "path": args.path, "inception": inception.trunk_name}
    with open(out, "wb") as f:
        pickle.dump(data, f)
    return out


if __name__ == "__main__":
    main()
