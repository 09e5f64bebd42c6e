"""Fréchet Inception distance of a trained generator — the reference's fid.py on this package:

    python -m stylerenderer_amd.fid --inception STATS.pkl [--truncation 1] [--truncation_mean 4096] [--batch 64]
                                    [--n_sample 50000] [--size 256] [--gpu 0] [--seed S]
                                    [--inception-weights FILE] CHECKPOINT

Same flags, same checkpoint key ('g_ema', else 'g'), the same draws in the same order (`g.mean_latent(truncation_mean)`
first when truncation < 1, then per batch `randn(batch, 512)` and the generator's own noise), the reference's
`calc_fid` on host float64 with scipy.linalg.sqrtm, `fid: <value>` on stdout.  STATS.pkl is the reference's pickle
{'mean', 'cov', 'size', 'path'} (calc_inception.py of either project writes it).

On device tensors the generator, the Inception trunk (inception.InceptionV3FID, csrc/inception.hip) and the feature
statistics (inception.FeatureStats: fp64 sum and Gram matrix on the device) run natively; only the finalised mean and
covariance reach the host.

Differences from the reference, on purpose:
  * no DataParallel: one device (--gpu), the reference's undefined `device` and global `g` are fixed;
  * when n_sample is a multiple of batch the empty trailing batch is skipped (the reference runs a zero-size batch);
  * `extract_feature_from_samples` returns the running statistics, not the [n_sample, 2048] features: the features
    of 50 000 samples are never gathered on the host;
  * the Inception trunk is the deterministic synthetic fill unless --inception-weights names pytorch-fid's
    pt_inception-2015-12-05-6726825d.pth: without it the value is NOT comparable with published FID (stderr says
    so), and a stats file made with a different trunk (its 'inception' key) draws a warning.
"""
import argparse
import contextlib
import pickle
import sys
import time

import numpy as np
import torch
from scipy import linalg

from . import checkpoint
from . import inception as _inception


def batch_sizes(n_sample, batch):
    n_batch = n_sample // batch
    resid = n_sample - n_batch * batch
    return [batch] * n_batch + ([resid] if resid else [])


@torch.no_grad()
def extract_feature_from_samples(generator, inception, truncation, truncation_latent, batch_size, n_sample, device,
                                 timer=None):
    """Samples n_sample images in batches (reference fid.py:15-28) and accumulates their Inception features into a
    FeatureStats.  `timer(phase)` is a context-manager factory called around 'generator', 'inception' and 'stats'
    (scripts/bench_fid.py)."""
    phase = timer or (lambda name: contextlib.nullcontext())
    stats = _inception.FeatureStats()
    for batch in batch_sizes(n_sample, batch_size):
        latent = torch.randn(batch, 512, device=device)
        with phase("generator"):
            img, _ = generator([latent], truncation=truncation, truncation_latent=truncation_latent)
        with phase("inception"):
            feat = inception(img).view(img.shape[0], -1)
        with phase("stats"):
            stats.update(feat)
    return stats


def calc_fid(sample_mean, sample_cov, real_mean, real_cov, eps=1e-6):
    """Reference fid.py:30-45: |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr(sqrtm(S1 S2)), retried with eps I added to both
    covariances when the product's square root is not finite; a significant imaginary part raises."""
    cov_sqrt, _ = linalg.sqrtm(sample_cov @ real_cov, disp=False)
    if not np.isfinite(cov_sqrt).all():
        print("product of cov matrices is singular")
        offset = np.eye(sample_cov.shape[0]) * eps
        cov_sqrt = linalg.sqrtm((sample_cov + offset) @ (real_cov + offset))
    if np.iscomplexobj(cov_sqrt):
        if not np.allclose(np.diagonal(cov_sqrt).imag, 0, atol=1e-3):
            m = np.max(np.abs(cov_sqrt.imag))
            raise ValueError("Imaginary component %f" % m)
        cov_sqrt = cov_sqrt.real
    mean_diff = sample_mean - real_mean
    mean_norm = mean_diff @ mean_diff
    trace = np.trace(sample_cov) + np.trace(real_cov) - 2 * np.trace(cov_sqrt)
    return mean_norm + trace


def warn_trunk(trunk_name, weights_given, stats=None):
    """The stderr warnings of both CLIs: synthetic trunk, and a stats file made with another trunk."""
    if not weights_given:
        sys.stderr.write("warning: no --inception-weights given: the Inception trunk is the deterministic synthetic "
                         "fill, so this value is not comparable with published FID\n")
    if stats is not None:
        theirs = stats.get("inception")
        if theirs is None:
            sys.stderr.write("warning: the statistics file does not name its Inception trunk; this run uses %s\n"
                             % trunk_name)
        elif theirs != trunk_name:
            sys.stderr.write("warning: the statistics file was made with Inception trunk %s, this run uses %s: the "
                             "distance compares different feature spaces\n" % (theirs, trunk_name))


def pick_device(gpu):
    if torch.cuda.is_available() and 0 <= gpu < torch.cuda.device_count():
        return "cuda:%d" % gpu
    return "cpu"


def main(argv=None):
    ap = argparse.ArgumentParser(description="Calculate FID scores")
    ap.add_argument("--truncation", type=float, default=1, help="truncation factor [%(default)f]")
    ap.add_argument("--truncation_mean", type=int, default=4096,
                    help="number of samples to calculate mean for truncation [%(default)d]")
    ap.add_argument("--batch", type=int, default=64, help="batch size for the generator [%(default)d]")
    ap.add_argument("--n_sample", type=int, default=50000, help="number of the samples for calculating FID")
    ap.add_argument("--size", type=int, default=256, help="image sizes for generator [%(default)d]")
    ap.add_argument("--inception", type=str, required=True, help="path to precomputed inception embedding")
    ap.add_argument("--gpu", type=int, default=0, help="use gpu id to test")
    ap.add_argument("--seed", type=int, default=-1, help="random seed for generating images")
    ap.add_argument("--inception-weights", default=None, metavar="FILE",
                    help="pytorch-fid pt_inception-2015-12-05-6726825d.pth for the Inception trunk")
    ap.add_argument("ckpt", metavar="CHECKPOINT", help="path to generator checkpoint")
    args = ap.parse_args(argv)
    if args.seed < 0:
        args.seed = int(time.time())
    torch.manual_seed(args.seed)
    device = pick_device(args.gpu)
    if device != "cpu":
        torch.cuda.manual_seed(args.seed)
    with open(args.inception, "rb") as f:
        embeds = pickle.load(f)
    inception = _inception.load_inception(args.inception_weights, device)
    warn_trunk(inception.trunk_name, bool(args.inception_weights), embeds)
    g = checkpoint.load_generator(args.ckpt, args.size, 512, 8, device=device)
    with torch.no_grad():
        mean_latent = g.mean_latent(args.truncation_mean) if args.truncation < 1 else None
    stats = extract_feature_from_samples(g, inception, args.truncation, mean_latent, args.batch, args.n_sample, device)
    print("extracted %d features" % stats.count)
    sample_mean, sample_cov = stats.finalize()
    fid = calc_fid(sample_mean, sample_cov, embeds["mean"], embeds["cov"])
    print("fid: %f" % fid)
    return fid


if __name__ == "__main__":
    main()
