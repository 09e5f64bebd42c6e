"""Adaptive discriminator augmentation (ADA) on one GPU: the native kernels (stylerenderer_amd.op.augment) against
today's composite on device tensors, and the graphed BASELINE config[2] iteration with and without --augment.

    python scripts/bench_augment.py [--reps 50] [--warmup 5] [--iters 20] [--rounds 3] [--skip-trainer]

One JSON line per configuration:
  * ada_b{4,16}_s256: device time per call (CUDA events over --reps calls after --warmup) of
      fwd        draw + sr_ada_params + sr_ada_apply (what utils_3d.augment runs on a device tensor)
      apply      sr_ada_apply alone;  bwd  sr_ada_apply_grad alone
      composite  the composite form (CPU draws and grid, grid_sample + matmul on the device): fwd and fwd + bwd
    the launches per call (counted with torch.profiler), and the ALGORITHMIC bytes of apply / bwd (image in + out,
    3 channels, fp32) over their time, against the 8 TB/s of HBM;
  * graphed_config2_augment: ms per graphed iteration of GeneratorWithMap(256) + Discriminator(256), batch 4, mesh,
    with augment=True (adaptive p) and without, alternated in --rounds rounds of --iters iterations each.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylerenderer_amd import utils_3d as u  # noqa: E402
from stylerenderer_amd.op import augment as ada  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def bench_kernels(b, size, reps, warmup):
    dev = "cuda:0"
    x = torch.rand(b, 3, size, size, device=dev) * 2 - 1
    g = torch.randn_like(x)
    rec = ada.params(ada.draws(b, dev), size, size, 1.0)          # every sample augmented: the kernels' full work
    pose_p, color_p = u._pose2d_sigmas(list(ada.POSE_P)), u._color_sigmas(list(ada.COLOR_P))
    xg = x.clone().requires_grad_(True)

    def composite():
        zp, zc = u._pose2d_draws(b, pose_p), u._color_draws(b, color_p)
        pick = torch.rand(b, 1, 1, 1, device=dev)
        return u._augment_from_draws(xg, zp, zc, pick, 1.0)

    def composite_fb():
        composite().backward(g)

    def native_fb():
        ada.augment(xg, 1.0).backward(g)

    res = {
        "fwd_ms": timed(lambda: ada.augment(x, 1.0), reps, warmup),
        "apply_ms": timed(lambda: ada.apply(x, rec), reps, warmup),
        "bwd_ms": timed(lambda: ada.apply_grad(g, rec), reps, warmup),
        "fwd_bwd_ms": timed(native_fb, reps, warmup),
        "composite_fwd_ms": timed(lambda: composite().detach(), reps, warmup),
        "composite_fwd_bwd_ms": timed(composite_fb, reps, warmup),
    }
    res = {k: round(v, 4) for k, v in res.items()}
    res["launches_fwd"] = launches(lambda: ada.augment(x, 1.0))
    res["launches_bwd"] = launches(lambda: ada.apply_grad(g, rec))
    res["launches_composite_fwd"] = launches(lambda: composite().detach())
    nbytes = 2 * 3 * b * size * size * 4
    for k in ("apply", "bwd"):
        res[k + "_tb_per_s"] = round(nbytes / (res[k + "_ms"] * 1e-3) / 1e12, 3)
        res[k + "_share_of_hbm"] = round(nbytes / (res[k + "_ms"] * 1e-3) / HBM_BYTES_PER_S, 3)
    print(json.dumps({"config": "ada_b%d_s%d" % (b, size), **res}), flush=True)


def bench_trainer(iters, rounds):
    from stylerenderer_amd import graph_train, train

    dev = torch.device("cuda:0")
    faces = train.SyntheticFaceSource(dev, seed=0)
    data = train.SyntheticImages(16, 256, dev)
    trs = {}
    for name, aug in (("plain", False), ("augment", True)):
        trs[name] = graph_train.GraphedTrainer(size=256, latent=512, n_mlp=8, channel_multiplier=2, use_mesh=True,
                                               device=dev, seed=0, batch=4, mesh_vertices=faces.model.dim[2] // 3,
                                               augment=aug)
        for _ in range(3):
            trs[name].step(data.batch(4), faces=faces, log=False)
    times = {k: [] for k in trs}
    for _ in range(rounds):
        for name, tr in trs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                tr.step(data.batch(4), faces=faces, log=False)
            b.record()
            torch.cuda.synchronize()
            times[name].append(round(a.elapsed_time(b) / iters, 3))
    best = {k: min(v) for k, v in times.items()}
    print(json.dumps({"config": "graphed_config2_augment", "ms_per_iter": times,
                      "delta_ms_best": round(best["augment"] - best["plain"], 3),
                      "delta_pct_best": round(100 * (best["augment"] / best["plain"] - 1), 2),
                      "ada_aug_p": trs["augment"].ada_aug_p}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-trainer", action="store_true")
    args = ap.parse_args()
    torch.manual_seed(0)
    for b in (4, 16):
        bench_kernels(b, 256, args.reps, args.warmup)
    if not args.skip_trainer:
        bench_trainer(args.iters, args.rounds)


if __name__ == "__main__":
    main()
