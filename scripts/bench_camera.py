"""The perspective camera in face reconstruction on one GPU, for profiles/reconstruct_camera_notes.md.  One measurement
per invocation, so that each runs under its own time limit:

    timeout 300 python scripts/bench_camera.py --batch 1 [--steps 50] [--rounds 7] [--configs off,fixed,fitted]
    timeout 300 python scripts/bench_camera.py --batch 8
    timeout 300 python scripts/bench_camera.py --batch 1 --configs off            # also runs on a commit without op.camera

The fit-shape inversion of profiles/reconstruct_batch_notes.md (GeneratorWithMap(256), the face-sized synthetic 3DMM,
nv = 24 770, d = 80 + 64, the LPIPS trunk) at batch B with the camera off (camera=None), fixed (camera=0.3) and fitted
(camera=0.3, fit_camera=True).  All inverters live in one process; after the warm-up and capture of each, the rounds
alternate between them; per configuration the median round counts and the rounds' minimum and maximum are its spread.
Replayed steps/s (one replay of the captured graph is one step of all B images), the ratios to `off` and the kernel nodes
of each captured step.  `--configs off` alone is what is run on the parent commit for the cost of the option when unused.

For the kernels' own times, the same command with one configuration under a kernel trace, in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o cam -- python scripts/bench_camera.py --batch 1 --configs fitted --rounds 2

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stylerenderer_amd import inversion, lpips, model, synth, train  # noqa: E402
from stylerenderer_amd.op import morph  # noqa: E402

DEV = torch.device("cuda:0")
CONFIGS = {"off": {}, "fixed": {"camera": 0.3}, "fitted": {"camera": 0.3, "fit_camera": True}}


def bench(size, batch, steps, rounds, names):
    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(DEV)
    src = train.SyntheticFaceSource(DEV)
    fm, tri = src.model, src.tri
    net = lpips.PNetLin().to(DEV)
    noise = [torch.from_numpy(synth.det_normal(tuple(n.shape), 300 + i)).to(DEV) for i, n in enumerate(g.make_noise())]
    with torch.no_grad():
        ims = []
        for k in range(batch):
            c_true = torch.from_numpy(synth.det_normal((1, fm.sigma.numel()), 8 + k)).to(DEV) * fm.sigma
            w_true = g.style(torch.from_numpy(synth.det_normal((1, 512), 40 + k)).to(DEV)).unsqueeze(1).repeat(
                1, g.n_latent, 1)
            pose = torch.tensor([[-0.3 + 0.6 * k / max(batch - 1, 1), -0.1, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
            v, n, _ = morph.morph_mesh(fm, c_true, pose, tri)
            ims.append(g([w_true], (v, n, tri), input_is_latent=True, noise=noise)[0])
        target = torch.cat(ims, 0).contiguous()
    invs = {}
    for key in names:
        torch.manual_seed(11)
        invs[key] = inversion.LatentInverter(g, net, target, None, lr=0.05, pose_lr=0.01, noise=noise, n_mean_latent=4096,
                                             use_graph=True, face=(fm, tri), fit_shape=True, coeff_lr=0.05, shape_reg=1e-3,
                                             **CONFIGS[key])
    for inv in invs.values():
        inv.run(8)                                     # warm-up iterations + capture
        torch.cuda.synchronize()
    ms = {k: [] for k in invs}
    for _ in range(rounds):
        for k, inv in invs.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                inv.graph.replay()
            e.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(e) / steps)
    out = {"what": "camera_fit", "size": size, "batch": batch, "nv": int(fm.fc.bias.numel() // 3), "steps_per_round": steps,
           "rounds": rounds}
    for k, inv in invs.items():
        t = statistics.median(ms[k])
        out[k + "_ms_per_step"] = round(t, 4)
        out[k + "_steps_per_s"] = round(1000.0 / t, 2)
        out[k + "_rounds_ms"] = [round(x, 4) for x in ms[k]]
        out[k + "_spread"] = round((max(ms[k]) - min(ms[k])) / t, 4)
        out[k + "_kernel_nodes"] = inv.graph.kernel_nodes
        if "off" in invs and k != "off":
            out[k + "_over_off"] = round(statistics.median(ms["off"]) / t, 4)
            out[k + "_extra_us"] = round(1000.0 * (t - statistics.median(ms["off"])), 2)
        if getattr(inv, "camera", None) is not None:
            out[k + "_kappa"] = [round(float(x), 5) for x in inv.camera.detach().cpu()]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=256, help="the generator's picture size")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--configs", default="off,fixed,fitted", help="comma-separated subset of off, fixed, fitted")
    args = ap.parse_args()
    names = [c for c in args.configs.split(",") if c]
    if not names or any(c not in CONFIGS for c in names):
        raise SystemExit("bench_camera: --configs takes off, fixed and fitted")
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera: needs a GPU; a rate measured elsewhere says nothing")
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    bench(args.size, args.batch, args.steps, args.rounds, names)


if __name__ == "__main__":
    main()
