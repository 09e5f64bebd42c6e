"""Multi-view face reconstruction on one GPU, for profiles/reconstruct_multiview_notes.md.  One measurement per
invocation, so that each runs under its own time limit:

    timeout 300 python scripts/bench_multiview.py --what fit --views 4 [--steps 50] [--rounds 5]
    timeout 300 python scripts/bench_multiview.py --what fit --views 8
    timeout 120 python scripts/bench_multiview.py --what merge --views 4 --texture 512 [--iters 200]
    timeout 120 python scripts/bench_multiview.py --what merge --views 8 --texture 1024

fit:   the fit-shape inversion of profiles/reconstruct_batch_notes.md (GeneratorWithMap(256), the face-sized synthetic
       3DMM, d = 80 + 64, the LPIPS VGG16 trunk) at batch V, once as `--batch V` fits it and once with
       shared_identity = n_identity, both inverters in the same process, the rounds alternated and the median round
       counted: replayed image-steps/s (V steps per replay of the captured graph) of each, their ratio, and the kernel
       nodes of each captured step.
merge: op.texture.merge of V random bakes at T x T, C = 3, sharpness 2: device events around --iters calls after a
       warm-up; the time per call and the traffic it compares with, 4 (C + 1) V T^2 bytes read once and 4 (C + 1) T^2 + T^2
       written, over 6.3 TB/s (the HBM rate the kernel guide gives as achievable for element-wise work).

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
from stylerenderer_amd.op import morph, texture  # noqa: E402

DEV = torch.device("cuda:0")
HBM_ACHIEVABLE = 6.3e12


def bench_fit(size, views, steps, rounds):
    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(DEV)
    src = train.SyntheticFaceSource(DEV)
    fm, tri = src.model, src.tri
    net = lpips.PNetLin().to(DEV)
    noise = [torch.from_numpy(synth.det_normal(tuple(n.shape), 300 + i)).to(DEV) for i, n in enumerate(g.make_noise())]
    with torch.no_grad():
        # one subject, `views` poses
        c_true = torch.from_numpy(synth.det_normal((1, fm.sigma.numel()), 8)).to(DEV) * fm.sigma
        w_true = g.style(torch.from_numpy(synth.det_normal((1, 512), 9)).to(DEV)).unsqueeze(1).repeat(1, g.n_latent, 1)
        ims = []
        for k in range(views):
            yaw = -0.4 + 0.8 * k / max(views - 1, 1)
            pose = torch.tensor([[yaw, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
            v, n, _ = morph.morph_mesh(fm, c_true, pose, tri)
            ims.append(g([w_true], (v, n, tri), input_is_latent=True, noise=noise)[0])
        target = torch.cat(ims, 0).contiguous()
    invs = {}
    for key, kw in (("batch", {}), ("multiview", {"shared_identity": fm.n_identity})):
        torch.manual_seed(11)
        invs[key] = inversion.LatentInverter(g, net, target, None, lr=0.05, pose_lr=0.01, noise=noise, n_mean_latent=4096,
                                             use_graph=True, face=(fm, tri), fit_shape=True, coeff_lr=0.05, shape_reg=1e-3,
                                             **kw)
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
    out = {"what": "multiview_fit", "size": size, "views": views, "shared_identity": fm.n_identity,
           "steps_per_round": steps, "rounds": rounds}
    for k, inv in invs.items():
        t = statistics.median(ms[k])
        out[k + "_ms_per_step"] = round(t, 4)
        out[k + "_image_steps_per_s"] = round(views * 1000.0 / t, 2)
        out[k + "_rounds_ms"] = [round(x, 4) for x in ms[k]]
        out[k + "_kernel_nodes"] = inv.graph.kernel_nodes
    out["multiview_over_batch"] = round(out["multiview_image_steps_per_s"] / out["batch_image_steps_per_s"], 4)
    out["extra_kernel_nodes"] = out["multiview_kernel_nodes"] - out["batch_kernel_nodes"]
    c = invs["multiview"].coeff.detach()
    out["shared_columns_equal"] = bool((c[:, :fm.n_identity] == c[:1, :fm.n_identity]).all())
    print(json.dumps(out), flush=True)


def bench_merge(views, t, iters, sharpness=2, c_n=3):
    tex = torch.rand(views, c_n, t, t, device=DEV) * 2 - 1
    r = torch.rand(views, 1, t, t, device=DEV)
    weight = torch.where(r > 0.4, r * r * (3 - 2 * r), torch.zeros_like(r))       # two texels in five unseen per view
    for _ in range(10):
        texture.merge(tex, weight, sharpness)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        texture.merge(tex, weight, sharpness)
    stop.record()
    torch.cuda.synchronize()
    sec = start.elapsed_time(stop) / iters * 1e-3
    nbytes = 4 * (c_n + 1) * views * t * t + 4 * (c_n + 1) * t * t + t * t
    print(json.dumps({"what": "merge", "T": t, "views": views, "C": c_n, "sharpness": sharpness, "iters": iters,
                      "seconds_per_call_with_allocation": sec, "bytes": nbytes,
                      "traffic_floor_seconds": nbytes / HBM_ACHIEVABLE, "floor_over_time": nbytes / HBM_ACHIEVABLE / sec}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("fit", "merge"), required=True)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=256, help="fit: the generator's picture size")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--texture", type=int, default=512, metavar="T", help="merge: the texture's side")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiview: needs a GPU; a rate measured elsewhere says nothing")
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    if args.what == "fit":
        bench_fit(args.size, args.views, args.steps, args.rounds)
    else:
        bench_merge(args.views, args.texture, args.iters)


if __name__ == "__main__":
    main()
