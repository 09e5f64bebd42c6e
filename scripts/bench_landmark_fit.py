"""Landmark-guided face reconstruction on one GPU: the fit-shape inversion (LatentInverter(fit_shape=True)) at 256^2 on the
face-sized synthetic 3DMM, with and without the landmark term (op.landmark), at the batch sizes of --batch.

    python scripts/bench_landmark_fit.py [--batch 1,8] [--steps 100] [--rounds 5] [--dynamic] [--root DIR]

One JSON line per batch size: replayed image-steps/s (B steps per replay of the captured graph) of the inverter without
landmarks and of the one with 68 landmarks in the same process, the rounds alternated and the median round counted, the
kernel nodes and all nodes of each captured step, and the cost of the term (ratio of the rates, extra nodes).  With
--dynamic a third inverter runs the pose-aware term (contour lines on landmarks 0-16, 21 candidates each, and the
visibility gate 0,0.2) in the same alternation: its rate and nodes against the static term's.

--root DIR imports the package from another checkout (built there): a checkout from before the landmark term reports the
rate without landmarks only.  To compare two commits, run the script once per checkout in turn, twice each, in one
session: the no-landmark rates of the two agree when they differ by no more than two runs of the same checkout do.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

DEV = torch.device("cuda:0")


def build(pkg, size, batch, with_landmarks, dynamic=False):
    inversion, lpips, model, synth, train = pkg["inversion"], pkg["lpips"], pkg["model"], pkg["synth"], pkg["train"]
    morph = pkg["morph"]
    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(DEV)
    src = train.SyntheticFaceSource(DEV)
    fm, tri = src.model, src.tri
    net = lpips.PNetLin().to(DEV)
    noise = [torch.from_numpy(synth.det_normal(tuple(n.shape), 300 + i)).to(DEV) for i, n in enumerate(g.make_noise())]
    pose = torch.tensor([[0.2, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
    with torch.no_grad():
        c_true = torch.from_numpy(synth.det_normal((1, fm.sigma.numel()), 8)).to(DEV) * fm.sigma
        v, n, _ = morph.morph_mesh(fm, c_true, pose, tri)
        w_true = g.style(torch.from_numpy(synth.det_normal((1, 512), 9)).to(DEV)).unsqueeze(1).repeat(1, g.n_latent, 1)
        target, _, _ = g([w_true], (v, n, tri), input_is_latent=True, noise=noise)
    kw = {}
    if with_landmarks:
        from stylerenderer_amd import face_model
        from stylerenderer_amd.op import landmark

        nv = v.shape[1]
        idx, bary = face_model.landmark_embedding(np.linspace(0, nv - 1, 68).round().astype(np.int64))
        lmk = landmark.project(landmark.landmark_points(v.double().cpu(), idx, bary.double()), size)[0].numpy()
        kw = dict(landmarks=np.repeat(lmk[None], batch, 0), landmark_embedding=(idx, bary))
        if dynamic:
            main = face_model.landmark_vertices((idx, bary))
            cand = np.concatenate([(main[l] + np.arange(21)) % nv for l in range(17)])
            kw.update(landmark_lines=(np.arange(17), np.where(np.arange(17) < 8, 1, -1), 21 * np.arange(18), cand),
                      landmark_axis=(int(main[27]), int(main[8])), landmark_vis=(0.0, 0.2))
    torch.manual_seed(11)
    return inversion.LatentInverter(g, net, target.expand(batch, -1, -1, -1).contiguous(), None, lr=0.05, pose_lr=0.01,
                                    noise=noise, n_mean_latent=4096, use_graph=True, face=(fm, tri), fit_shape=True,
                                    coeff_lr=0.05, shape_reg=1e-3, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", default="1,8", metavar="B1,B2,...")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dynamic", action="store_true",
                    help="also measure the pose-aware term (contour lines and the visibility gate)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose package is measured [this one]")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_landmark_fit: needs a GPU; a rate measured elsewhere says nothing")
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    sys.path.insert(0, os.path.abspath(args.root))
    from stylerenderer_amd import align, inversion, lpips, model, synth, train
    from stylerenderer_amd.op import morph

    pkg = dict(inversion=inversion, lpips=lpips, model=model, synth=synth, train=train, morph=morph)
    has_term = hasattr(align, "pose_from_landmarks")
    for b in (int(x) for x in args.batch.split(",")):
        torch.cuda.empty_cache()
        invs = {"plain": build(pkg, args.size, b, False)}
        if has_term:
            invs["landmarks"] = build(pkg, args.size, b, True)
        if has_term and args.dynamic:
            invs["dynamic"] = build(pkg, args.size, b, True, dynamic=True)
        for inv in invs.values():
            inv.run(8)                                     # warm-up iterations + capture
            torch.cuda.synchronize()
        ms = {k: [] for k in invs}
        for _ in range(args.rounds):
            for k, inv in invs.items():
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.steps):
                    inv.graph.replay()
                e.record()
                torch.cuda.synchronize()
                ms[k].append(a.elapsed_time(e) / args.steps)
        out = {"what": "landmark_fit", "root": os.path.abspath(args.root), "size": args.size, "batch": b,
               "steps_per_round": args.steps, "rounds": args.rounds}
        for k, inv in invs.items():
            t = statistics.median(ms[k])
            out[k + "_ms_per_step"] = round(t, 4)
            out[k + "_image_steps_per_s"] = round(b * 1000.0 / t, 2)
            out[k + "_rounds_ms"] = [round(x, 4) for x in ms[k]]
            out[k + "_kernel_nodes"], out[k + "_nodes"] = inv.graph.kernel_nodes, inv.graph.nodes
        if has_term:
            out["landmarks_over_plain"] = round(out["landmarks_image_steps_per_s"] / out["plain_image_steps_per_s"], 4)
            out["extra_kernel_nodes"] = out["landmarks_kernel_nodes"] - out["plain_kernel_nodes"]
        if "dynamic" in invs:
            out["dynamic_over_landmarks"] = round(out["dynamic_image_steps_per_s"] / out["landmarks_image_steps_per_s"], 4)
            out["dynamic_extra_kernel_nodes"] = out["dynamic_kernel_nodes"] - out["landmarks_kernel_nodes"]
        print(json.dumps(out), flush=True)
        del invs


if __name__ == "__main__":
    main()
