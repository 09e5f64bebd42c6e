"""Region-weighted face reconstruction on one GPU: the fit-shape inversion (LatentInverter(fit_shape=True)) at 256^2 on the
face-sized synthetic 3DMM without a region, with mask= and with mask= + mask_mesh=True (op.region), at the batch sizes of
--batch.

    python scripts/bench_mask_fit.py [--batch 1,8] [--steps 100] [--rounds 5] [--root DIR]

One JSON line per batch size: replayed image-steps/s (B steps per replay of the captured graph) of the three inverters in
the same process, the rounds alternated and the median round counted, the kernel nodes and all nodes of each captured
step, and the cost of the region (ratio of the rates, extra nodes).

--root DIR imports the package from another checkout (built there): a checkout from before the region reports the rate
without one only.  To compare two commits, run the script once per checkout in turn, twice each, in one session: the
no-mask rates of the two agree when they differ by no more than two runs of the same checkout do.
"""
import argparse
import json
import os
import statistics
import sys

import torch

DEV = torch.device("cuda:0")


def build(pkg, size, batch, how):
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
    if how != "plain":
        # an ellipse over the middle of the picture, the size of a face's hull
        ys, xs = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
        inside = ((xs - size / 2) / (0.32 * size)) ** 2 + ((ys - size / 2) / (0.42 * size)) ** 2 <= 1
        kw = dict(mask=inside.float().view(1, 1, size, size).expand(batch, -1, -1, -1).contiguous(),
                  mask_mesh=how == "mask_mesh")
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
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose package is measured [this one]")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mask_fit: needs a GPU; a rate measured elsewhere says nothing")
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    sys.path.insert(0, os.path.abspath(args.root))
    from stylerenderer_amd import inversion, lpips, model, synth, train
    from stylerenderer_amd.op import morph

    pkg = dict(inversion=inversion, lpips=lpips, model=model, synth=synth, train=train, morph=morph)
    has_region = os.path.isfile(os.path.join(os.path.dirname(inversion.__file__), "op", "region.py"))
    for b in (int(x) for x in args.batch.split(",")):
        torch.cuda.empty_cache()
        invs = {"plain": build(pkg, args.size, b, "plain")}
        if has_region:
            invs["mask"] = build(pkg, args.size, b, "mask")
            invs["mask_mesh"] = build(pkg, args.size, b, "mask_mesh")
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
        out = {"what": "mask_fit", "root": os.path.abspath(args.root), "size": args.size, "batch": b,
               "steps_per_round": args.steps, "rounds": args.rounds}
        for k, inv in invs.items():
            t = statistics.median(ms[k])
            out[k + "_ms_per_step"] = round(t, 4)
            out[k + "_image_steps_per_s"] = round(b * 1000.0 / t, 2)
            out[k + "_rounds_ms"] = [round(x, 4) for x in ms[k]]
            out[k + "_kernel_nodes"], out[k + "_nodes"] = inv.graph.kernel_nodes, inv.graph.nodes
        for k in ("mask", "mask_mesh"):
            if k in invs:
                out[k + "_over_plain"] = round(out[k + "_image_steps_per_s"] / out["plain_image_steps_per_s"], 4)
                out[k + "_extra_kernel_nodes"] = out[k + "_kernel_nodes"] - out["plain_kernel_nodes"]
        if "mask_mesh" in invs:
            out["mask_area_last_step"] = round(float(invs["mask_mesh"].mask_fit.mean()), 4)
        print(json.dumps(out), flush=True)
        del invs


if __name__ == "__main__":
    main()
