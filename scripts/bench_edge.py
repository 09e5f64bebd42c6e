"""op.edge on one GPU, for profiles/edge_notes.md.  One measurement per invocation, so that each runs under its own time
limit:

    timeout 300 python scripts/bench_edge.py --what entries [--mesh synthetic|dense] [--batch 1]
    timeout 600 python scripts/bench_edge.py --what step [--steps 60]

entries: the three launches (sr_edge_aa_fwd, sr_edge_aa_bwd_image, sr_edge_aa_bwd_corner) at 256^2, C = 3, on the synthetic
3DMM's mesh or on a 49 536-face ellipsoid (uv_ellipsoid(259, 96)), each called `reps` times between two device events
after a warm-up; per launch the median of `rounds` windows in microseconds per call.  Also the face map (one rasterizer
pass and its torch operations), the corners-to-vertices launch (sr_explode_bwd) and the whole node forward + backward
through autograd.  The forward and the image gradient stream the picture once (C planes read, C written, the face map
read); the figure in GB/s counts those bytes.
step: the captured iteration of a 256^2 fit on the synthetic 3DMM with and without silhouette=, and its photometric
iteration with and without photo_edges: image-steps per second (the median of `rounds` windows of `steps` replays, the
variants alternating in one process) and the kernel nodes of each graph.

Prints one JSON line.  There is no CPU path: without a device the script fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stylerenderer_amd import face_model, inversion, lpips, model, synth, train  # noqa: E402
from stylerenderer_amd.op import edge  # noqa: E402
from stylerenderer_amd.op._dispatch import native  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps, rounds):
    """Median, minimum and maximum over `rounds` windows of the microseconds per call of fn."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        us.append(1000.0 * a.elapsed_time(e) / reps)
    return statistics.median(us), min(us), max(us)


def mesh_of(kind, batch):
    if kind == "dense":
        v0, tri = synth.uv_ellipsoid(259, 96)
        v = torch.from_numpy(synth.random_poses(v0, batch)).float().to(DEV)
        return v.contiguous(), torch.from_numpy(tri).to(DEV)
    src = train.SyntheticFaceSource(DEV)
    with torch.no_grad():
        v = src.model.mesh(torch.zeros(batch, src.model.n_coeff, device=DEV), torch.zeros(batch, 7, device=DEV), src.tri)[0]
    return v.contiguous(), src.tri.contiguous()


def entries(kind, batch, size, reps, rounds):
    v, tri = mesh_of(kind, batch)
    c, nv, nf = 3, int(v.shape[1]), int(tri.shape[0])
    image = torch.from_numpy(synth.det_uniform((batch, c, size, size), 1)).to(DEV)
    g = torch.from_numpy(synth.det_normal((batch, c, size, size), 2)).to(DEV)
    face, zbuf = edge.face_map(v, tri, size)
    opp = edge.adjacency(tri, nv)
    out, gi = torch.empty_like(image), torch.empty_like(image)
    gc = torch.empty((batch, 3 * nf, 3), device=DEV)
    dims = (batch, c, size, size, nv, nf)
    run = native(image)
    edge._corners_to_vertices(gc.zero_(), tri, nv)                               # the incidence list, once per topology
    vr, ir = v.clone().requires_grad_(True), image.clone().requires_grad_(True)

    def whole():
        res = edge.antialias(ir, vr, tri, face, zbuf, opp)
        torch.autograd.grad(res, (ir, vr), grad_outputs=g)

    plane = 4.0 * batch * size * size
    cases = [("fwd", lambda: run.sr_edge_aa_fwd(out, image, v, tri, opp, face, zbuf, *dims), plane * (2 * c + 1)),
             ("bwd_image", lambda: run.sr_edge_aa_bwd_image(gi, g, v, tri, opp, face, zbuf, *dims), plane * (2 * c + 1)),
             ("bwd_corner", lambda: run.sr_edge_aa_bwd_corner(gc, g, image, v, tri, opp, face, zbuf, *dims), None),
             ("corners_to_vertices", lambda: edge._corners_to_vertices(gc, tri, nv), None),
             ("face_map", lambda: edge.face_map(v, tri, size), None),
             ("node_fwd_bwd", whole, None)]
    boxes = edge.box_pixels(v, tri, size)
    changed = int((edge.antialias(image, v, tri, face, zbuf, opp) != image).any(1).sum())
    res = dict(vertices=nv, faces=nf, covered=float((face >= 0).float().mean()), pixels_changed=changed,
               box_pixels_median=int(boxes.median()), box_pixels_max=int(boxes.max()),
               faces_by_wave=int((boxes > edge.BIG).sum()))
    for name, fn, nbytes in cases:
        med, lo, hi = timed(fn, reps, rounds)
        res[name + "_us"] = round(med, 2)
        res[name + "_us_min_max"] = [round(lo, 2), round(hi, 2)]
        if nbytes is not None:
            res[name + "_algorithmic_GBps"] = round(nbytes / med / 1e3, 1)
    return res


def step(size, tsize, steps, rounds):
    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(DEV)
    src = train.SyntheticFaceSource(DEV)
    fm, tri = src.model, src.tri
    with torch.no_grad():
        v = fm.mesh(torch.zeros(1, fm.n_coeff, device=DEV), torch.zeros(1, 7, device=DEV), tri)[0]
    layout = face_model.uv_layout(v[0].cpu(), tri)
    target = torch.from_numpy(synth.det_uniform((1, 3, size, size), 19)).to(DEV)
    sil = edge.coverage(v + torch.tensor([0.02, 0.01, 0.0], device=DEV), tri, size).detach()
    net = lpips.PNetLin().to(DEV)
    invs = {}
    for key, kw in (("plain", {}), ("silhouette", dict(silhouette=sil)), ("photo", {}), ("photo_edges", dict(photo_edges=True))):
        torch.manual_seed(11)
        more = dict(photometric=layout, photo_size=tsize) if key.startswith("photo") else {}
        inv = inversion.LatentInverter(g, net, target, None, n_mean_latent=256, face=(fm, tri), fit_shape=True,
                                       shape_reg=1e-3, **more, **kw)
        flag = key.startswith("photo")
        inv.run(8)
        if flag:
            inv.set_texture(torch.zeros_like(inv.texture))
            inv.run(8, photometric=True)
        invs[key] = (inv, flag)
    rates = {k: [] for k in invs}
    for _ in range(rounds):
        for key, (inv, flag) in invs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inv.run(steps, photometric=flag)
            torch.cuda.synchronize()
            rates[key].append(steps / (time.perf_counter() - t0))
    out = {}
    for key, (inv, flag) in invs.items():
        graph = inv.graph_photo if flag else inv.graph
        out[key + "_steps_per_second"] = round(statistics.median(rates[key]), 2)
        out[key + "_spread"] = [round(min(rates[key]), 2), round(max(rates[key]), 2)]
        out[key + "_kernel_nodes"] = graph.kernel_nodes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="entries", choices=("entries", "step"))
    ap.add_argument("--mesh", default="synthetic", choices=("synthetic", "dense"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--texture", type=int, default=512)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edge: no GPU")
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    out = {"what": "edge_" + args.what, "device": torch.cuda.get_device_name(0), "pixels": [args.size, args.size]}
    if args.what == "entries":
        out.update(mesh=args.mesh, batch=args.batch)
        out.update(entries(args.mesh, args.batch, args.size, args.reps, args.rounds))
    else:
        out.update(steps=args.steps, texels=args.texture)
        out.update(step(args.size, args.texture, args.steps, min(args.rounds, 5)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
