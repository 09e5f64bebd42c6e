"""Numbers for profiles/reconstruct_photo_notes.md (a GPU).

  * `TapPlanner.build` against an uncached `op.texture.tap_plan` call on the same uv map, alternating in one process: the
    time of a call (device events around `--iters` calls after a warm-up, `--rounds` rounds, the median) and the launches
    of a call (kernel nodes of a captured build; aten operators of a tap_plan call), at B = 1 and 8, 256^2 pixels, T = 512;
  * the backward of `op.texture.explode` against that of the indexing v[:, tri.reshape(-1)] on the face-sized mesh;
  * the replay rate of the photometric iteration against the plain iteration of the same inverter (256^2 generator, the
    synthetic 3DMM of the benchmark's inversion leg, T = 512), and both graphs' node counts.

One JSON line per measurement.

    python scripts/bench_photo_fit.py [--size 256] [--texture 512] [--iters 200] [--rounds 3] [--steps 60]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stylerenderer_amd import face_model, graphs, inversion, lpips, model, synth, train  # noqa: E402
from stylerenderer_amd.op import texture  # noqa: E402


def timed(fn, iters, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters * 1e-3


def pair(what, shape, old, new, iters, rounds, **more):
    """Times the two alternately, `rounds` times each; prints the medians and their ratio."""
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(old, iters))
        b.append(timed(new, iters))
    sa, sb = float(np.median(a)), float(np.median(b))
    print(json.dumps(dict(shape, what=what, torch_seconds=sa, native_seconds=sb, ratio=sb / sa,
                          torch_spread=[min(a), max(a)], native_spread=[min(b), max(b)], **more)), flush=True)


def aten_calls(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    with Spy():
        fn()
    return len(seen)


def captured_nodes(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(fn)
    return graph.kernel_nodes, graph.nodes


def plans(args, dev):
    v0, tri = synth.face_sized_mesh()
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    tri_t = torch.from_numpy(tri).to(dev)
    for batch in (1, 8):
        v = torch.from_numpy(synth.random_poses(v0, batch)).to(dev)
        with torch.no_grad():
            uvmap, cover = texture.uv_map(v, tri_t, uv.to(dev), tri_uv, args.size, keep.to(dev))
        for bt in sorted({1, batch}):
            planner = texture.TapPlanner(batch, args.size, args.size, args.texture, bt, dev)

            def old():
                texture._PLAN_CACHE.clear()
                texture.tap_plan(uvmap, cover, args.texture, bt)

            def new():
                planner.build(uvmap, cover)

            want = texture.tap_plan(uvmap, cover, args.texture, bt)
            got = planner.build(uvmap, cover)
            same = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
            pair("tap list", dict(B=batch, Bt=bt, size=args.size, texture=args.texture), old, new, args.iters, args.rounds,
                 equal=same, torch_aten_calls=aten_calls(old), native_kernel_nodes=captured_nodes(new)[0],
                 passes=planner.passes, covered=float(cover.float().mean()))
    # the corner explode's adjoint
    for batch in (1, 8):
        v = torch.from_numpy(synth.random_poses(v0, batch)).to(dev).requires_grad_(True)
        g = torch.from_numpy(synth.det_uniform((batch, 3 * tri.shape[0], 3), 3)).to(dev)
        flat = tri_t.reshape(-1)
        texture.explode(v, tri_t).backward(g)                                  # the incidence list, once per topology

        def old():
            torch.autograd.grad(v[:, flat], v, g)

        def new():
            torch.autograd.grad(texture.explode(v, tri_t), v, g)

        pair("explode forward + backward", dict(B=batch, corners=int(flat.numel()), vertices=int(v.shape[1])), old, new,
             args.iters, args.rounds, torch_aten_calls=aten_calls(old), native_aten_calls=aten_calls(new))


def iterations(args, dev):
    g = model.GeneratorWithMap(args.size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(dev)
    src = train.SyntheticFaceSource(dev)
    fm, tri = src.model, src.tri
    with torch.no_grad():
        v = fm.mesh(torch.zeros(1, fm.n_coeff, device=dev), torch.zeros(1, 7, device=dev), tri)[0]
    layout = face_model.uv_layout(v[0].cpu(), tri)
    target = torch.from_numpy(synth.det_uniform((1, 3, args.size, args.size), 19)).to(dev)
    torch.manual_seed(11)
    inv = inversion.LatentInverter(g, lpips.PNetLin().to(dev), target, None, n_mean_latent=256, face=(fm, tri),
                                   fit_shape=True, shape_reg=1e-3, photometric=layout, photo_size=args.texture)
    inv.run(8)
    inv.set_texture(torch.zeros_like(inv.texture))
    inv.run(8, photometric=True)
    rates = {"plain": [], "photometric": []}
    for _ in range(args.rounds):
        for key, flag in (("plain", False), ("photometric", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            inv.run(args.steps, photometric=flag)
            torch.cuda.synchronize()
            rates[key].append(args.steps / (time.perf_counter() - t0))
    print(json.dumps(dict(what="replay rate", size=args.size, texture=args.texture, steps=args.steps,
                          plain_steps_per_second=float(np.median(rates["plain"])),
                          photometric_steps_per_second=float(np.median(rates["photometric"])),
                          plain_spread=[min(rates["plain"]), max(rates["plain"])],
                          photometric_spread=[min(rates["photometric"]), max(rates["photometric"])],
                          plain_kernel_nodes=inv.graph.kernel_nodes, plain_nodes=inv.graph.nodes,
                          photometric_kernel_nodes=inv.graph_photo.kernel_nodes, photometric_nodes=inv.graph_photo.nodes,
                          photometric_memsets_replaced=inv.graph_photo.memset_nodes_replaced)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--texture", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--skip_iterations", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photo_fit: needs a GPU (a host timing says nothing about the device)")
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    dev = torch.device("cuda")
    plans(args, dev)
    if not args.skip_iterations:
        iterations(args, dev)


if __name__ == "__main__":
    main()
