"""op.light on one GPU, for profiles/light_notes.md.  One measurement per invocation, so that each runs under its own time
limit:

    timeout 300 python scripts/bench_light.py --what entries [--batch 1] [--lights 3]      # the tool's sizes
    timeout 300 python scripts/bench_light.py --what stream                                 # 1024^2 x 8
    timeout 300 python scripts/bench_light.py --what refine [--steps 50]                    # a --texture_refine step

entries: the five C entries at the tool's sizes (texel_attribute and moments at T = 512, shade forward / backward with the
light's gradient / unshade at 256^2 pixels, C = 3), each called `reps` times between two device events after a warm-up;
per entry the median of `rounds` windows in microseconds per call.  At these sizes a call is a few launches of a few
microseconds of work: the figure is launch-bound and is named as such.
stream: the same calls on 1024^2 x 8, where the streaming kernels can be read as GB/s of their algorithmic bytes (float32
planes read and written once; the mask one byte per pixel; gamma and the partial rows not counted).
refine: reconstruct.texture_refine's step (T = 512 texture, one 256^2 view) with and without a light, the two alternating
in one process.

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

from stylerenderer_amd import face_model, reconstruct, synth  # noqa: E402
from stylerenderer_amd.op import light, texture  # noqa: E402

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


def pictures(b, c, h, w, cl):
    a = torch.from_numpy(synth.det_uniform((b, c, h, w), 1)).to(DEV)
    normals = torch.from_numpy(synth.det_normal((b, 3, h, w), 2)).to(DEV)
    normals[:, 2] = normals[:, 2].abs() + 0.5
    on = torch.from_numpy(synth.det_uniform((b, h, w), 3) > -0.8).to(DEV)
    gamma = torch.zeros((b, cl, 9), device=DEV)
    gamma[:, :, 0], gamma[:, :, 3] = 0.8, 0.4
    g = torch.from_numpy(synth.det_normal((b, c, h, w), 4)).to(DEV)
    return a, normals, on, gamma, g


def entries(b, c, h, w, cl, tsize, reps, rounds):
    a, normals, on, gamma, g = pictures(b, c, h, w, cl)
    weight = on.unsqueeze(1).float().contiguous()
    buf = torch.zeros(gamma.numel(), device=DEV)
    ar, nr = a.clone().requires_grad_(True), normals.clone().requires_grad_(True)

    def backward():
        out = light.shade(ar, nr, on, gamma, ggamma_out=buf)
        torch.autograd.grad(out, (ar, nr), grad_outputs=g)

    def forward_only():
        with torch.no_grad():
            light.shade(a, normals, on, gamma)

    plane = 4.0 * b * h * w
    res = {}
    cases = [("shade_fwd", forward_only, plane * (2 * c + 3) + b * h * w),
             ("shade_fwd_bwd", backward, plane * (2 * c + 3) + plane * (3 * c + 3 + 3) + 2 * b * h * w),
             ("unshade", lambda: light.unshade(a, normals, on, gamma), plane * (2 * c + 3) + b * h * w),
             ("moments", lambda: light.moments(a, normals, weight), plane * (c + 3 + 1))]
    v0, tri = synth.uv_ellipsoid(64, 48)
    vp = synth.random_poses(v0, b)
    n = torch.from_numpy(synth.vertex_normals(vp, tri)).float().to(DEV)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    face, coeff = texture.texel_map(uv.to(DEV), tri_uv, tsize, keep)
    tri_d = torch.from_numpy(tri).to(DEV)
    cases.append(("texel_attribute", lambda: light.texel_attribute(n, tri_d, face, coeff), 4.0 * b * 3 * tsize * tsize))
    for name, fn, nbytes in cases:
        med, lo, hi = timed(fn, reps, rounds)
        res[name + "_us"] = round(med, 2)
        res[name + "_us_min_max"] = [round(lo, 2), round(hi, 2)]
        res[name + "_algorithmic_GBps"] = round(nbytes / med / 1e3, 1)
    return res


def refine(steps, rounds, tsize, size):
    v0, tri = synth.uv_ellipsoid(64, 48)
    vp = synth.random_poses(v0, 1)
    v = torch.from_numpy(vp).float().to(DEV)
    n = torch.from_numpy(synth.vertex_normals(vp, tri)).float().to(DEV)
    tri_d = torch.from_numpy(tri).to(DEV)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    uvmap, cover = texture.uv_map(v, tri_d, uv.to(DEV), tri_uv, size, keep)
    target = torch.from_numpy(synth.det_uniform((1, 3, size, size), 5)).to(DEV)
    tex = torch.from_numpy(synth.det_uniform((1, 3, tsize, tsize), 6)).to(DEV)
    views = [(uvmap, cover, target)]
    gamma = torch.zeros((1, 3, 9), device=DEV)
    gamma[:, :, 0], gamma[:, :, 3] = 0.8, 0.4
    pair = [[gamma, light.normal_map(v, n, tri_d, size)]]
    ms = {"plain": [], "light": []}
    for key in ("plain", "light"):                                                # warm-up: the tap list, first launches
        reconstruct.texture_refine(tex, views, 3, light=pair if key == "light" else None)
    for _ in range(rounds):
        for key in ("plain", "light"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reconstruct.texture_refine(tex, views, steps, light=pair if key == "light" else None)
            torch.cuda.synchronize()
            ms[key].append(1000.0 * (time.perf_counter() - t0) / steps)
    out = {}
    for key, vals in ms.items():
        out["refine_%s_ms_per_step" % key] = round(statistics.median(vals), 4)
        out["refine_%s_ms_min_max" % key] = [round(min(vals), 4), round(max(vals), 4)]
    out["refine_light_over_plain"] = round(out["refine_light_ms_per_step"] / out["refine_plain_ms_per_step"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="entries", choices=("entries", "stream", "refine"))
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--lights", type=int, default=3, choices=(1, 3))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_light: no GPU")
    out = {"what": "light_" + args.what, "device": torch.cuda.get_device_name(0)}
    if args.what == "entries":
        out.update(batch=args.batch, lights=args.lights, pixels=[256, 256], texels=512)
        out.update(entries(args.batch, 3, 256, 256, args.lights, 512, args.reps, args.rounds))
    elif args.what == "stream":
        out.update(batch=8, lights=args.lights, pixels=[1024, 1024], texels=1024)
        out.update(entries(8, 3, 1024, 1024, args.lights, 1024, max(args.reps // 10, 10), args.rounds))
    else:
        out.update(steps=args.steps, texels=512, pixels=[256, 256])
        out.update(refine(args.steps, args.rounds, 512, 256))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
