"""Times op.texture on the device for profiles/reconstruct_texture_notes.md: the bake at T = 1024 from a 1024^2 picture for
B = 1 and 8, one padding pass, and the traffic floor they compare with.  Device events around `--iters` calls after a warm-up;
prints one JSON line per measurement.

    python scripts/bench_texture.py [--size 1024] [--picture 1024] [--iters 200]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stylerenderer_amd import face_model, synth  # noqa: E402
from stylerenderer_amd.op import texture  # noqa: E402

HBM_ACHIEVABLE = 6.3e12          # bytes / s: the element-wise ceiling the kernel guide quotes for the MI355X


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--picture", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture: needs a GPU")
    dev = torch.device("cuda")
    v0, tri = synth.face_sized_mesh()
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    face, coeff = texture.texel_map(uv.to(dev), tri_uv, args.size, keep)
    tri_d = torch.from_numpy(tri).to(dev)
    t, c_n = args.size, 3
    for batch in (1, 8):
        v = torch.from_numpy(synth.random_poses(v0, batch)).to(dev)
        n = torch.from_numpy(synth.vertex_normals(v.cpu().numpy(), tri)).to(dev)
        img = torch.rand(batch, c_n, args.picture, args.picture, device=dev) * 2 - 1
        zbuf = texture.depth_buffer(v, tri_d, min(1024, t))
        sec = timed(lambda: texture.bake(v, n, tri_d, face, coeff, img, zbuf), args.iters)
        floor = (16 * t * t + 4 * (c_n + 1) * batch * t * t) / HBM_ACHIEVABLE
        print(json.dumps({"what": "bake", "T": t, "picture": args.picture, "B": batch, "seconds": sec,
                          "traffic_floor_seconds": floor, "floor_over_time": floor / sec}))
        tex, weight = texture.bake(v, n, tri_d, face, coeff, img, zbuf)
        one = timed(lambda: texture.pad(tex, weight, 1), args.iters)
        eight = timed(lambda: texture.pad(tex, weight, 8), args.iters)
        print(json.dumps({"what": "pad", "T": t, "B": batch, "seconds_1_pass_with_setup": one,
                          "seconds_per_further_pass": (eight - one) / 7,
                          "coverage": float(texture.coverage(face, weight).mean())}))


if __name__ == "__main__":
    main()
