"""Times the texture look-up node on the device for profiles/texture_render_notes.md: the three launches of op.texture.sample
(forward, the uv map's gradient, the texture's gradient), the build of the tap list, `uv_map`, one step of
`reconstruct --texture_refine`, and for comparison torch's F.grid_sample forward plus backward on the same tensors (that
call is a library's: it runs outside SR_STRICT_NATIVE, is never a fallback of this project, and its backward adds with
float atomics).  256^2 pixels, T = 512, C = 3, the synthetic face mesh; B = 1 and 8, Bt = 1 and B.  Device events around
`--iters` calls after a warm-up; prints one JSON line per measurement.

    python scripts/bench_texture_render.py [--size 256] [--texture 512] [--iters 200]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stylerenderer_amd import face_model, reconstruct, synth  # noqa: E402
from stylerenderer_amd.op import texture  # noqa: E402
from stylerenderer_amd.op._dispatch import native  # noqa: E402

HBM_ACHIEVABLE = 6.3e12          # bytes / s: the element-wise ceiling the kernel guide quotes for the MI355X


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--texture", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture_render: needs a GPU")
    if os.environ.get("SR_STRICT_NATIVE") == "1":
        raise SystemExit("bench_texture_render: the grid_sample comparison is a library call; run without SR_STRICT_NATIVE=1")
    dev = torch.device("cuda")
    s, t, c_n = args.size, args.texture, 3
    v0, tri = synth.face_sized_mesh()
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    uv_d, tri_d, keep_d = uv.to(dev), torch.from_numpy(tri).to(dev), keep.to(dev)
    for batch in (1, 8):
        v = torch.from_numpy(synth.random_poses(v0, batch)).to(dev)
        sec = timed(lambda: texture.uv_map(v, tri_d, uv_d, tri_uv, s, keep_d), max(args.iters // 10, 5), warm=3)
        uvmap, cover = texture.uv_map(v, tri_d, uv_d, tri_uv, s, keep_d)
        print(json.dumps({"what": "uv_map", "size": s, "B": batch, "seconds": sec,
                          "covered_share": float(cover.float().mean())}))
        g = torch.rand(batch, c_n, s, s, device=dev) * 2 - 1
        for bt in sorted({1, batch}):
            tex = torch.rand(bt, c_n, t, t, device=dev) * 2 - 1
            shape = dict(size=s, T=t, B=batch, Bt=bt, C=c_n)

            def plan():
                texture._PLAN_CACHE.clear()
                return texture.tap_plan(uvmap, cover, (t, t), bt)

            print(json.dumps(dict(shape, what="tap_plan", seconds=timed(plan, max(args.iters // 10, 5), warm=3))))
            off, entries = plan()
            out, guv, gtex = torch.empty_like(g), torch.empty_like(uvmap), torch.empty_like(tex)
            dims = (batch, bt, c_n, s, s, t, t)
            lib = native(tex)
            fwd = timed(lambda: lib.sr_texture_sample_fwd(out, tex, uvmap, cover, *dims, -1.0), args.iters)
            # the pixels' side: the uv map and cover read, C planes written; the texels' side is gathered through the caches
            floor = batch * s * s * (9 + 4 * c_n) / HBM_ACHIEVABLE
            print(json.dumps(dict(shape, what="sample_fwd", seconds=fwd, traffic_floor_seconds=floor)))
            sec = timed(lambda: lib.sr_texture_sample_bwd_uv(guv, g, tex, uvmap, cover, *dims), args.iters)
            print(json.dumps(dict(shape, what="sample_bwd_uv", seconds=sec,
                                  traffic_floor_seconds=batch * s * s * (17 + 4 * c_n) / HBM_ACHIEVABLE)))
            sec = timed(lambda: lib.sr_texture_sample_bwd_tex(gtex, g, uvmap, cover, off, entries, *dims), args.iters)
            counts = (off[1:bt * t * t + 1] - off[:bt * t * t])
            print(json.dumps(dict(shape, what="sample_bwd_tex", seconds=sec, longest_list=int(counts.max()),
                                  mean_list=float(counts.float().mean()),
                                  traffic_floor_seconds=(4 * c_n * bt * t * t + 16 * batch * s * s) / HBM_ACHIEVABLE)))
            # the library call on the same tensors: forward plus backward to the texture and the grid
            grid = torch.stack((2 * uvmap[..., 0] - 1, 1 - 2 * uvmap[..., 1]), -1).requires_grad_(True)
            tex_g = (tex if bt == batch else tex.expand(batch, -1, -1, -1)).clone().requires_grad_(True)

            def library():
                y = torch.nn.functional.grid_sample(tex_g, grid, mode="bilinear", padding_mode="border", align_corners=False)
                torch.autograd.grad(y, (tex_g, grid), g)

            print(json.dumps(dict(shape, what="grid_sample_fwd_bwd (comparison only)", seconds=timed(library, args.iters))))
            tq, mq = tex.clone().requires_grad_(True), uvmap.clone().requires_grad_(True)
            texture.tap_plan(mq, cover, (t, t), bt)

            def ours():
                y = texture.sample(tq, mq, cover, -1.0)
                torch.autograd.grad(y, (tq, mq), g)

            print(json.dumps(dict(shape, what="sample_fwd_bwd through autograd", seconds=timed(ours, args.iters))))
        # one refinement step: all views on one texture
        target = torch.rand(batch, c_n, s, s, device=dev) * 2 - 1
        views = [(uvmap[k:k + 1].contiguous(), cover[k:k + 1].contiguous(), target[k:k + 1]) for k in range(batch)]
        start_tex = torch.zeros(1, c_n, t, t, device=dev)
        steps = max(args.iters // 4, 10)
        reconstruct.texture_refine(start_tex, views, 3)                                  # warm-up: the plan, code objects
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        reconstruct.texture_refine(start_tex, views, steps)
        end.record()
        torch.cuda.synchronize()
        print(json.dumps({"what": "texture_refine step (with the call's set-up spread over %d steps)" % steps, "size": s,
                          "T": t, "views": batch, "seconds": begin.elapsed_time(end) / steps * 1e-3}))


if __name__ == "__main__":
    main()
