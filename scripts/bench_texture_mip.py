"""Numbers for profiles/texture_mip_notes.md.

Timings (a GPU): every launch of the mip-mapped look-up (csrc/texture_mip.hip) beside the plain sampler's launch on the same
inputs in the same process, the two alternating — sr_mip_sample_fwd / _bwd_uv / _bwd_pyr against sr_texture_sample_fwd /
_bwd_uv / _bwd_tex, sr_mip_build_fwd / _bwd and sr_mip_lod on their own — at T = 512 under 256^2 pixels, C = 3, B = 1 and 3,
one shared texture; then one `reconstruct.texture_refine` step with and without mip.  Device events around `--iters` calls
after a warm-up, `--rounds` rounds per pair; one JSON line per measurement with the ratio mip / plain.

Quality (`--quality`, runs on the host): on a posed ellipsoid with `face_model.uv_layout`,
  * the share of the seen texels (bake weight > 0) that take a non-zero gradient in one refinement step, plain and mip;
  * the mean absolute error of a texture with texel-scale detail drawn at half its resolution, plain and mip, against a
    bilinear draw at four times the picture's resolution averaged down 4 x 4.

    python scripts/bench_texture_mip.py [--size 256] [--texture 512] [--iters 200] [--rounds 3]
    python scripts/bench_texture_mip.py --quality [--size 64] [--texture 128]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stylerenderer_amd import face_model, reconstruct, synth  # noqa: E402
from stylerenderer_amd.op import texture  # noqa: E402
from stylerenderer_amd.op._dispatch import native  # noqa: E402


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


def pair(what, shape, plain, mip, iters, rounds):
    """Times the two alternately, `rounds` times each; prints the medians and their ratio."""
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(plain, iters))
        b.append(timed(mip, iters))
    sa, sb = float(np.median(a)), float(np.median(b))
    print(json.dumps(dict(shape, what=what, plain_seconds=sa, mip_seconds=sb, ratio=sb / sa,
                          plain_spread=[min(a), max(a)], mip_spread=[min(b), max(b)])))


def scene(batch, dev):
    v0, tri = synth.face_sized_mesh()
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    v = torch.from_numpy(synth.random_poses(v0, batch)).to(dev)
    return v, torch.from_numpy(tri).to(dev), uv.to(dev), tri_uv, keep.to(dev)


def timings(args):
    if not torch.cuda.is_available():
        raise SystemExit("bench_texture_mip: the timings need a GPU (--quality runs on the host)")
    dev = torch.device("cuda")
    s, t, c_n = args.size, args.texture, 3
    layout = texture.mip_layout((t, t))
    n_l, p = len(layout), layout[-1][0] + layout[-1][1] * layout[-1][2]
    for batch in (1, 3):
        v, tri, uv, tri_uv, keep = scene(batch, dev)
        uvmap, cover = texture.uv_map(v, tri, uv, tri_uv, s, keep)
        shape = dict(size=s, T=t, B=batch, Bt=1, C=c_n, levels=n_l)
        g = torch.rand(batch, c_n, s, s, device=dev) * 2 - 1
        tex = torch.rand(1, c_n, t, t, device=dev) * 2 - 1
        lib = native(tex)
        pyr, gpyr = torch.empty(1, c_n, p, device=dev), torch.rand(1, c_n, p, device=dev) * 2 - 1
        lod = torch.empty(batch, s, s, device=dev)
        out, guv, gtex = torch.empty_like(g), torch.empty_like(uvmap), torch.empty_like(tex)
        lib.sr_mip_build_fwd(pyr, tex, c_n, t, t, n_l)
        lib.sr_mip_lod(lod, uvmap, cover, batch, s, s, t, t, n_l, 0.0)
        live = cover & torch.isfinite(uvmap).all(-1)
        print(json.dumps(dict(shape, what="lod", covered_share=float(cover.float().mean()),
                              mean_lod=float(lod[live].mean()), max_lod=float(lod[live].max()),
                              whole_share=float((lod[live] == torch.floor(lod[live])).float().mean()))))
        off, entries = texture.tap_plan(uvmap, cover, (t, t), 1)
        moff, mentries = texture.mip_tap_plan(uvmap, cover, lod, (t, t), None, 1)
        counts, mcounts = (off[1:t * t + 1] - off[:t * t]), (moff[1:p + 1] - moff[:p])
        print(json.dumps(dict(shape, what="tap lists", plain_mean=float(counts.float().mean()),
                              plain_longest=int(counts.max()), mip_mean=float(mcounts.float().mean()),
                              mip_longest=int(mcounts.max()))))
        dims, mdims = (batch, 1, c_n, s, s, t, t), (batch, 1, c_n, s, s, t, t, n_l)
        for what, fn in (("mip_build_fwd", lambda: lib.sr_mip_build_fwd(pyr, tex, c_n, t, t, n_l)),
                         ("mip_build_bwd", lambda: lib.sr_mip_build_bwd(gtex, gpyr, 1, c_n, t, t, n_l)),
                         ("mip_lod", lambda: lib.sr_mip_lod(lod, uvmap, cover, batch, s, s, t, t, n_l, 0.0))):
            runs = [timed(fn, args.iters) for _ in range(args.rounds)]
            print(json.dumps(dict(shape, what=what, seconds=float(np.median(runs)), spread=[min(runs), max(runs)])))
        pair("sample_fwd", shape, lambda: lib.sr_texture_sample_fwd(out, tex, uvmap, cover, *dims, -1.0),
             lambda: lib.sr_mip_sample_fwd(out, pyr, uvmap, cover, lod, *mdims, -1.0), args.iters, args.rounds)
        pair("sample_bwd_uv", shape, lambda: lib.sr_texture_sample_bwd_uv(guv, g, tex, uvmap, cover, *dims),
             lambda: lib.sr_mip_sample_bwd_uv(guv, g, pyr, uvmap, cover, lod, *mdims), args.iters, args.rounds)
        pair("sample_bwd_tex / _bwd_pyr", shape,
             lambda: lib.sr_texture_sample_bwd_tex(gtex, g, uvmap, cover, off, entries, *dims),
             lambda: lib.sr_mip_sample_bwd_pyr(gpyr, g, uvmap, cover, lod, moff, mentries, *mdims), args.iters, args.rounds)
        # one refinement step: all views on one texture
        target = torch.rand(batch, c_n, s, s, device=dev) * 2 - 1
        views = [(uvmap[k:k + 1].contiguous(), cover[k:k + 1].contiguous(), target[k:k + 1]) for k in range(batch)]
        start_tex = torch.zeros(1, c_n, t, t, device=dev)
        steps = max(args.iters // 4, 10)

        def refine(mip):
            reconstruct.texture_refine(start_tex, views, 3, mip=mip)                     # warm-up: the plan, code objects
            torch.cuda.synchronize()
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            reconstruct.texture_refine(start_tex, views, steps, mip=mip)
            end.record()
            torch.cuda.synchronize()
            return begin.elapsed_time(end) / steps * 1e-3

        a, b = [], []
        for _ in range(args.rounds):
            a.append(refine(None))
            b.append(refine(0.0))
        print(json.dumps({"what": "texture_refine step (with the call's set-up spread over %d steps)" % steps, "size": s,
                          "T": t, "views": batch, "plain_seconds": float(np.median(a)), "mip_seconds": float(np.median(b)),
                          "ratio": float(np.median(b) / np.median(a))}))


def quality(args):
    s, t = args.size, args.texture
    v0, tri0 = synth.uv_ellipsoid(16, 14)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri0)
    vp = synth.random_poses(v0, 1)
    v, n = torch.from_numpy(vp).float(), torch.from_numpy(synth.vertex_normals(vp, tri0)).float()
    tri = torch.from_numpy(tri0)
    uvmap, cover = texture.uv_map(v, tri, uv, tri_uv, s, keep)
    detail = torch.from_numpy(synth.det_uniform((1, 3, t, t), 77).astype(np.float32))       # texel-scale detail
    lod = texture.mip_lod(uvmap, cover, (t, t))
    live = cover & torch.isfinite(uvmap).all(-1)
    print(json.dumps(dict(what="scene", size=s, T=t, covered_pixels=int(cover.sum()), mean_lod=float(lod[live].mean()),
                          max_lod=float(lod[live].max()))))
    # 1. the share of the seen texels that take a gradient in one refinement step
    # (the seen texels: a bake of this view gives them weight > 0)
    face, coeff = texture.texel_map(uv, tri_uv, t, keep)
    weight = texture.bake(v, n, tri, face, coeff, torch.zeros(1, 3, s, s), texture.depth_buffer(v, tri, s))[1]
    region = (face >= 0) & (weight[0, 0] > 0)
    target = torch.zeros(1, 3, s, s)
    on = cover.unsqueeze(1).float()
    grads = {}
    for name, mip in (("plain", None), ("mip", 0.0)):
        p = detail.clone().requires_grad_(True)
        img = texture.sample(p, uvmap, cover) if mip is None else texture.sample_mip(p, uvmap, cover, bias=mip)
        (grad,) = torch.autograd.grad((((img - target) * on) ** 2).sum(), p)
        grads[name] = (grad != 0).any(1)[0]
    print(json.dumps(dict(what="share of texels with a non-zero gradient in one refine step", region_texels=int(region.sum()),
                          plain=float(grads["plain"][region].float().mean()), mip=float(grads["mip"][region].float().mean()))))
    # 2. the re-render error against a supersampled draw
    fine_uv, fine_cover = texture.uv_map(v, tri, uv, tri_uv, 4 * s, keep)
    fine = texture.sample(detail, fine_uv, fine_cover, 0.0)
    ref = torch.nn.functional.avg_pool2d(fine, 4)
    whole = torch.nn.functional.avg_pool2d(fine_cover.float().unsqueeze(1), 4)[:, 0] == 1
    counted = cover & whole
    err = {}
    for name, img in (("plain", texture.sample(detail, uvmap, cover)), ("mip", texture.sample_mip(detail, uvmap, cover))):
        err[name] = float(((img - ref).abs() * counted.unsqueeze(1)).sum()) / (int(counted.sum()) * 3)
    print(json.dumps(dict(what="rerender error against a 4x supersampled bilinear draw averaged down",
                          counted_pixels=int(counted.sum()), plain=err["plain"], mip=err["mip"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quality", action="store_true", help="the two quality numbers, on the host")
    ap.add_argument("--size", type=int, default=None)
    ap.add_argument("--texture", type=int, default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.quality:
        args.size, args.texture = args.size or 64, args.texture or 128
        quality(args)
    else:
        args.size, args.texture = args.size or 256, args.texture or 512
        timings(args)


if __name__ == "__main__":
    main()
