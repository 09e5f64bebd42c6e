"""Face reconstruction on one GPU: the fit-shape inversion (LatentInverter(fit_shape=True), W+ + pose + 3DMM coefficients)
against the pose-only inversion (BASELINE config[4]) at 256^2 on the face-sized synthetic 3DMM (d = 80 + 64), and the
device time of the morphable-mesh node's kernels (csrc/morph.hip).

    python scripts/bench_reconstruct.py [--steps 100] [--rounds 3] [--reps 50] [--batch 1,4,8,16]
        [--face morph|flame|facewarehouse]

One JSON line per measurement:
  * inversion: replayed steps/s of both inverters in the same process (hipGraph replays, alternated in --rounds rounds
    of --steps replays each; the median round counts), launches per step (kernel nodes of the captured graph) and the
    ratio fit-shape / pose-only;
  * kernels: device time per call (CUDA events) of sr_morph_fwd, sr_vertex_normals_bwd_f32 and sr_morph_gcoeff (both
    passes), WARM (back-to-back calls: W = fc.weight, 42.8 MB, stays in the 256 MiB Infinity Cache) and COLD (a 512 MiB
    write between calls evicts it; only the call itself is between the events), with the HBM bytes each call must move
    at least and the achieved bytes/s against the 8 TB/s peak.

With --batch B1,B2,... only the batched fit-shape inverter is measured instead (one line per batch size): B images in one
captured step, replayed --steps times per round, --rounds rounds, the median round; replayed ms per step, image-steps/s
(B steps per replay) and kernel nodes per captured step.

With --face flame the skinned fit (op.skin on train.synthetic_flame_dict: the same mesh, shape_dim 144, five joints in
FLAME's tree) is measured against the linear fit-shape step in the same process, rounds alternated, the median round:
steps/s and kernel nodes of both, their ratio, and the warm device time per call of the node's new kernels
(sr_skin_joints_fwd, sr_skin_fwd, sr_skin_bwd, sr_skin_joints_bwd).

With --face facewarehouse a synthetic bilinear blendshape model at FaceWarehouse's own dimensions (ds = 149, de = 46,
nv = 11 510: W = 974 MB, train.synthetic_facewarehouse_dict on a UV ellipsoid of that many vertices) is fitted at the
batch sizes of --batch (default 1,8): image-steps/s and kernel nodes per captured step; then the two contraction kernels
alone (sr_blend_fwd, sr_blend_gz) at the same batch sizes: device time, bytes of W / time, and next to it the rate of a
device-to-device copy of the same number of bytes timed in the same run.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylerenderer_amd import _lib, inversion, lpips, model, synth, train, utils_3d  # noqa: E402
from stylerenderer_amd.op import morph  # noqa: E402

HBM_BYTES_PER_S = 8.0e12
DEV = torch.device("cuda:0")


def make_inverters(size):
    g = model.GeneratorWithMap(size, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=7)
    g = g.to(DEV)
    src = train.SyntheticFaceSource(DEV)
    fm, tri = src.model, src.tri
    net = lpips.PNetLin().to(DEV)
    noise = [torch.from_numpy(synth.det_normal(tuple(n.shape), 300 + i)).to(DEV) for i, n in enumerate(g.make_noise())]
    with torch.no_grad():
        c_true = torch.from_numpy(synth.det_normal((1, fm.sigma.numel()), 8)).to(DEV) * fm.sigma
        pose = torch.tensor([[0.2, -0.1, 0.0, 0.0, 0.0, 0.0, 0.0]], device=DEV)
        v, n, _ = morph.morph_mesh(fm, c_true, pose, tri)
        w_true = g.style(torch.from_numpy(synth.det_normal((1, 512), 9)).to(DEV)).unsqueeze(1).repeat(1, g.n_latent, 1)
        target, _, _ = g([w_true], (v, n, tri), input_is_latent=True, noise=noise)
        zero = torch.zeros(1, fm.sigma.numel(), device=DEV)
        v0, n0, _ = morph.morph_mesh(fm, zero, torch.zeros(1, 7, device=DEV), tri)       # the mean face
    common = dict(lr=0.05, pose_lr=0.01, noise=noise, n_mean_latent=4096, use_graph=True)
    torch.manual_seed(11)
    pose_only = inversion.LatentInverter(g, net, target, (v0, n0, tri), **common)
    torch.manual_seed(11)
    fit_shape = inversion.LatentInverter(g, net, target, None, face=(fm, tri), fit_shape=True, coeff_lr=0.05,
                                         shape_reg=1e-3, **common)
    return {"pose_only": pose_only, "fit_shape": fit_shape}, fm, tri


def bench_inversion(size, steps, rounds):
    invs, _, _ = make_inverters(size)
    for inv in invs.values():
        inv.run(8)                                     # warm-up iterations + capture
        torch.cuda.synchronize()
    rates = {k: [] for k in invs}
    for _ in range(rounds):
        for k, inv in invs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                inv.graph.replay()
            b.record()
            torch.cuda.synchronize()
            rates[k].append(steps * 1000.0 / a.elapsed_time(b))
    out = {"what": "inversion", "size": size, "steps_per_round": steps, "rounds": rounds}
    for k, inv in invs.items():
        out[k + "_steps_per_s"] = round(statistics.median(rates[k]), 2)
        out[k + "_rounds"] = [round(r, 2) for r in rates[k]]
        out[k + "_launches_per_step"] = inv.graph.kernel_nodes
    out["ratio_fit_over_pose"] = round(out["fit_shape_steps_per_s"] / out["pose_only_steps_per_s"], 4)
    print(json.dumps(out), flush=True)


def bench_batches(size, batches, steps, rounds):
    invs, fm, tri = make_inverters(size)
    base = invs["pose_only"]
    g, net, noise, target = base.g, base.perceptual, base.noise, base.target
    del invs, base
    for b in batches:
        torch.cuda.empty_cache()
        torch.manual_seed(11)
        inv = inversion.LatentInverter(g, net, target.expand(b, -1, -1, -1).contiguous(), None, lr=0.05, pose_lr=0.01,
                                       noise=noise, n_mean_latent=4096, use_graph=True, face=(fm, tri), fit_shape=True,
                                       coeff_lr=0.05, shape_reg=1e-3)
        inv.run(8)                                     # warm-up iterations + capture
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                inv.graph.replay()
            e.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(e) / steps)
        t = statistics.median(ms)
        print(json.dumps({"what": "batched_inversion", "size": size, "batch": b, "steps_per_round": steps,
                          "rounds": rounds, "ms_per_step": round(t, 4), "steps_per_s": round(1000.0 / t, 2),
                          "image_steps_per_s": round(b * 1000.0 / t, 2), "rounds_ms": [round(x, 4) for x in ms],
                          "kernel_nodes_per_step": inv.graph.kernel_nodes}), flush=True)
        del inv


def event_time(fn, reps, flush=None):
    ts = []
    fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        if flush is not None:
            flush.fill_(1.0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts)


def bench_kernels(reps):
    src = train.SyntheticFaceSource(DEV)
    fm, tri = src.model, src.tri
    w, bias, sigma = fm.fc.weight.detach().contiguous(), fm.fc.bias.detach().contiguous(), fm.sigma.detach().contiguous()
    nv, d, b = bias.numel() // 3, w.shape[1], 1
    c = (torch.from_numpy(synth.det_normal((b, d), 8)).to(DEV) * sigma).contiguous()
    pose = torch.tensor([[0.2, -0.1, 0.05, 0.01, 0.02, 0.0, 0.1]], device=DEV)
    off, adj, _ = utils_3d.incidence_lists(tri, nv)
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.current_stream(DEV)
    lin, rot = torch.empty(b, 3, 3, device=DEV), torch.empty(b, 3, 3, device=DEV)
    vs, v, ns, n = (torch.empty(b, nv, 3, device=DEV) for _ in range(4))
    normc, reg = torch.empty(b, nv, device=DEV), torch.empty((), device=DEV)
    gv, gn = torch.randn(b, nv, 3, device=DEV), torch.randn(b, nv, 3, device=DEV)
    gvs, gc, greg = torch.empty(b, nv, 3, device=DEV), torch.empty(b, d, device=DEV), torch.ones((), device=DEV)
    scratch = torch.empty(int(L.sr_morph_gcoeff_scratch_floats(3 * nv, b, d)), device=DEV)
    _lib.check(L.sr_pose_batch_fwd(ptr(lin), ptr(rot), ptr(pose), b, st))
    calls = {
        "sr_morph_fwd": (lambda: L.sr_morph_fwd(ptr(v), ptr(vs), ptr(reg), ptr(w), ptr(bias), ptr(c), ptr(lin), ptr(pose),
                                                ptr(sigma), 1e-3, b, nv, d, st),
                         # W + bias + vs + v
                         4 * (w.numel() + bias.numel() + 2 * 3 * nv * b)),
        "sr_vertex_normals_bwd_f32": (lambda: L.sr_vertex_normals_bwd_f32(
            ptr(gvs), ptr(gv), ptr(gn), ptr(lin), ptr(rot), ptr(vs), ptr(ns), ptr(normc), ptr(tri), ptr(off), ptr(adj),
            b, nv, tri.size(0), 1e-8, st),
            # gv, gn, vs, ns, normc, gvs + tri + CSR lists (each read once at best)
            4 * (5 * 3 * nv * b + nv * b) + 8 * tri.numel() + 4 * (adj.numel() + off.numel())),
        "sr_morph_gcoeff": (lambda: L.sr_morph_gcoeff(ptr(gc), ptr(scratch), ptr(w), ptr(gvs), ptr(c), ptr(sigma), 1e-3,
                                                      ptr(greg), b, 3 * nv, d, st),
                            4 * (w.numel() + 3 * nv * b + 2 * scratch.numel())),
    }
    _lib.check(L.sr_vertex_normals_f32(ptr(ns), ptr(normc), ptr(vs), ptr(tri), ptr(off), ptr(adj), b, nv, tri.size(0),
                                       1e-8, st))
    flush = torch.empty(128 * 1024 * 1024, device=DEV)              # 512 MiB: twice the Infinity Cache
    for name, (fn, nbytes) in calls.items():
        for state, fl in (("warm", None), ("cold", flush)):
            t = event_time(fn, reps, fl)
            print(json.dumps({"what": "kernel", "name": name, "cache": state, "nv": nv, "d": d, "B": b,
                              "us": round(t * 1e6, 2), "hbm_bytes": int(nbytes),
                              "bytes_per_s": round(nbytes / t / 1e12, 3) * 1e12,
                              "share_of_8TBps": round(nbytes / t / HBM_BYTES_PER_S, 3)}), flush=True)


def bench_flame(size, steps, rounds, reps):
    from stylerenderer_amd import face_model
    from stylerenderer_amd.op import skin

    invs, _, _ = make_inverters(size)
    base = invs.pop("pose_only")
    g, net, noise, target = base.g, base.perceptual, base.noise, base.target
    del base
    fm, tri = face_model.load_flame(train.synthetic_flame_dict())
    fm, tri = fm.to(DEV), tri.to(DEV)
    torch.manual_seed(11)
    invs["fit_flame"] = inversion.LatentInverter(g, net, target, None, lr=0.05, pose_lr=0.01, noise=noise,
                                                 n_mean_latent=4096, use_graph=True, face=(fm, tri), fit_shape=True,
                                                 coeff_lr=0.05, shape_reg=1e-3)
    for inv in invs.values():
        inv.run(8)
        torch.cuda.synchronize()
    rates = {k: [] for k in invs}
    for _ in range(rounds):
        for k, inv in invs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                inv.graph.replay()
            b.record()
            torch.cuda.synchronize()
            rates[k].append(steps * 1000.0 / a.elapsed_time(b))
    out = {"what": "inversion_flame", "size": size, "steps_per_round": steps, "rounds": rounds}
    for k, inv in invs.items():
        out[k + "_steps_per_s"] = round(statistics.median(rates[k]), 2)
        out[k + "_rounds"] = [round(r, 2) for r in rates[k]]
        out[k + "_kernel_nodes"] = inv.graph.kernel_nodes
    out["ratio_flame_over_morph"] = round(out["fit_flame_steps_per_s"] / out["fit_shape_steps_per_s"], 4)
    out["extra_kernel_nodes"] = out["fit_flame_kernel_nodes"] - out["fit_shape_kernel_nodes"]
    print(json.dumps(out), flush=True)
    # the node's new kernels, warm
    b = 1
    stt, tmpl, wts, j0, js, parent, sigma, pinv = skin._native_args(fm)
    nv, nj, ds = tmpl.numel() // 3, j0.shape[0], fm.dim[0]
    dfull = stt.shape[1]
    c = torch.from_numpy(synth.det_normal((b, ds + 3 * (nj - 1)), 8)).to(DEV) * 0.2
    pose = torch.tensor([[0.2, -0.1, 0.05, 0.01, 0.02, 0.0, 0.1]], device=DEV)
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.current_stream(DEV)
    cx, tg, chain = torch.empty(b, dfull, device=DEV), torch.empty(b, nj, 12, device=DEV), torch.empty(b, nj, 15, device=DEV)
    reg, greg = torch.empty((), device=DEV), torch.ones((), device=DEV)
    v, vp, gvp = (torch.empty(b, nv, 3, device=DEV) for _ in range(3))
    gv, gvn = torch.randn(b, nv, 3, device=DEV), torch.randn(b, nv, 3, device=DEV)
    nblk = (nv + 255) // 256
    part = torch.empty(int(L.sr_skin_bwd_scratch_floats(nv, b, nj)), device=DEV)
    gcx, gc, gp = torch.randn(b, dfull, device=DEV), torch.empty_like(c), torch.empty_like(pose)
    calls = {
        "sr_skin_joints_fwd": lambda: L.sr_skin_joints_fwd(ptr(cx), ptr(tg), ptr(chain), ptr(reg), ptr(c), ptr(pose),
                                                           ptr(j0), ptr(js), ptr(parent), ptr(sigma), ptr(pinv), 1e-3, b,
                                                           nj, 1, ds, st),
        "sr_skin_fwd": lambda: L.sr_skin_fwd(ptr(v), ptr(vp), ptr(stt), ptr(tmpl), ptr(cx), ptr(wts), ptr(tg), b, nv,
                                             dfull, nj, st),
        "sr_skin_bwd": lambda: L.sr_skin_bwd(ptr(gvp), ptr(part), ptr(gv), ptr(gvn), ptr(vp), ptr(wts), ptr(tg), b, nv,
                                             nj, st),
        "sr_skin_joints_bwd": lambda: L.sr_skin_joints_bwd(ptr(gc), ptr(gp), ptr(gcx), ptr(part), ptr(c), ptr(pose),
                                                           ptr(chain), ptr(js), ptr(parent), ptr(sigma), ptr(pinv), 1e-3,
                                                           ptr(greg), b, nblk, nj, 1, ds, st),
    }
    for name, fn in calls.items():
        _lib.check(fn(), name)
        t = event_time(fn, reps)
        print(json.dumps({"what": "kernel", "name": name, "cache": "warm", "nv": nv, "D": dfull, "nj": nj, "B": b,
                          "us": round(t * 1e6, 2)}), flush=True)


def bench_facewarehouse(size, batches, steps, rounds, reps):
    from stylerenderer_amd import face_model
    from stylerenderer_amd.op import blend
    from stylerenderer_amd.op._dispatch import native

    invs, _, _ = make_inverters(size)
    base = invs.pop("pose_only")
    g, net, noise, target = base.g, base.perceptual, base.noise, base.target
    del base, invs
    ds, de = 149, 46
    fm, tri = face_model.load_facewarehouse(train.synthetic_facewarehouse_dict(ds, de, mesh=synth.uv_ellipsoid(138, 84)), 2.0)
    fm, tri = fm.to(DEV), tri.to(DEV)
    nv = fm.dim[2] // 3
    w_bytes = fm.weight.numel() * 4
    for b in batches:
        torch.cuda.empty_cache()
        torch.manual_seed(11)
        inv = inversion.LatentInverter(g, net, target.expand(b, -1, -1, -1).contiguous(), None, lr=0.05, pose_lr=0.01,
                                       noise=noise, n_mean_latent=4096, use_graph=True, face=(fm, tri), fit_shape=True,
                                       coeff_lr=0.05, shape_reg=1e-3)
        inv.run(8)
        torch.cuda.synchronize()
        ms = []
        for _ in range(rounds):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                inv.graph.replay()
            e.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(e) / steps)
        t = statistics.median(ms)
        print(json.dumps({"what": "inversion_facewarehouse", "size": size, "batch": b, "nv": nv, "ds": ds, "de": de,
                          "w_bytes": w_bytes, "ms_per_step": round(t, 4), "image_steps_per_s": round(b * 1000.0 / t, 2),
                          "rounds_ms": [round(x, 4) for x in ms], "kernel_nodes_per_step": inv.graph.kernel_nodes}),
              flush=True)
        del inv
    L, ptr, st = _lib.lib(), _lib.ptr, _lib.current_stream(DEV)
    src = torch.empty(w_bytes // 4, device=DEV)
    dst = torch.empty_like(src)
    t_copy = event_time(lambda: dst.copy_(src), reps)
    del dst, src
    print(json.dumps({"what": "copy", "bytes": w_bytes, "us": round(t_copy * 1e6, 2),
                      "bytes_per_s": round(w_bytes / t_copy / 1e12, 3)}), flush=True)
    for b in batches:
        c = torch.from_numpy(synth.det_normal((b, ds + de), 8)).to(DEV)
        pose = torch.zeros(b, 7, device=DEV)
        lin = torch.eye(3, device=DEV).repeat(b, 1, 1).contiguous()
        xs, xe, prior, z = blend._head(native(c), c, fm.beta.detach(), 1e-3, ds, de)
        v, vs, gvs = (torch.randn(b, nv, 3, device=DEV) for _ in range(3))
        reg = torch.empty((), device=DEV)
        gz = torch.empty(b, (ds + 1) * (de + 1), device=DEV)
        calls = {
            "sr_blend_fwd": lambda: L.sr_blend_fwd(ptr(v), ptr(vs), ptr(reg), ptr(fm.weight), ptr(z), ptr(prior), ptr(lin),
                                                   ptr(pose), b, nv, ds, de, st),
            "sr_blend_gz": lambda: L.sr_blend_gz(ptr(gz), ptr(fm.weight), ptr(gvs), b, nv, ds, de, st),
        }
        for name, fn in calls.items():
            _lib.check(fn(), name)
            t = event_time(fn, reps)
            print(json.dumps({"what": "kernel", "name": name, "B": b, "nv": nv, "w_bytes": w_bytes, "us": round(t * 1e6, 2),
                              "w_bytes_per_s": round(w_bytes / t / 1e12, 3),
                              "over_copy_rate": round(t_copy / t, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--batch", default=None, metavar="B1,B2,...",
                    help="measure the batched fit-shape inverter at these batch sizes instead")
    ap.add_argument("--face", choices=("morph", "flame", "facewarehouse"), default="morph",
                    help="flame: the skinned fit against the linear fit-shape step, and the skinning kernels; "
                         "facewarehouse: the blendshape fit at FaceWarehouse's dimensions and its contraction kernels")
    args = ap.parse_args()
    os.environ.setdefault("SR_STRICT_NATIVE", "1")
    if args.face == "facewarehouse":
        bench_facewarehouse(args.size, [int(x) for x in (args.batch or "1,8").split(",")], args.steps, args.rounds,
                            args.reps)
        return
    if args.face == "flame":
        bench_flame(args.size, args.steps, args.rounds, args.reps)
        return
    if args.batch:
        bench_batches(args.size, [int(x) for x in args.batch.split(",")], args.steps, args.rounds)
        return
    bench_kernels(args.reps)
    bench_inversion(args.size, args.steps, args.rounds)


if __name__ == "__main__":
    main()
