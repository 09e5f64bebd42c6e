"""Records what LatentInverter computes on the tests' tiny problem, over the matrix of its optional parts, and compares two
recordings bit for bit: the check that a restructuring of the inverter changes no number and no captured graph.

    python scripts/record_inverter.py record OUT.npz [--device cpu|cuda] [--configs 3,5] [--nodes OUT.json --commit HASH]
    python scripts/record_inverter.py compare A.npz B.npz

`record` runs in the tree it is started from (the same file copied into a checkout of another commit records that commit).
The problem is tests/test_reconstruct_batch_cpu.batch_problem (16 x 16 targets, the 14-coefficient model) with
make_inverter's settings (n_mean_latent=64, seed 3; the perceptual network on the device, as the GPU tests build it),
test_landmark_cpu.tiny_landmarks and test_landmark_dynamic_cpu.tiny_lines.  Every configuration of CONFIGS runs STEPS
steps, then `reset` to the targets flipped along the batch (same landmarks and mask) and STEPS more.  Stored per
configuration and run: the loss history, the final w, pose, coeff and kappa, landmarks_fit, contour_fit,
landmark_visibility and mask_fit where they exist, fitted_mesh() and fitted_mesh(projected=False); on cuda in eager and in
graph mode, with the captured step's kernel nodes.  On the CPU the script runs with one thread: with several the B = 1
fits are not reproducible from one process to the next.  --nodes writes the graph mode's node counts (integers only) and the
commit they were recorded at: tests/golden/inverter_nodes_parent.json.

`compare` demands the same keys, and every array equal bit for bit (node counts are arrays of one integer); it prints the
first difference and exits 1 on one.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEPS = 6
# number -> (name, batch, generator with a map, fit_shape)
CONFIGS = {1: ("fixed_b1", 1, True, False), 2: ("shape_b1", 1, True, True), 3: ("shape_b3", 3, True, True),
           4: ("landmarks", 3, True, True), 5: ("landmarks_pose_aware", 3, True, True), 6: ("mask_mesh", 3, True, True),
           7: ("shared_identity", 3, True, True), 8: ("camera_fixed", 3, True, True),
           9: ("camera_fitted_landmarks", 3, True, True), 10: ("plain_generator_landmarks", 3, False, True),
           11: ("mask_mesh_b1", 1, True, True)}
_PROBLEMS = {}


def problem(device):
    """batch_problem on `device`, the plain Generator of the same size, and the host's face model for the landmarks."""
    if device not in _PROBLEMS:
        from test_inversion_cpu import tiny_setup
        from test_reconstruct_batch_cpu import batch_problem

        host = batch_problem("cpu")
        _PROBLEMS[device] = (host if device == "cpu" else batch_problem(device), tiny_setup(device, with_map=False)[0],
                             host[2])
    return _PROBLEMS[device]


def keywords(number, device):
    """The inverter's keywords of configuration `number` beyond make_inverter's."""
    from test_landmark_cpu import tiny_landmarks
    from test_landmark_dynamic_cpu import tiny_lines

    batch = CONFIGS[number][1]
    host_face = problem(device)[2]
    kw = {}
    if number in (4, 5, 9, 10):
        emb, lmk = tiny_landmarks(host_face)
        kw.update(landmarks=np.stack([lmk] * batch), landmark_embedding=emb)
    if number == 5:
        lines, axis = tiny_lines(host_face, kw["landmark_embedding"])
        kw.update(landmark_lines=lines, landmark_axis=axis)
    if number in (5, 9):
        kw.update(landmark_vis=(0.0, 0.2))
    if number in (6, 11):
        box = torch.zeros(batch, 1, 16, 16, device=device)
        box[:, :, 4:12, 3:13] = 1.0
        kw.update(mask=box, mask_mesh=True)
    if number == 7:
        kw.update(shared_identity=10)
    if number == 8:
        kw.update(camera=0.25)
    if number == 9:
        kw.update(camera=[0.1, 0.25, 0.4], fit_camera=True, camera_lr=0.02)
    return kw


def make(number, device, use_graph):
    """(inverter, its targets, the landmarks and mask a reset takes) of configuration `number`."""
    from stylerenderer_amd import inversion, lpips

    (g, mesh, face, noise, targets), plain_g, _ = problem(device)
    _, batch, with_map, fit_shape = CONFIGS[number]
    kw = keywords(number, device)
    if fit_shape:
        kw.update(face=face, fit_shape=True, coeff_lr=0.05, shape_reg=1e-3)
    targets = targets[:batch].contiguous()
    torch.manual_seed(3)                                      # the mean latent's draws
    inv = inversion.LatentInverter(g if with_map else plain_g, lpips.PNetLin().to(device), targets,
                                   None if fit_shape else mesh, lr=0.05, pose_lr=0.02, noise=noise, n_mean_latent=64,
                                   use_graph=use_graph, **kw)
    again = {k: kw[k] for k in ("landmarks", "mask") if k in kw}
    return inv, targets, again


def state(inv, hist):
    out = {"history": hist, "w": inv.w, "pose": inv.pose, "coeff": inv.coeff, "kappa": inv.camera,
           "landmarks_fit": inv.landmarks_fit, "contour_fit": inv.contour_fit,
           "landmark_visibility": inv.landmark_visibility, "mask_fit": inv.mask_fit}
    out["fitted_v"], out["fitted_n"], _ = inv.fitted_mesh()
    out["camera_space_v"], out["camera_space_n"], _ = inv.fitted_mesh(projected=False)
    return {k: t.detach().cpu().numpy().copy() for k, t in out.items() if t is not None}


def run(number, device, use_graph):
    """{key: array} of configuration `number`: both runs' state and, in graph mode, the kernel nodes."""
    inv, targets, again = make(number, device, use_graph)
    out = {"first/" + k: a for k, a in state(inv, inv.run(STEPS)).items()}
    inv.reset(targets.flip(0).contiguous(), **again)
    out.update(("second/" + k, a) for k, a in state(inv, inv.run(STEPS)).items())
    if use_graph:
        out["kernel_nodes"] = np.array([inv.graph.kernel_nodes], np.int64)
    return out


def record(path, device, numbers, nodes_path=None, commit=None):
    if device == "cpu":
        torch.set_num_threads(1)
    else:
        os.environ.setdefault("SR_STRICT_NATIVE", "1")        # as the GPU suite runs: no library fallback
    arrays, nodes = {}, {}
    for number in numbers:
        for mode in ("eager", "graph") if device != "cpu" else ("eager",):
            got = run(number, device, mode == "graph")
            arrays.update(("%02d_%s/%s/%s" % (number, CONFIGS[number][0], mode, k), a) for k, a in got.items())
            if mode == "graph":
                nodes[CONFIGS[number][0]] = int(got["kernel_nodes"][0])
            print("recorded %2d %-28s %-5s last loss %s%s" % (
                number, CONFIGS[number][0], mode, np.array2string(got["second/history"][-1], precision=6),
                "  kernel nodes %d" % nodes[CONFIGS[number][0]] if mode == "graph" else ""), flush=True)
    np.savez(path, **arrays)
    if nodes_path is not None:
        with open(nodes_path, "w") as f:
            json.dump({"recorded_at_commit": commit, "steps": STEPS, "kernel_nodes": nodes}, f, indent=1, sort_keys=True)
            f.write("\n")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    if sorted(a.files) != sorted(b.files):
        print("DIFFERENT keys: only in one of them:", sorted(set(a.files) ^ set(b.files))[:8])
        return 1
    for key in sorted(a.files):
        x, y = a[key], b[key]
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            where = ""
            if x.shape == y.shape and x.dtype == y.dtype:
                differ = np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)
                i = np.flatnonzero(differ.reshape(-1, x.dtype.itemsize).any(1))
                where = ": %d of %d elements, the first at %d: %r and %r" % (i.size, x.size, i[0], x.reshape(-1)[i[0]],
                                                                            y.reshape(-1)[i[0]])
            print("DIFFERENT %s %s %s / %s %s%s" % (key, x.dtype, x.shape, y.dtype, y.shape, where))
            return 1
    print("identical: %d arrays, %d of them node counts, bit for bit" % (
        len(a.files), sum(k.endswith("kernel_nodes") for k in a.files)))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    rec = sub.add_parser("record")
    rec.add_argument("out")
    rec.add_argument("--device", default="cpu", choices=("cpu", "cuda"))
    rec.add_argument("--configs", default=",".join(str(k) for k in CONFIGS), help="numbers of the matrix, comma-separated")
    rec.add_argument("--nodes", default=None, help="also write the graph mode's kernel nodes to this .json (cuda)")
    rec.add_argument("--commit", default=None, help="the commit of the recorded tree, for --nodes")
    cmp_ = sub.add_parser("compare")
    cmp_.add_argument("a")
    cmp_.add_argument("b")
    args = ap.parse_args()
    if args.mode == "compare":
        sys.exit(compare(args.a, args.b))
    record(args.out, args.device, [int(k) for k in args.configs.split(",")], args.nodes, args.commit)


if __name__ == "__main__":
    main()
