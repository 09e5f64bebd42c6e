"""TEST INFRASTRUCTURE — writes tests/golden/reconstruct_morph.npz and tests/golden/reconstruct_obj_<form>.obj by RUNNING
THE REFERENCE where its sources lie.  Never imported by a test (the reference does not exist on the GPU machine).
Re-run:  python tests/make_golden_reconstruct.py

* The morphable mesh is the reference's face_model.LinearMorphableModel (constructed with the bases of
  tests/reconstruct_cases.py), posed with its utils_3d.euler_mat(., "yxz") as random_apply_pose3D does
  (v @ (exp(s) R) + t), normals by its utils_3d.mesh_point_normal, prior by its LinearMorphableModel.regulation.
* Stored per case: v, n (the vertex sample of the case) and the gradients w.r.t. coeff and pose of
      L = sum(v * gv) + sum(n * gn) + REG_WEIGHT * regulation(coeff)
  from a float64 run, and the reference's own float32-vs-float64 relative errors of each (the tests' bars).
* The .obj files are the reference's utils_3d.save_obj output for the four face-record forms.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import reconstruct_cases as rc  # noqa: E402
import ref_shim  # noqa: E402

OUT = os.path.join(HERE, "golden")


def reference_modules():
    ref_shim.load()                       # the reference's op / layers importable on this host
    sys.path.insert(0, ref_shim.REF)
    import face_model as ref_face_model   # noqa: E402
    import utils_3d as ref_utils_3d       # noqa: E402

    return ref_face_model, ref_utils_3d


def run_reference(fm, u3d, name, dtype):
    v0, tri, wsh, wex, cu, pose, gv, gn, idx = rc.case(name)
    _, ds, de, b, _ = rc.CASES[name]
    model = fm.LinearMorphableModel(v0.shape[0], ds, de, v0, wsh, wex).to(dtype)
    with torch.no_grad():           # sigma as float32 values (as a float32-built model holds them) in both runs
        model.sigma.copy_(model.sigma.float())
    coeff = (torch.from_numpy(cu).to(dtype) * model.sigma.detach()).requires_grad_(True)
    p = torch.from_numpy(pose).to(dtype).requires_grad_(True)
    trit = torch.from_numpy(tri)
    vs = model(coeff)
    T = torch.exp(p[:, 6]).view(-1, 1, 1) * u3d.euler_mat(p[:, :3], "yxz")
    v = torch.matmul(vs, T) + p[:, 3:6].view(-1, 1, 3)
    n = u3d.mesh_point_normal(v, trit)
    loss = ((v * torch.from_numpy(gv).to(dtype)).sum() + (n * torch.from_numpy(gn).to(dtype)).sum()
            + rc.REG_WEIGHT * model.regulation(coeff))
    gc, gp = torch.autograd.grad(loss, (coeff, p))
    out = {"v": v[:, idx], "n": n[:, idx], "gcoeff": gc, "gpose": gp}
    return {k: t.detach().double().numpy() for k, t in out.items()}


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def main():
    fm, u3d = reference_modules()
    arrays = {}
    for name in rc.CASES:
        # mesh_point_normal builds its sparse incidence values with torch.ones (default dtype): float64 default for the
        # float64 run, or sparse.mm refuses the mix
        torch.set_default_dtype(torch.float64)
        try:
            r64 = run_reference(fm, u3d, name, torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        r32 = run_reference(fm, u3d, name, torch.float32)
        for k in r64:
            arrays["%s_%s" % (name, k)] = r64[k]
            arrays["%s_%s_err32" % (name, k)] = np.float64(rel(r32[k], r64[k]))
            print("%-6s %-7s shape %-16s ref fp32 vs fp64 rel err %.3e" % (name, k, r64[k].shape, rel(r32[k], r64[k])))
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "reconstruct_morph.npz"), **arrays)
    for form in rc.OBJ_FORMS:
        kw, v, tri = rc.obj_args(form)
        path = os.path.join(OUT, "reconstruct_obj_%s.obj" % form)
        u3d.save_obj(path, v, tri, **kw)
        print("wrote", path, os.path.getsize(path), "bytes")
    print("wrote", os.path.join(OUT, "reconstruct_morph.npz"), os.path.getsize(os.path.join(OUT, "reconstruct_morph.npz")))


if __name__ == "__main__":
    main()
