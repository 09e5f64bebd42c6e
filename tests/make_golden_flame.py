"""TEST INFRASTRUCTURE — writes tests/golden/flame_skin.npz by RUNNING THE REFERENCE where its sources lie.  Never imported
by a test (the reference does not exist on the GPU machine).  Re-run:  python tests/make_golden_flame.py

* The skinned mesh is the reference's face_model.load_flame on the FLAME-shaped dict of tests/flame_cases.py, its
  LinearBlendSkinningModel.forward, posed with its utils_3d.euler_mat(., "yxz") (v @ (exp(s) R) + t), normals by its
  utils_3d.mesh_point_normal, prior by its regulation.  The reference holds the model's four arrays and pose_inv outside
  the module, so the float64 run converts them by hand.
* Stored per case: v, n (the vertex sample of the case), the gradients w.r.t. coeff and pose of
      L = sum(v * gv) + sum(n * gn) + REG_WEIGHT * regulation(coeff)
  and regulation(coeff), from a float64 run, and the reference's own float32-vs-float64 relative errors (the tests' bars).
  The coefficient gradient is also stored in its two parts, of the data term and of regulation(coeff) alone, with the
  reference's fp32 errors per block (shape, joints: flame_cases.block_errors) and entry by entry for the prior: FLAME's
  eye-roll sigma of 1e-5 degrees makes two prior entries ~1e11, which a max-norm over the whole vector would let hide
  everything else.
* utils_3d.rodrigues values and gradients of sum(R * G) on flame_cases.RODRIGUES_VECTORS (float64).
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
import flame_cases as fc  # noqa: E402
import ref_shim  # noqa: E402

OUT = os.path.join(HERE, "golden")


def reference_modules():
    ref_shim.load()
    sys.path.insert(0, ref_shim.REF)
    import face_model as ref_face_model   # noqa: E402
    import utils_3d as ref_utils_3d       # noqa: E402

    return ref_face_model, ref_utils_3d


def run_reference(fm, u3d, name, dtype):
    d, tri, coeff, pose, gv, gn, idx = fc.case(name)
    model, rtri = fm.load_flame(d)
    assert np.array_equal(rtri.numpy(), tri)
    model = model.to(dtype)
    model.fc = [t.detach().to(dtype) for t in model.fc]
    model.weight = [t.detach().to(dtype) for t in model.weight]
    model.pose_inv = model.pose_inv.detach().to(dtype)
    c = torch.from_numpy(coeff).to(dtype).requires_grad_(True)
    p = torch.from_numpy(pose).to(dtype).requires_grad_(True)
    trit = torch.from_numpy(tri)
    vs = model(c)
    T = torch.exp(p[:, 6]).view(-1, 1, 1) * u3d.euler_mat(p[:, :3], "yxz")
    v = torch.matmul(vs, T) + p[:, 3:6].view(-1, 1, 3)
    n = u3d.mesh_point_normal(v, trit)
    reg = model.regulation(c)
    loss = (v * torch.from_numpy(gv).to(dtype)).sum() + (n * torch.from_numpy(gn).to(dtype)).sum() + fc.REG_WEIGHT * reg
    data = (v * torch.from_numpy(gv).to(dtype)).sum() + (n * torch.from_numpy(gn).to(dtype)).sum()
    gc, gp = torch.autograd.grad(loss, (c, p), retain_graph=True)
    (gc_data,) = torch.autograd.grad(data, c, retain_graph=True)
    (gc_prior,) = torch.autograd.grad(reg, c)
    out = {"v": v[:, idx], "n": n[:, idx], "gcoeff": gc, "gpose": gp, "reg": reg, "gcoeff_data": gc_data,
           "gcoeff_prior": gc_prior}
    return {k: t.detach().double().numpy() for k, t in out.items()}


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def main():
    fm, u3d = reference_modules()
    arrays = {}
    for name in fc.CASES:
        torch.set_default_dtype(torch.float64)      # mesh_point_normal's torch.ones and forward's torch.eye follow it
        try:
            r64 = run_reference(fm, u3d, name, torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        r32 = run_reference(fm, u3d, name, torch.float32)
        for k in r64:
            arrays["%s_%s" % (name, k)] = r64[k]
            arrays["%s_%s_err32" % (name, k)] = np.float64(rel(r32[k], r64[k]))
            print("%-6s %-7s shape %-16s ref fp32 vs fp64 rel err %.3e" % (name, k, r64[k].shape, rel(r32[k], r64[k])))
        # the coefficient gradient block by block (flame_cases.block_errors): the data term, and the prior entry by entry
        ds = fc.CASES[name][1]
        for blk, e in fc.block_errors(r32["gcoeff_data"], r64["gcoeff_data"], ds).items():
            arrays["%s_gcoeff_data_%s_err32" % (name, blk)] = np.float64(e)
            print("%-6s gcoeff_data %-5s ref fp32 vs fp64 rel err %.3e" % (name, blk, e))
        e = fc.elementwise_error(r32["gcoeff_prior"], r64["gcoeff_prior"])
        arrays["%s_gcoeff_prior_elem_err32" % name] = np.float64(e)
        print("%-6s gcoeff_prior elementwise ref fp32 vs fp64 rel err %.3e" % (name, e))
    r = torch.from_numpy(fc.RODRIGUES_VECTORS).requires_grad_(True)
    G = torch.from_numpy(np.arange(9, dtype=np.float64).reshape(1, 3, 3) / 4 - 1) * torch.ones(len(r), 1, 1, dtype=torch.float64)
    R = u3d.rodrigues(r)
    (gr,) = torch.autograd.grad((R * G).sum(), r)
    arrays["rodrigues_R"] = R.detach().numpy()
    arrays["rodrigues_grad"] = gr.numpy()
    r1 = torch.from_numpy(fc.RODRIGUES_VECTORS[3]).requires_grad_(True)          # the [3] -> [3, 3] form
    arrays["rodrigues_R_single"] = u3d.rodrigues(r1).detach().numpy()
    assert np.isfinite(arrays["rodrigues_R"]).all() and np.isfinite(arrays["rodrigues_grad"]).all()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "flame_skin.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
