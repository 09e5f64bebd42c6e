"""TEST INFRASTRUCTURE — writes tests/golden/blendshape.npz by RUNNING THE REFERENCE where its sources lie.  Never imported
by a test (the reference does not exist on the GPU machine).  Re-run:  python tests/make_golden_blendshape.py

* The mesh is the reference's face_model.load_facewarehouse on the FaceWarehouse-shaped dict of tests/blendshape_cases.py
  (for a case whose beta_shape is not the loader's .01: its BlendShapeModel on the loader's own weight with that
  beta_shape), its BlendShapeModel.forward, posed with its utils_3d.euler_mat(., "yxz") (v @ (exp(s) R) + t), normals by
  its utils_3d.mesh_point_normal, prior by its regulation.
* Stored per case: v, n (the vertex sample of the case), regulation(coeff) and the gradients w.r.t. coeff and pose of
      L = sum(v * gv) + sum(n * gn) + REG_WEIGHT * regulation(coeff)
  from a float64 run, the coefficient gradient also in its two parts (of the data term and of regulation(coeff) alone),
  and per array the reference's own float32-vs-float64 relative error (`*_err32`, the tests' bars).  The prior's gradient
  also gets an entry-by-entry error: with beta = .01 its entries span orders of magnitude (a max-norm would let the
  large ones hide the rest), as make_golden_flame.py explains for FLAME's eye-roll sigma.  Every float32 run is checked
  to be finite (the `large` case holds coefficients of magnitude 30).
* state_dict key names and shapes, and the beta vector of the constructor's three argument forms (blendshape_cases.BETA_FORMS).
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
import blendshape_cases as bc  # noqa: E402
import ref_shim  # noqa: E402

OUT = os.path.join(HERE, "golden")


def reference_modules():
    ref_shim.load()
    sys.path.insert(0, ref_shim.REF)
    import face_model as ref_face_model   # noqa: E402
    import utils_3d as ref_utils_3d       # noqa: E402

    return ref_face_model, ref_utils_3d


def reference_model(fm, name):
    d, tri, beta_shape = bc.case(name)[:3]
    _, ds, de = bc.CASES[name][:3]
    model, rtri = fm.load_facewarehouse(d)
    assert np.array_equal(rtri.numpy(), tri) and model.dim[:2] == [ds, de]
    if beta_shape != .01:
        model = fm.BlendShapeModel(d["v"].shape[1], ds, de, model.weight.detach().numpy(), beta_shape)
    return model


def run_reference(fm, u3d, name, dtype):
    _, tri, _, coeff, pose, gv, gn, idx = bc.case(name)
    model = reference_model(fm, name).to(dtype)
    c = torch.from_numpy(coeff).to(dtype).requires_grad_(True)
    p = torch.from_numpy(pose).to(dtype).requires_grad_(True)
    trit = torch.from_numpy(tri)
    vs = model(c)
    T = torch.exp(p[:, 6]).view(-1, 1, 1) * u3d.euler_mat(p[:, :3], "yxz")
    v = torch.matmul(vs, T) + p[:, 3:6].view(-1, 1, 3)
    n = u3d.mesh_point_normal(v, trit)
    reg = model.regulation(c)
    data = (v * torch.from_numpy(gv).to(dtype)).sum() + (n * torch.from_numpy(gn).to(dtype)).sum()
    loss = data + bc.REG_WEIGHT * reg
    gc, gp = torch.autograd.grad(loss, (c, p), retain_graph=True)
    if c.shape[1]:
        (gc_data,) = torch.autograd.grad(data, c, retain_graph=True)
        (gc_prior,) = torch.autograd.grad(reg, c)
    else:
        gc_data = gc_prior = torch.zeros_like(c)
    out = {"v": v[:, idx], "n": n[:, idx], "gcoeff": gc, "gpose": gp, "reg": reg, "gcoeff_data": gc_data,
           "gcoeff_prior": gc_prior}
    return {k: t.detach().double().numpy() for k, t in out.items()}


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def main():
    fm, u3d = reference_modules()
    arrays = {}
    for name in bc.CASES:
        torch.set_default_dtype(torch.float64)      # mesh_point_normal's torch.ones follows it
        try:
            r64 = run_reference(fm, u3d, name, torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
        r32 = run_reference(fm, u3d, name, torch.float32)
        for k in r64:
            assert np.isfinite(r64[k]).all() and np.isfinite(r32[k]).all(), (name, k)
            arrays["%s_%s" % (name, k)] = r64[k]
            arrays["%s_%s_err32" % (name, k)] = np.float64(rel(r32[k], r64[k]))
            print("%-6s %-12s shape %-14s ref fp32 vs fp64 rel err %.3e" % (name, k, r64[k].shape, rel(r32[k], r64[k])))
        e = bc.elementwise_error(r32["gcoeff_prior"], r64["gcoeff_prior"])
        arrays["%s_gcoeff_prior_elem_err32" % name] = np.float64(e)
        print("%-6s gcoeff_prior elementwise ref fp32 vs fp64 rel err %.3e" % (name, e))
    ds, de = bc.BETA_DIMS
    for form, (bsh, bex) in bc.BETA_FORMS.items():
        m = fm.BlendShapeModel(4, ds, de, None, bsh, bex)
        arrays["beta_" + form] = m.beta.detach().double().numpy()
    sd = reference_model(fm, "small").state_dict()
    arrays["state_dict_keys"] = np.array(list(sd.keys()))
    for k, t in sd.items():
        arrays["state_dict_shape_" + k] = np.array(t.shape, np.int64)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "blendshape.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
