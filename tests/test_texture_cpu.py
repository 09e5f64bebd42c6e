"""CPU: texture baking — the host definitions of op.texture (texel map, bake, padding, fill) on scenes whose answer is
known in closed form, the layouts of face_model (uv_layout, load_uv), utils_3d.save_textured_obj, the argument checks of
the C ABI, and `reconstruct --texture` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, synth, utils_3d
from stylerenderer_amd.op import texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD_UV = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
QUAD_TRI = torch.tensor([[0, 1, 2], [0, 2, 3]])


# ---- texel_map -------------------------------------------------------------------------------------------------------
def reproduced(face, coeff, uv, tri_uv):
    """sum_k coeff_k uv[tri_uv[f, k]] per texel, float64 (garbage where face < 0)."""
    corners = uv.double()[tri_uv[face.long().clamp_min(0)]]                 # [Th, Tw, 3, 2]
    return (coeff.double().unsqueeze(-1) * corners).sum(-2)


@pytest.mark.parametrize("size", [8, (5, 7)])
def test_texel_map_on_a_quad(size):
    face, coeff = texture.texel_map(QUAD_UV, QUAD_TRI, size)
    th, tw = (size, size) if isinstance(size, int) else size
    assert face.dtype == torch.int32 and tuple(face.shape) == (th, tw) and tuple(coeff.shape) == (th, tw, 3)
    assert coeff.dtype == torch.float32
    assert int(face.min()) >= 0 and sorted(face.unique().tolist()) == [0, 1]          # all covered, both faces appear
    centres = texture.texel_centres(size)
    assert float((reproduced(face, coeff, QUAD_UV, QUAD_TRI) - centres).abs().max()) <= 1e-6
    assert float(centres[0, 0, 1]) > float(centres[-1, 0, 1])                         # row 0 is the top: v points up
    assert texture.texel_map(QUAD_UV, QUAD_TRI, size)[0] is face                      # cached per layout and size
    # every face's winding reversed: the same map up to the face split along the diagonal
    rev = QUAD_TRI[:, [0, 2, 1]].contiguous()
    face_r, coeff_r = texture.texel_map(QUAD_UV, rev, size)
    assert int(face_r.min()) >= 0 and sorted(face_r.unique().tolist()) == [0, 1]
    assert float((reproduced(face_r, coeff_r, QUAD_UV, rev) - centres).abs().max()) <= 1e-6
    diag = (centres[..., 0] - centres[..., 1]).abs() < 1e-9
    assert torch.equal(face_r[~diag], face[~diag])
    # keep drops face 1 and nothing else
    keep = torch.tensor([True, False])
    face_k, coeff_k = texture.texel_map(QUAD_UV, QUAD_TRI, size, keep)
    was1 = face == 1
    assert bool(was1.any()) and bool((face_k[was1] == -1).all()) and bool((coeff_k[was1] == 0).all())
    assert torch.equal(face_k[~was1], face[~was1]) and torch.equal(coeff_k[~was1], coeff[~was1])
    # a zero-area face is never drawn, wherever it stands in the list
    uv5 = torch.cat((QUAD_UV, torch.tensor([[0.5, 0.5]])))
    tri5 = torch.tensor([[0, 2, 4], [0, 1, 2], [0, 2, 3]])                            # face 0: three points of the diagonal
    face_z, coeff_z = texture.texel_map(uv5, tri5, size)
    assert sorted(face_z.unique().tolist()) == [1, 2]
    assert torch.equal(face_z - 1, face) and torch.equal(coeff_z, coeff)


def test_texel_map_refuses_bad_layouts():
    with pytest.raises(ValueError):
        texture.texel_map(QUAD_UV * 2, QUAD_TRI, 8)                                  # outside [0, 1]
    with pytest.raises(ValueError):
        texture.texel_map(QUAD_UV, QUAD_TRI + 2, 8)                                  # index past the coordinates
    with pytest.raises(ValueError):
        texture.texel_map(QUAD_UV, QUAD_TRI, 8, torch.tensor([True]))                # keep of another length


# ---- the exact scene -------------------------------------------------------------------------------------------------
# Two quads facing +z: the back one spans [-3/4, 3/4]^2 at z = 0, the front one [-1/4, 1/4]^2 at z = 1/2.  The layout
# puts them side by side: the back quad on u in [0, 1/2], the front quad on u in [1/2, 1].
BACK, FRONT = 0.75, 0.25
AFFINE = np.array([[0.010, -0.020, 0.30], [-0.015, 0.005, 0.10], [0.020, 0.010, -0.70]])      # per channel: a x + b y + d


def scene(shift=(0.0, 0.0), dtype=torch.float32):
    """(v [1, 8, 3], n, tri [4, 3], uv [8, 2], tri_uv) of the two quads, moved by `shift` in x and y."""
    def quad(r, z):
        return [[-r, -r, z], [r, -r, z], [r, r, z], [-r, r, z]]

    v = torch.tensor(quad(BACK, 0.0) + quad(FRONT, 0.5), dtype=torch.float64)
    v[:, 0] += shift[0]
    v[:, 1] += shift[1]
    n = torch.tensor([[0.0, 0.0, 1.0]] * 8, dtype=torch.float64)
    tri = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]])
    uv = torch.tensor([[0.0, 0.0], [0.5, 0.0], [0.5, 1.0], [0.0, 1.0], [0.5, 0.0], [1.0, 0.0], [1.0, 1.0], [0.5, 1.0]])
    return v.to(dtype)[None], n.to(dtype)[None], tri, uv, tri.clone()


def scene_batch(shifts, dtype=torch.float32):
    parts = [scene(s, dtype) for s in shifts]
    return (torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])) + parts[0][2:]


def affine_picture(c_n, hs, ws, batch=1, dtype=torch.float32):
    y, x = torch.meshgrid(torch.arange(hs, dtype=torch.float64), torch.arange(ws, dtype=torch.float64), indexing="ij")
    planes = [AFFINE[c, 0] * x + AFFINE[c, 1] * y + AFFINE[c, 2] for c in range(c_n)]
    return torch.stack(planes)[None].expand(batch, -1, -1, -1).to(dtype).contiguous()


def texel_points(face, size, shift):
    """P [Th, Tw, 3] float64 of every texel's surface point, in closed form from the layout (NaN on empty texels)."""
    c = texture.texel_centres(size)
    u, w = c[..., 0], c[..., 1]
    back = face < 2
    x = torch.where(back, (u / 0.5) * 2 * BACK - BACK, ((u - 0.5) / 0.5) * 2 * FRONT - FRONT) + shift[0]
    y = torch.where(back, w * 2 * BACK - BACK, w * 2 * FRONT - FRONT) + shift[1]
    z = torch.where(back, torch.zeros_like(u), torch.full_like(u, 0.5))
    p = torch.stack((x, y, z), -1)
    return torch.where((face >= 0).unsqueeze(-1), p, torch.full_like(p, float("nan")))


def expected_weight(face, size, shift, zsize, psize):
    """(want [Th, Tw] in {0, 1}, sure bool [Th, Tw]) in closed form: a front-quad texel is seen; a back-quad texel is
    hidden where the front quad covers its z-buffer pixel; both only inside the picture.  `sure` leaves out the texels
    whose 3 x 3 block of z-buffer pixels touches the front quad's outline, and those within 1e-3 pixels of the picture's
    border."""
    hz, wz = zsize
    hs, ws = psize
    p = texel_points(face, size, shift)
    qx, qy = (1 + p[..., 0]) * wz / 2 - 0.5, (1 - p[..., 1]) * hz / 2 - 0.5
    ix, iy = torch.floor(qx + 0.5), torch.floor(qy + 0.5)
    all_in = torch.ones_like(face, dtype=torch.bool)
    none_in = torch.ones_like(face, dtype=torch.bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            cx = (ix + dx + 0.5) * 2 / wz - 1 - shift[0]                     # the pixel's centre in the front quad's frame
            cy = 1 - (iy + dy + 0.5) * 2 / hz - shift[1]
            covered = (cx.abs() < FRONT) & (cy.abs() < FRONT)
            all_in &= covered
            none_in &= ~covered
    sx, sy = (1 + p[..., 0]) * ws / 2 - 0.5, (1 - p[..., 1]) * hs / 2 - 0.5
    inside = (sx >= -0.5) & (sx <= ws - 0.5) & (sy >= -0.5) & (sy <= hs - 0.5)
    edge = torch.stack((sx + 0.5, sx - (ws - 0.5), sy + 0.5, sy - (hs - 0.5))).abs().min(0).values
    # (inside the picture implies inside the z-buffer: both cover the same model square)
    front = face >= 2
    live = face >= 0
    want = torch.where(front | none_in, torch.ones_like(qx), torch.zeros_like(qx)) * inside.double() * live.double()
    sure = live & (edge > 1e-3) & (front | none_in | all_in | ~inside)
    return want, sure


def bake_scene(size, shift, psize=(48, 64), zsize=(48, 64), c_n=3, flip_normals=False, dtype=torch.float32):
    v, n, tri, uv, tri_uv = scene(shift, dtype)
    if flip_normals:
        n = -n
    face, coeff = texture.texel_map(uv, tri_uv, size)
    zbuf = texture.depth_buffer(v, tri, zsize)
    assert tuple(zbuf.shape) == (1,) + tuple(zsize)
    tex, weight = texture.bake(v, n, tri, face, coeff, affine_picture(c_n, *psize, dtype=dtype), zbuf, facing=(0.0, 0.5),
                               z_bias=1.0 / 64)
    return face, tex, weight


@pytest.mark.parametrize("size", [(8, 8), (33, 65)])
def test_bake_on_the_exact_scene(size):
    face, tex, weight = bake_scene(size, (0.0, 0.0))
    assert tuple(tex.shape) == (1, 3) + size and tuple(weight.shape) == (1, 1) + size and tex.dtype == torch.float32
    w = weight[0, 0]
    assert bool((face >= 0).all())
    assert bool((w[face >= 2] == 1).all())                                  # the front quad: exactly 1
    want, sure = expected_weight(face, size, (0.0, 0.0), (48, 64), (48, 64))
    back = sure & (face < 2)
    assert int((want[back] == 0).sum()) >= 4 and int((want[back] == 1).sum()) >= 8
    assert torch.equal(w[sure].double(), want[sure])                       # the back quad: exactly 0 behind the front quad
    # the colour: the affine picture at the texel's projected point
    p = texel_points(face, size, (0.0, 0.0))
    sx, sy = (1 + p[..., 0]) * 64 / 2 - 0.5, (1 - p[..., 1]) * 48 / 2 - 0.5
    seen = w > 0
    for c in range(3):
        colour = AFFINE[c, 0] * sx + AFFINE[c, 1] * sy + AFFINE[c, 2]
        assert float((tex[0, c].double() - colour)[seen].abs().max()) <= 1e-5
        assert bool((tex[0, c][~seen] == 0).all())
    # the float64 definition agrees
    face64, tex64, weight64 = bake_scene(size, (0.0, 0.0), dtype=torch.float64)
    assert tex64.dtype == torch.float64 and torch.equal(weight64[0, 0][sure], want[sure])
    # normals turned away: nothing is seen
    _, tex_f, weight_f = bake_scene(size, (0.0, 0.0), flip_normals=True)
    assert bool((weight_f == 0).all()) and bool((tex_f == 0).all())


@pytest.mark.parametrize("size", [(8, 8), (33, 65)])
@pytest.mark.parametrize("shift", [(0.5, 0.125), (-0.3, -0.6)])
def test_bake_gives_no_weight_outside_the_picture(size, shift):
    face, tex, weight = bake_scene(size, shift)
    want, sure = expected_weight(face, size, shift, (48, 64), (48, 64))
    p = texel_points(face, size, shift)
    outside = sure & ((p[..., 0].abs() > 1) | (p[..., 1].abs() > 1))
    assert int(outside.sum()) >= 4 and bool((want[outside] == 0).all())
    assert torch.equal(weight[0, 0][sure].double(), want[sure])
    assert bool((tex[0][:, weight[0, 0] == 0] == 0).all())


def test_bake_at_another_picture_size_and_channel_count():
    """The picture's resolution is its own: (5, 7) with one channel against the (48, 64) z-buffer."""
    face, tex, weight = bake_scene((8, 8), (0.0, 0.0), psize=(5, 7), c_n=1)
    want, sure = expected_weight(face, (8, 8), (0.0, 0.0), (48, 64), (5, 7))
    assert torch.equal(weight[0, 0][sure].double(), want[sure])
    p = texel_points(face, (8, 8), (0.0, 0.0))
    sx, sy = (1 + p[..., 0]) * 7 / 2 - 0.5, (1 - p[..., 1]) * 5 / 2 - 0.5
    # replicate at the border: the affine function of the clamped position between the outermost pixel centres
    colour = AFFINE[0, 0] * sx.clamp(0, 6) + AFFINE[0, 1] * sy.clamp(0, 4) + AFFINE[0, 2]
    seen = weight[0, 0] > 0
    assert float((tex[0, 0].double() - colour)[seen].abs().max()) <= 1e-5


def test_bake_refuses_bad_arguments():
    v, n, tri, uv, tri_uv = scene()
    face, coeff = texture.texel_map(uv, tri_uv, 8)
    img, zbuf = affine_picture(3, 5, 7), texture.depth_buffer(v, tri, 16)
    with pytest.raises(ValueError):
        texture.bake(v, n[:, :4], tri, face, coeff, img, zbuf)
    with pytest.raises(ValueError):
        texture.bake(v, n, tri, face, coeff, img, zbuf, facing=(0.5, 0.1))
    with pytest.raises(ValueError):
        texture.bake(v, n, tri, face, coeff, img.expand(2, -1, -1, -1), zbuf)
    with pytest.raises(ValueError):
        texture.bake(v, n, tri, face.long(), coeff, img, zbuf)
    tex, weight = texture.bake(v, n, tri, face, coeff, img, zbuf, facing=(0.3, 0.3))          # hi == lo: a step
    assert sorted(weight.unique().tolist()) == [0.0, 1.0]


# ---- padding ---------------------------------------------------------------------------------------------------------
def pad_loops(tex, filled):
    """One pass, as a literal double loop (numpy float32)."""
    b, c_n, th, tw = tex.shape
    out, fo = tex.copy(), filled.copy()
    for s in range(b):
        for y in range(th):
            for x in range(tw):
                if filled[s, 0, y, x]:
                    continue
                near = [(y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                        if (dy or dx) and 0 <= y + dy < th and 0 <= x + dx < tw and filled[s, 0, y + dy, x + dx]]
                if not near:
                    continue
                for c in range(c_n):
                    acc = np.float32(0)
                    for yy, xx in near:
                        acc = np.float32(acc + tex[s, c, yy, xx])
                    out[s, c, y, x] = np.float32(acc / np.float32(len(near)))
                fo[s, 0, y, x] = 1
    return out, fo


def pad_case(kind, shape=(2, 3, 9, 11), seed=3):
    b, c_n, th, tw = shape
    tex = torch.from_numpy(synth.det_uniform(shape, seed).astype(np.float32))
    weight = torch.zeros(b, 1, th, tw)
    if kind == "one":
        weight[0, 0, 4, 6] = 0.25
        weight[1, 0, 0, 10] = 1.0                                            # a corner texel
    elif kind == "all":
        weight[:] = 0.5
    elif kind == "sparse":
        weight = (torch.from_numpy(synth.det_uniform((b, 1, th, tw), seed + 1)) > 0.8).float() * 0.75
    tex = tex * (weight > 0)
    return tex, weight


@pytest.mark.parametrize("kind", ["one", "none", "all", "sparse"])
@pytest.mark.parametrize("passes", [0, 1, 2])
def test_pad_equals_the_literal_loops(kind, passes):
    tex, weight = pad_case(kind)
    keep_w = weight.clone()
    got, filled = texture.pad(tex, weight, passes)
    want, wf = tex.numpy().copy(), (weight > 0).numpy().astype(np.uint8)
    for _ in range(passes):
        want, wf = pad_loops(want, wf)
    assert filled.dtype == torch.uint8 and tuple(filled.shape) == tuple(weight.shape)
    assert np.array_equal(got.numpy(), want) and np.array_equal(filled.numpy(), wf)
    assert torch.equal(weight, keep_w) and got.data_ptr() != tex.data_ptr()
    if kind in ("none", "all"):
        assert torch.equal(got, tex) and torch.equal(filled, (weight > 0).to(torch.uint8))     # nothing changes
    if kind == "one" and passes:
        assert int(filled[0].sum()) == (2 * passes + 1) ** 2 and int(filled[1].sum()) == (passes + 1) ** 2
        block = got[0, :, 4 - passes:5 + passes, 6 - passes:7 + passes]         # means of copies of the one colour
        assert float((block - tex[0, :, 4, 6].view(3, 1, 1)).abs().max()) <= 1e-6


def test_pad_refuses_bad_arguments():
    tex, weight = pad_case("one")
    for passes in (-1, 65):
        with pytest.raises(ValueError):
            texture.pad(tex, weight, passes)
    with pytest.raises(ValueError):
        texture.pad(tex, weight[:, :, :5], 1)


def test_fill_mean():
    tex, weight = pad_case("one")
    out, filled = texture.pad(tex, weight, 1)
    full = texture.fill_mean(out, weight, filled)
    on = filled.bool().expand_as(out)
    assert torch.equal(full[on], out[on])
    for s, (y, x) in enumerate(((4, 6), (0, 10))):                         # one weighted texel: its colour is the mean
        assert torch.allclose(full[s, :, 8, 0], tex[s, :, y, x], atol=1e-6)
    tex0, weight0 = pad_case("none")
    out0, filled0 = texture.pad(tex0, weight0, 2)
    full0 = texture.fill_mean(out0, weight0, filled0)
    assert bool((full0 == 0).all())                                        # total weight 0: stays 0


# ---- layouts ---------------------------------------------------------------------------------------------------------
def uv_areas(uv, tri_uv):
    p = uv.double()[tri_uv]
    return ((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 2, 0] - p[:, 0, 0]) * (p[:, 1, 1] - p[:, 0, 1]))


def test_uv_layout_of_the_synthetic_mean():
    v, tri = synth.face_sized_mesh()
    uv, tri_uv, keep = face_model.uv_layout(v, tri)
    assert uv.dtype == torch.float32 and tuple(uv.shape) == (v.shape[0], 2) and keep.dtype == torch.bool
    assert np.array_equal(tri_uv.numpy(), tri) and tri.shape[0] == 49536
    assert float(uv.min()) >= 1 / 64 - 1e-7 and float(uv.max()) <= 1 - 1 / 64 + 1e-7
    assert int((~keep).sum()) == 432 and int(keep.sum()) == 49104          # the faces across the seam at the back
    assert int((uv_areas(uv, tri_uv)[keep] > 0).sum()) == 49104
    uv0 = face_model.uv_layout(torch.from_numpy(v), torch.from_numpy(tri), margin=0)[0]
    assert float(uv0.min()) == 0 and float(uv0.max()) == 1
    with pytest.raises(ValueError):
        face_model.uv_layout(v, tri, margin=0.5)


def small_layout():
    v, tri = synth.uv_ellipsoid(6, 5)
    uv, tri_uv, _ = face_model.uv_layout(v, tri)
    # a layout with its own coordinate list: every face gets three coordinates of its own
    vt = uv[tri_uv.reshape(-1)].contiguous()
    ft = torch.arange(vt.shape[0]).view(-1, 3)
    return v, tri, vt, ft


def test_load_uv_round_trips_obj_and_npz(tmp_path):
    v, tri, vt, ft = small_layout()
    obj = str(tmp_path / "layout.obj")
    utils_3d.save_obj(obj, v, tri, vt=vt, trit=ft)
    got_vt, got_ft = face_model.load_uv(obj, torch.from_numpy(tri))
    assert got_vt.dtype == torch.float32 and got_ft.dtype == torch.int64
    assert torch.equal(got_ft, ft) and float((got_vt - vt).abs().max()) <= 1e-6          # (%f keeps six decimals)
    with_n = str(tmp_path / "layout_n.obj")
    utils_3d.save_obj(with_n, v, tri, vt=vt, trit=ft, vn=synth.vertex_normals(v, tri))      # a/t/n records
    assert torch.equal(face_model.load_uv(with_n, tri)[1], ft)
    npz = str(tmp_path / "layout.npz")
    np.savez(npz, vt=vt.numpy(), ft=ft.numpy())
    got_vt, got_ft = face_model.load_uv(npz, tri)
    assert torch.equal(got_vt, vt) and torch.equal(got_ft, ft)


def test_load_uv_rejects_other_faces(tmp_path):
    v, tri, vt, ft = small_layout()
    obj = str(tmp_path / "layout.obj")
    other = tri.copy()
    other[3] = other[3][[1, 2, 0]]
    utils_3d.save_obj(obj, v, other, vt=vt, trit=ft)
    with pytest.raises(ValueError, match="differ from the mesh's tri"):
        face_model.load_uv(obj, tri)
    plain = str(tmp_path / "plain.obj")
    utils_3d.save_obj(plain, v, tri)                                                       # no texture records at all
    with pytest.raises(ValueError):
        face_model.load_uv(plain, tri)
    npz = str(tmp_path / "short.npz")
    np.savez(npz, vt=vt.numpy(), ft=ft.numpy()[:-1])
    with pytest.raises(ValueError):
        face_model.load_uv(npz, tri)


# ---- the file writer -------------------------------------------------------------------------------------------------
def _kinds(path):
    kinds = {}
    for line in open(path):
        k = line.split(" ", 1)[0]
        kinds[k] = kinds.get(k, 0) + 1
    return kinds


def test_save_textured_obj(tmp_path):
    v, tri, vt, ft = small_layout()
    vn = synth.vertex_normals(v, tri)
    path = str(tmp_path / "head_textured.obj")
    assert utils_3d.save_textured_obj(path, v, tri, vt, ft, vn, "head_texture.png")
    lines = open(path).read().split("\n")
    assert lines[:2] == ["mtllib head_textured.mtl", "usemtl face"]
    assert _kinds(path) == {"mtllib": 1, "usemtl": 1, "v": v.shape[0], "vt": vt.shape[0], "vn": v.shape[0],
                            "f": tri.shape[0]}
    first_f = next(line for line in lines if line.startswith("f "))
    assert first_f == "f " + " ".join("%d/%d/%d" % (tri[0, k] + 1, ft[0, k] + 1, tri[0, k] + 1) for k in range(3))
    assert open(str(tmp_path / "head_textured.mtl")).read() == "newmtl face\nKd 1 1 1\nmap_Kd head_texture.png\n"
    # save_obj's own output: the same records without the two lines, and the text the reference's contract pins
    plain = str(tmp_path / "plain.obj")
    utils_3d.save_obj(plain, v, tri, vt=vt, trit=ft, vn=vn)
    assert open(plain).read() == "\n".join(lines[2:])
    tiny = str(tmp_path / "tiny.obj")
    utils_3d.save_obj(tiny, [[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], [[0, 1, 2]], vn=[[0, 0, 1]] * 3)
    assert open(tiny).read() == ("v 0.000000 0.000000 0.000000\nv 1.000000 0.000000 0.000000\nv 0.000000 1.000000 0.500000\n"
                                 "vn 0.000000 0.000000 1.000000\nvn 0.000000 0.000000 1.000000\n"
                                 "vn 0.000000 0.000000 1.000000\nf 1//1 2//2 3//3\n")


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu():
    """NULL pointers and non-positive sizes are refused before any launch; zero texels is a no-op."""
    from stylerenderer_amd import _lib

    L = _lib.lib()
    nine = [None] * 9
    sizes = dict(B=1, C=3, nv=8, nf=4, Th=8, Tw=8, Hs=5, Ws=7, Hz=16, Wz=16)

    def bake(**over):
        s = dict(sizes, **over)
        return L.sr_texture_bake(*nine, *[s[k] for k in ("B", "C", "nv", "nf", "Th", "Tw", "Hs", "Ws", "Hz", "Wz")],
                                 0.1, 0.4, 0.25, None)

    assert bake() == -1                                                    # NULL pointers
    for name in ("C", "nv", "nf", "Hs", "Ws", "Hz", "Wz"):
        assert bake(**{name: 0}) == -1, name
    assert bake(B=-1) == -1 and bake(Th=-1) == -1
    assert bake(Th=0) == 0 and bake(Tw=0) == 0 and bake(B=0) == 0          # zero texels
    assert L.sr_texture_bake(*nine, 1, 3, 8, 4, 8, 8, 5, 7, 16, 16, 0.4, 0.1, 0.25, None) == -1      # lo > hi
    assert L.sr_texture_pad(None, None, None, None, 1, 3, 8, 8, None) == -1
    assert L.sr_texture_pad(None, None, None, None, 1, 0, 8, 8, None) == -1
    assert L.sr_texture_pad(None, None, None, None, 1, 3, -1, 8, None) == -1
    assert L.sr_texture_pad(None, None, None, None, 1, 3, 0, 8, None) == 0
    assert L.sr_texture_pad(None, None, None, None, 0, 3, 8, 8, None) == 0


# ---- float32 against float64: the guard of the GPU test's ordinary case ------------------------------------------------
def ordinary_case(dtype=torch.float32, device="cpu", size=(33, 65), batch=3):
    """The posed ellipsoid, its layout and texel map, a smooth non-affine picture and the z-buffer, in `dtype` on
    `device` (the map is float32 by definition).  Returns a dict of bake's arguments and the picture's largest
    neighbouring-pixel difference D."""
    v0, tri = synth.uv_ellipsoid(16, 14)
    vp = synth.random_poses(v0, batch)
    n = synth.vertex_normals(vp, tri)
    uv, tri_uv, keep = face_model.uv_layout(v0, tri)
    uv = uv.to(device)
    face, coeff = texture.texel_map(uv, tri_uv, size, keep)
    y, x = torch.meshgrid(torch.arange(48, dtype=torch.float64), torch.arange(64, dtype=torch.float64), indexing="ij")
    img = torch.stack([torch.stack([torch.sin(0.11 * (c + 1) * x + 0.07 * y + 0.5 * c + s)
                                    * torch.cos(0.05 * x - 0.09 * (c + 1) * y) for c in range(3)]) for s in range(batch)])
    d = max(float((img[..., 1:] - img[..., :-1]).abs().max()), float((img[..., 1:, :] - img[..., :-1, :]).abs().max()))
    v = torch.from_numpy(vp).to(device=device, dtype=dtype)
    tri_t = torch.from_numpy(tri).to(device)
    args = dict(v=v, n=torch.from_numpy(n).to(device=device, dtype=dtype), tri=tri_t, face=face, coeff=coeff,
                image=img.to(device=device, dtype=dtype), zbuf=texture.depth_buffer(v, tri_t, (48, 64)))
    return args, d, (uv, tri_uv, keep)


def decisions_differ(args32, args64):
    """(differ bool [B, Th, Tw], live bool [Th, Tw]): where float32's vis / inside decision is not float64's."""
    z32 = 4.0 / 64
    p32 = texture.bake_composite(*[args32[k].cpu() for k in ("v", "n", "tri", "face", "coeff", "image", "zbuf")],
                                 (0.1, 0.4), z32, parts=True)
    p64 = texture.bake_composite(*[args64[k].cpu() for k in ("v", "n", "tri", "face", "coeff", "image", "zbuf")],
                                 (0.1, 0.4), z32, parts=True)
    return (p32[2] != p64[2]) | (p32[3] != p64[3]), args32["face"].cpu() >= 0, p64


def test_float32_against_float64_on_the_ordinary_case():
    args32, d, _ = ordinary_case(torch.float32)
    args64, _, _ = ordinary_case(torch.float64)
    assert args64["zbuf"].dtype == torch.float64 and args32["coeff"].dtype == torch.float32
    differ, live, p64 = decisions_differ(args32, args64)
    n_live = int(live.sum()) * differ.shape[0]
    assert int(live.sum()) > 0.5 * live.numel()
    assert int(differ.sum()) <= 0.005 * n_live, (int(differ.sum()), n_live)
    tex32, w32 = texture.bake(**args32)
    tex64, w64 = p64[0], p64[1]
    bound = d * (48 + 64) * 2.0 ** -22 + 2.0 ** -22
    same = ~differ
    assert float((w32.double() - w64)[:, 0][same].abs().max()) <= bound
    assert float((tex32.double() - tex64).permute(1, 0, 2, 3)[:, same].abs().max()) <= bound
    seen = w64[:, 0] > 0
    assert 0.1 < float(seen.sum()) / n_live < 0.9                           # the front is seen, the back is not


# ---- command line ----------------------------------------------------------------------------------------------------
def _env():
    return dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


def test_reconstruct_cli_with_texture(tmp_path):
    from stylerenderer_amd import model

    g = model.GeneratorWithMap(16, 512, 8)
    synth.fill_state_dict(g.state_dict(), salt=5)
    ckpt = str(tmp_path / "g.pt")
    torch.save({"g_ema": g.state_dict()}, ckpt)
    img = str(tmp_path / "face_a.npy")
    np.save(img, synth.det_uniform((3, 24, 24), 9))                      # CHW, resized to 16 on the host
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "stylerenderer_amd.reconstruct", "--size", "16", "--steps", "4", "--n_mean_latent",
           "64", "--texture", "32", "--out", out, ckpt, img]
    res = subprocess.run(cmd, env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    assert sorted(os.listdir(out)) == sorted(
        ["face_a.obj", "face_a_canonical.obj", "face_a_render.png", "face_a_normal.png", "face_a.npz",
         "face_a_texture.png", "face_a_texture_weight.png", "face_a_textured.obj", "face_a_textured.mtl"])
    from PIL import Image

    tex = Image.open(os.path.join(out, "face_a_texture.png"))
    assert tex.size == (32, 32) and tex.mode == "RGB"
    wpic = Image.open(os.path.join(out, "face_a_texture_weight.png"))
    assert wpic.size == (32, 32) and wpic.mode == "L" and np.asarray(wpic).max() > 0
    r = np.load(os.path.join(out, "face_a.npz"))
    assert 0 < float(r["texture_coverage"]) < 1
    v0, tri = synth.face_sized_mesh()
    nv, nf = v0.shape[0], tri.shape[0]
    path = os.path.join(out, "face_a_textured.obj")
    assert _kinds(path) == {"mtllib": 1, "usemtl": 1, "v": nv, "vt": nv, "vn": nv, "f": nf}
    first_f = next(line for line in open(path) if line.startswith("f "))
    assert first_f.split() == ["f"] + ["%d/%d/%d" % (i + 1, i + 1, i + 1) for i in tri[0]]
    assert open(os.path.join(out, "face_a_textured.mtl")).read().endswith("map_Kd face_a_texture.png\n")
    # the posed vertices are those of <stem>.obj
    plain = [line for line in open(os.path.join(out, "face_a.obj")) if line.startswith("v ")]
    assert plain == [line for line in open(path) if line.startswith("v ")]
    # the other texture options need --texture
    bad = subprocess.run([sys.executable, "-m", "stylerenderer_amd.reconstruct", "--uv", "layout.obj", ckpt, img],
                         env=_env(), cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert bad.returncode == 2 and "need --texture" in bad.stderr
