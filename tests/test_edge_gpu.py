"""op.edge on the device: sr_edge_aa_fwd / sr_edge_aa_bwd_image / sr_edge_aa_bwd_corner against the host float32 composite,
bit for bit (the vertex gradient by the first rule of DESIGN 7p: the host definition sums in the kernel's order)."""
import functools

import pytest
import torch

import edge_cases as ec
from stylerenderer_amd import _lib, graphs
from stylerenderer_amd.op import edge
from stylerenderer_amd.op._dispatch import native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _hand(name):
    return {"edge25": lambda: ec.vertical_edge(0.25), "edge50": lambda: ec.vertical_edge(0.5),
            "edge75": lambda: ec.vertical_edge(0.75), "quad": ec.quad, "overlap": ec.overlap,
            "fold": lambda: ec.fold(True), "unfold": lambda: ec.fold(False), "centre": ec.through_centre,
            "tie": ec.z_tie}[name]()


HAND = ("edge25", "edge50", "edge75", "quad", "overlap", "fold", "unfold", "centre", "tie")
# (name, size, B, C): the CPU suite's shapes, then 33 x 33 and 64 x 64 (more than one workgroup, rows no multiple of a wave)
MESHES = (("ellipsoid", (16, 16), 1, 3), ("coarse", (5, 7), 3, 1), ("coarse", (16, 12), 3, 4),
          ("ellipsoid", (33, 33), 1, 4), ("ellipsoid", (64, 64), 3, 3), ("disc", (33, 33), 1, 1),
          ("disc", (64, 64), 1, 3), ("coarse", (33, 33), 1, 1), ("coarse", (64, 64), 3, 3), ("nan", (16, 16), 3, 3),
          ("far", (16, 16), 3, 3))


@functools.lru_cache(maxsize=None)
def host_case(name, size=(8, 8), b=1, c=1):
    """Everything of one case on the host, computed once: inputs, face map and the float32 composite's results."""
    if name in HAND:
        sc = _hand(name)
        v, tri, size = sc.v, sc.tri, sc.size
    elif name == "disc":
        v, tri = ec.facing_disc(size, shift=(0.3, 0.2))
    else:
        v, tri = ec.ellipsoid(4, 6, b=b) if name == "coarse" else ec.ellipsoid(b=b)
        if name == "nan":
            v[1, 5, 0] = float("nan")
        if name == "far":
            v[1, 7] = torch.tensor([1e6, -1e6, 0.0])
            v[2, 9] = torch.tensor([-1e6, 3.0, 0.0])
    v = v.expand(b, -1, -1).contiguous() if v.shape[0] != b else v
    gen = torch.Generator().manual_seed(5)
    image = torch.rand((b, c) + tuple(size), generator=gen)
    g = torch.randn((b, c) + tuple(size), generator=gen)
    face, zbuf = edge.face_map(v, tri, size)
    opp = edge.adjacency(tri, int(v.shape[1]))
    im, vv = image.clone().requires_grad_(True), v.clone().requires_grad_(True)
    out = edge.antialias_composite(im, vv, tri, face, zbuf, opp)
    gi, gv = torch.autograd.grad(out, (im, vv), grad_outputs=g)
    return dict(v=v, tri=tri, size=size, image=image, g=g, face=face, zbuf=zbuf, opp=opp, out=out.detach(), gi=gi, gv=gv)


def device_case(ref):
    d = {k: ref[k].to(DEV) for k in ("v", "tri", "image", "g")}
    face, zbuf = edge.face_map(d["v"], d["tri"], ref["size"])
    assert torch.equal(face.cpu(), ref["face"]) and torch.equal(zbuf.cpu(), ref["zbuf"])       # the rasterizer's parity
    d.update(face=face, zbuf=zbuf, opp=edge.adjacency(d["tri"], int(d["v"].shape[1])))
    assert torch.equal(d["opp"].cpu(), ref["opp"])
    return d


def run_device(d):
    im, vv = d["image"].clone().requires_grad_(True), d["v"].clone().requires_grad_(True)
    out = edge.antialias(im, vv, d["tri"], d["face"], d["zbuf"], d["opp"])
    gi, gv = torch.autograd.grad(out, (im, vv), grad_outputs=d["g"])
    return out.detach(), gi, gv


def bits(a, b):
    a, b = a.cpu(), b.cpu()
    return torch.equal(a, b) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def check(ref):
    out, gi, gv = run_device(device_case(ref))
    hits = int((ref["out"] != ref["image"]).any(1).sum())
    print("pixels changed: %d; |gv| max %.3g" % (hits, float(ref["gv"].abs().max())))
    assert bits(out, ref["out"])
    assert bits(gi, ref["gi"])
    assert bits(gv, ref["gv"])
    assert float(gv[..., 2].abs().max()) == 0.0
    return hits


@pytest.mark.parametrize("name", HAND)
def test_hand_scenes_equal_the_host_composite(name):
    hits = check(host_case(name))
    assert (hits > 0) == (name not in ("edge50", "unfold"))


@pytest.mark.parametrize("name,size,b,c", MESHES)
def test_meshes_equal_the_host_composite(name, size, b, c):
    hits = check(host_case(name, size, b, c))
    assert hits >= 2


def test_nothing_and_everything_covered_return_the_image():
    ref = host_case("edge25")
    image = ref["image"].to(DEV)
    off = ref["v"] + torch.tensor([0.0, 5.0, 0.0])                               # 20 pixels up: out of the picture
    out = edge.antialias(image, off.to(DEV), ref["tri"].to(DEV))
    assert torch.equal(out, image)
    sc = ec._soup([((-40.0, -20.0, -0.5), (40.0, -20.0, -0.5), (4.0, 60.0, -0.5))])
    face, _ = edge.face_map(sc.v.to(DEV), sc.tri.to(DEV), sc.size)
    assert int(face.min()) == 0
    assert torch.equal(edge.antialias(image, sc.v.to(DEV), sc.tri.to(DEV)), image)


def test_corner_kernel_on_both_sides_of_its_threshold():
    """The cases above hold faces whose box is scanned by one lane and faces left to their wave; here the split is
    asserted, and one picture holds both kinds in the same wave of faces."""
    assert _lib.lib().sr_edge_big_pixels() == edge.BIG
    small = host_case("ellipsoid", (64, 64), 3, 3)
    assert int(edge.box_pixels(small["v"], small["tri"], small["size"]).max()) <= edge.BIG
    for name, size, b, c in (("coarse", (64, 64), 3, 3),):                      # one of MESHES: compared above
        assert (name, size, b, c) in MESHES
        ref = host_case(name, size, b, c)
        n = edge.box_pixels(ref["v"], ref["tri"], ref["size"])
        print("%s %s: boxes %d..%d pixels, %d above %d" % (name, size, int(n.min()), int(n.max()), int((n > edge.BIG).sum()),
                                                        edge.BIG))
        assert int((n > edge.BIG).sum()) > 0 and int(((n > 0) & (n <= edge.BIG)).sum()) > 0
    # just below and just above: one triangle whose box is 16 x 16 = 256 and one whose box is 16 x 17 = 272 pixels
    for rows, above in ((13.0, False), (14.0, True)):
        sc = ec._soup([((0.5, 0.5, 0.0), (13.5, 0.5, 0.0), (0.5, rows + 0.5, 0.0))], size=(32, 32))
        n = int(edge.box_pixels(sc.v, sc.tri, sc.size)[0, 0])
        assert (n > edge.BIG) == above and abs(n - edge.BIG) <= 16, n
        v, tri = sc.v.to(DEV).requires_grad_(True), sc.tri.to(DEV)
        gen = torch.Generator().manual_seed(3)
        image, g = torch.rand((1, 3, 32, 32), generator=gen), torch.randn((1, 3, 32, 32), generator=gen)
        gv, = torch.autograd.grad(edge.antialias(image.to(DEV), v, tri), v, grad_outputs=g.to(DEV))
        vh = sc.v.clone().requires_grad_(True)
        gh, = torch.autograd.grad(edge.antialias_composite(image, vh, sc.tri), vh, grad_outputs=g)
        assert float(gh.abs().max()) > 0 and bits(gv, gh)


def test_reruns_are_bit_identical_and_nothing_depends_on_what_the_buffers_held():
    ref = host_case("disc", (64, 64), 1, 3)
    d = device_case(ref)
    first = run_device(d)
    again = run_device(d)
    assert all(bits(a, b) for a, b in zip(first, again))
    b, c, h, w = ref["image"].shape
    nv, nf = int(ref["v"].shape[1]), int(ref["tri"].shape[0])
    dims = (b, c, h, w, nv, nf)
    run = native(d["image"])
    for fill in (0x7F, 0xFF):                                                   # 0xff..: the int32 -1, a NaN as float
        def poisoned(*shape):
            return torch.full((int(torch.tensor(shape).prod()) * 4,), fill, dtype=torch.uint8, device=DEV).view(torch.float32).view(shape)

        out, gi, gc = poisoned(b, c, h, w), poisoned(b, c, h, w), poisoned(b, 3 * nf, 3)
        run.sr_edge_aa_fwd(out, d["image"], d["v"], d["tri"], d["opp"], d["face"], d["zbuf"], *dims)
        run.sr_edge_aa_bwd_image(gi, d["g"], d["v"], d["tri"], d["opp"], d["face"], d["zbuf"], *dims)
        run.sr_edge_aa_bwd_corner(gc, d["g"], d["image"], d["v"], d["tri"], d["opp"], d["face"], d["zbuf"], *dims)
        gv = edge._corners_to_vertices(gc, d["tri"], nv)
        assert bits(out, first[0]) and bits(gi, first[1]) and bits(gv, first[2])
        assert bool(torch.isfinite(gc).all()) and float(gc[..., 2].abs().max()) == 0.0


def test_captured_forward_and_backward_replay_on_changed_values():
    ref = host_case("ellipsoid", (33, 33), 1, 4)
    d = device_case(ref)
    image, v, g = d["image"].clone().requires_grad_(True), d["v"].clone().requires_grad_(True), d["g"]
    tri = d["tri"]
    opp = d["opp"]
    out = {}

    def body():
        face, zbuf = edge.face_map(v, tri, ref["size"])
        res = edge.antialias(image, v, tri, face, zbuf, opp)
        gi, gv = torch.autograd.grad(res, (image, v), grad_outputs=g)
        out.update(res=res.detach(), gi=gi, gv=gv)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    print("captured face map + forward + backward: %d kernel nodes of %d" % (graph.kernel_nodes, graph.nodes))
    held = dict(out)
    for step in (1, 2, 3):
        with torch.no_grad():
            image.mul_(0.5).add_(0.1 * step)
            v.add_(torch.tensor([0.011 * step, -0.007 * step, 0.0], device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        got = {k: t.clone() for k, t in held.items()}
        body()
        torch.cuda.synchronize()
        assert all(bits(got[k], out[k]) for k in got), step
    vh, ih = v.detach().cpu().requires_grad_(True), image.detach().cpu().requires_grad_(True)
    res = edge.antialias_composite(ih, vh, ref["tri"])
    gi, gv = torch.autograd.grad(res, (ih, vh), grad_outputs=ref["g"])
    assert bits(got["res"], res.detach()) and bits(got["gi"], gi) and bits(got["gv"], gv)


def test_strict_mode_refuses_what_the_kernels_do_not_take(monkeypatch):
    ref = host_case("edge25")
    monkeypatch.setenv("SR_STRICT_NATIVE", "1")
    d = device_case(ref)
    with pytest.raises(RuntimeError, match="SR_STRICT_NATIVE"):
        edge.antialias(d["image"].double(), d["v"].double(), d["tri"], d["face"], d["zbuf"].double(), d["opp"])


# ---- the terms in the captured fit ---------------------------------------------------------------------------------------
def disc_mask(b_n, size=16):
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    rows = [(((xx - size / 2 + 1.5 * k) ** 2 + (yy - size / 2) ** 2) < (0.3 * size) ** 2).float() for k in range(b_n)]
    return torch.stack(rows).to(DEV)


@pytest.mark.parametrize("b_n,more", [(1, {}), (2, {"shared_identity": 10})])
def test_silhouette_and_photo_edges_eager_equals_captured(b_n, more, monkeypatch):
    """The linear model at B = 1, and B = 2 with a shared identity, a camera and landmarks: the plain step carries the
    silhouette term, the photometric step carries it and photo_edges; both captured graphs against eager, bit for bit."""
    from test_photometric_gpu import inverter, linear_kw, problem, start_texture, state

    monkeypatch.setenv("SR_STRICT_NATIVE", "1")
    targets = problem("linear")[3][:b_n].contiguous()
    kw = dict(more, silhouette=disc_mask(b_n), silhouette_weight=2.0, photo_edges=True)
    if b_n > 1:
        kw.update(linear_kw(b_n))
    runs = {}
    for key, use_graph in (("eager", False), ("graph", True)):
        inv = inverter("linear", targets, use_graph, **kw)
        plain = state(inv, inv.run(5))
        inv.set_texture(start_texture(1))
        runs[key] = plain + state(inv, inv.run(5, photometric=True)) + [inv.coverage_fit.cpu().clone(),
                                                                        inv.sil.rows.detach().cpu().clone()]
        assert ((inv.graph is not None) == use_graph) and ((inv.graph_photo is not None) == use_graph)
        if use_graph:
            print("B", b_n, "silhouette step: kernel nodes", inv.graph.kernel_nodes, "; photometric step with edges:",
                  inv.graph_photo.kernel_nodes)
        del inv
    for i, (a, b) in enumerate(zip(runs["graph"], runs["eager"])):
        assert torch.equal(a, b), (b_n, i)
    assert all(bool(torch.isfinite(t).all()) for t in runs["graph"])
    assert float(runs["graph"][-1].min()) > 0                                    # the term is there
    # without the arguments the inverter is the one of before: same history as one built without them
    base = inverter("linear", targets, True, **{k: v for k, v in kw.items() if k not in ("silhouette", "silhouette_weight",
                                                                                          "photo_edges")})
    assert base.sil is None and not base.photo.edges
    assert not torch.equal(base.run(5).cpu(), runs["graph"][0])


@pytest.mark.parametrize("flags,images", [((), 1), (("--batch", "2", "--photo", "--photo_steps", "3", "--photo_edges"), 2)])
def test_reconstruct_with_a_silhouette_on_the_device(tmp_path, flags, images):
    from test_edge_cpu import check_tool_outputs, silhouette_dir
    from test_photometric_cpu import run_tool

    res, out = run_tool(tmp_path, "out", ("--silhouette_dir", silhouette_dir(tmp_path), "--gpu", "0") + flags,
                        {"SR_STRICT_NATIVE": "1"}, images=images)
    assert res.returncode == 0, res.stderr[-3000:]
    check_tool_outputs(out, ["face_b", "face_c"][:images])
