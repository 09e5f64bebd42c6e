"""GPU: the pose-aware landmark kernels (csrc/landmark.hip: sr_landmark_dyn_fwd / sr_landmark_dyn_bwd) against the float64
composite, their accumulate flag and graph behaviour, and a captured inverter step with contour lines and the gate."""
import numpy as np
import pytest
import torch

from stylerenderer_amd import face_model, graphs, synth
from stylerenderer_amd.op import landmark

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
HW = (48, 64)                                                            # H / 2 = 24, W / 2 = 32
VIS = (-0.25, 0.75)      # hi - lo = 1: the smoothstep's slope is at most 1.5, so m's fp32 rounding (1.2e-7) stays below 1e-6
EDGE = [1, 2, 63, 64, 65, 130]                                           # a wave's edge and the loop past it


def lengths_of(n_c, nv):
    if nv < 100:
        return [2] * (n_c - 1) + [3]                                     # (the pool of a small mesh holds no more)
    rest = [3 + (5 * k) % 11 for k in range(n_c)]
    return (EDGE + rest)[:n_c] if n_c >= len(EDGE) else rest


_CASES = {}


def case(b, n_l, nv, n_c, exact_u, seed=0):
    """Host float64 inputs on which the fp32 projection is exact (coordinates and normals in multiples of 1/128, weights
    of 1/4, targets of 1/64), as in test_landmark_gpu.case, with n_c contour lines on landmarks 1, 2, 4, 5, ... (all
    landmarks when n_c = n_l).  Every line's winner is put at 2 side u (rounded to 1/128), beyond every other score
    (|x| + |y| <= 1.75 / sqrt 2 on the random vertices), at a position that differs from line to line and sample to
    sample.  exact_u: the anchors give u = (1, 0) exactly; else their random coordinates give a generic direction.
    Traps: line 0's first candidate is vertex 0, which landmarks 0 and n_l - 1 carry statically (when they are not
    contour landmarks themselves); every line from the second on that has two candidates or more ends with the first
    candidate of the line before it (one vertex in two lines, of opposite sides); every line of four or more lists its
    candidate 1 again at position 2; the longest line has further vertices with the winner's coordinates at higher
    positions, 2, 64 and 66 after it (exact ties between lanes, between a lane's rounds and across both: the lowest
    position wins); the last sample of a batch has confidence 0 throughout.  On a small mesh
    (nv < 100, where 70 landmarks would otherwise touch every vertex) the last line has three candidates and the embedding
    stays off that line's own ones, so that every sample keeps an unselected candidate that carries nothing."""
    key = (b, n_l, nv, n_c, exact_u, seed)
    if key in _CASES:
        return _CASES[key]
    v = np.round(synth.det_uniform((b, nv, 3), 140 + seed) * 112) / 128
    nrm = np.round(synth.det_uniform((b, nv, 3), 141 + seed) * 112) / 128
    up, down = nv - 1, nv - 2
    if exact_u:
        v[:, up, :2], v[:, down, :2] = (0.25, 0.5), (0.25, -0.25)
    a = v[:, up, :2] - v[:, down, :2]
    u = np.stack((a[:, 1], -a[:, 0]), 1) / np.linalg.norm(a, axis=1, keepdims=True)
    assert np.linalg.norm(a, axis=1).min() > 0.05
    # lines
    line_lmk = list(range(n_l)) if n_c == n_l else [l for l in range(n_l) if l % 3][:n_c]
    assert len(line_lmk) == n_c
    lens = lengths_of(n_c, nv)
    pool = (1 + np.random.RandomState(7 + seed).permutation(nv - 3)).tolist()            # not vertex 0, not the anchors
    lines, side = [], [1 if c % 2 == 0 else -1 for c in range(n_c)]
    for c, n in enumerate(lens):
        ids = [pool.pop() for _ in range(n)]
        if c == 0 and n_c < n_l:
            ids[0] = 0
        if c >= 1 and n >= 2:
            ids[-1] = lines[c - 1][0]
        if n >= 4:
            ids[2] = ids[1]
        lines.append(ids)
    # the embedding: on a small mesh it leaves the last line's own candidates alone, so that an unselected one carries nothing
    own = [i for i in lines[-1] if i != 0 and (n_c == 1 or i != lines[-2][0])] if nv < 100 else []
    free = np.array([i for i in range(nv) if i not in own])
    idx = np.zeros((n_l, 3), np.int64)
    bary = np.zeros((n_l, 3), np.float32)
    for l in range(n_l):
        if l % 3 == 0:
            idx[l], bary[l] = free[(5 * l) % len(free)], (1, 0, 0)
        else:
            idx[l] = free[[(7 * l) % len(free), (7 * l + 1) % len(free), (7 * l + 3) % len(free)]]
            bary[l] = (0.5, 0.25, 0.25) if l % 3 == 1 else (0.25, 0.25, 0.5)
    idx[-1], bary[-1] = idx[0], (1, 0, 0)
    for s in range(b):
        for c, ids in enumerate(lines):
            pos = (5 * s + 3 * c + 1) % len(ids)
            if len(ids) >= 4 and pos == 2:
                pos = 3
            if c + 1 < n_c and len(lines[c + 1]) >= 2 and pos == 0:
                pos = 1 % len(ids)                       # (candidate 0 is the next line's last: it is not moved about)
            if c >= 1 and len(ids) >= 2 and pos == len(ids) - 1:
                pos = len(ids) - 2
            v[s, ids[pos], :2] = np.round(side[c] * 2.0 * u[s] * 128) / 128
    longest = int(np.argmax(lens))
    if lens[longest] >= 6:
        for s in range(b):
            scores = side[longest] * (v[s, lines[longest], :2] @ u[s])
            first = int(np.argmax(scores))
            # twins at higher positions, other vertices (not the repeated one): one in the winner's own stride of 64 (the
            # rule between lanes), and where the line is long enough one at first + 64 (the same lane, the next round of
            # its loop) and one at first + 66 (another lane, another round)
            for step in (2, 64, 66):
                if first + step < lens[longest] - 1:
                    twin = lines[longest][first + step]
                    assert twin != lines[longest][first]
                    v[s, twin, :2] = v[s, lines[longest][first], :2]
            assert first + 2 < lens[longest] - 1 and (lens[longest] < 130 or first + 66 < lens[longest] - 1)
    off = np.concatenate(([0], np.cumsum(lens)))
    tables = (np.array(line_lmk), np.array(side), off, np.array([i for ids in lines for i in ids]))
    idx_t, bary_t = torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(bary)
    v64, n64 = torch.from_numpy(v), torch.from_numpy(nrm)
    axis = (up, down)
    zero = torch.zeros(b, n_l, 2, dtype=torch.float64)
    p = landmark.landmark_dynamic_composite(v64, idx_t, bary_t.double(), zero, zero[..., 0], HW, lines=tables, axis=axis)[1]
    target = p - torch.from_numpy(np.round(synth.det_uniform((b, n_l, 2), 142 + seed) * 4 * 64) / 64)
    conf = torch.from_numpy(np.abs(synth.det_uniform((b, n_l), 143 + seed)) + 0.125)
    if b > 1:
        conf[-1] = 0.0
    gout = torch.from_numpy(synth.det_normal((b,), 144 + seed)) + 2.0
    assert torch.equal(target.float().double(), target) and torch.equal(v64.float().double(), v64)
    _CASES[key] = dict(v=v64, normals=n64, idx=idx_t, bary=bary_t, target=target, conf=conf, gout=gout, lines=tables,
                       axis=axis, lens=lens)
    return _CASES[key]


def gaps(v, lines, axis):
    """Best minus second-best score of every (sample, line) in float64, candidates at the winner's own coordinates (the
    deliberate exact ties, and a vertex listed twice) left aside; inf where there is no other candidate."""
    lm, side, off, cand = lines
    out = np.full((v.shape[0], len(lm)), np.inf)
    ties = 0
    for b in range(v.shape[0]):
        vb = v[b].numpy()
        a = vb[axis[0], :2] - vb[axis[1], :2]
        u = np.array([a[1], -a[0]]) / np.hypot(a[0], a[1])
        for c in range(len(lm)):
            ids = cand[off[c]:off[c + 1]]
            s = side[c] * (vb[ids, :2] @ u)
            j = int(np.argmax(s))
            same = np.all(vb[ids, :2] == vb[ids[j], :2], axis=1)
            ties += int(len(set(ids[same])) > 1)
            if not same.all():
                out[b, c] = s[j] - s[~same].max()
    return out, ties


def run(c, dtype=torch.float32, vis=VIS, beta=0.75, weight=1.5, **over):
    """(rows, p, sel, gate, gv) through landmark_loss_ex on the device in `dtype` (float64: the composite)."""
    t = lambda x: x.to(DEV, dtype) if x.is_floating_point() else x.to(DEV)                       # noqa: E731
    d = {k: t(x) for k, x in dict(c, **over).items() if isinstance(x, torch.Tensor)}
    v = d["v"].clone().requires_grad_(True)
    rows, p, sel, gate = landmark.landmark_loss_ex(v, d["idx"], d["bary"], d["target"], d["conf"], HW, beta, weight,
                                                   normals=d["normals"] if vis is not None else None, lines=c["lines"],
                                                   axis=c["axis"], vis=vis)
    (gv,) = torch.autograd.grad((rows * d["gout"]).sum(), v)
    return rows.detach(), p.detach(), sel, gate.detach(), gv


SHAPES = [(1, 5, 40, 1, True), (3, 5, 1000, 1, False), (3, 70, 1000, 17, False), (1, 70, 1000, 17, True),
          (3, 70, 1000, 70, True), (3, 70, 40, 17, False)]              # C = 70: more lines than waves, no static landmark


@pytest.mark.parametrize("b,n_l,nv,n_c,exact_u", SHAPES)
def test_kernels_against_the_float64_composite(b, n_l, nv, n_c, exact_u):
    c = case(b, n_l, nv, n_c, exact_u)
    gap, ties = gaps(c["v"], c["lines"], c["axis"])
    print("b %d L %d nv %d C %d: smallest score gap %.4g over %d (sample, line) pairs, %d exact ties, line lengths %s"
          % (b, n_l, nv, n_c, gap.min(), gap.size, ties, sorted(set(c["lens"]))))
    assert gap.min() >= 1e-3                                             # every line of every sample
    if max(c["lens"]) >= 6:
        assert ties >= b
    rows, p, sel, gate, gv = run(c)
    assert rows.shape == (b,) and p.shape == (b, n_l, 2) and gv.shape == (b, nv, 3)
    assert sel.shape == (b, n_c) and sel.dtype == torch.int32 and gate.shape == (b, n_l)
    w_rows, w_p, w_sel, w_gate, w_gv = run(c, torch.float64)
    assert torch.equal(sel, w_sel)
    if b > 1 and max(c["lens"]) > 2:
        assert not torch.equal(sel[0], sel[1])                           # the selection follows the sample's vertices
    err_p = float((p.double() - w_p).abs().max())
    err_rows = (rows.double() - w_rows).abs()
    err_gv = float((gv.double() - w_gv).abs().max())
    err_gate = float((gate.double() - w_gate).abs().max())
    print("  rows rel %.3g, gv %.3g of max %.3g, p %.3g px, gate %.3g (gates in (0, 1): %d)" % (
        float((err_rows / w_rows.abs().clamp_min(1e-30)).max()), err_gv, float(w_gv.abs().max()), err_p, err_gate,
        int(((w_gate > 0) & (w_gate < 1)).sum())))
    assert err_p <= 1e-4
    assert bool((err_rows <= 1e-5 * w_rows.abs()).all()), (rows, w_rows)
    assert float(w_rows[0]) > 0 and err_gv <= 1e-5 * float(w_gv.abs().max())
    assert err_gate <= 1e-6
    lm = torch.from_numpy(c["lines"][0]).to(DEV)
    assert bool((gate[:, lm] == 1).all())
    if n_c < n_l:
        assert bool(((w_gate > 0) & (w_gate < 1)).any()) and bool((w_gate == 0).any())
    if b > 1:
        assert float(rows[-1]) == 0.0 and float(gv[-1].abs().max()) == 0.0
    # exactly 0 in z and on every vertex that carries nothing in this sample, unselected candidates included
    static = torch.zeros(n_l, dtype=torch.bool)
    static[:] = True
    static[c["lines"][0]] = False
    used = torch.zeros(b, nv, dtype=torch.bool, device=DEV)
    used[:, c["idx"][static].long()[c["bary"][static] != 0].to(DEV)] = True
    used.scatter_(1, w_sel.long(), True)
    assert bool((~used).any(1).all())                                    # every sample has vertices that carry nothing
    assert float(gv[..., 2].abs().max()) == 0.0 and float(gv[~used].abs().max()) == 0.0
    assert float(gv[0][used[0]][:, :2].abs().max()) > 0
    cand = torch.from_numpy(np.unique(c["lines"][3])).to(DEV)
    idle = ~used[0, cand]
    if max(c["lens"]) > 1:
        assert bool(idle.any()) and float(gv[0, cand[idle]].abs().max()) == 0.0
    # reruns: the same bits
    again = run(c)
    for x, y in zip((rows, p, sel, gate, gv), again):
        assert torch.equal(x, y)
    # without the gate every gate is 1 and the selection is the same
    _, _, sel_n, gate_n, _ = run(c, vis=None)
    assert torch.equal(sel_n, sel) and bool((gate_n == 1).all())


def test_without_lines_and_gate_the_dynamic_kernels_equal_the_static_ones():
    """C = 0 and no gate through sr_landmark_dyn_*: the same sums in the same order as sr_landmark_loss_*."""
    c = case(3, 70, 1000, 17, False)
    d = {k: (x.to(DEV, torch.float32) if x.is_floating_point() else x.to(DEV)) for k, x in c.items()
         if isinstance(x, torch.Tensor)}
    rows, p, g, lists = landmark.landmark_forward(d["v"], d["idx"], d["bary"], d["target"], d["conf"], HW, 0.75, 1.5)
    gv = landmark.landmark_backward(g, d["gout"], lists, 1000, HW)
    r2, p2, g2, sel, gate, t = landmark.landmark_dynamic_forward(d["v"], d["idx"], d["bary"], d["target"], d["conf"], HW,
                                                                 0.75, 1.5)
    gv2 = landmark.landmark_dynamic_backward(g2, d["gout"], sel, t, 1000, HW)
    assert sel.shape == (3, 0) and bool((gate == 1).all())
    for a, b in ((rows, r2), (p, p2), (g, g2), (gv, gv2)):
        assert torch.equal(a, b)


def test_accumulate_flag_adds_to_the_last_bit():
    c = case(3, 70, 1000, 17, False, seed=3)
    d = {k: (x.to(DEV, torch.float32) if x.is_floating_point() else x.to(DEV)) for k, x in c.items()
         if isinstance(x, torch.Tensor)}
    rows, p, g, sel, gate, t = landmark.landmark_dynamic_forward(d["v"], d["idx"], d["bary"], d["target"], d["conf"], HW,
                                                                 1.0, 1.0, d["normals"], c["lines"], c["axis"], VIS)
    plain = landmark.landmark_dynamic_backward(g, d["gout"], sel, t, 1000, HW)
    gv_in = torch.from_numpy(synth.det_normal((3, 1000, 3), 160)).to(DEV)
    out = gv_in.clone()
    assert landmark.landmark_dynamic_backward(g, d["gout"], sel, t, 1000, HW, out=out) is out
    assert torch.equal(out, gv_in + plain) and not torch.equal(out, gv_in)
    one = d["gout"][:1].expand(3)                                        # a broadcast incoming gradient: stride 0
    assert one.stride(0) == 0
    assert torch.equal(landmark.landmark_dynamic_backward(g, one, sel, t, 1000, HW),
                       landmark.landmark_dynamic_backward(g, one.contiguous(), sel, t, 1000, HW))


def test_second_order_goes_through_the_composite():
    c = case(3, 5, 1000, 1, False, seed=4)
    d = {k: (x.to(DEV, torch.float32) if x.is_floating_point() else x.to(DEV)) for k, x in c.items()
         if isinstance(x, torch.Tensor)}
    v = d["v"].clone().requires_grad_(True)
    rows, _ = landmark.landmark_loss(v, d["idx"], d["bary"], d["target"], d["conf"], HW, normals=d["normals"],
                                     lines=c["lines"], axis=c["axis"], vis=VIS)
    (gv,) = torch.autograd.grad((rows * d["gout"]).sum(), v, create_graph=True)
    (g2,) = torch.autograd.grad((gv ** 2).sum(), v)
    v64 = c["v"].to(DEV).requires_grad_(True)
    r64 = landmark.landmark_dynamic_composite(v64, d["idx"], d["bary"].double(), c["target"].to(DEV), c["conf"].to(DEV), HW,
                                              normals=c["normals"].to(DEV), lines=c["lines"], axis=c["axis"], vis=VIS)[0]
    (gv64,) = torch.autograd.grad((r64 * c["gout"].to(DEV)).sum(), v64, create_graph=True)
    (w2,) = torch.autograd.grad((gv64 ** 2).sum(), v64)
    assert float((g2.double() - w2).abs().max()) <= 1e-4 * float(w2.abs().max()) and float(w2.abs().max()) > 0


def test_captured_forward_and_backward_equal_eager_and_follow_their_buffers():
    c = case(3, 70, 1000, 17, False, seed=5)
    o = case(3, 70, 1000, 17, False, seed=6)                             # other vertices: another selection
    f32 = lambda x: x.to(DEV, torch.float32)                                                     # noqa: E731
    v, nrm, target, conf, gout = (f32(c[k]) for k in ("v", "normals", "target", "conf", "gout"))
    v.requires_grad_(True)
    out = {}

    def body():
        rows, p, sel, gate = landmark.landmark_loss_ex(v, c["idx"], c["bary"], target, conf, HW, normals=nrm,
                                                       lines=c["lines"], axis=c["axis"], vis=VIS)
        (gv,) = torch.autograd.grad((rows * gout).sum(), v)
        out.update(rows=rows.detach(), p=p, sel=sel, gate=gate, gv=gv)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                                           # the lists are built here, once
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = graphs.capture(body)
    print("captured forward + backward: %d kernel nodes of %d" % (graph.kernel_nodes, graph.nodes))
    held = dict(out)
    sels = []
    for src in (c, o, c):
        with torch.no_grad():
            v.copy_(f32(src["v"]))
            target.copy_(f32(src["target"]))
            conf.copy_(f32(src["conf"]).flip(0) if src is o else f32(src["conf"]))
        graph.replay()
        got = [held[k].clone() for k in ("rows", "p", "sel", "gate", "gv")]
        want = run(dict(c, v=v.detach(), target=target, conf=conf), beta=1.0, weight=1.0)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        sels.append(got[2])
    assert torch.equal(sels[0], sels[2]) and not torch.equal(sels[0], sels[1])


# ---- a captured inverter step with lines and gate -------------------------------------------------------------------------
def _hand_lines(fm, emb):
    """Lines on the 68 evenly spread landmarks of test_landmark_gpu's face: landmarks 0-16 slide over their own vertex and
    the 20 that follow it in the mesh; the anchors are the vertices of landmarks 27 and 8."""
    main = face_model.landmark_vertices(emb)
    nv = fm.fc.bias.numel() // 3
    cand = np.concatenate([(main[l] + np.arange(21)) % nv for l in range(17)])
    lines = (np.arange(17), np.where(np.arange(17) < 8, 1, -1), 21 * np.arange(18), cand)
    return lines, (int(main[27]), int(main[8]))


def test_captured_step_with_lines_and_gate_stays_native_and_adds_no_launch():
    """Counted like test_landmark_gpu.test_step_with_landmarks_stays_native_and_adds_few_launches: the captured step with
    contour lines and the gate has the kernel nodes and the nodes of the step with the static term."""
    import os

    from torch.utils._python_dispatch import TorchDispatchMode

    from test_landmark_gpu import _embedding, _face, _inverter, _landmarks, _state
    from test_reconstruct_batch_gpu import _faces

    assert os.environ.get("SR_STRICT_NATIVE") == "1"
    fm, _ = _face()
    lines, axis = _hand_lines(fm, _embedding(fm))
    dyn = dict(landmark_lines=lines, landmark_axis=axis, landmark_vis=(0.0, 0.2))
    faces, lmk = _faces(2), _landmarks(2)
    banned = ("aten::mm", "aten::addmm", "aten::mv", "aten::linear", "aten::matmul", "aten::bmm", "aten::index_add_",
              "aten::index_add", "aten::addmv", "aten::baddbmm", "aten::convolution", "aten::cudnn_convolution",
              "aten::miopen_convolution", "aten::index_put_", "aten::index_put", "aten::scatter_add", "aten::scatter_add_")
    seen = []

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func._schema.name in banned:
                seen.append(func._schema.name)
            return func(*args, **(kwargs or {}))

    eager = _inverter(faces, False, landmarks=lmk, **dyn)
    eager._iteration()                                   # lazy preparation outside the spy
    with Spy():
        eager._iteration()
    assert not seen, seen
    del eager
    eager = _inverter(faces, False, landmarks=lmk, **dyn)
    want = _state(eager, eager.run(8)) + [eager.contour_fit.cpu(), eager.landmark_visibility.cpu()]
    del eager
    nodes = {}
    for key, kw in (("static", {}), ("dynamic", dyn)):
        inv = _inverter(faces, True, landmarks=lmk, **kw)
        hist = inv.run(8)
        nodes[key] = (inv.graph.kernel_nodes, inv.graph.nodes)
        if kw:
            got = _state(inv, hist) + [inv.contour_fit.cpu(), inv.landmark_visibility.cpu()]
            assert got[5].shape == (2, 17) and got[6].shape == (2, 68)
        del inv
    print("(kernel nodes, nodes) of the captured step:", nodes)
    assert nodes["dynamic"] == nodes["static"]
    for a, b in zip(got, want):
        assert torch.equal(a, b)
