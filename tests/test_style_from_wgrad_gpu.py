"""Style gradient from the weight gradient's per-sample partial slabs (csrc/wgrad_style_finish.h, op/wgrad_style.py,
op.conv._conv_grads; SR_STYLE_FROM_WGRAD=0 restores the row-dot pass).

Reference: float64 on the CPU from the definitions — dxu = the adjoint convolution of oscale * g with W,
gis[b, c] = sum_p x * dxu, dW = sum_b corr(iscale * x, oscale * g).  Error measure and bar are those of the kernel family
(tests/test_wgrad_s2_wino_gpu.py): max |got - float64| / (the same sum over absolute values) < 2e-6.  Which path a call
takes is read from the native query (op.wgrad_style.part_floats) and from the helper's own counters, never assumed."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-6
SWITCH = "SR_STYLE_FROM_WGRAD"
GEOM = {"c3": (3, 1, 1, False), "t3s2": (3, 2, 0, True)}

# (geom, B, C, N, H, W, whole K slices per sample the plan is expected to have)
ALIGNED = [
    ("c3", 3, 64, 64, 32, 16, 1),        # 16 chunks per sample = one slice each; batch not a power of two
    ("c3", 2, 64, 128, 64, 16, 2),       # two slices per sample, two 64-wide n blocks: the partial sum over them runs
    ("t3s2", 3, 128, 32, 8, 16, 2),      # k_wgrad_s2p under its force switch: two one-patch slices per sample
]
# the fused stride-1 node needs maps the forward Winograd kernel takes (H % 8 == 0, W % 32 == 0): the same chunk counts
# per sample as the first two shapes, on 16 x 32 and 32 x 32 maps
NODES = [("c3", 3, 64, 64, 16, 32, 1), ("c3", 2, 64, 128, 32, 32, 2), ALIGNED[2]]
NOT_ALIGNED = ("c3", 2, 64, 64, 8, 32)   # 8 chunks per sample in slices of 16
IDS = lambda s: "%s-B%d-C%d-N%d-%dx%d" % tuple(s[:6])  # noqa: E731


def _out_size(geom, h, w):
    return (2 * h + 1, 2 * w + 1) if geom == "t3s2" else (h, w)


def _inputs(geom, b, c, n, h, w, seed=0):
    g = torch.Generator().manual_seed(1000 * b + 10 * c + n + h + seed)
    oh, ow = _out_size(geom, h, w)
    return dict(x=torch.randn(b, c, h, w, generator=g), gy=torch.randn(b, n, oh, ow, generator=g),
                wt=torch.randn(9, c, n, generator=g) / (3 * c ** 0.5), iscale=torch.randn(b, c, generator=g),
                oscale=torch.randn(b, n, generator=g).abs() + 0.5)


def _f64(geom, x, gy, wt, iscale, oscale):
    """float64 (gx, dW [9, C, N], gis [B, C]) and the absolute-product sums of dW and gis."""
    c, n = wt.shape[1:]

    def run(x, gy, wt, iscale, oscale):
        w4 = wt.view(3, 3, c, n)
        gs = gy * oscale[:, :, None, None] if oscale is not None else gy
        xs = x * iscale[:, :, None, None]
        if geom == "c3":        # y = conv(xs, w): adjoint = correlation with flipped taps, channels swapped
            dxu = F.conv2d(gs, w4.permute(2, 3, 0, 1).flip(2, 3), padding=1)
            cols = F.unfold(xs, 3, padding=1).view(x.shape[0], c, 9, -1)                       # [B, C, tap, P]
            dw = torch.einsum("bctp,bnp->tcn", cols, gs.flatten(2))
        else:                   # y = conv_transpose(xs, w, stride 2): adjoint = the stride-2 convolution
            dxu = F.conv2d(gs, w4.permute(2, 3, 0, 1), stride=2)
            cols = F.unfold(gs, 3, stride=2).view(x.shape[0], n, 9, -1)                        # [B, N, tap, P]
            dw = torch.einsum("bntp,bcp->tcn", cols, xs.flatten(2))
        return dxu * iscale[:, :, None, None], dw, (x * dxu).sum((2, 3))

    D = lambda t: None if t is None else t.detach().cpu().double()  # noqa: E731
    A = lambda t: None if t is None else t.detach().cpu().double().abs()  # noqa: E731
    gx, dw, gis = run(D(x), D(gy), D(wt), D(iscale), D(oscale))
    _, dw_mag, gis_mag = run(A(x), A(gy), A(wt), A(iscale), A(oscale))
    return gx, dw, gis, dw_mag, gis_mag


def _rel(got, want, mag):
    return float(((got.detach().cpu().double() - want).abs() / (mag + 1e-30)).max())


def _dev(d):
    return {k: (None if v is None else v.to(DEV)) for k, v in d.items()}


def _query(geom, x, gy):
    from stylerenderer_amd.op import wgrad_style

    return wgrad_style.part_floats(x, gy, *GEOM[geom])


def _grads(geom, t, need=(True, True, True)):
    """(gx, gw, gis) of the shared backward helper outside a recorded pass, and which path it counted."""
    from stylerenderer_amd.op import conv as cv

    before = dict(cv.STYLE_PATH_COUNTS)
    with torch.no_grad():
        out = cv._conv_grads(t["x"], t["gy"], t["wt"], t["iscale"], t["oscale"], geom, *need)
    took = {k: cv.STYLE_PATH_COUNTS[k] - before[k] for k in before}
    return out, took


def _set(monkeypatch, geom, on):
    monkeypatch.setenv("SR_WGRAD_S2_WINO", "force") if geom == "t3s2" else monkeypatch.delenv("SR_WGRAD_S2_WINO", raising=False)
    monkeypatch.delenv(SWITCH, raising=False) if on else monkeypatch.setenv(SWITCH, "0")


# ---- 1. the operator against float64 ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("with_oscale", [True, False], ids=["oscale", "plain"])
@pytest.mark.parametrize("shape", ALIGNED, ids=IDS)
def test_style_and_weight_gradient_vs_float64_and_bit_repeatable(shape, with_oscale, monkeypatch):
    from util import kernel_ran, launched_kernels

    geom, sps = shape[0], shape[6]
    t = _inputs(*shape[:6])
    if not with_oscale:
        t["oscale"] = None
    want_gx, want_dw, want_gis, dw_mag, gis_mag = _f64(geom, **t)
    t = _dev(t)
    _set(monkeypatch, geom, True)
    b, c, n = shape[1:4]
    nfl = _query(geom, t["x"], t["gy"])
    assert nfl == (b * n * c if geom == "t3s2" else b * c * (n // 64)), "the plan has no whole slices per sample"
    ((gx, gw, gis), took), names = launched_kernels(lambda: _grads(geom, t))
    assert took == {"wgrad": 1, "rowdot": 0}
    assert kernel_ran(names, "k_wgrad_style_finish") and kernel_ran(names, "k_wgrad_style_sum"), names
    assert not kernel_ran(names, "k_rowdot") and not kernel_ran(names, "k_wgrad_wino_finish"), names
    assert not kernel_ran(names, "k_wgrad_s2p_finish"), names
    assert kernel_ran(names, "k_wgrad_s2p" if geom == "t3s2" else "k_wgrad_wino"), names
    (gx2, gw2, gis2), _ = _grads(geom, t)
    _set(monkeypatch, geom, False)
    assert _query(geom, t["x"], t["gy"]) == nfl                    # the native query answers for the plan, not the switch
    ((gx0, gw0, gis0), took0), names0 = launched_kernels(lambda: _grads(geom, t))
    assert took0 == {"wgrad": 0, "rowdot": 1}
    assert kernel_ran(names0, "k_rowdot") and not kernel_ran(names0, "k_wgrad_style_finish"), names0
    e_gis, e_gis0 = _rel(gis, want_gis, gis_mag), _rel(gis0, want_gis, gis_mag)
    e_dw, e_dw0 = _rel(gw, want_dw, dw_mag), _rel(gw0, want_dw, dw_mag)
    print("style-from-wgrad %s (%d slices/sample, oscale %s): gis error %.3e (row-dot path %.3e), dW error %.3e (plain "
          "finish %.3e) of the absolute-product sums, bar %.1e" % (IDS(shape), sps, with_oscale, e_gis, e_gis0, e_dw, e_dw0, BAR))
    assert e_gis < BAR and e_dw < BAR
    assert e_gis0 < BAR and e_dw0 < BAR
    assert torch.equal(gis, gis2) and torch.equal(gw, gw2) and torch.equal(gx, gx2)
    assert torch.equal(gx, gx0), "the adjoint convolution's store rounds iscale * dxu differently from the row-dot pass"
    assert _rel(gx, want_gx, want_gx.abs().max()) < 1e-5


# ---- 2. the fused nodes, switch on against switch off --------------------------------------------------------------------
class _Recorder:
    """Stands in for op.conv.conv2d_wgrad_mfma: keeps the operands of the 3x3 calls (the cotangent that reaches the
    convolution is made inside the node)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, x, gy, xscale=None, gscale=None, ksize=3, stride=1, pad=1, transposed=False):
        if ksize == 3:
            self.calls.append((x.detach(), gy.detach(), xscale, gscale))
        return self.real(x, gy, xscale, gscale, ksize, stride, pad, transposed)


def _node(geom, t, noise, nw, ab, kernel):
    from stylerenderer_amd.op import conv as cv

    if geom == "t3s2":
        return cv.upconv_nba(t["x"], t["wt"], t["iscale"], t["oscale"], kernel, (1, 1), noise, nw, ab)
    assert cv.conv_nba_supported(t["x"], t["wt"], noise)
    return cv.conv2d_nba(t["x"], t["wt"], t["iscale"], t["oscale"], noise, nw, ab)


def _node_case(shape, seed=3):
    geom, (b, c, n, h, w) = shape[0], shape[1:6]
    t = _dev(_inputs(geom, b, c, n, h, w, seed))
    oh, ow = (2 * h, 2 * w) if geom == "t3s2" else (h, w)
    g = torch.Generator().manual_seed(77 + b + n)
    noise = torch.randn(1, 1, oh, ow, generator=g).to(DEV)
    nw, ab = torch.randn(1, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    proj = torch.randn(b, n, oh, ow, generator=g).to(DEV)
    k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
    kernel = (k1[None, :] * k1[:, None] / 64.0 * 4.0).to(DEV)
    return geom, t, noise, nw, ab, kernel, proj


def _node_grads(case, wrt, create_graph=False):
    from stylerenderer_amd.op import conv as cv

    geom, t, noise, nw, ab, kernel, proj = case
    leaf = {k: (v.clone().requires_grad_(k in wrt) if v is not None else None) for k, v in t.items()}
    y = _node(geom, leaf, noise, nw, ab, kernel)
    before = dict(cv.STYLE_PATH_COUNTS)
    grads = torch.autograd.grad((y * proj).sum(), [leaf[k] for k in wrt], create_graph=create_graph)
    took = {k: cv.STYLE_PATH_COUNTS[k] - before[k] for k in before}
    return [g.detach() for g in grads], took


@gpu
@pytest.mark.parametrize("shape", NODES, ids=IDS)
def test_fused_nodes_with_the_switch_on_and_off(shape, monkeypatch):
    from stylerenderer_amd.op import conv as cv

    case = _node_case(shape)
    geom, t = case[0], case[1]
    _set(monkeypatch, geom, False)
    rec = _Recorder(cv.conv2d_wgrad_mfma)
    monkeypatch.setattr(cv, "conv2d_wgrad_mfma", rec)
    (gx0, gw0, gis0), took0 = _node_grads(case, ("x", "wt", "iscale"))
    monkeypatch.setattr(cv, "conv2d_wgrad_mfma", rec.real)
    assert took0 == {"wgrad": 0, "rowdot": 1} and len(rec.calls) == 1
    _set(monkeypatch, geom, True)
    (gx, gw, gis), took = _node_grads(case, ("x", "wt", "iscale"))
    assert took == {"wgrad": 1, "rowdot": 0}
    xr, gyr, xs, gs = rec.calls[0]                               # the convolution's own cotangent, as the node made it
    assert torch.equal(xs, t["iscale"]) and torch.equal(gs, t["oscale"])
    _, want_dw, want_gis, dw_mag, gis_mag = _f64(geom, xr, gyr, t["wt"], xs, gs)
    e = {"gis on": _rel(gis, want_gis, gis_mag), "gis off": _rel(gis0, want_gis, gis_mag),
         "dW on": _rel(gw, want_dw, dw_mag), "dW off": _rel(gw0, want_dw, dw_mag)}
    print("node %s: %s (bar %.1e)" % (IDS(shape), ", ".join("%s %.3e" % kv for kv in e.items()), BAR))
    assert max(e.values()) < BAR, e
    assert torch.equal(gx, gx0)


# ---- 3. everything else keeps the row-dot path, bit for bit ---------------------------------------------------------------
@gpu
@pytest.mark.parametrize("what", ["gw not wanted", "create_graph", "not aligned"])
def test_fallbacks_are_bit_identical_to_the_switch_off(what, monkeypatch):
    shape = (NOT_ALIGNED if what == "not aligned" else NODES[0][:6])
    case = _node_case(shape)
    geom, t = case[0], case[1]
    wrt = ("x", "iscale") if what == "gw not wanted" else ("x", "wt", "iscale")
    res = {}
    for on in (False, True):
        _set(monkeypatch, geom, on)
        res[on] = _node_grads(case, wrt, create_graph=(what == "create_graph"))
    assert (_query(geom, t["x"], t["gy"]) < 0) == (what == "not aligned")     # (the plan alone: what the native side knows)
    (g_off, took_off), (g_on, took_on) = res[False], res[True]
    assert took_on["wgrad"] == 0 and took_on["rowdot"] >= 1 and took_on == took_off, (took_on, took_off)
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b), what
