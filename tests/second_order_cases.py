"""First- and second-order results of the fused convolution nodes and the activation tails, in plain torch.

With the LeakyReLU sign pattern fixed every node is multilinear in its inputs:

    v   = blur(oscale * conv(iscale * x, wt)) + noise_w * noise + bias + addend        (each piece optional)
    y   = m * v,  m in {gain, slope * gain} per element                                (nodes with an activation)
    rgb = sum_c ws[b, j, c] * y[b, c] + rgb_bias                                       (the forked node)

so ONE composite (`compose`, the "twin" of a node once the node's keys are chosen) differentiated by float64 autograd
gives every first- and second-order result, and the same composite on the absolute values of every input, cotangent,
probe and mask gives, per element of each result, the exact sum of the absolute terms that make it up (`mag`): the
scale a float32 evaluation's round-off is measured against.  The mask is an INPUT: `mask_of(y_device)`, the device's
own forward output, which is also where the device's recorded backward takes the mask of every order from.

`evaluate` is the driver for both sides (the twin on the CPU, the device node on the GPU), `compare` the comparator,
`CASES` the table the GPU tests run and the CPU tests prove `mag` dominance and the float32 self-check on, `bars` the
round-off bar of every result from the passes on its longest path.  The mirror functions at the end restate the
recursion of op.conv.ConvFn / WgradFn in torch so that a CPU test can break one rule at a time (`MUTATIONS`)."""
import math

import torch
from torch.autograd import Function
from torch.nn import functional as F

GEOM = {  # name -> (ksize, stride, pad, transposed), as op.conv._GEOM
    "c3": (3, 1, 1, False), "c3s2": (3, 2, 0, False), "t3s2": (3, 2, 0, True), "c1": (1, 1, 0, False),
    "c1s2": (1, 2, 0, False),
}
ADJOINT = {"c3": "c3", "c3s2": "t3s2", "t3s2": "c3s2", "c1": "c1"}
DIFF = ("x", "wt", "iscale", "oscale", "bias", "noise_w", "addend", "ws", "rgb_bias")     # differentiable inputs
COTANGENTS = (("y", "gy"), ("rgb", "g_rgb"))
SLOPE, GAIN = 0.2, math.sqrt(2.0)


# ---- the composite ------------------------------------------------------------------------------------------------------
def conv(x, wt, geom):
    """wt [k*k, C, N] tap-major (op.conv.conv2d_mfma)."""
    k, stride, pad, tr = GEOM[geom]
    _, c, n = wt.shape
    w4 = wt.reshape(k, k, c, n)
    if tr:
        return F.conv_transpose2d(x, w4.permute(2, 3, 0, 1), stride=stride, padding=pad)
    return F.conv2d(x, w4.permute(3, 2, 0, 1), stride=stride, padding=pad)


def _bc(s):
    return s[:, :, None, None]


def compose(t, mut=None):
    """{"y": ..., ["rgb": ...]} from the keys present in `t` (a key holding None counts as absent).  `mut`: None, or the
    name of one broken rule (MUTATIONS) — the convolution then runs through the mirror functions below."""
    from stylerenderer_amd.op.upfirdn2d import _upfirdn2d_cpu

    has = lambda k: t.get(k) is not None  # noqa: E731
    v = t["x"]
    if has("wt"):
        if mut is None:
            v = conv(v * _bc(t["iscale"]) if has("iscale") else v, t["wt"], t["geom"])
            if has("oscale"):
                v = v * _bc(t["oscale"])
        else:
            inner_bias = has("bias") and not any(has(k) for k in ("m", "kernel", "noise", "addend"))      # ConvFn's own bias
            v = MirrorConv.apply(v, t["wt"], t.get("iscale"), t.get("oscale"), t["bias"] if inner_bias else None,
                                 t["geom"], mut)
            if inner_bias:
                t = dict(t, bias=None)
    if has("kernel"):
        v = _upfirdn2d_cpu(v, t["kernel"], 1, 1, t["pad"])
    if has("noise"):
        v = v + t["noise_w"] * t["noise"]
    if has("bias"):
        v = v + t["bias"][None, :, None, None]
    if has("addend"):
        v = v + t["addend"]
    if has("m"):
        m = t["m"]
        if mut == "mask_recomputed":
            m = mask_of(v.detach(), t["slope"], t["gain"]).to(v.dtype)
        v = m * v
    out = {"y": v}
    if has("ws"):
        out["rgb"] = torch.einsum("bjc,bchw->bjhw", t["ws"], v)
        if has("rgb_bias"):
            out["rgb"] = out["rgb"] + t["rgb_bias"][None, :, None, None]
    return out


def mask_of(y, slope=SLOPE, gain=GAIN):
    """The activation's factor per element from a forward OUTPUT (the sign of y is the sign of the pre-activation; with
    slope 0 the non-positive side is 0 either way)."""
    return torch.where(y > 0, 1.0, float(slope)).to(torch.float64) * float(gain)


# which keys make up each node (beyond geom / slope / gain / pad); compose() of exactly these keys is the node's twin
NODE_KEYS = {
    "ConvFn": ("x", "wt", "iscale", "oscale", "bias"),
    "ConvNBAFn": ("x", "wt", "iscale", "oscale", "noise", "noise_w", "bias", "m"),
    "UpConvNBAFn": ("x", "wt", "iscale", "oscale", "kernel", "noise", "noise_w", "bias", "m"),
    "ConvNBAForkFn": ("x", "wt", "iscale", "oscale", "noise", "noise_w", "bias", "m", "ws", "rgb_bias"),
    "Conv1x1AddFn": ("x", "wt", "oscale", "addend"),
    "_NBA": ("x", "noise", "noise_w", "bias", "m"),
    "_BlurNBA": ("x", "kernel", "noise", "noise_w", "bias", "m"),
    "fused_leaky_relu": ("x", "bias", "m"),
}
_SETTINGS = ("geom", "slope", "gain", "pad", "node")


def twin(node, mut=None):
    """The float64 composite of one node: compose() restricted to the node's own keys."""
    keys = NODE_KEYS[node] + _SETTINGS

    def run(t):
        return compose({k: t[k] for k in keys if k in t}, mut)

    return run


TWINS = {node: twin(node) for node in NODE_KEYS}


# ---- demodulation link of wiring "plr": oscale = rsqrt((s * s) @ wsq + 1e-8), outside the node --------------------------
class _AbsRsqrt1(Function):
    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return 0.5 * u ** -1.5

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g * 0.75 * u ** -2.5


class _AbsRsqrt(Function):
    """rsqrt whose first and second derivative carry their ABSOLUTE values (the true ones alternate in sign): the link of
    the `mag` evaluation.  wsq > 0, so u is the same number in both evaluations."""

    @staticmethod
    def forward(ctx, u):
        ctx.save_for_backward(u)
        return u.rsqrt()

    @staticmethod
    def backward(ctx, g):
        (u,) = ctx.saved_tensors
        return g * _AbsRsqrt1.apply(u)


def demod_link(s, wsq, absolute=False):
    u = (s * s) @ wsq + 1e-8
    return _AbsRsqrt.apply(u) if absolute else torch.rsqrt(u)


# ---- the driver ----------------------------------------------------------------------------------------------------------
def wiring_plan(t, wiring):
    """(leaves, first-order targets, second-order targets) — names — of one wiring for the tensors present in `t`."""
    const = tuple(t.get("const", ()))                # inputs the node itself takes as constants
    present = [k for k in DIFF if t.get(k) is not None and k not in const]
    cots = [c for _, c in COTANGENTS if t.get(c) is not None]
    if wiring == "full":
        return present + cots, present, present + cots
    if wiring == "plr":
        # train.g_path_regularize: the image's gradient w.r.t. the latents (here: the layer's input and its style, the
        # demodulation scale being a function of the style), then the parameters' gradient of its norm
        leaves = [k for k in present if k != "oscale"] + ["wsq"]
        second = [k for k in ("wt", "wsq", "noise_w", "bias", "x") if k in leaves]
        return leaves, ["x", "iscale"], second
    if wiring == "r1":
        # train.d_r1_loss: the logits' gradient w.r.t. the input, then the parameters' gradient of its square; the
        # discriminator's layers have no style and a constant output scale
        assert t.get("iscale") is None
        return [k for k in present if k != "oscale"], ["x"], [k for k in ("wt", "bias") if k in present]
    raise ValueError(wiring)


def evaluate(fn, tensors, dtype=torch.float64, absolute=False, wiring="full", order=2, device="cpu"):
    """{"y", ["rgb"], "g_<input>" per first-order target, "h_<input or cotangent>" per second-order target}, float64 on
    the CPU, of `fn` (a twin, or the device node) at `tensors`:

        first order    g_i = d <outputs, cotangents> / d input_i
        second order   q = sum_i <g_i, P_i> over ALL first-order results with independent probes P_i, differentiated
                       with respect to every second-order target of the wiring

    absolute: every tensor is replaced by its absolute value (the evaluation of `mag`).  order 1: no recorded backward
    (create_graph off — the device's fast kernels).  A result nobody produced (None from autograd) is zero."""
    def prep(v):
        v = v.detach().to(device=device, dtype=dtype if v.is_floating_point() else None)
        return v.abs() if absolute else v

    t = {k: (prep(v) if isinstance(v, torch.Tensor) else v) for k, v in tensors.items()}
    leaves, first, second = wiring_plan(t, wiring)
    for k in leaves:
        t[k] = t[k].clone().requires_grad_(True)
    call = {k: v for k, v in t.items() if k != "wsq" and not k.startswith("P_")}
    if wiring == "plr":
        call["oscale"] = demod_link(t["iscale"], t["wsq"], absolute)
    outs = fn(call)
    pairs = [(outs[o], t[c]) for o, c in COTANGENTS if o in outs and t.get(c) is not None]
    res = {o: v.detach() for o, v in outs.items()}
    grads = torch.autograd.grad([o for o, _ in pairs], [t[k] for k in first], [c for _, c in pairs],
                                create_graph=order > 1, allow_unused=True)
    for k, g in zip(first, grads):
        res["g_" + k] = torch.zeros_like(t[k]) if g is None else g.detach()
    if order > 1:
        q = sum((g * t["P_" + k]).sum() for k, g in zip(first, grads) if g is not None)
        hess = torch.autograd.grad(q, [t[k] for k in second], allow_unused=True)
        for k, h in zip(second, hess):
            res["h_" + k] = torch.zeros_like(t[k]) if h is None else h.detach()
    return {k: v.double().cpu() for k, v in res.items()}


def compare(got, want, mag, bars):
    """`_check` of test_dispatch_edges_gpu.py over the dict: {tensor: max |got - want| / mag}; fails with the tensor's
    name.  Every tensor of `want` must be in `got` and have a bar."""
    ratios, bad = {}, []
    for k in want:
        assert k in got, "%s: result missing" % k
        assert got[k].shape == want[k].shape, (k, tuple(got[k].shape), tuple(want[k].shape))
        ratios[k] = float(((got[k].double() - want[k]).abs() / (mag[k] + 1e-30)).max())
        if not ratios[k] <= bars[k]:
            bad.append("%s: error %.3e of the absolute-term sum (bar %.1e)" % (k, ratios[k], bars[k]))
    assert not bad, "; ".join(bad)
    return ratios


# ---- bars -----------------------------------------------------------------------------------------------------------------
# One pass of float32 round-off relative to `mag`, as the suite already states them:
D = 2e-6                # a direct MFMA convolution / weight gradient, or a reduction pass         (test_conv_vs_float64)
W = 4e-6                # a Winograd convolution pass                                  (test_winograd_conv_vs_float64_and_direct)
E = 10 * 2.0 ** -24     # a purely element-wise pass                                               (test_styled_map_tail_vs_float64)
CAP = 1.6e-5


def bars(t, wino=False):
    """{result: bar}: the sum over the chained passes on the result's longest path (profiles/second_order_notes.md holds
    the table with the code lines the chains were read from).  c = one convolution pass (W where the case's stride-1 3x3
    forward / adjoint takes the Winograd kernel), f = the blur where the node has one, a = the activation's
    element-wise pass where it has one."""
    has = lambda k: t.get(k) is not None  # noqa: E731
    c = (W if wino else D) if has("wt") else 0.0
    f = D if has("kernel") else 0.0
    a = E if has("m") else 0.0
    out = {
        "y": c + f + a + E,                       # conv, blur, tail (noise + bias + activation; scales in the store)
        "rgb": c + a + E + D,                     # y, then the ToRGB row product
        "g_x": a + f + c + 2 * E,                 # activation backward (+ ToRGB dx), blur^T, adjoint conv, * iscale
        "g_wt": a + f + D + E,                    # ... weight gradient
        "g_iscale": a + f + c + D + 2 * E,        # ... adjoint conv, row-dot with x (4e-6 in test_input_side_gradients)
        "g_oscale": c + f + a + D + 2 * E,        # y0 rebuilt from the output, row-dot with g, / oscale
        "g_bias": a + D + E, "g_noise_w": a + D + E,
        "g_addend": E,
        "g_ws": c + a + E + D, "g_rgb_bias": D,
        # second order: every term of q is one more chain of the same operators over inputs and probes; the longest:
        "h_x": a + f + c + D + 3 * E,             # P_is * dxu, dxu an adjoint conv; via gos: row-dot backward, adjoint conv
        "h_wt": c + f + a + 2 * D + E,            # adjoint conv, row-dot, weight gradient
        "h_iscale": c + f + a + D + 3 * E,        # adjoint conv (probe as weight), row-dot with x
        "h_oscale": c + f + a + D + 3 * E,        # conv of the probe, row-dot with g
        "h_wsq": c + f + a + 2 * D + 3 * E,       # gos (y0, row-dot), the link's derivative, s*s product
        "h_bias": a + D + E, "h_noise_w": a + D + E, "h_addend": E,
        "h_ws": c + f + a + D + 3 * E, "h_rgb_bias": D,
        "h_gy": c + f + a + D + 3 * E,            # x * P_is, adjoint's adjoint (a conv), blur, mask
        "h_g_rgb": c + f + a + 2 * D + 3 * E,     # ... then the ToRGB row product
    }
    assert max(out.values()) <= CAP
    return out


# ---- the case table ---------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, node, shape, wirings, geom="c3", scaled=True, bias=True, noise="sample", slope=SLOPE, cots=("gy",),
                 wino=False, env=None, tag=""):
        self.node, self.shape, self.wirings, self.geom, self.scaled = node, shape, wirings, geom, scaled
        self.bias, self.noise, self.slope, self.cots, self.wino, self.env, self.tag = bias, noise, slope, cots, wino, env, tag

    @property
    def id(self):
        parts = [self.node, self.geom if "wt" in NODE_KEYS[self.node] else "", "x".join(str(v) for v in self.shape),
                 "scaled" if self.scaled else "plain", self.tag]
        return "-".join(p for p in parts if p)


def _conv_cases():
    out = []
    for geom in GEOM:                              # stride 2: odd maps only (what the model produces)
        for scaled in (True, False):
            out.append(Case("ConvFn", (2, 8, 8, 9, 9), ("full", "plr" if scaled else "r1"), geom, scaled))
    # each scale and the bias absent on its own
    out.append(Case("ConvFn", (2, 8, 8, 9, 9), ("full",), "c3", "iscale", bias=False, tag="iscale-only"))
    out.append(Case("ConvFn", (2, 8, 8, 9, 9), ("full", "r1"), "c3", "oscale", bias=True, tag="oscale-only"))
    for geom in ("c3", "t3s2"):                    # Winograd / fused up-sampling forward inside the recorded graph
        out.append(Case("ConvFn", (2, 16, 64, 8, 32), ("full", "plr"), geom, True, wino=True))
    for hw, tag in (((64, 64), "gemm"), ((64, 62), "window")):         # test_conv1x1_gemm_threshold_vs_float64
        out.append(Case("ConvFn", (4, 64, 256) + hw, ("full", "r1"), "c1", "oscale", bias=False, tag=tag))
    nba = lambda *a, **k: Case("ConvNBAFn", *a, wino=True, **k)  # noqa: E731
    out += [nba((2, 16, 64, 8, 32), ("full", "plr"), noise="sample"),
            nba((3, 24, 128, 16, 32), ("full", "plr"), noise="shared"),
            nba((1, 128, 64, 8, 32), ("full", "plr"), noise="shared", tag="kslices"),
            nba((2, 16, 64, 8, 32), ("full", "plr"), noise=None, tag="nonoise"),
            nba((2, 16, 64, 8, 32), ("full", "r1"), scaled=False, noise=None, slope=0.0, tag="relu")]
    for env in (None, "0"):
        out.append(Case("UpConvNBAFn", (2, 16, 64, 8, 32), ("full", "plr"), "t3s2", wino=True,
                        env={} if env is None else {"SR_BLUR_BWD_FUSED": env}, tag="two-kernel" if env else ""))
    for shape, noise in (((2, 16, 64, 8, 32), "sample"), ((3, 24, 128, 16, 32), "shared")):
        for cots in (("gy", "g_rgb"), ("g_rgb",), ("gy",)):
            out.append(Case("ConvNBAForkFn", shape, ("full", "plr"), noise=noise, cots=cots, wino=True, tag="+".join(cots)))
    # test_conv1x1_add_fused_equals_the_two_operators_incl_gradients
    out.append(Case("Conv1x1AddFn", (2, 32, 128, 16, 16), ("full", "r1"), "c1", "oscale", bias=False,
                    env={"SR_CONV1X1_GEMM": "force"}))
    for shape, noise in (((2, 6, 6, 8, 8), "sample"), ((3, 5, 5, 16, 12), "shared"), ((2, 5, 5, 33, 33), "sample")):
        for node in ("_NBA", "_BlurNBA", "fused_leaky_relu"):
            out.append(Case(node, shape, ("full",), noise=noise))
    return out


CASES = _conv_cases()
N_RGB = 3


def make(case):
    """The case's tensors, float32 on the CPU, from its own seed: inputs, cotangents, one probe per possible first-order
    result, and the settings.  No mask yet: `m` comes from a forward output (`with_mask`)."""
    b, c, n, h, w = case.shape
    g = torch.Generator().manual_seed(sum(ord(ch) for ch in case.id))
    mk = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    keys = NODE_KEYS[case.node]
    t = {"node": case.node, "slope": case.slope, "gain": GAIN, "x": mk(b, c, h, w)}
    oh, ow = h, w
    if "wt" in keys:
        k, stride, pad, tr = GEOM[case.geom]
        t["geom"] = case.geom
        t["wt"] = mk(k * k, c, n) / (k * c ** 0.5)
        if tr:
            oh, ow = (h - 1) * stride + k - 2 * pad, (w - 1) * stride + k - 2 * pad
        else:
            oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        if case.scaled in (True, "iscale"):
            t["iscale"] = mk(b, c)
        if case.scaled in (True, "oscale"):
            t["oscale"] = mk(b, n).abs() + 0.5
        t["wsq"] = mk(c, n).abs() / c + 0.01
        t["P_wt"], t["P_iscale"], t["P_oscale"] = mk(k * k, c, n), mk(b, c), mk(b, n)
    if "kernel" in keys:
        k1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
        t["kernel"], t["pad"] = k1[None, :] * k1[:, None] / 64.0 * (4.0 if "wt" in keys else 1.0), (1, 1)
        oh, ow = oh + t["pad"][0] + t["pad"][1] - 3, ow + t["pad"][0] + t["pad"][1] - 3
    if "noise" in keys and case.noise is not None:
        t["noise"], t["noise_w"], t["P_noise_w"] = mk(b if case.noise == "sample" else 1, 1, oh, ow), mk(1), mk(1)
    if "bias" in keys and case.bias:
        t["bias"], t["P_bias"] = mk(n), mk(n)
    if "addend" in keys:
        t["addend"], t["P_addend"], t["const"] = mk(b, n, oh, ow), mk(b, n, oh, ow), ("oscale",)
    if "ws" in keys:
        t["ws"], t["rgb_bias"] = mk(b, N_RGB, n) / n ** 0.5, mk(N_RGB)
        t["P_ws"], t["P_rgb_bias"] = mk(b, N_RGB, n), mk(N_RGB)
        if "g_rgb" in case.cots:
            t["g_rgb"] = mk(b, N_RGB, oh, ow)
    if "gy" in case.cots:
        t["gy"] = mk(b, n, oh, ow)
    t["P_x"] = mk(b, c, h, w)
    return t


def with_mask(t, y):
    """`t` with the mask taken from the forward output y (nodes without an activation: unchanged)."""
    return dict(t, m=mask_of(y, t["slope"], t["gain"])) if "m" in NODE_KEYS[t["node"]] else t


def pre_activation(t, absolute=False, dtype=torch.float64, wiring="full"):
    """The pre-activation v (or, absolute, its sum of absolute terms) of the node's twin: the mask set to one (wiring
    "plr": with the linked demodulation scale, as `evaluate` builds it)."""
    tt = {k: ((v.abs() if absolute else v).to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
          for k, v in dict(t, m=torch.ones(())).items()}
    if wiring == "plr":
        tt["oscale"] = demod_link(tt["iscale"], tt["wsq"])
    with torch.no_grad():
        return TWINS[t["node"]](tt)["y"].double()


# ---- mirrors of op.conv.ConvFn / WgradFn, one rule breakable at a time ----------------------------------------------------
MUTATIONS = (
    "dx_scale",              # a wrong scale factor on the data-gradient path only
    "noflip",                # un-flipped taps in the adjoint of c3
    "wgrad_no_oscale",       # the oscale factor missing from WgradFn.backward's cotangent gradient
    "y0_bias",               # the bias included in y0 of the demodulation gradient
    "mask_recomputed",       # the mask from a recomputed pre-activation instead of the given output (compose)
)


def _adjoint_weight(wt, geom):
    wt = wt.flip(0) if geom == "c3" else wt
    return wt.transpose(1, 2)


def _data_grad(g, wt, oscale, geom, mut, like):
    """dxu = adjoint convolution of oscale * g — op.conv._input_grads."""
    flip_geom = "c1" if (geom == "c3" and mut == "noflip") else geom          # "c1": channels swapped, taps kept
    if geom == "c1s2":
        inner = MirrorConv.apply(g, _adjoint_weight(wt, "c1"), oscale, None, None, "c1", mut)
        dxu = torch.zeros_like(like)
        dxu[:, :, ::2, ::2] = inner
    else:
        dxu = MirrorConv.apply(g, _adjoint_weight(wt, flip_geom), oscale, None, None, ADJOINT[geom], mut)
    return dxu * 1.1 if mut == "dx_scale" else dxu


class MirrorConv(Function):
    """y = oscale * conv(iscale * x, wt) + bias with the backward of op.conv.ConvFn."""

    @staticmethod
    def forward(ctx, x, wt, iscale, oscale, bias, geom, mut):
        ctx.save_for_backward(x, wt, iscale, oscale, bias)
        ctx.geom, ctx.mut = geom, mut
        y = conv(x * _bc(iscale) if iscale is not None else x, wt, geom)
        y = y * _bc(oscale) if oscale is not None else y
        return y + bias[None, :, None, None] if bias is not None else y

    @staticmethod
    def backward(ctx, g):
        x, wt, iscale, oscale, bias = ctx.saved_tensors
        geom, mut = ctx.geom, ctx.mut
        need = ctx.needs_input_grad
        gx = gw = gis = gos = gb = None
        if need[0] or need[2]:
            dxu = _data_grad(g, wt, oscale, geom, mut, x)
            gx = dxu * _bc(iscale) if iscale is not None else dxu
            gis = (x * dxu).sum((2, 3)) if need[2] else None
        if need[1]:
            gw = MirrorWgrad.apply(x, g, iscale, oscale, geom, mut)
        if need[3]:
            out = MirrorConv.apply(x, wt, iscale, oscale, bias, geom, mut)
            y0 = out - bias[None, :, None, None] if (bias is not None and mut != "y0_bias") else out
            gos = (g * y0).sum((2, 3)) / oscale
        if need[4]:
            gb = g.sum((0, 2, 3))
        return gx, gw, gis, gos, gb, None, None


class MirrorWgrad(Function):
    """dW = sum_b corr(iscale * x, oscale * g) with the backward of op.conv.WgradFn."""

    @staticmethod
    def forward(ctx, x, g, iscale, oscale, geom, mut):
        ctx.save_for_backward(x, g, iscale, oscale)
        ctx.geom, ctx.mut = geom, mut
        k = GEOM[geom][0]
        xs = x * _bc(iscale) if iscale is not None else x
        go = g * _bc(oscale) if oscale is not None else g
        with torch.enable_grad():
            w0 = torch.zeros(k * k, x.shape[1], g.shape[1], dtype=x.dtype, requires_grad=True)
            (dw,) = torch.autograd.grad(conv(xs.detach(), w0, geom), w0, go.detach())
        return dw

    @staticmethod
    def backward(ctx, gg):
        x, g, iscale, oscale = ctx.saved_tensors
        geom, mut = ctx.geom, ctx.mut
        need = ctx.needs_input_grad
        gx = g_g = gis = gos = None
        if need[0] or need[2]:
            dxu = _data_grad(g, gg, oscale, geom, mut, x)
            gx = dxu * _bc(iscale) if iscale is not None else dxu
            gis = (x * dxu).sum((2, 3)) if need[2] else None
        if need[1] or need[3]:
            dgu = MirrorConv.apply(x, gg, iscale, None, None, geom, mut)
            gos = (g * dgu).sum((2, 3)) if need[3] else None
            g_g = dgu * _bc(oscale) if (oscale is not None and mut != "wgrad_no_oscale") else dgu
        return gx, g_g, gis, gos, None, None
