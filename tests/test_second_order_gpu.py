"""The fused convolution nodes and the activation tails against their float64 twins (tests/second_order_cases.py):
forward and first order on the fast kernels, first order on the recorded branch, and the complete second order from it.

Per case and wiring the device node runs three times from the same inputs — (a) forward + first order without
create_graph, (b) first order with create_graph, (c) second order from (b) — and every result is measured per element
against `mag`, the twin on absolute values, with the bar `second_order_cases.bars` derives from the chained passes.  The
mask of the twin is the device's own forward output's (`mask_of`), so no element is nudged or excluded; that this
output has the float64 pre-activation's sign wherever that sign is decided beyond round-off is asserted separately."""
import pytest
import torch

import second_order_cases as soc
from second_order_cases import CASES, TWINS, bars, compare, evaluate, make, pre_activation, with_mask
from util import kernel_ran, launched_kernels

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _device_fn(case, seen):
    """The node on device tensors, {"y", ["rgb"]}; asserts the node's own predicate (no silent composite)."""
    from stylerenderer_amd.op import conv as cv
    from stylerenderer_amd.op import fork_tail, fused_elem
    from stylerenderer_amd.op.fused_act import fused_leaky_relu

    node = case.node

    def fn(t):
        g = t.get
        if node == "ConvFn":
            return {"y": cv.conv2d(t["x"], t["wt"], g("iscale"), g("oscale"), g("bias"), t["geom"])}
        if node == "ConvNBAFn":
            assert cv.conv_nba_supported(t["x"], t["wt"], g("noise"))
            return {"y": cv.conv2d_nba(t["x"], t["wt"], g("iscale"), g("oscale"), g("noise"), g("noise_w"), t["bias"],
                                       t["slope"], t["gain"])}
        if node == "UpConvNBAFn":
            assert cv.upconv_nba_supported(t["x"], t["wt"], g("noise"), 2 * t["x"].shape[2], 2 * t["x"].shape[3])
            return {"y": cv.upconv_nba(t["x"], t["wt"], g("iscale"), g("oscale"), t["kernel"], t["pad"], g("noise"),
                                       g("noise_w"), t["bias"], t["slope"], t["gain"])}
        if node == "ConvNBAForkFn":
            assert cv.conv_nba_supported(t["x"], t["wt"], g("noise"))
            assert fork_tail.supported(t["x"], t["wt"].shape[2], t["ws"].shape[1], g("noise"), t["oscale"])
            y, rgb = fork_tail.conv2d_nba_fork(t["x"], t["wt"], g("iscale"), t["oscale"], g("noise"), g("noise_w"),
                                               t["bias"], t["slope"], t["gain"], t["ws"], t["rgb_bias"])
            return {"y": y, "rgb": rgb}
        if node == "Conv1x1AddFn":
            y = cv.conv1x1_add(t["x"], t["wt"], t["oscale"], t["addend"])
            assert type(y.grad_fn).__name__.startswith("Conv1x1AddFn"), y.grad_fn
            return {"y": y}
        if node == "_NBA":
            seen["fusable"] = fused_elem._fusable(t["x"], t["noise"])
            return {"y": fused_elem.noise_bias_act(t["x"], t["noise"], t["noise_w"], t["bias"], t["slope"], t["gain"])}
        if node == "_BlurNBA":
            return {"y": fused_elem.blur_noise_bias_act(t["x"], t["kernel"], t["pad"], t["noise"], t["noise_w"], t["bias"],
                                                        t["slope"], t["gain"])}
        assert node == "fused_leaky_relu"
        return {"y": fused_leaky_relu(t["x"], t["bias"], t["slope"], t["gain"])}

    return fn


def _any(names, *bases):
    return any(kernel_ran(names, b) for b in bases)


def _assert_paths(case, wiring, t, fast, recorded, took, seen):
    """The kernels of the intended path ran: `fast` / `recorded` are the kernel names of run (a) / runs (b) + (c), `took`
    what op.conv counted for the style gradient in run (a)."""
    from stylerenderer_amd.op import wgrad_style

    node, b = case.node, case.shape[0]
    if node == "ConvFn":
        assert _any(fast, "k_conv_mfma", "k_conv_wino", "k_conv1x1_gemm", "k_convt_fused", "k_convt_wino", "k_convt_taps_gemm",
                    "k_conv_s2_wino", "k_conv_s2_bf16x3", "k_convt_bf16x3"), fast
        if case.wino and case.geom == "c3":
            assert kernel_ran(fast, "k_conv_wino") and kernel_ran(recorded, "k_conv_wino"), (fast, recorded)
        if case.tag in ("gemm", "window"):
            assert kernel_ran(fast, "k_conv1x1_gemm") == (case.tag == "gemm"), fast
    if node in ("ConvNBAFn", "ConvNBAForkFn"):
        assert kernel_ran(fast, "k_conv_wino"), fast
        assert kernel_ran(fast, "k_wino_reduce") == (case.tag == "kslices"), fast
    if node == "ConvNBAFn":
        assert kernel_ran(fast, "k_nba_bwd"), fast
        # the recorded branch: the demodulated layer re-derives its VJP (row-dots of op.conv._input_grads / rowdot_div);
        # the plain one records the activation backward itself, whose own backward is the forward kernel on the cotangent
        assert kernel_ran(recorded, "k_rowdot" if case.scaled else "k_nba_bwd"), recorded
        if not case.scaled and wiring == "full":
            assert kernel_ran(recorded, "k_nba_fwd"), recorded
    if node == "UpConvNBAFn":
        assert _any(fast, "k_fir4_band_fwd", "k_fir4_tile"), fast
        one_pass = _any(fast, "k_fir4_band_nba_bwd", "k_fir4_nba_bwd")
        assert one_pass == (not case.env), fast
        assert kernel_ran(fast, "k_nba_bwd") == bool(case.env), fast
        assert kernel_ran(recorded, "k_rowdot"), recorded
    if node == "ConvNBAForkFn":
        assert kernel_ran(fast, "k_smallconv_fwd"), fast
        # one pass for the ToRGB backward and the activation backward iff there is a ToRGB cotangent and its row
        # gradient is wanted (op.fork_tail.ConvNBAForkFn.backward); never on the recorded branch
        assert kernel_ran(fast, "k_fork_nba_bwd") == ("g_rgb" in case.cots and wiring == "full"), fast
        assert not kernel_ran(recorded, "k_fork_nba_bwd") and kernel_ran(recorded, "k_rowdot"), recorded
    if node == "Conv1x1AddFn":
        assert kernel_ran(fast, "k_conv1x1_gemm"), fast
    if node == "_NBA":
        assert seen["fusable"] == ((case.shape[3] * case.shape[4]) % 4 == 0)          # 33 x 33: the two-step path
        assert kernel_ran(fast, "k_nba_fwd") == seen["fusable"] and kernel_ran(fast, "k_nba_bwd") == seen["fusable"], fast
        assert seen["fusable"] or _any(fast, "k_bias_act_scalar", "k_bias_act_vec4"), fast
    if node == "_BlurNBA":
        # one node where the activation backward can read the output as rows of float4, else the two operators
        one_node = ((case.shape[3] - 1) * (case.shape[4] - 1)) % 4 == 0
        assert _any(fast, "k_fir4_band_fwd", "k_fir4_tile", "k_upfirdn_generic"), fast
        assert kernel_ran(fast, "k_nba_bwd") == one_node, fast
        assert one_node or _any(fast, "k_bias_act_scalar", "k_bias_act_vec4"), fast
    if node == "fused_leaky_relu":
        assert _any(fast, "k_bias_act_scalar", "k_bias_act_vec4") and _any(fast, "k_act_bwd_rows", "k_bias_grad_small"), fast
    if "wt" in soc.NODE_KEYS[node] and case.geom in ("c3", "t3s2") and case.scaled is True and wiring == "full":
        # weight and style gradient both wanted: the style gradient comes out of the weight gradient's finish kernel
        # exactly where the plan cuts K into whole slices per sample
        k, stride, pad, tr = soc.GEOM[case.geom]
        h, w = case.shape[3:]
        oh, ow = ((h - 1) * stride + k - 2 * pad, (w - 1) * stride + k - 2 * pad) if tr else (h, w)
        x = torch.empty(case.shape[0], case.shape[1], h, w, device=DEV)
        gy = torch.empty(b, case.shape[2], oh, ow, device=DEV)
        want = "wgrad" if wgrad_style.part_floats(x, gy, k, stride, pad, tr) >= 0 else "rowdot"
        assert took == {"wgrad": int(want == "wgrad"), "rowdot": int(want == "rowdot")}, (took, want)


PAIRS = [(c, w) for c in CASES for w in c.wirings]


@pytest.mark.parametrize("case,wiring", PAIRS, ids=["%s-%s" % (c.id, w) for c, w in PAIRS])
def test_node_vs_float64_twin(case, wiring, monkeypatch, capsys):
    from stylerenderer_amd.op import conv as cv

    for k, v in (case.env or {}).items():
        monkeypatch.setenv(k, v)
    t = make(case)
    seen = {}
    fn = _device_fn(case, seen)
    run = lambda order: evaluate(fn, t, dtype=torch.float32, wiring=wiring, order=order, device=DEV)  # noqa: E731
    before = dict(cv.STYLE_PATH_COUNTS)
    fast, fast_names = launched_kernels(lambda: run(1))                                # (a)
    took = {k: cv.STYLE_PATH_COUNTS[k] - before[k] for k in before}
    rec, rec_names = launched_kernels(lambda: run(2))                                  # (b) + (c)
    _assert_paths(case, wiring, t, fast_names, rec_names, took, seen)
    assert torch.equal(fast["y"], rec["y"])

    tm = with_mask(t, rec["y"])
    want = evaluate(TWINS[case.node], tm, wiring=wiring)
    mag = evaluate(TWINS[case.node], tm, absolute=True, wiring=wiring)
    bar = bars(tm, case.wino)
    if "m" in tm:
        # the forward output has the float64 pre-activation's sign wherever round-off cannot decide it
        v, vmag = pre_activation(tm, wiring=wiring), pre_activation(tm, absolute=True, wiring=wiring)
        decided = v.abs() > bar["y"] * vmag
        assert bool(((rec["y"] > 0) == (v > 0))[decided].all())
    ratios = dict(("fast:" + k, r) for k, r in compare(fast, {k: want[k] for k in fast}, mag, bar).items())
    ratios.update(compare(rec, want, mag, bar))
    # (a) and (b) agree with each other at the first-order bar (each is within it of the same float64 value; their
    # difference is asserted at that bar too, not at twice it)
    first = [k for k in fast if k.startswith("g_")]
    compare({k: fast[k] for k in first}, {k: rec[k] for k in first}, mag, bar)
    with capsys.disabled():
        print("\nmi355x %s-%s " % (case.id, wiring) + " ".join("%s=%.1e" % kv for kv in sorted(ratios.items())))
