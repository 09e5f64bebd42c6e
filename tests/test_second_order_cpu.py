"""The float64 twins of tests/second_order_cases.py are right, their `mag` dominates, float32 alone stays under the bars,
and the comparator rejects every mutated rule — all on the CPU, for every case the GPU file runs."""
import pytest
import torch

import second_order_cases as soc
from second_order_cases import CASES, MUTATIONS, TWINS, bars, compare, evaluate, make, pre_activation, with_mask

_CACHE = {}


def _reference(case, wiring):
    """(tensors with the mask of the float32 CPU forward, want, mag), computed once per (case, wiring)."""
    key = (case.id, wiring)
    if key not in _CACHE:
        t = make(case)
        t = with_mask(t, pre_activation(t, dtype=torch.float32, wiring=wiring))
        fn = TWINS[case.node]
        _CACHE[key] = (t, evaluate(fn, t, wiring=wiring), evaluate(fn, t, absolute=True, wiring=wiring))
    return _CACHE[key]


PAIRS = [(c, w) for c in CASES for w in c.wirings]
IDS = ["%s-%s" % (c.id, w) for c, w in PAIRS]


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case,wiring", PAIRS, ids=IDS)
def test_mag_dominates_and_float32_twin_is_within_the_bars(case, wiring, capsys):
    t, want, mag = _reference(case, wiring)
    for k in want:
        assert bool((mag[k] >= want[k].abs()).all()), k                 # a cancelled element cannot pass by a loose bar
    got = evaluate(TWINS[case.node], t, dtype=torch.float32, wiring=wiring)
    ratios = compare(got, want, mag, bars(t, case.wino))
    with capsys.disabled():
        print("\nf32 %s-%s " % (case.id, wiring) + " ".join("%s=%.1e" % kv for kv in sorted(ratios.items())))


def _tiny(node, geom="c3"):
    """B = 1, C, N <= 3, 5x5, float64, a fixed mask."""
    g = torch.Generator().manual_seed(len(node) + len(geom))
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    keys = soc.NODE_KEYS[node]
    k = soc.GEOM[geom][0]
    c, n = (2, 3) if "wt" in keys else (3, 3)
    t = {"node": node, "geom": geom, "slope": 0.2, "gain": soc.GAIN, "pad": (1, 1), "x": mk(1, c, 5, 5),
         "wt": mk(k * k, c, n), "iscale": mk(1, c), "oscale": mk(1, n).abs() + 0.5, "noise_w": mk(1), "bias": mk(n),
         "ws": mk(1, 2, n), "rgb_bias": mk(2)}
    t = {key: v for key, v in t.items() if key in keys + soc._SETTINGS}
    if "kernel" in keys:
        t["kernel"] = mk(4, 4).abs()
    y = TWINS[node](dict(t, noise=None, addend=None, m=None))["y"]
    if "noise" in keys:
        t["noise"] = mk(1, 1, *y.shape[2:])
    if "addend" in keys:
        t["addend"] = mk(*y.shape)
    if "m" in keys:
        t["m"] = soc.mask_of(mk(*y.shape), 0.2, soc.GAIN)
    return t


TINY = [("ConvFn", g) for g in soc.GEOM] + [(n, "t3s2" if n == "UpConvNBAFn" else "c1" if n == "Conv1x1AddFn" else "c3")
                                            for n in soc.NODE_KEYS if n != "ConvFn"]


@pytest.mark.parametrize("node,geom", TINY, ids=["%s-%s" % p for p in TINY])
def test_twin_gradgradcheck(node, geom):
    t = _tiny(node, geom)
    names = [k for k in soc.DIFF if k in t]
    leaves = [t[k].clone().requires_grad_(True) for k in names]

    def f(*vals):
        out = TWINS[node](dict(t, **dict(zip(names, vals))))
        return tuple(out.values())

    assert torch.autograd.gradcheck(f, leaves)
    assert torch.autograd.gradgradcheck(f, leaves)


# ---- mutations ---------------------------------------------------------------------------------------------------------------
# (mutation, case id, wiring, second-order results the broken rule touches: each must be rejected)
MUTATED = [
    ("dx_scale", "ConvNBAFn-c3-2x16x64x8x32-scaled", "full", ("h_wt", "h_gy", "h_oscale", "h_iscale")),
    ("dx_scale", "ConvFn-c3s2-2x8x8x9x9-scaled", "full", ("h_wt", "h_gy")),
    ("noflip", "ConvFn-c3-2x8x8x9x9-scaled", "full", ("h_wt", "h_x", "h_iscale")),   # (h_gy: two wrong adjoints cancel)
    ("noflip", "ConvFn-c3-2x8x8x9x9-plain", "r1", ("h_wt",)),
    ("wgrad_no_oscale", "ConvFn-c3-2x8x8x9x9-scaled", "full", ("h_gy",)),
    ("wgrad_no_oscale", "ConvFn-t3s2-2x8x8x9x9-scaled", "full", ("h_gy",)),
    ("y0_bias", "ConvFn-c3-2x8x8x9x9-scaled", "full", ("h_gy", "h_bias")),
    ("y0_bias", "ConvFn-c1s2-2x8x8x9x9-scaled", "plr", ("h_wsq", "h_bias")),
]
_BY_ID = {c.id: c for c in CASES}


@pytest.mark.parametrize("node,geom", [("ConvFn", g) for g in soc.GEOM] + [("ConvNBAFn", "c3"), ("UpConvNBAFn", "t3s2")])
def test_unbroken_mirror_equals_the_twin(node, geom):
    """The restated ConvFn / WgradFn recursion with no rule broken gives the twin's results (all orders): what a
    mutation changes is the mutation."""
    case = next(c for c in CASES if c.node == node and c.geom == geom and c.scaled is True)
    for wiring in case.wirings:
        t, want, mag = _reference(case, wiring)
        got = evaluate(soc.twin(node, "none"), t, wiring=wiring)
        compare(got, want, mag, {k: 1e-12 for k in want})


@pytest.mark.parametrize("mut,cid,wiring,touched", MUTATED, ids=["%s-%s-%s" % m[:3] for m in MUTATED])
def test_comparator_rejects_mutated_rules(mut, cid, wiring, touched):
    assert mut in MUTATIONS
    case = _BY_ID[cid]
    t, want, mag = _reference(case, wiring)
    got = evaluate(soc.twin(case.node, mut), t, wiring=wiring)
    bar = bars(t, case.wino)
    for k in touched:
        ratio = float(((got[k] - want[k]).abs() / (mag[k] + 1e-30)).max())
        assert ratio > 10 * bar[k], "%s not visible in %s: %.2e of mag (bar %.1e)" % (mut, k, ratio, bar[k])
    with pytest.raises(AssertionError):
        compare(got, want, mag, bar)


@pytest.mark.parametrize("cid", ["ConvNBAFn-c3-2x16x64x8x32-scaled", "_NBA-3x5x5x16x12-scaled"])
def test_comparator_rejects_a_mask_from_a_recomputed_pre_activation(cid):
    """The device's forward output decides the mask of every order.  A few elements next to the kink are given the other
    sign in the `given` output (a float32 forward may land there); a backward that recomputes the pre-activation — here
    in float64 — takes the other slope at exactly those elements."""
    case = _BY_ID[cid]
    t = make(case)
    v = pre_activation(t)
    y = v.clone()
    idx = v.abs().flatten().argsort()[:5]                                  # the five elements closest to the kink
    y.view(-1)[idx] = -v.view(-1)[idx]
    t = with_mask(t, y)
    want, mag = evaluate(TWINS[case.node], t), evaluate(TWINS[case.node], t, absolute=True)
    got = evaluate(soc.twin(case.node, "mask_recomputed"), t)
    bar = bars(t, case.wino)
    for k in ("g_x", "h_gy"):
        assert float(((got[k] - want[k]).abs() / (mag[k] + 1e-30)).max()) > 10 * bar[k], k
    with pytest.raises(AssertionError):
        compare(got, want, mag, bar)
    # and with the given mask the same evaluation passes
    compare(evaluate(TWINS[case.node], t, dtype=torch.float32), want, mag, bar)
