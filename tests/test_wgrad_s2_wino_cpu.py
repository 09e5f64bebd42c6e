"""CPU: the polyphase stride-2 3x3 weight gradient (csrc/conv_wgrad_s2_wino.hip) — its algebra in numpy, its place in
the weight-gradient dispatch plan (host-only queries), and the scratch the chosen path needs against the size callers
allocate (tests/golden/conv_plan_parent.json)."""
import json

import numpy as np
import pytest

import make_golden_conv_plan as G
from conv_plan_cases import MISALIGNED, SWITCHES, conv_args
from stylerenderer_amd import _lib as P

BAR = 2e-6
SWITCH = "SR_WGRAD_S2_WINO"


@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCHES + [SWITCH]:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


# ---- the algebra ------------------------------------------------------------------------------------------------------
SLOT = (0, 1, 2, 1, 3)            # product -> accumulator, per dimension
VSEL = (0, 0, 1, 1, 2)            # product -> v^ = (v0, v1, v0 + v1), per dimension
S = ((0, 3), (1,), (2, 3))        # tap -> accumulators summed, per dimension


@pytest.mark.parametrize("k", [8, 128])
def test_polyphase_weight_gradient_algebra_in_numpy(k):
    """25 products into 16 accumulators over K tiles in float32, in tile order, and the 16 -> 9 combination, against a
    float64 direct sum.  Bar: that of the kernels, 2e-6 of the sum of absolute products (a float32 chain of 4 K terms
    plus the three adds of the combination is far inside it for these K)."""
    rng = np.random.default_rng(k)
    cu, cv = 3, 5
    tw = 4
    th = k // tw
    u = rng.standard_normal((cu, 4 * th + 1, 4 * tw + 1)).astype(np.float32)
    v = rng.standard_normal((cv, 2 * th, 2 * tw)).astype(np.float32)
    want = np.zeros((3, 3, cu, cv))
    mag = np.zeros_like(want)
    for ky in range(3):
        for kx in range(3):
            win = u[:, ky:ky + 4 * th:2, kx:kx + 4 * tw:2].astype(np.float64)
            want[ky, kx] = np.einsum("uyx,vyx->uv", win, v.astype(np.float64))
            mag[ky, kx] = np.einsum("uyx,vyx->uv", np.abs(win), np.abs(v).astype(np.float64))

    def xform_u(s):                                                   # five samples along axis 0
        return np.stack([s[0] - s[2], s[1], s[4] - s[2], s[3], s[2]])

    acc = np.zeros((4, 4, cu, cv), np.float32)
    nprod = 0
    for ty in range(th):
        for tx in range(tw):
            d = u[:, 4 * ty:4 * ty + 5, 4 * tx:4 * tx + 5]            # [cu, 5, 5]
            uh = xform_u(np.moveaxis(d, 1, 0))                        # [i, cu, 5]
            uh = xform_u(np.moveaxis(uh, 2, 0))                       # [j, i, cu]
            uh = np.swapaxes(uh, 0, 1).astype(np.float32)             # [i, j, cu]
            t = v[:, 2 * ty:2 * ty + 2, 2 * tx:2 * tx + 2]            # [cv, 2, 2]
            rows = np.stack([t[:, 0], t[:, 1], t[:, 0] + t[:, 1]])    # [y^, cv, 2]
            vh = np.stack([rows[:, :, 0], rows[:, :, 1], rows[:, :, 0] + rows[:, :, 1]], 1).astype(np.float32)   # [y^, x^, cv]
            for i in range(5):
                for j in range(5):
                    a, b = SLOT[i], SLOT[j]
                    acc[a, b] = acc[a, b] + uh[i, j][:, None] * vh[VSEL[i], VSEL[j]][None, :]
                    nprod += 1
    assert nprod == 25 * k
    got = np.zeros((3, 3, cu, cv), np.float32)
    for ky in range(3):
        for kx in range(3):
            parts = [sum((acc[a, b] for b in S[kx][1:]), acc[a, S[kx][0]]) for a in S[ky]]
            got[ky, kx] = parts[0] if len(parts) == 1 else parts[0] + parts[1]
    err = float((np.abs(got.astype(np.float64) - want) / mag).max())
    print("polyphase wgrad algebra K=%d tiles: error %.3e of the absolute-product sum" % (k, err))
    assert err < BAR


# ---- the plan ---------------------------------------------------------------------------------------------------------
# 3x3 stride 2 pad 0, either direction (G = the smaller map, U channels = C | N transposed, V channels the other):
# k_wgrad_s2p iff GW % 16 == 0, GH % 4 == 0, U channels % 32 == 0, V channels % 128 == 0 and
# work = 18 B CU CV GH GW >= 6.0e9 (SR_WGRAD_S2_WINO=force: any work, =0: never); behind the opt-in split-bf16 path, in
# front of k_wgrad_s2_dma.  No alignment rule: the 16-byte LDS-DMA takes 4-byte aligned rows.
ROWS = [
    ("t3s2", (3, 512, 256, 32, 32), {}, None, P.WGRAD_PATH_S2_WINO),                    # 7.25e9
    ("t3s2", (2, 512, 256, 32, 32), {}, None, P.WGRAD_PATH_S2_DMA),                     # 4.83e9
    ("t3s2", (4, 512, 512, 16, 16), {}, None, P.WGRAD_PATH_S2_DMA),                     # 4.83e9: the 16^2 layer at batch 4
    ("t3s2", (5, 512, 512, 16, 16), {}, None, P.WGRAD_PATH_S2_WINO),                    # 6.04e9
    ("c3s2", (8, 128, 256, 257, 257), {}, None, P.WGRAD_PATH_S2_WINO),                  # the discriminator's 257^2 -> 128^2
    ("c3s2", (3, 64, 256, 129, 129), {}, None, P.WGRAD_PATH_S2_DMA),                    # 3.62e9: stays bit for bit
    ("t3s2", (16, 512, 512, 16, 16), {}, None, P.WGRAD_PATH_S2_WINO),                   # the headline's smallest: 1.93e10
    ("t3s2", (2, 512, 256, 32, 32), {SWITCH: "force"}, None, P.WGRAD_PATH_S2_WINO),
    ("t3s2", (2, 128, 32, 16, 16), {SWITCH: "force"}, None, P.WGRAD_PATH_S2_WINO),
    ("t3s2", (5, 512, 256, 32, 32), {SWITCH: "0"}, None, P.WGRAD_PATH_S2_DMA),
    ("t3s2", (5, 512, 256, 32, 32), {}, MISALIGNED, P.WGRAD_PATH_S2_WINO),              # no alignment rule
    ("t3s2", (5, 512, 256, 32, 32), {"SR_WGRAD_DMA": "0"}, None, P.WGRAD_PATH_S2_WINO),  # that switch is k_wgrad_s2_dma's
    # each eligibility rule, under force: today's path
    ("t3s2", (2, 128, 32, 16, 24), {SWITCH: "force"}, None, P.WGRAD_PATH_DIRECT),       # GW % 16 = 8
    ("t3s2", (2, 128, 32, 6, 16), {SWITCH: "force"}, None, P.WGRAD_PATH_DIRECT),        # GH % 4 = 2
    ("t3s2", (2, 128, 48, 16, 16), {SWITCH: "force"}, None, P.WGRAD_PATH_DIRECT),       # U channels % 32 = 16
    ("t3s2", (2, 64, 32, 16, 16), {SWITCH: "force"}, None, P.WGRAD_PATH_DIRECT),        # V channels % 128 = 64
    ("c3", (2, 32, 128, 16, 16), {SWITCH: "force", "SR_WINOGRAD": "0"}, None, P.WGRAD_PATH_DIRECT),   # stride 1
    # split-bf16 opt-in still first
    ("t3s2", (5, 512, 256, 32, 32), {"SR_CONV_SPLIT_BF16": "1"}, None, P.WGRAD_PATH_BF16_S2),
    ("t3s2", (5, 512, 256, 32, 32), {"SR_CONV_SPLIT_BF16": "1", SWITCH: "force"}, None, P.WGRAD_PATH_BF16_S2),
]


def _row_id(row):
    return "%s-B%d-C%d-N%d-%dx%d-%s" % ((row[0],) + row[1] + ("-".join("%s=%s" % kv for kv in row[2].items()) or "unset",))


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_wgrad_path_follows_the_rules(row, clean_env):
    geom, shape, env, x_ptr, path = row
    for kv in env.items():
        clean_env.setenv(*kv)
    assert P.lib().sr_conv2d_wgrad_path(*conv_args(geom, shape), x_ptr, None) == path


def test_pad_1_is_ineligible_under_force(clean_env):
    clean_env.setenv(SWITCH, "force")
    L = P.lib()
    assert L.sr_conv2d_wgrad_path(2, 32, 128, 32, 32, 16, 16, 3, 2, 1, 0, None, None) == P.WGRAD_PATH_DIRECT
    assert L.sr_conv2d_wgrad_path(2, 32, 128, 33, 33, 16, 16, 3, 2, 0, 0, None, None) == P.WGRAD_PATH_S2_WINO


def test_path_floats_invalid_geometry(clean_env):
    assert P.lib().sr_conv2d_wgrad_path_floats(1, 8, 8, 16, 16, 16, 16, 5, 1, 2, 0, None, None) == -1


@pytest.mark.parametrize("switch", [None, "force"], ids=["unset", "force"])
def test_chosen_wgrad_path_fits_the_sized_scratch(clean_env, switch):
    """For every weight-gradient shape of the sweep, the path taken with aligned buffers writes no more than
    sr_conv2d_wgrad_scratch_floats said (the recorded figure): one 16-position slab per slice against two of 9."""
    with open(G.OUT) as f:
        doc = json.load(f)
    rows = G.shapes()
    sized = [v[1] for v in doc["unset"]]
    assert len(sized) == len(rows)
    if switch is not None:
        clean_env.setenv(SWITCH, switch)
    L = P.lib()
    bad, taken = [], 0
    for r, s in zip(rows, sized):
        if s < 0:
            continue                                         # not a weight-gradient geometry
        need = L.sr_conv2d_wgrad_path_floats(*r[1:], None, None)
        taken += L.sr_conv2d_wgrad_path(*r[1:], None, None) == P.WGRAD_PATH_S2_WINO
        assert L.sr_conv2d_wgrad_scratch_floats(*r[1:]) == s
        if not 0 <= need <= s:
            bad.append((r, need, s))
    assert not bad, "%d rows, first: %s" % (len(bad), bad[:3])
    assert taken > 0
