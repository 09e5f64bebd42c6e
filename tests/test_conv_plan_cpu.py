"""CPU: the dispatch plan of the dense convolutions (csrc/conv_dispatch.hip, csrc/conv_wgrad_dispatch.hip) through its
host-only queries — no GPU is touched.

  * scratch sizes and the Winograd query equal, row for row and under every switch, what the selection code they
    replaced answered (tests/golden/conv_plan_parent.json, recorded by tests/make_golden_conv_plan.py);
  * the weight-gradient path and what it needs equal, row for row, under every switch and with either buffer
    misaligned, what the parent's selection answered (tests/golden/wgrad_plan_parent.json, recorded by
    tests/make_golden_wgrad_plan.py);
  * sr_conv2d_path / sr_conv2d_wgrad_path say what the written rules say, one shape on each side of every threshold;
  * the scratch a chosen path needs never exceeds the size the caller was told to allocate.
"""
import json

import pytest

import make_golden_conv_plan as G
import make_golden_wgrad_plan as W
from conv_plan_cases import FORWARD, MISALIGNED, SWITCHES, WGRAD, case_id, conv_args
from stylerenderer_amd import _lib


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        doc = json.load(f)
    assert doc["rows"] == len(G.shapes()) == len(doc["unset"])
    assert sorted(doc["settings"]) == sorted(G.setting_key(n, v) for n, v in G.SETTINGS)
    return doc


@pytest.fixture(scope="module")
def wgrad_golden():
    with open(W.OUT) as f:
        doc = json.load(f)
    assert doc["rows"] == len(G.shapes()) == len(doc["unset"])
    assert sorted(doc["settings"]) == sorted(G.setting_key(n, v) for n, v in W.SETTINGS)
    return doc


@pytest.fixture
def clean_env(monkeypatch):
    for name in sorted(set(SWITCHES) | {name for name, _ in W.SETTINGS}):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def _mismatches(got, want, rows):
    return [(rows[j], got[j], want[j]) for j in range(len(rows)) if got[j] != want[j]]


def test_sizes_and_winograd_query_match_parent_unset(golden, clean_env):
    rows = G.shapes()
    bad = _mismatches(G.query(_lib.lib(), rows), golden["unset"], rows)
    assert not bad, "%d rows differ, first: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("setting", G.SETTINGS, ids=lambda s: G.setting_key(*s))
def test_sizes_and_winograd_query_match_parent_under_switch(golden, clean_env, setting):
    rows = G.shapes()
    want = list(golden["unset"])
    for j, v in golden["settings"][G.setting_key(*setting)].items():
        want[int(j)] = v
    clean_env.setenv(*setting)
    bad = _mismatches(G.query(_lib.lib(), rows), want, rows)
    assert not bad, "%d rows differ, first: %s" % (len(bad), bad[:3])


@pytest.mark.parametrize("setting", (None,) + W.SETTINGS, ids=lambda s: "unset" if s is None else G.setting_key(*s))
def test_wgrad_path_and_floats_match_parent(wgrad_golden, clean_env, setting):
    """Every row of the sweep, asked with (x, gy) = (NULL, NULL), (misaligned, NULL), (NULL, misaligned): the path
    taken and the floats it needs are the parent's."""
    rows = G.shapes()
    want = list(wgrad_golden["unset"])
    if setting is not None:
        for j, v in wgrad_golden["settings"][G.setting_key(*setting)].items():
            want[int(j)] = v
        clean_env.setenv(*setting)
    bad = _mismatches(W.query(_lib.lib(), rows), want, rows)
    assert not bad, "%d rows differ, first: %s" % (len(bad), bad[:3])


# ---- the path queries against the written rules (conv_plan_cases.py) --------------------------------------------------
@pytest.mark.parametrize("row", FORWARD, ids=case_id)
def test_forward_path_follows_the_rules(row, clean_env):
    geom, shape, env, in_ptr, have, path, _ = row
    for kv in env.items():
        clean_env.setenv(*kv)
    got = _lib.lib().sr_conv2d_path(*conv_args(geom, shape), in_ptr, None, None, 0, have)
    assert got == path


def test_forward_path_misaligned_weights_and_invalid_geometry(clean_env):
    L = _lib.lib()
    args = conv_args("c1", (8, 512, 512, 32, 32))
    assert L.sr_conv2d_path(*args, None, None, None, 512, 1) == _lib.CONV_PATH_GEMM1X1
    assert L.sr_conv2d_path(*args, None, None, MISALIGNED, 512, 1) == _lib.CONV_PATH_DIRECT      # 16-byte aligned operands
    assert L.sr_conv2d_path(*args, None, MISALIGNED, None, 512, 1) == _lib.CONV_PATH_DIRECT
    assert L.sr_conv2d_path(1, 8, 8, 16, 16, 16, 16, 5, 1, 2, 0, None, None, None, 0, 1) == -1   # 5x5
    assert L.sr_conv2d_path(1, 8, 8, 16, 16, 32, 32, 3, 2, 0, 1, None, None, None, 0, 1) == -1   # OH != 2 IH + 1
    assert L.sr_conv2d_path_floats(1, 8, 8, 16, 16, 32, 32, 3, 2, 0, 1, None, None, None, 0, 1) == -1


@pytest.mark.parametrize("row", WGRAD, ids=case_id)
def test_wgrad_path_follows_the_rules(row, clean_env):
    geom, shape, env, x_ptr, path, _ = row
    for kv in env.items():
        clean_env.setenv(*kv)
    assert _lib.lib().sr_conv2d_wgrad_path(*conv_args(geom, shape), x_ptr, None) == path


def test_wgrad_path_invalid_geometry(clean_env):
    assert _lib.lib().sr_conv2d_wgrad_path(1, 8, 8, 16, 16, 16, 16, 5, 1, 2, 0, None, None) == -1


@pytest.mark.parametrize("setting", (None,) + G.SETTINGS, ids=lambda s: "unset" if s is None else G.setting_key(*s))
def test_chosen_path_fits_the_sized_scratch(golden, clean_env, setting):
    """What the in-launch re-checks against the scratch size used to guard: for every shape of the sweep the path taken
    with aligned buffers and the sized scratch needs no more than sr_conv2d_scratch_floats said (the recorded figure)."""
    sized = [v[0] for v in golden["unset"]]
    if setting is not None:
        for j, v in golden["settings"][G.setting_key(*setting)].items():
            sized[int(j)] = v[0]
        clean_env.setenv(*setting)
    L = _lib.lib()
    rows = G.shapes()
    bad = [(r, need, s) for r, s in zip(rows, sized)
           for need in [L.sr_conv2d_path_floats(*r[1:], None, None, None, 0, 1)] if not 0 <= need <= s]
    assert not bad, "%d rows, first: %s" % (len(bad), bad[:3])
