"""CPU: the host side of the rasterizer (csrc/rasterize.hip, csrc/raster_layout.h) through entries that never touch the
device.

  * sr_rasterize_scratch_bytes / sr_rasterize_grad_scratch_bytes, sr_rasterize_levels_supported (SR_RASTER_TILED unset,
    0 and 1) and the status of every host entry for invalid, out-of-range and empty argument sets equal, row for row,
    what the library answered before rasterize.hip was split and its scratch layouts became structs
    (tests/golden/raster_layout_parent.json, recorded by tests/make_golden_raster_layout.py);
  * the gradient state `big` that op/rasterize.py allocates has the size the layout struct gives
    (sr_rasterize_grad_state_ints).
"""
import json

import pytest

import make_golden_raster_layout as G
from stylerenderer_amd import _lib


@pytest.fixture(scope="module")
def golden():
    with open(G.OUT) as f:
        doc = json.load(f)
    assert len(doc["sizes"]) == len(G.SIZES) and len(doc["status"]) == len(G.STATUS)
    assert sorted(doc["levels"]) == sorted("unset" if v is None else v for v in G.TILED_SETTINGS)
    assert all(len(v) == len(G.LEVELS) for v in doc["levels"].values())
    return doc


@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv("SR_RASTER_TILED", raising=False)
    return monkeypatch


def _mismatches(got, want, rows):
    return [(rows[j], got[j], want[j]) for j in range(len(rows)) if got[j] != want[j]]


def test_scratch_sizes_match_parent(golden, clean_env):
    bad = _mismatches(G.query_sizes(_lib.lib()), golden["sizes"], G.SIZES)
    assert not bad, "%d rows differ, first: %s" % (len(bad), bad[:3])
    # the table is not degenerate: both bounds of the forward scratch occur, and a valid word is crossed
    got = dict(zip(G.SIZES, golden["sizes"]))
    assert got[(2, 1000, 32, 32, 0, 3)][0] > got[(2, 1000, 32, 33, 0, 3)][0] == 2 * 32 * 33 * 8 + 16
    assert got[(1, 65, 16, 16, 0, 3)][1] - got[(1, 64, 16, 16, 0, 3)][1] == 24 * 4 + 12 + 8


@pytest.mark.parametrize("tiled", G.TILED_SETTINGS, ids=lambda v: "unset" if v is None else "tiled=" + v)
def test_levels_supported_matches_parent(golden, clean_env, tiled):
    if tiled is not None:
        clean_env.setenv("SR_RASTER_TILED", tiled)
    want = golden["levels"]["unset" if tiled is None else tiled]
    bad = _mismatches(G.query_levels(_lib.lib()), want, G.LEVELS)
    assert not bad, "%d rows differ, first: %s" % (len(bad), bad[:3])


def test_levels_supported_rows_sit_on_both_sides_of_each_condition(golden):
    """The recorded answers themselves: every pair of neighbouring rows of LEVELS that straddles a condition of tiled_ok
    or of the entry's own range checks answers differently where the table says it should."""
    unset, off, on = (dict(zip([repr(r) for r in G.LEVELS], golden["levels"][k])) for k in ("unset", "0", "1"))
    row = lambda *r: repr(tuple(r))                                                                      # noqa: E731
    assert (unset[row(1, 4095, 100, [32], [32])], unset[row(1, 4096, 100, [32], [32])]) == (1, 0)
    assert (unset[row(1, 1023, 100, [64], [64])], unset[row(1, 1024, 100, [64], [64])]) == (1, 0)
    assert (unset[row(1, 4096, 1024, [32], [32])], unset[row(1, 4096, 1025, [32], [32])]) == (0, 1)
    assert (off[row(1, 65535, 10, [8], [8])], off[row(1, 65536, 10, [8], [8])]) == (1, 0)
    assert (on[row(1, 4096, 100, [32], [33])], on[row(1, 4096, 0, [32], [32])]) == (1, 1)
    assert on[row(1, 4095, 100, [32], [32])] == 0 and off[row(1, 4096, 100, [32], [32])] == 1
    n = G.MAX_LEVELS
    assert (unset[row(n, 4, 100, [16] * n, [16] * n)], unset[row(n + 1, 4, 100, [16] * (n + 1), [16] * (n + 1))]) == (1, 0)
    assert unset[row(0, 4, 100, [32], [32])] == 0
    assert (unset[row(1, 2, 100, [32768], [32768])], unset[row(1, 2, 100, [32768], [32767])]) == (0, 1)


def test_host_entries_status_matches_parent(golden, clean_env):
    got = G.query_status(_lib.lib())
    bad = _mismatches(got, golden["status"], G.STATUS)
    assert not bad, "%d rows differ, first: %s" % (len(bad), bad[:3])
    assert {_lib.lib().sr_error_string(rc) is not None for rc in set(got)} == {True}
    assert len(set(got)) == 3                             # SR_OK, SR_EINVAL and SR_ERANGE all occur


@pytest.mark.parametrize("b,nf", [(1, 1), (2, 105), (3, 21), (4, 49536), (64, 49536), (1, 0)])
def test_python_sizes_the_gradient_state_like_the_layout(b, nf):
    """`big` = [count | b * nf ids | b * nf leader table | state word]: op/rasterize.py allocates it, GradState
    (csrc/raster_layout.h) carves it."""
    import importlib

    R = importlib.import_module("stylerenderer_amd.op.rasterize")
    assert R.grad_state_ints(b, nf) == _lib.lib().sr_rasterize_grad_state_ints(b, nf) == 2 + 2 * b * nf
