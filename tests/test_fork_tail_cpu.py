"""sr_fork_nba_bwd and its scratch query reject bad arguments on the host, before anything is launched: no pointer below
is ever dereferenced (they are made-up addresses), and every call must come back with SR_EINVAL."""
import pytest

from stylerenderer_amd import _lib

SR_EINVAL = -1          # include/stylerenderer_amd.h
A = 0x10000000          # a made-up, 16-byte aligned address; + 0x100000 per argument

# gpre gbias gnoise_w rowdot dws gb_rgb g_above y g_rgb ws noise noise_w bias
PTRS = ["gpre", "gbias", "gnoise_w", "rowdot", "dws", "gb_rgb", "g_above", "y", "g_rgb", "ws", "noise", "noise_w", "bias"]


def _args(**over):
    a = {name: A + i * 0x100000 for i, name in enumerate(PTRS)}
    a.update(alpha=0.2, scale=2 ** 0.5, B=2, C=64, N=3, hw=256, nstride=256, scratch=A + 0x4000000, stream=None)
    a.update(over)
    return [a[n] for n in PTRS] + [a["alpha"], a["scale"], a["B"], a["C"], a["N"], a["hw"], a["nstride"], a["scratch"],
                                   a["stream"]]


def _rc(**over):
    return _lib.lib().sr_fork_nba_bwd(*_args(**over))


def test_einval_is_the_code_under_test():
    assert _lib.lib().sr_error_string(SR_EINVAL) is not None
    # a call the host checks reject for one reason only, as every case below
    assert _rc(gpre=None) == SR_EINVAL


@pytest.mark.parametrize("name", ["gpre", "rowdot", "dws", "y", "g_rgb", "ws", "scratch"])
def test_null_pointer_of_a_required_argument(name):
    assert _rc(**{name: None}) == SR_EINVAL


def test_noise_without_its_strength():
    assert _rc(noise_w=None) == SR_EINVAL


@pytest.mark.parametrize("name", ["gpre", "g_above", "y", "g_rgb", "noise"])
@pytest.mark.parametrize("skew", [4, 8])
def test_misaligned_vector_buffer(name, skew):
    assert _rc(**{name: A + PTRS.index(name) * 0x100000 + skew}) == SR_EINVAL


@pytest.mark.parametrize("over", [
    dict(B=1024, C=64),                   # B * C = 65536
    dict(B=16, C=4100),                   # B * C > 65535 and C > 4096
    dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(hw=0), dict(hw=-256),
    dict(C=66),                           # not a multiple of the four rows a workgroup takes
    dict(hw=258),                         # rows that are no whole float4
    dict(N=0), dict(N=5),
    dict(nstride=255),
    dict(alpha=0.0), dict(scale=0.0),
    dict(g_above=A),                      # the cotangent from above as the output
], ids=lambda o: ",".join("%s=%s" % kv for kv in o.items()))
def test_rejected_geometry(over):
    assert _rc(**over) == SR_EINVAL


@pytest.mark.parametrize("bad", [(0, 64, 3, 256), (2, 0, 3, 256), (2, 64, 0, 256), (2, 64, 3, 0), (-1, 64, 3, 256),
                                 (2, 64, 3, -4)])
def test_scratch_query_of_an_empty_or_negative_geometry_is_small_and_positive(bad):
    assert 0 < _lib.lib().sr_fork_nba_bwd_scratch_floats(*bad) <= 4


@pytest.mark.parametrize("b,c,n,hw", [(2, 64, 3, 256), (1, 64, 3, 4608), (3, 128, 3, 512), (16, 64, 3, 65536)])
def test_scratch_query_holds_the_layouts_of_the_entries_it_replaces(b, c, n, hw):
    L = _lib.lib()
    got = L.sr_fork_nba_bwd_scratch_floats(b, c, n, hw)
    nba = L.sr_noise_bias_act_bwd_dot_scratch_floats(b, c, hw)
    dw = L.sr_smallconv_dw_scratch_floats(b, c, n, hw)
    assert nba + dw <= got <= nba + dw + 1          # (+ 1: the second block starts on an even float)
