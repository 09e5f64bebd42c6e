"""Records the host-side decisions of the rasterizer of a GIVEN library build, for tests/test_raster_layout_cpu.py.

  STYLERENDERER_AMD_LIB=<libstylerenderer_hip.so of the commit to record> python tests/make_golden_raster_layout.py

writes tests/golden/raster_layout_parent.json:

  sizes    [sr_rasterize_scratch_bytes, sr_rasterize_grad_scratch_bytes] for every row of SIZES;
  levels   sr_rasterize_levels_supported for every row of LEVELS with SR_RASTER_TILED unset, "0" and "1";
  status   the return value of a host entry for every row of STATUS: argument sets that are invalid, out of range or
           empty, so that the entry returns before it launches anything (no GPU is needed, no pointer is followed).

The file was recorded with the library of the commit BEFORE csrc/rasterize.hip was split by pass and its scratch
layouts moved into csrc/raster_layout.h: the layout structs and the validation that stayed in rasterize.hip have to
reproduce these values, quirks of order and precedence included (SR_ERANGE before the `b == 0` SR_OK, ...).
"""
import ctypes
import json
import os

from stylerenderer_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "raster_layout_parent.json")
MAX_LEVELS = 12                                          # SR_RASTER_MAX_LEVELS (include/stylerenderer_amd.h)
TILED_SETTINGS = (None, "0", "1")                        # SR_RASTER_TILED

# ---- (b, nf, h, w, is_double, tex_c) ----------------------------------------------------------------------------------
# The forward scratch is the larger of the key buffer (8 or 12 bytes per pixel) and, for square fp32 images, the tile
# lists: 2 049 words per 32 x 32 tile hold at least 2.001 words per pixel, so on EVERY square fp32 size the tile lists
# are the larger — the two sides of "the tiled bound overtakes the key bound" are square against non-square (one pixel
# apart: 32 x 32 / 32 x 33) and fp32 against fp64, not small against large.
SIZES = []
for _sq in (1, 31, 32, 33, 64, 65, 256, 1024):
    SIZES += [(2, 1000, _sq, _sq, 0, 3), (2, 1000, _sq, _sq, 1, 3), (2, 1000, _sq, _sq + 1, 0, 3),
              (2, 1000, _sq + 1, _sq, 0, 3)]
SIZES += [(2, 100, 40, 24, 0, 3), (3, 7, 24, 40, 1, 6), (64, 49536, 256, 256, 0, 3), (4, 49536, 256, 256, 0, 4),
          (1, 49536, 256, 256, 1, 1)]
SIZES += [(0, 0, 0, 0, 0, 1), (0, 10, 8, 8, 0, 3), (-1, 5, 8, 8, 0, 3), (2, -3, 8, 8, 0, 3), (2, 5, -8, 8, 0, 3),
          (2, 5, 0, 8, 0, 3), (2, 5, 8, 0, 1, 3), (2, 5, -8, -8, 0, 3), (2, 0, 8, 8, 0, 3), (-2, -3, 8, 8, 1, 0)]
# b * nf at and around multiples of 64 (one valid word per 64 records)
for _b, _nf in ((1, 63), (1, 64), (1, 65), (1, 127), (1, 128), (1, 129), (2, 32), (3, 21), (3, 43), (5, 64), (7, 9),
                (1, 1), (64, 1)):
    SIZES += [(_b, _nf, 16, 16, 0, 3), (_b, _nf, 16, 16, 1, 6)]
SIZES = tuple(SIZES)

# ---- (n, b, nf, [h], [w]); h / w None = NULL ---------------------------------------------------------------------------
# tiled_ok (csrc/rasterize_tiled.hip): square, nf > 0, b <= 65535, then by size b * ntile >= 4096 and nf <= 1024 * ntile
_PYR = [4, 8, 16, 32, 64, 128, 256]
LEVELS = (
    (1, 4095, 100, [32], [32]), (1, 4096, 100, [32], [32]),              # b * ntile = 4095 / 4096 with one tile
    (1, 1023, 100, [64], [64]), (1, 1024, 100, [64], [64]),              # ... with four
    (1, 4096, 1024, [32], [32]), (1, 4096, 1025, [32], [32]),            # nf = 1024 * ntile and one more
    (1, 1024, 4096, [64], [64]), (1, 1024, 4097, [64], [64]),
    (1, 65535, 10, [8], [8]), (1, 65536, 10, [8], [8]),                  # b = 65535 / 65536
    (1, 4096, 100, [32], [33]), (1, 4096, 100, [33], [32]),              # h != w
    (1, 4096, 0, [32], [32]),                                            # no triangles: never tiled
    (0, 4, 100, [32], [32]), (-1, 4, 100, [32], [32]),                   # n = 0
    (MAX_LEVELS, 4, 100, [16] * MAX_LEVELS, [16] * MAX_LEVELS),
    (MAX_LEVELS + 1, 4, 100, [16] * (MAX_LEVELS + 1), [16] * (MAX_LEVELS + 1)),
    (7, 4, 49536, _PYR, _PYR), (7, 1, 49536, _PYR, _PYR), (7, 64, 49536, _PYR, _PYR),
    (2, 4096, 100, [16, 32], [16, 32]), (2, 4095, 100, [32, 16], [32, 16]),
    (1, 0, 100, [32], [32]), (1, -1, 100, [32], [32]),                   # b <= 0
    (1, 4, 100, None, [32]), (1, 4, 100, [32], None),                    # NULL extents
    (1, 4, 100, [0], [32]), (1, 4, 100, [32], [-1]), (1, 1, 1, [0x80000000], [1]), (1, 1, 1, [1], [0x80000000]),
    (1, 2, 100, [32768], [32768]), (1, 2, 100, [32768], [32767]),        # b * h * w at 2^31 and below
    (1, 1, 100, [46341], [46341]), (1, 1, 100, [46340], [46340]),
)

# ---- (entry, [arguments]) ----------------------------------------------------------------------------------------------
# P stands for "some non-null pointer"; none of these argument sets lets the entry follow it.  A list among the
# arguments becomes an array (of int64 for extents, of pointers otherwise).
P = 64
_BIG_NF = 0x7FFFFFFF // 3


def _fwd(b=1, nv=3, nf=1, h=8, w=8, v=P, tri=P, index=P, coeff=P, zbuf=P, tex=None, tex_c=0, attr=None, win=None, big=None,
         work=P, flags=0):
    return [b, nv, nf, h, w, 0, 1, flags, v, tri, index, coeff, zbuf, 1e-6, tex, tex_c, attr, win, big, work, None]


def _bwd(b=1, n=3, h=2, w=2, v=P, index=P, dcoeff=P):
    return [b, n, h, w, 0, 0, v, index, dcoeff, 1e-6, None]


def _grad(b=1, nv=3, nf=1, h=8, w=8, v=P, tex=P, tex_c=3, tri=P, win=P, big=P, go=P, adj_off=P, adj=P, slot=P, grad_v=P,
          grad_tex=P, work=P, flags=0):
    return [b, nv, nf, h, w, 1, flags, v, tex, tex_c, tri, win, big, go, adj_off, adj, 0, 0, slot, grad_v, grad_tex, 1e-6,
            work, None]


def _fwd_levels(n=1, b=1, nv=3, nf=1, h=(8,), w=(8,), v=P, tri=P, tex=P, tex_c=3, attr=(P,), win=None, big=None, work=(P,)):
    as_list = lambda x: None if x is None else list(x)                                                   # noqa: E731
    return [n, b, nv, nf, as_list(h), as_list(w), 0, 1, 0, v, tri, 1e-6, tex, tex_c, as_list(attr), as_list(win),
            as_list(big), as_list(work), None]


def _grad_levels(n=1, b=1, nv=3, nf=1, h=(8,), w=(8,), v=P, tex=P, tex_c=3, tri=P, win=(P,), big=(P,), go=(P,), adj_off=P,
                 adj=P, slot=P, grad_v=P, grad_tex=P, work=(P,)):
    as_list = lambda x: None if x is None else list(x)                                                   # noqa: E731
    return [n, b, nv, nf, as_list(h), as_list(w), 1, 0, v, tex, tex_c, tri, as_list(win), as_list(big), as_list(go), adj_off,
            adj, 0, 0, slot, grad_v, grad_tex, 1e-6, as_list(work), None]


def _cpu_fwd(b=1, nv=3, nf=1, h=8, w=8, v=P, tri=P, index=P, coeff=P):
    return [b, nv, nf, h, w, 0, 1, 0, v, tri, index, coeff, None, 1e-6]


def _cpu_bwd(b=1, n=3, h=2, w=2, v=P, index=P, dcoeff=P):
    return [b, n, h, w, 0, v, index, dcoeff, 1e-6]


def _status_rows():
    rows = []
    for suf in ("f32", "f64"):
        f, bw, g = "sr_rasterize_forward_" + suf, "sr_rasterize_backward_" + suf, "sr_rasterize_grad_" + suf
        rows += [(f, a) for a in (
            _fwd(b=-1), _fwd(nv=-1), _fwd(nf=-1), _fwd(h=0), _fwd(w=-3), _fwd(b=-1, nf=0xFFFFFFFE),
            _fwd(b=0, nf=0xFFFFFFFE),                                  # out of range comes before the empty batch
            _fwd(b=0, nf=0xFFFFFFFD), _fwd(b=0, nf=0x7FFFFFFF, win=P), _fwd(b=0, nf=0x7FFFFFFF),
            _fwd(b=0, nf=0x7FFFFFFE, win=P), _fwd(b=2, nf=0x40000000, big=P), _fwd(b=2, nf=0x40000000, work=None),
            _fwd(b=0, v=None, tri=None, index=None, coeff=None, zbuf=None, work=None), _fwd(work=None), _fwd(v=None),
            _fwd(tri=None), _fwd(nf=0, v=None, tri=None, work=None), _fwd(attr=P, tex=None, tex_c=3),
            _fwd(attr=P, tex=P, tex_c=0), _fwd(attr=P, tex=P, tex_c=-1), _fwd(h=0, flags=2), _fwd(work=None, flags=3))]
        rows += [(bw, a) for a in (
            _bwd(b=-1), _bwd(n=-1), _bwd(h=-1), _bwd(w=-1), _bwd(b=0, v=None, index=None, dcoeff=None), _bwd(h=0, v=None),
            _bwd(w=0), _bwd(v=None), _bwd(index=None), _bwd(dcoeff=None))]
        rows += [(g, a) for a in (
            _grad(b=-1), _grad(nv=-1), _grad(nf=-1), _grad(h=-1), _grad(w=-1), _grad(tex_c=0), _grad(tex_c=-2, b=0),
            _grad(b=0), _grad(nv=0), _grad(grad_v=None, grad_tex=None), _grad(b=0, nf=_BIG_NF),
            _grad(grad_v=None, grad_tex=None, b=65536), _grad(b=65536), _grad(b=65535, work=None), _grad(nf=_BIG_NF),
            _grad(nf=_BIG_NF - 1, work=None), _grad(tex_c=0x80000000), _grad(tex_c=0x7FFFFFFF, work=None),
            _grad(b=65536, v=None), _grad(v=None), _grad(tex=None), _grad(go=None), _grad(adj_off=None), _grad(work=None),
            _grad(tri=None), _grad(adj=None), _grad(win=None), _grad(big=None),
            _grad(nf=0, tri=None, adj=None, win=None, big=None, h=65536, w=65536),
            _grad(h=46341, w=46341), _grad(b=2, h=32768, w=32768), _grad(h=46341, w=46341, work=None),
            _grad(h=46341, w=46341, flags=6), _grad(slot=None, work=None))]
    rows += [("sr_rasterize_forward_levels_f32", a) for a in (
        _fwd_levels(n=-1), _fwd_levels(b=-1), _fwd_levels(nv=-1), _fwd_levels(nf=-1), _fwd_levels(tex_c=0),
        _fwd_levels(n=0, h=None, w=None, attr=None, work=None), _fwd_levels(b=0, h=None), _fwd_levels(n=0, tex_c=0),
        _fwd_levels(h=None), _fwd_levels(w=None), _fwd_levels(attr=None), _fwd_levels(work=None), _fwd_levels(tex=None),
        _fwd_levels(v=None), _fwd_levels(tri=None), _fwd_levels(nf=0, v=None, tri=None, attr=(None,)),
        _fwd_levels(n=MAX_LEVELS + 1, h=(8,) * 13, w=(8,) * 13, attr=(P,) * 13, work=(P,) * 13),
        _fwd_levels(b=65536), _fwd_levels(h=(0,)), _fwd_levels(b=4096, nf=100, h=(32,), w=(32,)),
        _fwd_levels(attr=(None,)), _fwd_levels(work=(None,)), _fwd_levels(n=2, h=(8, 4), w=(8, 4), attr=(P, None), work=(P, P)),
        _fwd_levels(n=2, h=(8, 4), w=(8, 4), attr=(P, P), work=(P, None)))]
    rows += [("sr_rasterize_grad_levels_f32", a) for a in (
        _grad_levels(n=0), _grad_levels(n=-1), _grad_levels(n=MAX_LEVELS + 1), _grad_levels(b=0), _grad_levels(nv=0),
        _grad_levels(nf=0), _grad_levels(tex_c=0), _grad_levels(tex_c=5), _grad_levels(h=None), _grad_levels(w=None),
        _grad_levels(v=None), _grad_levels(tex=None), _grad_levels(tri=None), _grad_levels(win=None), _grad_levels(big=None),
        _grad_levels(go=None), _grad_levels(adj_off=None), _grad_levels(adj=None), _grad_levels(slot=None),
        _grad_levels(work=None), _grad_levels(grad_v=None, grad_tex=None), _grad_levels(b=65536),
        _grad_levels(b=65536, v=None), _grad_levels(nf=_BIG_NF), _grad_levels(nf=_BIG_NF, tex_c=5), _grad_levels(h=(0,)),
        _grad_levels(w=(-1,)), _grad_levels(win=(None,)), _grad_levels(big=(None,)), _grad_levels(go=(None,)),
        _grad_levels(work=(None,)), _grad_levels(b=2, h=(32768,), w=(32768,)),
        _grad_levels(b=2, h=(32768,), w=(32768,), work=(None,)),
        _grad_levels(n=2, b=2, h=(32768, 0), w=(32768, 8), win=(P, P), big=(P, P), go=(P, P), work=(P, P)))]
    for suf in ("f32", "f64"):
        rows += [("sr_rasterize_forward_cpu_" + suf, a) for a in (
            _cpu_fwd(b=-1), _cpu_fwd(nv=-1), _cpu_fwd(nf=-1), _cpu_fwd(h=0), _cpu_fwd(w=0),
            _cpu_fwd(b=0, v=None, tri=None, index=None, coeff=None), _cpu_fwd(index=None), _cpu_fwd(coeff=None),
            _cpu_fwd(v=None), _cpu_fwd(tri=None))]
        rows += [("sr_rasterize_backward_cpu_" + suf, a) for a in (
            _cpu_bwd(b=-1), _cpu_bwd(n=-1), _cpu_bwd(h=-1), _cpu_bwd(w=-1), _cpu_bwd(b=0, v=None), _cpu_bwd(h=0),
            _cpu_bwd(v=None), _cpu_bwd(index=None), _cpu_bwd(dcoeff=None))]
    return tuple(rows)


STATUS = _status_rows()


def bind(handle, names):
    for name in names:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return handle


def _c_args(name, args):
    """Python lists -> arrays: int64 where the signature's slot precedes the first scalar flag (the extents h / w of the
    levels entries, slots 4 and 5), pointers elsewhere.  The arrays are returned too, so that they outlive the call."""
    out, keep = [], []
    for j, a in enumerate(args):
        if isinstance(a, list):
            kind = ctypes.c_int64 if name.endswith("levels_f32") and j in (4, 5) else ctypes.c_void_p
            a = (kind * len(a))(*a)
            keep.append(a)
        out.append(a)
    return out, keep


def query_sizes(handle):
    return [[handle.sr_rasterize_scratch_bytes(b, nf, h, w, dbl), handle.sr_rasterize_grad_scratch_bytes(b, nf, c, dbl)]
            for b, nf, h, w, dbl, c in SIZES]


def query_levels(handle):
    """Under the CURRENT environment."""
    out = []
    for n, b, nf, h, w in LEVELS:
        hs = None if h is None else (ctypes.c_int64 * len(h))(*h)
        ws = None if w is None else (ctypes.c_int64 * len(w))(*w)
        out.append(handle.sr_rasterize_levels_supported(n, b, nf, hs, ws))
    return out


def query_status(handle):
    out = []
    for name, args in STATUS:
        cargs, keep = _c_args(name, args)
        out.append(getattr(handle, name)(*cargs))
    return out


NAMES = sorted({"sr_rasterize_scratch_bytes", "sr_rasterize_grad_scratch_bytes", "sr_rasterize_levels_supported"} |
               {name for name, _ in STATUS})


def main():
    path = os.environ.get("STYLERENDERER_AMD_LIB")
    if not path:
        raise SystemExit("set STYLERENDERER_AMD_LIB to the library of the commit to record")
    if "SR_RASTER_TILED" in os.environ:
        raise SystemExit("unset SR_RASTER_TILED first")
    handle = bind(ctypes.CDLL(path), NAMES)
    doc = {"sizes": query_sizes(handle), "levels": {}, "status": query_status(handle)}
    for value in TILED_SETTINGS:
        if value is not None:
            os.environ["SR_RASTER_TILED"] = value
        try:
            doc["levels"]["unset" if value is None else value] = query_levels(handle)
        finally:
            os.environ.pop("SR_RASTER_TILED", None)
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%s: %d sizes, %d level rows x %d settings, %d status rows" %
          (OUT, len(SIZES), len(LEVELS), len(TILED_SETTINGS), len(STATUS)))


if __name__ == "__main__":
    main()
