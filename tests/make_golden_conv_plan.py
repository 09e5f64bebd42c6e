"""Records what the dense-convolution dispatch of a GIVEN library build answers, for tests/test_conv_plan_cpu.py.

  STYLERENDERER_AMD_LIB=<libstylerenderer_hip.so of the commit to record> python tests/make_golden_conv_plan.py

writes tests/golden/conv_plan_parent.json: for every shape of `shapes()` the three host-only queries

  sr_conv2d_scratch_floats, sr_conv2d_wgrad_scratch_floats, sr_conv2d_uses_winograd (NULL buffers; in = (void*)4)

once with no switch set and once per entry of SETTINGS (one switch at a time).  The file was recorded with the library
of the commit BEFORE the dispatch plan was introduced: the plan has to reproduce that selection and those sizes exactly.
Rows hold values only ([forward, wgrad, wino(NULL), wino(in = 4)], in the order of `shapes()`); a setting stores the rows
that differ from the unset run ({row index: values}).  No GPU is needed: the queries never touch the device.
"""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "conv_plan_parent.json")

GEOM = {  # op/conv.py's _GEOM: name -> (ksize, stride, pad, transposed)
    "c3": (3, 1, 1, 0), "c3s2": (3, 2, 0, 0), "t3s2": (3, 2, 0, 1), "c1": (1, 1, 0, 0), "c1s2": (1, 2, 0, 0),
}
BATCHES = (1, 2, 4, 8, 16)
CHANNELS = (3, 4, 32, 64, 128, 256, 320, 512)
# (C, N): the diagonal, and pairs across the small / large and 256 / 320 / 512 boundaries
PAIRS = tuple((c, c) for c in CHANNELS) + (
    (3, 4), (4, 3), (3, 128), (512, 3), (32, 64), (64, 32), (128, 256), (256, 128), (320, 512), (512, 320), (512, 256),
    (256, 512))
SQUARES = tuple((s, s) for s in (4, 8, 16, 32, 64, 128, 256))
ODD = ((33, 30), (12, 32), (8, 64))                       # the non-square maps of the GPU tests
POW2P1 = tuple((s, s) for s in (9, 17, 33, 65, 129, 257))  # inputs of the stride-2 3x3 convolution

SETTINGS = (
    ("SR_WINOGRAD", "0"), ("SR_WINO_SPLIT", "0"), ("SR_CONV_S2_WINO", "0"), ("SR_CONV_S2_WINO", "force"),
    ("SR_CONVT_TAPS", "0"), ("SR_CONVT_TAPS", "1"), ("SR_CONVT_TAPS_GEMM", "0"), ("SR_CONVT_FUSED", "0"),
    ("SR_CONVT_FUSED", "1"), ("SR_CONVT_FUSED_KS", "0"), ("SR_CONVT_STRIPS", "0"), ("SR_CONV1X1_GEMM", "0"),
    ("SR_WGRAD_SMALL", "0"), ("SR_WGRAD_DMA", "0"), ("SR_CONV_SPLIT_BF16", "1"),
)


def out_size(ih, iw, k, stride, pad, transposed):
    if transposed:
        return (ih - 1) * stride + k - 2 * pad, (iw - 1) * stride + k - 2 * pad
    return (ih + 2 * pad - k) // stride + 1, (iw + 2 * pad - k) // stride + 1


def shapes():
    """[(geom, B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed)] in a fixed order."""
    rows = []
    for name, (k, stride, pad, tr) in GEOM.items():
        maps = SQUARES + ODD + (POW2P1 if name == "c3s2" else ())
        for ih, iw in maps:
            oh, ow = out_size(ih, iw, k, stride, pad, tr)
            for b in BATCHES:
                for c, n in PAIRS:
                    rows.append((name, b, c, n, ih, iw, oh, ow, k, stride, pad, tr))
    return rows


def setting_key(name, value):
    return "%s=%s" % (name, value)


def bind_queries(handle):
    L, i, p = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    handle.sr_conv2d_scratch_floats.restype = L
    handle.sr_conv2d_scratch_floats.argtypes = [L] * 7 + [i] * 4
    handle.sr_conv2d_wgrad_scratch_floats.restype = L
    handle.sr_conv2d_wgrad_scratch_floats.argtypes = [L] * 7 + [i] * 4
    handle.sr_conv2d_uses_winograd.restype = i
    handle.sr_conv2d_uses_winograd.argtypes = [L] * 5 + [p, p]
    return handle


def query(handle, rows):
    """[[forward floats, wgrad floats, wino with NULL buffers, wino with in = (void*)4]] under the current environment."""
    out = []
    for _, b, c, n, ih, iw, oh, ow, k, stride, pad, tr in rows:
        out.append([handle.sr_conv2d_scratch_floats(b, c, n, ih, iw, oh, ow, k, stride, pad, tr),
                    handle.sr_conv2d_wgrad_scratch_floats(b, c, n, ih, iw, oh, ow, k, stride, pad, tr),
                    handle.sr_conv2d_uses_winograd(b, c, n, ih, iw, None, None),
                    handle.sr_conv2d_uses_winograd(b, c, n, ih, iw, 4, None)])
    return out


def main():
    path = os.environ.get("STYLERENDERER_AMD_LIB")
    if not path:
        raise SystemExit("set STYLERENDERER_AMD_LIB to the library of the commit to record")
    for name, _ in SETTINGS:
        if name in os.environ:
            raise SystemExit("unset %s first" % name)
    handle = bind_queries(ctypes.CDLL(path))
    rows = shapes()
    base = query(handle, rows)
    doc = {"rows": len(rows), "columns": ["scratch_floats", "wgrad_scratch_floats", "uses_winograd_null", "uses_winograd_in4"],
           "unset": base, "settings": {}}
    for name, value in SETTINGS:
        os.environ[name] = value
        try:
            got = query(handle, rows)
        finally:
            del os.environ[name]
        doc["settings"][setting_key(name, value)] = {str(j): v for j, (v, v0) in enumerate(zip(got, base)) if v != v0}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%s: %d rows, %s" % (OUT, len(rows), {k: len(v) for k, v in doc["settings"].items()}))


if __name__ == "__main__":
    main()
