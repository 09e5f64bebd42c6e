"""Records which path the weight-gradient dispatch of a GIVEN library build takes and what that path needs, for
tests/test_conv_plan_cpu.py.

  STYLERENDERER_AMD_LIB=<libstylerenderer_hip.so of the commit to record> python tests/make_golden_wgrad_plan.py

writes tests/golden/wgrad_plan_parent.json: for every shape of make_golden_conv_plan.shapes() the two host-only queries

  sr_conv2d_wgrad_path, sr_conv2d_wgrad_path_floats

asked three ways — (x, gy) = (NULL, NULL), ((void*)4, NULL), (NULL, (void*)4): alignment unknown, x misaligned, gy
misaligned — once with no switch set and once per entry of SETTINGS (make_golden_conv_plan's, and the two positions of
SR_WGRAD_S2_WINO it lacks).  The file was recorded with the library of the commit BEFORE the weight-gradient plan moved
into csrc/conv_wgrad_dispatch.hip: the candidate list there has to reproduce that selection exactly.  A row is
[path, floats] x the three pointer forms, in the order of `shapes()`; a setting stores the rows that differ from the
unset run ({row index: values}).  No GPU is needed: the queries never touch the device.
"""
import ctypes
import json
import os

import make_golden_conv_plan as G

OUT = os.path.join(G.HERE, "golden", "wgrad_plan_parent.json")
SETTINGS = G.SETTINGS + tuple(s for s in (("SR_WGRAD_S2_WINO", "0"), ("SR_WGRAD_S2_WINO", "force")) if s not in G.SETTINGS)
MISALIGNED = 4                                            # conv_plan_cases.MISALIGNED
POINTERS = ((None, None), (MISALIGNED, None), (None, MISALIGNED))      # (x, gy)


def bind_queries(handle):
    L, i, p = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    handle.sr_conv2d_wgrad_path.restype = i
    handle.sr_conv2d_wgrad_path.argtypes = [L] * 7 + [i] * 4 + [p, p]
    handle.sr_conv2d_wgrad_path_floats.restype = L
    handle.sr_conv2d_wgrad_path_floats.argtypes = [L] * 7 + [i] * 4 + [p, p]
    return handle


def query(handle, rows):
    """[[path, floats, path, floats, path, floats]] (one pair per entry of POINTERS) under the current environment."""
    out = []
    for row in rows:
        got = []
        for x, gy in POINTERS:
            got += [handle.sr_conv2d_wgrad_path(*row[1:], x, gy), handle.sr_conv2d_wgrad_path_floats(*row[1:], x, gy)]
        out.append(got)
    return out


def main():
    path = os.environ.get("STYLERENDERER_AMD_LIB")
    if not path:
        raise SystemExit("set STYLERENDERER_AMD_LIB to the library of the commit to record")
    for name, _ in SETTINGS:
        if name in os.environ:
            raise SystemExit("unset %s first" % name)
    handle = bind_queries(ctypes.CDLL(path))
    rows = G.shapes()
    base = query(handle, rows)
    doc = {"rows": len(rows), "columns": ["path", "path_floats"], "pointers": ["null", "x=4", "gy=4"], "unset": base,
           "settings": {}}
    for name, value in SETTINGS:
        os.environ[name] = value
        try:
            got = query(handle, rows)
        finally:
            del os.environ[name]
        doc["settings"][G.setting_key(name, value)] = {str(j): v for j, (v, v0) in enumerate(zip(got, base)) if v != v0}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%s: %d rows, %s" % (OUT, len(rows), {k: len(v) for k, v in doc["settings"].items()}))


if __name__ == "__main__":
    main()
