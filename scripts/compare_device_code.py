#!/usr/bin/env python3
"""Is the device code of two source trees the same?  (The "speed stays" argument of a host-side refactor.)

  python scripts/compare_device_code.py TREE_A TREE_B [file.hip ...] [-j N]

For every .hip file of stylerenderer_amd/build.py's SOURCES (or the files named) both trees are compiled device-only
with that tree's own flags,

  hipcc <flags> --offload-device-only --no-gpu-bundle-output -c X.hip -o X.co

and compared per kernel symbol: the set of kernels, each kernel's disassembly (llvm-objdump -d, with addresses,
encodings and the pc-relative offsets of globals stripped: they move with a kernel's place in the code object) and its
resource numbers from the code object's metadata (llvm-readelf --notes: registers, LDS, scratch, kernarg size, ...).
Needs no GPU.  Exit status 0 iff everything is identical.

  python scripts/compare_device_code.py --union TREE_A TREE_B [-j N]

compares the UNION of the kernels over all sources of each tree instead of file against file, so a kernel that moved to
another translation unit still meets its parent: every kernel of TREE_A must exist in TREE_B with the same instructions
and resource numbers, and TREE_B may add none.  Kernels are matched by their demangled symbol (llvm-cxxfilt, or
binutils' c++filt where ROCm ships none) with every "(anonymous namespace)::" taken out: a kernel with internal linkage
carries that decoration in its own name and in the names of its argument types, so it changes when, say, a parameter
struct moves from a file's anonymous namespace into a shared header although the kernel is the same.  A kernel compiled in several files of a tree (a template in a header)
must be the same in all of them.
"""
import argparse
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

RESOURCES = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
             ".group_segment_fixed_size", ".private_segment_fixed_size", ".kernarg_segment_size",
             ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack")


def load_build(tree):
    path = os.path.join(tree, "stylerenderer_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(tree))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def llvm_tool(hipcc, name):
    for d in (os.path.join(os.path.dirname(os.path.realpath(shutil.which(hipcc) or hipcc)), "..", "llvm", "bin"),
              os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def compile_device(build, name, flags, out):
    cmd = [build._hipcc()] + build.COMMON + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c",
                                                      os.path.join(build.CSRC, name), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)


def kernels_of(co, objdump, readelf):
    """{kernel: (instruction text, {resource: value})}"""
    notes = subprocess.run([readelf, "--notes", co], check=True, stdout=subprocess.PIPE, text=True).stdout
    meta, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"^  (- | {2})(\.[a-z_]+):\s*(.*)$", line)         # keys of one amdhsa.kernels entry
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        if cur is None:
            continue
        cur[m.group(2)] = m.group(3).strip().strip("'")
        if m.group(2) == ".name":
            meta[cur[".name"]] = cur
    dis = subprocess.run([objdump, "-d", co], check=True, stdout=subprocess.PIPE, text=True).stdout
    code, sym, pc = {}, None, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            sym, pc = m.group(1), None
            code[sym] = []
        elif sym and line.strip():
            text = line.split("//")[0].strip()
            if text == "...":                                 # alignment padding behind a kernel
                continue
            # pc-relative address of a global (s_getpc_b64 s[a:b]; s_add_u32 sa, sa, <offset>; s_addc_u32 sb, sb, <offset>):
            # the offset is an address — it moves with the kernel's place in the code object
            if text.startswith("s_getpc_b64"):
                pc = 3                                        # the add / addc pair follows within three instructions
            elif pc:
                pc -= 1
                a = re.match(r"(s_addc?_u32) (\w+), (\w+), (0x[0-9a-f]+|-?\d+)$", text)
                if a and a.group(2) == a.group(3):
                    text = "%s %s, %s, <pc-relative>" % a.group(1, 2, 3)
            code[sym].append(text)
    for lines in code.values():                               # zero dwords that pad a kernel to its alignment
        while lines and lines[-1] == "v_cndmask_b32_e32 v0, s0, v0, vcc":
            lines.pop()
    return {k: ("\n".join(code.get(k, ())), {r: v.get(r) for r in RESOURCES}) for k, v in meta.items()}


def diff_kernels(ka, kb):
    diffs = ["kernel set: -%s +%s" % (sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka)))] if set(ka) != set(kb) else []
    for k in sorted(set(ka) & set(kb)):
        if ka[k][0] != kb[k][0]:
            diffs.append("instructions differ: " + k)
        if ka[k][1] != kb[k][1]:
            diffs.append("resources differ: %s %s -> %s" % (k, ka[k][1], kb[k][1]))
    return diffs


def union_of(tree_files, cxxfilt):
    """{file: kernels_of()} of one tree -> ({undecorated kernel name: (file, instructions, resources)}, [clashes])"""
    symbols = sorted({k for ks in tree_files.values() for k in ks})
    plain = subprocess.run([cxxfilt], input="\n".join(symbols), check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    plain = {s: p.replace("(anonymous namespace)::", "") for s, p in zip(symbols, plain)}
    union, clashes = {}, []
    for name in sorted(tree_files):
        for sym, (text, res) in tree_files[name].items():
            text = text.replace(sym, "<kernel>")              # the kernel's own symbol in its branch-target labels
            first = union.setdefault(plain[sym], (name, text, res))
            if first[1:] != (text, res):
                clashes.append("%s differs between %s and %s of one tree" % (plain[sym], first[0], name))
    return union, clashes


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("files", nargs="*")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--union", action="store_true", help="match kernels over all files of each tree, not file by file")
    a = ap.parse_args()
    builds = [load_build(os.path.abspath(t)) for t in (a.tree_a, a.tree_b)]
    flags = [dict(b.SOURCES) for b in builds]
    names = a.files or sorted(set(flags[0]) | set(flags[1]))
    objdump, readelf, cxxfilt = (llvm_tool(builds[0]._hipcc(), t) for t in ("llvm-objdump", "llvm-readelf", "llvm-cxxfilt"))
    if not shutil.which(cxxfilt):
        cxxfilt = "c++filt"                                   # binutils' demangler: not every ROCm ships llvm-cxxfilt
    tmp = tempfile.mkdtemp(prefix="devcode_")
    try:
        jobs = []
        with ThreadPoolExecutor(a.j) as pool:
            for name in names:
                for side in (0, 1):
                    if name in flags[side] and (a.union or name in flags[1 - side]):
                        out = os.path.join(tmp, "%d_%s.co" % (side, name))
                        jobs.append(pool.submit(compile_device, builds[side], name, flags[side][name], out))
            for j in jobs:
                j.result()
        if a.union:
            trees = [{n: kernels_of(os.path.join(tmp, "%d_%s.co" % (s, n)), objdump, readelf) for n in names if n in flags[s]}
                     for s in (0, 1)]
            (ua, clash_a), (ub, clash_b) = (union_of(t, cxxfilt) for t in trees)
            diffs = clash_a + clash_b + diff_kernels({k: v[1:] for k, v in ua.items()}, {k: v[1:] for k, v in ub.items()})
            for k in sorted(set(ua) & set(ub)):
                if ua[k][0] != ub[k][0]:
                    print("moved: %s  %s -> %s" % (k, ua[k][0], ub[k][0]))
            for d in diffs:
                print("    " + d)
            print("%d + %d files, %d kernels compared by symbol: %s" %
                  (len(trees[0]), len(trees[1]), len(ua), "identical" if not diffs else "%d differences" % len(diffs)))
            return 1 if diffs else 0
        bad = kernels = 0
        for name in names:
            if name not in flags[0] or name not in flags[1]:
                print("%-28s only in one tree" % name)
                bad += 1
                continue
            ka, kb = (kernels_of(os.path.join(tmp, "%d_%s.co" % (s, name)), objdump, readelf) for s in (0, 1))
            diffs = diff_kernels(ka, kb)
            kernels += len(ka)
            print("%-28s %3d kernels  %s" % (name, len(ka), "identical" if not diffs else "DIFFERENT"))
            for d in diffs:
                print("    " + d)
            bad += bool(diffs)
        print("%d files, %d kernels compared: %s" % (len(names), kernels, "identical" if not bad else "%d files differ" % bad))
        return 1 if bad else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
