#!/usr/bin/env python3
"""Is the gfx950 device code of two built trees the same?

    python scripts/compare_device_code.py TREE_A TREE_B [--unit NAME ...]

Both trees must have been built (`python -m ark_analysis_amd._build`): the objects of csrc/*.hip are read from
csrc/_obj/.  From each object the gfx950 code object is taken (llvm-objcopy, clang-offload-bundler), disassembled
(llvm-objdump) and its kernel descriptors read (llvm-readelf).  Compared over the whole library, whatever unit a
kernel lives in: the set of device functions (each exactly once), every function's instruction text, and per kernel
the VGPR / SGPR counts and the LDS and scratch sizes.  Prints the differing functions and one summary line; exit
status 1 on any difference.  For refactors of csrc/ that must not change a kernel.  --unit pxsom_batch_step compares that
unit's object alone (several may be named): the check after each step of such a refactor, one unit rebuilt at a time.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
DESCRIPTOR_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def tool(name):
    exe = shutil.which(name) or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", name)
    if not os.path.exists(exe):
        sys.exit(f"{name} not found (PATH, $ROCM_PATH/llvm/bin)")
    return exe


def code_object(obj, tmp):
    """The gfx950 code object inside a host object, or None when the unit has no device code."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([tool("llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj], check=False,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat,
                    "--output=" + co], check=True)
    return co if os.path.getsize(co) > 0 else None


def functions(co):
    """symbol -> instruction text (addresses and encodings stripped)"""
    out = subprocess.run([tool("llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                         text=True).stdout
    funcs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is not None and line.startswith("\t") and line.strip() != "...":   # ("...": zero padding behind a unit's last function)
            cur.append(line.split("//")[0].strip())
    return {k: "\n".join(v) for k, v in funcs.items()}


def descriptors(co):
    """kernel name -> the DESCRIPTOR_KEYS of its metadata"""
    out = subprocess.run([tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        if line.startswith("  - "):   # a new entry of amdhsa.kernels
            cur = {}
            line = "    " + line[4:]
        m = re.match(r"^    (\.[a-z_]+):\s*(\S.*)$", line)
        if cur is None or not m:
            continue
        if m.group(1) == ".name":
            kernels[m.group(2)] = cur
        elif m.group(1) in DESCRIPTOR_KEYS:
            cur[m.group(1)] = m.group(2)
    return kernels


def library(tree, units=()):
    """(symbol -> [(unit, text)], kernel -> descriptor) over every unit of the tree, or over `units` alone"""
    csrc = os.path.join(tree, "ark_analysis_amd", "csrc")
    funcs, descs = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for unit in units or sorted(os.path.basename(src)[:-4] for src in glob.glob(os.path.join(csrc, "*.hip"))):
            obj = os.path.join(csrc, "_obj", unit + ".o")
            if not os.path.exists(obj):
                sys.exit(f"{obj} is missing: build {tree} first")
            co = code_object(obj, tmp)
            if co is None:
                continue
            for sym, text in functions(co).items():
                funcs.setdefault(sym, []).append((unit, text))
            descs.update(descriptors(co))
    return funcs, descs


def main():
    args = sys.argv[1:]
    units = [args[i + 1] for i, a in enumerate(args[:-1]) if a == "--unit"]
    trees = [a for i, a in enumerate(args) if a != "--unit" and (i == 0 or args[i - 1] != "--unit")]
    if len(trees) != 2:
        sys.exit(__doc__)
    (fa, da), (fb, db) = library(trees[0], units), library(trees[1], units)
    bad = []
    for sym in sorted(set(fa) | set(fb)):   # a function defined by several units: by the same number of them on both sides
        na, nb = len(fa.get(sym, [])), len(fb.get(sym, []))
        if na != nb and na and nb:
            bad.append(f"defined {na} times in A, {nb} times in B: {sym}")
        for name, where in (("A", fa.get(sym, [])), ("B", fb.get(sym, []))):
            if len(set(t for _, t in where)) > 1:
                bad.append(f"copies differ inside {name}: {sym} ({', '.join(u for u, _ in where)})")
    for sym in sorted(set(fa) - set(fb)):
        bad.append(f"only in A: {sym} ({fa[sym][0][0]})")
    for sym in sorted(set(fb) - set(fa)):
        bad.append(f"only in B: {sym} ({fb[sym][0][0]})")
    for sym in sorted(set(fa) & set(fb)):
        if fa[sym][0][1] != fb[sym][0][1]:
            bad.append(f"instructions differ: {sym} ({fa[sym][0][0]} / {fb[sym][0][0]})")
        if da.get(sym) != db.get(sym):
            bad.append(f"descriptor differs: {sym}: {da.get(sym)} / {db.get(sym)}")
    for line in bad:
        print(line)
    print(f"{len(fa)} device functions in A, {len(fb)} in B ({len(da)} / {len(db)} kernels): {len(bad)} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
