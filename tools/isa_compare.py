#!/usr/bin/env python
"""Per-kernel comparison of the gfx950 code objects of two builds of libptts_hip.so (no GPU needed): which kernels exist in both, and whether
their instruction streams are identical.

  python tools/isa_compare.py OLD/libptts_hip.so [NEW/libptts_hip.so] ['OLD NAME=NEW NAME' ...] > profiles/<name>.txt

A change that only ADDS kernels must leave every kernel of the old build in place with the same instructions: a different stream in an
existing kernel means its code generation moved (a shared device function, a struct layout, an inlining decision) and is listed by name,
with the opcodes whose counts differ (old -> new): none for renamed registers or instructions that only moved, many for a reshaped loop.
A kernel that only changed its name (a template parameter added, a non-template made a template) is missing under its old name: where
its instruction stream equals that of an added kernel it is listed as "renamed, identical" with both names and not counted as missing.
'OLD NAME=NEW NAME' (substrings of the listed names) pairs a kernel that is gone on purpose with the one that replaces it, so that the two
instruction counts stand next to each other; it stays counted as missing.
Addresses and the disassembler's comments are ignored; branch offsets are relative, so identical code compares equal wherever it is placed."""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_audit import LLVM, ROOT, demangle, short  # noqa: E402


def kernels(lib):
    """{mangled kernel name: [instruction lines]} over every embedded gfx950 code object"""
    tmp = tempfile.mkdtemp(prefix="isa_compare_")
    try:
        path = os.path.join(tmp, "lib.so")
        shutil.copy(lib, path)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", path], capture_output=True, cwd=tmp)
        out = {}
        for f in sorted(f for f in os.listdir(tmp) if "amdgcn" in f):
            obj = os.path.join(tmp, f)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], capture_output=True, text=True).stdout
            names = set(re.findall(r"^\s+\.name:\s+(\S+)$", notes, flags=re.M))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], capture_output=True, text=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
                    continue
                if cur is not None and line.strip() and line.strip() != "...":  # "...": zero padding behind a kernel, no instruction
                    cur.append(re.sub(r"\s*//.*$", "", line).strip())
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    pairs = [a.split("=", 1) for a in sys.argv[2:] if "=" in a]
    libs = [a for a in sys.argv[1:] if "=" not in a]
    old_lib = libs[0]
    new_lib = libs[1] if len(libs) > 1 else os.path.join(ROOT, "parler_tts_amd", "libptts_hip.so")
    old, new = kernels(old_lib), kernels(new_lib)
    same = [k for k in old if k in new and old[k] == new[k]]
    differ = [k for k in old if k in new and old[k] != new[k]]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    renamed = {}  # old name -> added kernel with the same instruction stream (each added kernel claimed once)
    for k in gone:
        to = next((a for a in added if new[a] == old[k] and a not in renamed.values()), None)
        if to:
            renamed[k] = to
    gone = [k for k in gone if k not in renamed]
    added = [k for k in added if k not in renamed.values()]
    names = {k: short(dn) for ks in (old, new) for k, dn in zip(ks, demangle(list(ks)))}
    print(f"# tools/isa_compare.py: {len(old)} kernels in the old build, {len(new)} in the new one")
    print(f"identical instructions : {len(same)}")
    print(f"renamed, identical     : {len(renamed)}")
    print(f"different instructions : {len(differ)}")
    print(f"missing from the new   : {len(gone)}")
    print(f"added by the new       : {len(added)}")
    if renamed:
        print("\n## renamed, identical")
        for k in sorted(renamed, key=names.get):
            print(f"{names[k]}\n  -> {names[renamed[k]]}  ({len(old[k])} instructions)")
    for title, ks, both in (("different instructions", differ, True), ("missing from the new build", gone, False), ("added by the new build", added, False)):
        if ks:
            print(f"\n## {title}")
            for k in sorted(ks, key=names.get):
                print(f"{names[k]}" + (f"  ({len(old[k])} -> {len(new[k])} instructions)" if both else f"  ({len((new if k in new else old)[k])} instructions)"))
                if both:  # a renamed register or a moved instruction changes no count; a reshaped loop does
                    co, cn = (collections.Counter(line.split()[0] for line in b[k]) for b in (old, new))
                    moved = [f"{op} {co[op]} -> {cn[op]}" for op in sorted(set(co) | set(cn)) if co[op] != cn[op]]
                    print("    opcode counts: " + (", ".join(moved) if moved else "all equal"))
    if pairs:
        print("\n## replaced (old -> new instructions)")
        for o, n in pairs:
            ko, kn = [k for k in gone if o in names[k]], [k for k in added if n in names[k]]
            if len(ko) != 1 or len(kn) != 1:
                sys.exit(f"'{o}={n}' names {len(ko)} missing and {len(kn)} added kernels, not one of each")
            print(f"{names[ko[0]]}\n  -> {names[kn[0]]}  ({len(old[ko[0]])} -> {len(new[kn[0]])} instructions)")
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
