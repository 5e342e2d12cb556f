#!/usr/bin/env python3
"""Do two builds of one library hold the same device code and export the same names?

    python tools/lib_diff.py A.so B.so
    python tools/lib_diff.py --kernels A.so B.so

For a change that must not touch a kernel (a build-script or flag-neutral refactor).  The files themselves differ between any two
builds: hipcc puts a per-compilation id (__hip_cuid_<hash>, a function of the output path) into each object.  So this compares what
matters: the disassembly of every gfx950 code object (extracted as tools/isa_lint.py does; the ``file format`` line, which names the
temporary file, dropped), and the dynamic symbols apart from __hip_cuid_*.  It prints both sizes.  Exit status 1 on a difference.

--kernels reports per kernel instead (the listing split at its symbol labels, the addresses and raw words behind ``//`` dropped, so a
kernel does not differ because one in front of it moved).  A kernel is ``identical``; ``reordered (k lines)`` -- the same multiset of
instruction lines, k of them at another position, and the same VGPR, AGPR, SGPR, LDS and scratch numbers in the code object's
metadata note: the scheduler moved independent instructions and nothing else; or ``DIFFERENT``.  Only the kernels that are not
identical are listed.  Exit status 1 for a DIFFERENT kernel, one that appears or disappears, or other dynamic symbols."""
import collections
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

_spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa_lint.py"))
isa_lint = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_lint)

READELF = os.path.join(os.path.dirname(isa_lint.OBJDUMP), "llvm-readelf")
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def listings(lib, notes=None):
    out = []
    for _, elf in isa_lint.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(elf)
            f.flush()
            dis = subprocess.check_output([isa_lint.OBJDUMP, "-d", f.name], text=True)
            if notes is not None:
                notes.append(subprocess.check_output([READELF, "--notes", f.name], text=True))
        out.append("\n".join(l for l in dis.splitlines() if "file format" not in l))
    return out


def exports(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(" ".join(l.split()[1:]) for l in out.splitlines() if "__hip_cuid_" not in l)


def kernels(lib):
    """kernel symbol -> (instruction lines, resource numbers of its metadata entry)"""
    notes = []
    out = {}
    for index, dis in enumerate(listings(lib, notes)):
        code, used, name = {}, {}, None
        for raw in dis.splitlines():
            lab = re.match(r"^[0-9a-f]+ <([^>]+)>:", raw)
            if lab:
                if not lab.group(1).startswith("L"):
                    name = lab.group(1)
                    code[name] = []
                continue
            line = raw.split("//")[0].strip()
            if line and name:
                code[name].append(line)
        entry = {}
        for raw in notes[index].splitlines() + ["  - .end: 0"]:
            m = re.match(r"^(  - |    )\.(\w+):\s+(\S+)", raw)          # a kernel's own keys (its arguments' sit deeper)
            if m and m.group(1) == "  - ":
                if "name" in entry:
                    used[entry["name"]] = tuple(entry.get(k) for k in RESOURCES)
                entry = {}
            if m:
                entry[m.group(2)] = m.group(3)
        for k, v in code.items():      # (two sources may each hold a kernel of one name in their unnamed namespaces)
            out[k if k not in out else "%s [code object %d]" % (k, index)] = (v, used.get(k))
    return out


def kernel_report(a, b):
    ka, kb = kernels(a), kernels(b)
    bad = 0
    tally = collections.Counter()
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            verdict = "only in %s" % (a if name in ka else b)
        elif ka[name] == kb[name]:
            verdict = "identical"
        elif collections.Counter(ka[name][0]) == collections.Counter(kb[name][0]) and ka[name][1] == kb[name][1] and ka[name][1] is not None:
            verdict = "reordered (%d lines)" % sum(1 for x, y in zip(ka[name][0], kb[name][0]) if x != y)
        else:
            verdict = "DIFFERENT"
        tally[verdict.split(" (")[0].split(" in ")[0]] += 1
        if verdict != "identical":
            print("%s: %s" % (name, verdict))
            bad += not verdict.startswith("reordered")
    print("kernels: %d; %s" % (len(set(ka) | set(kb)), ", ".join("%d %s" % (n, v) for v, n in sorted(tally.items()))))
    return len(ka) > 0 and bad == 0


def main():
    per_kernel = sys.argv[1] == "--kernels"
    a, b = sys.argv[2:4] if per_kernel else sys.argv[1:3]
    if per_kernel:
        same_code = kernel_report(a, b)
        print("%s: %d bytes\n%s: %d bytes" % (a, os.path.getsize(a), b, os.path.getsize(b)))
    else:
        la, lb = listings(a), listings(b)
        same_code = len(la) > 0 and la == lb
        print("%s: %d bytes, %d code objects\n%s: %d bytes, %d code objects" % (a, os.path.getsize(a), len(la), b, os.path.getsize(b), len(lb)))
    same_names = exports(a) == exports(b)
    print("device code: %s; dynamic symbols: %s" % (("no DIFFERENT kernel" if per_kernel else "identical") if same_code else "DIFFERENT",
                                                    "identical" if same_names else "DIFFERENT"))
    return 0 if same_code and same_names else 1


if __name__ == "__main__":
    sys.exit(main())
