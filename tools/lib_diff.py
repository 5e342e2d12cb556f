#!/usr/bin/env python3
"""Do two builds of one library hold the same device code and export the same names?

    python tools/lib_diff.py A.so B.so

For a change that must not touch a kernel (a build-script or flag-neutral refactor).  The files themselves differ between any two
builds: hipcc puts a per-compilation id (__hip_cuid_<hash>, a function of the output path) into each object.  So this compares what
matters: the disassembly of every gfx950 code object (extracted as tools/isa_lint.py does; the ``file format`` line, which names the
temporary file, dropped), and the dynamic symbols apart from __hip_cuid_*.  It prints both sizes.  Exit status 1 on a difference."""
import importlib.util
import os
import subprocess
import sys
import tempfile

_spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(os.path.dirname(os.path.abspath(__file__)), "isa_lint.py"))
isa_lint = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_lint)


def listings(lib):
    out = []
    for _, elf in isa_lint.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(elf)
            f.flush()
            dis = subprocess.check_output([isa_lint.OBJDUMP, "-d", f.name], text=True)
        out.append("\n".join(l for l in dis.splitlines() if "file format" not in l))
    return out


def exports(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(" ".join(l.split()[1:]) for l in out.splitlines() if "__hip_cuid_" not in l)


def main():
    a, b = sys.argv[1:3]
    la, lb = listings(a), listings(b)
    same_code = len(la) > 0 and la == lb
    same_names = exports(a) == exports(b)
    print("%s: %d bytes, %d code objects\n%s: %d bytes, %d code objects" % (a, os.path.getsize(a), len(la), b, os.path.getsize(b), len(lb)))
    print("device code: %s; dynamic symbols: %s" % ("identical" if same_code else "DIFFERENT", "identical" if same_names else "DIFFERENT"))
    return 0 if same_code and same_names else 1


if __name__ == "__main__":
    sys.exit(main())
