"""What csrc/build.sh resolves its table of libraries to (``build.sh --list``; nothing is compiled): the tests assert on these values, not
on the script's text."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_SH = os.path.join(ROOT, "hse_facerec_tf_amd", "csrc", "build.sh")


@functools.lru_cache(maxsize=None)
def rows(dev=False):
    """name -> {"out", "srcs", "flags", "deps", "keep", "lint", ...} in build order, for the product build or the development one.
    ``srcs``, ``flags`` and ``deps`` are lists of words; a dependency is given from the repository's root."""
    env = {k: v for k, v in os.environ.items() if k not in ("HSEFR_DEV", "HSEFR_ASAN", "HSEFR_EXTRA_FLAGS")}
    if dev:
        env["HSEFR_DEV"] = "1"
    out = subprocess.run(["bash", BUILD_SH, "--list"], env=env, capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        row = dict(field.split("=", 1) for field in line.split("\t"))
        for key in [k for k in row if k in ("srcs", "deps") or k.startswith("flags")]:
            row[key] = row[key].split()
        row["deps"] = [os.path.relpath(os.path.join(os.path.dirname(BUILD_SH), d), ROOT) for d in row["deps"]]
        table[row.pop("name")] = row
    return table


def stale_against(name, *files):
    """Whether the objects of library ``name`` are rebuilt when one of ``files`` (csrc headers by name, anything else from the root) changes."""
    deps = rows()[name]["deps"]
    return all((f if "/" in f else "hse_facerec_tf_amd/csrc/" + f) in deps for f in files)
