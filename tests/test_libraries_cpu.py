"""CPU suite: what holds for EVERY shared library of the package, once, over _lib.LIBRARIES -- the public header, the library's dynamic
symbols and the binding table agree; the version; loaded once; gfx950 only; the ISA lint with each library's floor; no library, binding
table or header carries a name of another library; libhsefr.so's size and version; and csrc/build.sh's table names the same libraries
in the same order.  What is specific to one library stays in that library's own file.

A new library is a row in csrc/build.sh, a record in _lib.LIBRARIES, a header under include/ and a row in FLOORS here."""
import functools
import importlib.util
import os
import re
import subprocess

import pytest

import build_table
from hse_facerec_tf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBRARIES = _lib.LIBRARIES
IDS = [library.tag for library in LIBRARIES]
PAIRS = [(a, b) for a in LIBRARIES for b in LIBRARIES if a is not b]
# tag -> the kernel symbols and wide stores tools/isa_lint.py must at least see in the library: below that it did not look at the device code
FLOORS = {
    "hsefr": (51, 101),
    "hsefr_album": (1, 1),            # the kernel and its 16-byte store
    "hsefr_frames": (6, 3),           # the vector forms of both kernels: swap_kernel<true>, three turn_kernel instances with a 12-byte side
    "hsefr_forest": (7, 1),           # the seven kernels, and the candidate table's 16-byte store
    "hsefr_ragged": (9, 0),           # the pyramid, three convolution instances, the pooling, stage 1, the crops, two stage-finish instances
    "hsefr_mixed": (4, 4),            # the swap, the turn, two crop instances; the swap's unit, the turn's two directions, the crops' 16 bytes
    "hsefr_split": (4, 1),            # the build and the three chain instances; the build's pair of matrix entries
    "hsefr_geom": (10, 0),            # the rounds' seven, the engine's four
    "hsefr_shift": (14, 3),           # prep, norms x 2, member x 2, means, step, compact, rank, gather, suppress, centers, assign, info; the
                                      # 16-byte stores of the three row copies
    "hsefr_affinity": (19, 0),        # norms, sim, copy, minmax, hist, digit, prepare, sweep x 2, colsum, stop, select, assign, member_sum,
                                      # winner, relist, labels, trivial, info
}
# libhsefr.so alone exports weak symbols: instances of the C++ runtime's own templates (std::vector, std::map), which no flag of its
# build hides.  Nothing of the project is among them, and no other library has any
WEAK_NAMESPACES = {"hsefr": ("_ZNSt", "_ZNKSt", "_ZN9__gnu_cxx")}


def header(library):
    return os.path.join(ROOT, "include", library.tag + ".h")


def code(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def declared(library):
    return sorted(set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % library.tag, code(header(library)))))


@functools.lru_cache(maxsize=None)
def exported(path, kind="T"):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[-1] for l in out.splitlines() if " %s " % kind in l and not l.split()[-1].startswith(("_init", "_fini")))


def owner(name):
    """The library a name belongs to: the one with the longest prefix (hsefr_ itself is a prefix of every name)."""
    return max((library for library in LIBRARIES if name.startswith(library.tag + "_")), key=lambda library: len(library.tag))


# ---- surface -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("library", LIBRARIES, ids=IDS)
def test_header_library_and_binding_agree(library):
    names = declared(library)
    assert len(names) >= 3 and library.error_fn in names and library.version_fn in names
    assert os.path.exists(library.path), "run __graft_entry__.build() first"
    assert os.path.basename(library.path) == os.environ.get(library.env, library.file)
    assert exported(library.path) == names
    assert sorted(library.signatures) == names
    weak = exported(library.path, "W")
    assert [n for n in weak if not n.startswith(WEAK_NAMESPACES.get(library.tag, ()))] == []     # nothing of the C++ runtime's templates
    assert not [n for n in weak if "hsefr" in n]
    L = library.load()
    define = r"#define %s_VERSION (\d+)" % library.tag.upper()
    assert getattr(L, library.version_fn)() == int(re.search(define, open(header(library)).read()).group(1)) == library.version
    assert library.load() is L                                                          # loaded once
    assert isinstance(library.last_error(), str)


def test_the_module_names_are_the_registrys():
    assert IDS == ["hsefr", "hsefr_album", "hsefr_frames", "hsefr_forest", "hsefr_ragged", "hsefr_mixed", "hsefr_split", "hsefr_geom",
                   "hsefr_shift", "hsefr_affinity"]
    assert [library.version for library in LIBRARIES] == [141] + [100] * 9
    assert (_lib.LIB_PATH, _lib.SIGNATURES, _lib.DEV_SIGNATURES) == (LIBRARIES[0].path, LIBRARIES[0].signatures, LIBRARIES[0].optional)
    assert (_lib.lib, _lib.last_error, _lib.check) == (LIBRARIES[0].load, LIBRARIES[0].last_error, LIBRARIES[0].check)
    for library in LIBRARIES[1:]:
        x = library.tag[len("hsefr_"):]
        assert getattr(_lib, x.upper() + "_LIB_PATH") == library.path and getattr(_lib, x.upper() + "_SIGNATURES") is library.signatures
        assert (getattr(_lib, x + "_lib"), getattr(_lib, x + "_last_error"), getattr(_lib, x + "_check")) == \
            (library.load, library.last_error, library.check)
        assert library.env == "HSEFR_%s_LIB" % x.upper() and library.file == "lib%s.so" % library.tag
        assert getattr(_lib, x + "_lib")() is library.load()
    # the check behind a build walks this registry and no other table
    assert "for library in _lib.LIBRARIES:" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


@pytest.mark.parametrize("library", LIBRARIES, ids=IDS)
def test_a_status_raises_in_the_librarys_name(library, monkeypatch):
    monkeypatch.setattr(library, "last_error", lambda: "why")
    for status, error in ((_lib.ERR_INVALID, ValueError), (_lib.ERR_SHAPE, ValueError), (_lib.ERR_UNSUPPORTED, NotImplementedError),
                          (_lib.ERR_NOMEM, MemoryError), (_lib.ERR_HIP, _lib.HsefrError)):
        with pytest.raises(error) as e:
            library.check(status, "call")
        assert str(e.value) == "call: why (%s status %d)" % (library.tag, status)
    with pytest.raises(ValueError) as e:
        library.check(-1)
    assert str(e.value) == "why (%s status -1)" % library.tag
    assert library.check(0, "call") is None


# ---- target and lint -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("library", LIBRARIES, ids=IDS)
def test_code_object_targets_gfx950_only(library):
    blob = open(library.path, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx942", b"gfx90a", b"sm_90", b"gfx1100"):
        assert other not in blob


@pytest.mark.parametrize("library", LIBRARIES, ids=IDS)
def test_device_code_passes_the_isa_lint(library):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump on this machine")
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(ROOT, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    findings, n_symbols, n_stores = lint.lint(library.path)
    min_symbols, min_stores = FLOORS[library.tag]
    assert n_symbols >= min_symbols, "the lint did not see the kernels"
    assert n_stores >= min_stores, "the lint did not see the wide stores"
    assert findings == []


# ---- separation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a,b", PAIRS, ids=["%s-%s" % (a.tag[6:] or "hsefr", b.tag[6:] or "hsefr") for a, b in PAIRS])
def test_no_library_carries_a_name_of_another(a, b):
    """Library ``a`` -- its exports, its binding table, its header -- holds no name of library ``b``."""
    assert not [n for n in exported(a.path) if owner(n) is b]
    assert not [n for n in a.signatures if owner(n) is b] and not [n for n in a.optional if owner(n) is b]
    assert not [n for n in re.findall(r"\b(hsefr_[a-z0-9_]+)\s*\(", code(header(a))) if owner(n) is b]         # declares no function of b
    if LIBRARIES.index(a) < LIBRARIES.index(b):
        assert b.tag not in open(header(a)).read()                                      # nor do an earlier header's comments know a later library


def test_the_main_library_keeps_its_size_and_version():
    assert os.path.getsize(_lib.LIB_PATH) < 4_000_000
    assert _lib.lib().hsefr_version() == 141


# ---- the build table -----------------------------------------------------------------------------------------------------------------
def test_the_build_script_declares_the_same_libraries_in_the_same_order():
    for dev in (False, True):
        table = build_table.rows(dev)
        assert ["hsefr" if name == "hsefr" else "hsefr_" + name for name in table] == IDS
        main_out = "libhsefr_dev.so" if dev else "libhsefr.so"
        assert [os.path.basename(row["out"]) for row in table.values()] == [main_out] + [library.file for library in LIBRARIES[1:]]
        for name, row, library in zip(table, table.values(), LIBRARIES):
            assert "include/%s.h" % library.tag in row["deps"] and "hse_facerec_tf_amd/csrc/build.sh" in row["deps"], name
            assert row["lint"] == "1", name                                             # every library is linted where it is built
            assert "--offload-arch=gfx950" in row["flags"] and "-O3" in row["flags"], name
    later = [row for name, row in build_table.rows().items() if name != "hsefr"]
    assert all(row == dev_row for row, dev_row in zip(later, list(build_table.rows(True).values())[1:]))      # the same in every mode
    assert {row["keep"] for row in later} == {"_ZN*_kernel*"} and build_table.rows()["hsefr"]["keep"] == "_ZN5hsefr*_kernel*"
    # the lint is one unconditional statement of the script, which stops at the first failing command
    script = open(build_table.BUILD_SH).read()
    assert "\nset -euo pipefail\n" in script and len(re.findall(r"^\s*python3 \S*tools/isa_lint\.py \"\$out\"$", script, flags=re.M)) == 1
    assert script.count("isa_lint.py \"") == 1
