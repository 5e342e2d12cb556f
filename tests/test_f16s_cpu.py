"""csrc/f16s.h states the split-f16 vocabulary once: the split, the split rows' swizzle, relu6 and the three-MFMA product are written
there and nowhere else in csrc/*.hip and csrc/*.h -- apart from the places listed here by name, each with its reason.  Source text
only; the bits are pinned on the GPU (test_f16s_bits_gpu.py, test_stem_bits_gpu.py)."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hse_facerec_tf_amd", "csrc")
SOURCES = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}

STEMS = {"stem_patch.h", "stem2_fused.hip", "stem3_fused.hip", "stem4_fused.hip", "stem5_stream.hip"}
# the files that take the vocabulary from the header (stem_fused.hip is round 1's stem, development builds only)
ADOPTERS = {"pwconv_f16s.hip", "dwpw_f16s.hip", "pwblk_stream.hip", "pwconv_ps.hip", "dwconv.hip", "stem_fused.hip"} | STEMS
# a split: a convertvector of a difference whose subtrahend is a convertvector
SPLIT = re.compile(r"__builtin_convertvector\(\s*\w+\s*-\s*__builtin_convertvector\(")
F16_MFMA = re.compile(r"__builtin_amdgcn_mfma_f32_(?:32x32x16|16x16x32)_f16")
# Kernels that keep the three products spelt out, once each, because hipcc compiles them differently through a call of the helper
# (tools/lib_diff.py --kernels against the build before): pwblk_stream.hip's `mfmas` (another register numbering) and
# pwconv_ps.hip's `mfma_block` (its two accumulators' MFMAs alternate)
OWN_PRODUCT = {"pwblk_stream.hip", "pwconv_ps.hip"}


def files_with(pattern):
    return {name for name, text in SOURCES.items() if pattern.search(text)}


def test_the_split_is_written_in_the_header_alone():
    assert files_with(SPLIT) == {"f16s.h"}


def test_the_row_swizzle_and_relu6_are_defined_in_the_header_alone():
    # the split rows' swizzle is the one with the row-parity term; conv_bf16.hip and conv1x1_bf16.hip have a swzb of their own, another
    # function (bf16 tiles, key (row >> 1) & 7 alone), which stays
    swzb = files_with(re.compile(r"\bint swzb\s*\("))
    assert swzb == {"f16s.h", "conv_bf16.hip", "conv1x1_bf16.hip"}
    for name in ("conv_bf16.hip", "conv1x1_bf16.hip"):
        assert re.search(r"int swzb\(int row, int chunk\) \{ return row \* 128 \+ 16 \* \(chunk \^ \(\(row >> 1\) & 7\)\); \}", SOURCES[name]), name
    assert files_with(re.compile(r"\bint swz_key\s*\(")) == {"f16s.h", "bf16_dma.h"}      # (the bf16 kernels' own header has theirs)
    # dwpw_fused.hip is the fp32-MFMA block kernel: no split-f16 arithmetic in it, it includes common.h alone
    assert files_with(re.compile(r"\bfloat relu6\s*\(")) == {"f16s.h", "dwpw_fused.hip"}
    assert '"f16s.h"' not in SOURCES["dwpw_fused.hip"] and not F16_MFMA.search(SOURCES["dwpw_fused.hip"])
    for name in ADOPTERS:
        assert not re.search(r"typedef\s+(?:float|_Float16)\s+(?:f32x4|f32x16|f16x4|f16x8)\b", SOURCES[name]), name
        assert not re.search(r"\b(?:PB_)?ROWB\s*=", SOURCES[name]), name


def test_the_f16_mfma_builtins_stay_where_they_are_allowed():
    allowed = {"f16s.h", "devtools.hip"} | STEMS | OWN_PRODUCT
    assert files_with(F16_MFMA) <= allowed
    for name in OWN_PRODUCT:      # ... and there once: one lambda holds the product (three MFMAs; pwconv_ps.hip: in both operand orders, twice each)
        assert len(F16_MFMA.findall(SOURCES[name])) == {"pwblk_stream.hip": 3, "pwconv_ps.hip": 12}[name], name
    for name in ("pwconv_f16s.hip", "dwpw_f16s.hip", "stem_fused.hip"):
        assert re.search(r"\bmac3(?:_t)?\(", SOURCES[name]), name


def test_every_adopting_file_includes_the_header():
    assert '#include "f16s.h"' in SOURCES["stem_patch.h"]
    for name in ADOPTERS - {"stem_patch.h"}:
        text = SOURCES[name]
        assert '#include "f16s.h"' in text or (name in STEMS and '#include "stem_patch.h"' in text), name
    # the header holds functions, types and constants only, and common.h in front of them
    header = SOURCES["f16s.h"]
    assert '#include "common.h"' in header and "__global__" not in header and "namespace f16s" in header
    for line in header.splitlines():
        if re.match(r"^[\w:]+[\w\s\*&:]*\(", line) and not line.startswith(("typedef", "constexpr")):
            assert line.startswith("__device__ __forceinline__"), line


def test_one_activation_switch():
    # the launchers' three-way chain is common.h's macro; the stems' dispatch is a name for it
    assert "#define HSEFR_ACT_SWITCH(act, who, M)" in SOURCES["common.h"]
    assert "HSEFR_ACT_SWITCH(act, kernel, LAUNCH)" in SOURCES["stem_patch.h"]
    uses = {name: text.count("HSEFR_ACT_SWITCH(act, \"") for name, text in SOURCES.items()}
    assert (uses["pwconv_f16s.hip"], uses["dwpw_f16s.hip"], uses["pwconv_ps.hip"]) == (1, 3, 2)
    for name in ("pwconv_f16s.hip", "dwpw_f16s.hip"):
        assert "else if (act == HSEFR_ACT_RELU)" not in SOURCES[name], name
