#!/bin/bash
# Builds the project's shared libraries for gfx950 in-tree (hipcc cross-compiles without a GPU).  There are several because libhsefr.so
# is held below 4 MB and at its version by its tests: device code that came later lives in a library of its own, with its own public
# header, version and error string.  The table LIBS below declares them, one row each, and build_lib builds a row.
#   HSEFR_DEV=1 build.sh   builds libhsefr_dev.so in place of libhsefr.so: the same sources with -DHSEFR_DEV (tuning knobs as run-time
#                          variables, hsefr_debug_*, the calibration kernels of devtools.hip) -- for tools/kbench.py only.
#   build.sh --list        prints the resolved table and compiles nothing: per library its name, output, sources, the complete compile
#                          flags of the current mode and the files its objects are stale against (tests/test_libraries_cpu.py reads it)
# A new library is a row of LIBS, a record in hse_facerec_tf_amd/_lib.py's LIBRARIES at the same place, a header under include/ and a row
# of FLOORS in tests/test_libraries_cpu.py.
set -euo pipefail
cd "$(dirname "$0")"
# product sources.  Development builds add round 1's stem (reachable only through lower_graph(stem_fusion="stem")) and the first window 3x3
# convolution (conv3x3_w2_bf16.hip took its layers in round 5), each kept for A/B timing, plus the calibration kernels of devtools.hip.
SRCS="engine.hip conv_first.hip dwconv.hip pwconv_f32.hip pwconv_f16s.hip pwconv_ps.hip pool_dense.hip nn1.hip conv_bf16.hip conv1x1_bf16.hip preprocess.hip dwpw_fused.hip dwpw_f16s.hip pwblk_stream.hip stem2_fused.hip stem3_fused.hip stem4_fused.hip stem5_stream.hip conv_f32_mfma.hip smallnet.hip area_resize.hip stem7x7_pool.hip stem7s_stream.hip conv_dma_bf16.hip conv3x3_w2_bf16.hip conv1x1_w4_bf16.hip conv1x1_pair_bf16.hip mtcnn_post.hip linkage.hip hier_linkage.hip dbscan.hip rank_order.hip pca.hip partition_scores.hip linear_svm.hip rbf_svm.hip"
# -Wno-inline-asm: the LDS-DMA statements write M0 and say so in their clobber lists; clang warns that M0 is a
# reserved register for every instantiation -- the declaration is the point (the compiler must not assume M0 survives)
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-result -Wno-inline-asm"
# the device code objects ship without their local symbols (several KB per source; the product stays below 4 MB,
# tests/test_abi_cpu.py): the runtime, the profilers and tools/isa_lint.py need only the kernel symbols, which stay
DEVICE_STRIP="-Xoffload-linker --discard-all"
LINK="--offload-arch=gfx950"
# what the nine later libraries are compiled with in every mode (no -DHSEFR_DEV code in them): libhsefr.so's own product flags
COMMON="$FLAGS $DEVICE_STRIP"
# the three modes of the main library: its output, its build directory (the other libraries' objects go there too) and its flags
if [ "${HSEFR_ASAN:-0}" = "1" ]; then
  # HSEFR_ASAN=1 build.sh   the HOST half of the same sources under the address + undefined-behaviour sanitizers (no device code is
  #                         compiled and none runs: GPU sanitizers are not available on this pool) -> build_asan/libhsefr_asan.so +
  #                         build_asan/fuzz_plan, the driver tests/test_plan_blob_fuzz_cpu.py runs.  The compiler flags of that mode live
  #                         in build_asan_flags.sh, which .gpurunignore keeps off the GPU boxes (their launcher refuses any tree whose
  #                         build scripts mention a sanitizer): a CPU-only recipe.
  MODE=hostonly; OUT=build_asan/libhsefr_asan.so; BUILD=build_asan
  . ./build_asan_flags.sh
elif [ "${HSEFR_DEV:-0}" = "1" ]; then
  MODE=dev; OUT=../libhsefr_dev.so; BUILD=build_dev; SRCS="$SRCS stem_fused.hip conv3x3_win_bf16.hip devtools.hip"; FLAGS="$FLAGS -DHSEFR_DEV $DEVICE_STRIP"
else
  MODE=product; OUT=../libhsefr.so; BUILD=build; FLAGS="$COMMON"
fi
# ---- the libraries, in build order:  name | output | public headers (its own first) | sources | compile flags | symbols llvm-strip keeps
# The name is the prefix of a later library's objects (<name>_<source>.o: hier_linkage.hip is compiled twice); libhsefr.so's keep their
# plain names, which tools/build_ko.sh and tools/build_ps_ko.sh link.  Every object is stale against its source, EVERY header here (by
# glob: a new header needs no edit of this file), the row's public headers and this script.
#   album, mixed  -ffp-contract=off: OpenCV's resize taps are computed in the kernel, where a product fused with the subtraction behind it
#                 would round once instead of twice.  mixed compiles the per-pixel bodies of album.hip and frames.hip (cv_linear_px.h,
#                 frames_px.h) and must give their bits
#   forest        -ffp-contract=off: a candidate's score and a threshold are the restatement's fp64 operations one by one
#                 (tests/random_forest_ref.py)
#   ragged, split libhsefr.so's own flags: they compile bodies that library compiles (mtcnn_post_frame.h and area_resize_px.h;
#                 linkage_scan.h's feat_tile over mfma_dot.h) and must give their bits
#   geom          the same plus -DHSEFR_GEOM_LIB: besides geom_linkage.hip it compiles hier_linkage.hip a second time (the working matrix
#                 over feat_tile, and the rounds with Ward's rule).  The three update rules switch contraction off themselves (geom_rules.h)
#   shift         libhsefr.so's own flags: mean-shift clustering (mean_shift.hip), fp64 on the MFMA
#   affinity      libhsefr.so's own flags: affinity-propagation clustering (affinity.hip), fp64; the source switches contraction off itself
LIBS=(
  "hsefr|$OUT|hsefr.h|$SRCS|$FLAGS|_ZN5hsefr*_kernel*"
  "album|../libhsefr_album.so|hsefr_album.h|album.hip|$COMMON -ffp-contract=off|_ZN*_kernel*"
  "frames|../libhsefr_frames.so|hsefr_frames.h|frames.hip|$COMMON|_ZN*_kernel*"
  "forest|../libhsefr_forest.so|hsefr_forest.h|forest.hip|$COMMON -ffp-contract=off|_ZN*_kernel*"
  "ragged|../libhsefr_ragged.so|hsefr_ragged.h|mtcnn_ragged.hip|$COMMON|_ZN*_kernel*"
  "mixed|../libhsefr_mixed.so|hsefr_mixed.h|mixed_frames.hip|$COMMON -ffp-contract=off|_ZN*_kernel*"
  "split|../libhsefr_split.so|hsefr_split.h hsefr.h|group_split.hip|$COMMON|_ZN*_kernel*"
  "geom|../libhsefr_geom.so|hsefr_geom.h hsefr.h|geom_linkage.hip hier_linkage.hip|$COMMON -DHSEFR_GEOM_LIB|_ZN*_kernel*"
  "shift|../libhsefr_shift.so|hsefr_shift.h hsefr.h|mean_shift.hip|$COMMON|_ZN*_kernel*"
  "affinity|../libhsefr_affinity.so|hsefr_affinity.h hsefr.h|affinity.hip|$COMMON|_ZN*_kernel*"
)
if [ "$MODE" = hostonly ]; then LIBS=("${LIBS[0]}"); fi      # the host-only recipe has nothing of the other libraries

row() { IFS='|' read -r name out headers srcs flags keep <<< "$1"; }
object() { if [ "$name" = hsefr ]; then echo "$BUILD/${1%.hip}.o"; else echo "$BUILD/${name}_${1%.hip}.o"; fi; }
deps() { echo *.h $(printf '../../include/%s ' $headers) build.sh; }
# the HOST half of every source is optimised for size (launchers and argument checks, 28 KB less of them in libhsefr.so): -Xarch_host
# reaches the host compilation only, the device side keeps -O3 and its code objects hold the same instructions as without the flag.
# Not in the main library's other two modes, and not for engine.hip (the forward call itself)
compile_flags() {
  if [ "$name" = hsefr ] && { [ "$MODE" != product ] || [ "$1" = engine.hip ]; }; then echo "$flags${HSEFR_EXTRA_FLAGS:+ $HSEFR_EXTRA_FLAGS}"
  else echo "$flags -Xarch_host -Os${HSEFR_EXTRA_FLAGS:+ $HSEFR_EXTRA_FLAGS}"; fi
}

if [ "${1:-}" = "--list" ]; then
  for r in "${LIBS[@]}"; do
    row "$r"
    printf 'name=%s\tout=%s\tsrcs=%s\tflags=%s\tdeps=%s\tkeep=%s\tlint=%s' "$name" "$out" "$srcs" "$(compile_flags "")" "$(deps)" "$keep" \
      "$([ "$MODE" = hostonly ] && echo 0 || echo 1)"
    if [ "$name" = hsefr ]; then printf '\tflags[engine.hip]=%s' "$(compile_flags engine.hip)"; fi
    printf '\n'
  done
  exit 0
fi

# every stale compile of every library goes into one pool of at most 16 hipcc at a time; a failed compile fails the build (xargs
# exits 123, set -e)
mkdir -p "$BUILD"
: > "$BUILD/compile.list"
for r in "${LIBS[@]}"; do
  row "$r"
  for s in $srcs; do
    o="$(object "$s")"
    for dep in "$s" $(deps); do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then rm -f "$o"; fi
    done
    if [ ! -f "$o" ]; then echo "$(compile_flags "$s") -c $s -o $o" >> "$BUILD/compile.list"; fi
  done
done
xargs -r -P 16 -L 1 hipcc < "$BUILD/compile.list"

# link, strip, lint and report one row
build_lib() {
  row "$1"
  objs=""
  for s in $srcs; do objs="$objs $(object "$s")"; done
  if [ "$MODE" = hostonly ]; then
    # host-only objects still reference their translation unit's device image (__hip_fatbin_<id>, registered with the HIP runtime when the
    # library is loaded and parsed lazily at a first launch, which never happens here): empty images stand in for the device code that was
    # not compiled
    nm -u $objs | grep -o "__hip_fatbin_[0-9a-f]*" | sort -u |
      awk '{print "__attribute__((visibility(\"default\"), aligned(4096))) const char " $1 "[4096] = {0};"}' > "$BUILD/fatbin_stubs.c"
    /opt/rocm/lib/llvm/bin/clang -fPIC -c "$BUILD/fatbin_stubs.c" -o "$BUILD/fatbin_stubs.o"
    objs="$objs $BUILD/fatbin_stubs.o"
  fi
  hipcc $LINK -shared -fPIC -o "$out" $objs
  if [ "$name" != hsefr ] || [ "$MODE" = product ]; then
    # a shipped library goes without most of its host symbol table (.symtab / .strtab, about 70 KB of 100 in libhsefr.so): the exported
    # functions are in .dynsym and the device kernels' symbols in .hip_fatbin, both untouched; of .symtab only the kernels' host-side
    # handles stay, the data symbols from which hsefr_plan_describe reads a launched kernel's name and template arguments (engine.hip,
    # stub_names)
    /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol="$keep" --keep-symbol='!*__device_stub__*' "$out"
  fi
  if [ "$MODE" = hostonly ]; then
    hipcc $SAN_EXE_FLAGS -x c++ fuzz_plan.cc -o "$BUILD/fuzz_plan" -L"$BUILD" -lhsefr_asan -Wl,-rpath,"$(realpath $BUILD)"
  else
    # refuse a library with an unguarded gfx950 store-data hazard (see tools/isa_lint.py)
    python3 ../../tools/isa_lint.py "$out"
  fi
  echo "built $(realpath $out)"
}
for r in "${LIBS[@]}"; do build_lib "$r"; done
