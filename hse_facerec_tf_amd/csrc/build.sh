#!/bin/bash
# Builds libhsefr.so for gfx950 in-tree (hipcc cross-compiles without a GPU), and right after it libhsefr_album.so (include/hsefr_album.h:
# the album organiser's device code, a library of its own because libhsefr.so is held below 4 MB by its tests) and libhsefr_frames.so
# (include/hsefr_frames.h: the frame stack's channel swap and quarter turns, a library of its own for the same reason) and
# libhsefr_forest.so (include/hsefr_forest.h: the random forest classifier, a fourth library for the same reason) and
# libhsefr_ragged.so (include/hsefr_ragged.h: the detector pass over frames of different sizes, a fifth library for the same reason) and
# libhsefr_mixed.so (include/hsefr_mixed.h: the frames of such a pass turned, converted and cropped on the device, a sixth library for the
# same reason) and libhsefr_split.so (include/hsefr_split.h: the same-photo split of every cluster of a clustering in one pass, a seventh
# library for the same reason) and libhsefr_geom.so (include/hsefr_geom.h: centroid, median and Ward linkage, an eighth library for the
# same reason).
#   HSEFR_DEV=1 build.sh   builds libhsefr_dev.so instead: the same sources with -DHSEFR_DEV (tuning knobs as run-time
#                          variables, hsefr_debug_*, the calibration kernels of devtools.hip) -- for tools/kbench.py only.
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
# libhsefr_album.so: its own source list, the same flags in every mode (no -DHSEFR_DEV code in it).  -ffp-contract=off: album.hip computes
# OpenCV's resize taps in the kernel, where a product fused with the subtraction behind it would round once instead of twice
ALBUM_SRCS="album.hip"
ALBUM_FLAGS="$FLAGS $DEVICE_STRIP -ffp-contract=off"
# libhsefr_frames.so (include/hsefr_frames.h: the frames of a pass turned upright and converted to RGB on the device): a third library for
# the same reason, built as the second -- its own source list, the same flags in every mode
FRAMES_SRCS="frames.hip"
FRAMES_FLAGS="$FLAGS $DEVICE_STRIP"
# libhsefr_forest.so (include/hsefr_forest.h: the random forest fitted and applied on the device): a fourth library, built as the third.
# -ffp-contract=off: a candidate's score and a threshold are the restatement's fp64 operations one by one (tests/random_forest_ref.py)
FOREST_SRCS="forest.hip"
FOREST_FLAGS="$FLAGS $DEVICE_STRIP -ffp-contract=off"
# libhsefr_ragged.so (include/hsefr_ragged.h: one detector pass over frames of different sizes): a fifth library, built as the fourth.
# The flags are libhsefr.so's own: mtcnn_ragged.hip compiles the one-frame bodies that library compiles (mtcnn_post_frame.h,
# area_resize_px.h) and must give their bits
RAGGED_SRCS="mtcnn_ragged.hip"
RAGGED_FLAGS="$FLAGS $DEVICE_STRIP"
# libhsefr_mixed.so (include/hsefr_mixed.h: a mixed-size pass's frames turned and converted, and its faces cut, on the device): a sixth
# library, built as the fifth.  It compiles the per-pixel bodies of album.hip and frames.hip (cv_linear_px.h, frames_px.h) and must give
# their bits.  -ffp-contract=off: the crop taps are two separately rounded operations, as in album.hip
MIXED_SRCS="mixed_frames.hip"
MIXED_FLAGS="$FLAGS $DEVICE_STRIP -ffp-contract=off"
# libhsefr_split.so (include/hsefr_split.h: the same-photo split of every cluster of a clustering in one pass): a seventh library, built
# as the sixth.  The flags are libhsefr.so's own, as the fifth's: group_split.hip compiles the clustering distance that library compiles
# (linkage_scan.h's feat_tile over mfma_dot.h) and must give its bits
SPLIT_SRCS="group_split.hip"
SPLIT_FLAGS="$FLAGS $DEVICE_STRIP"
# libhsefr_geom.so (include/hsefr_geom.h: centroid, median and Ward linkage): an eighth library, built as the seventh.  The flags are
# libhsefr.so's own plus -DHSEFR_GEOM_LIB: besides geom_linkage.hip it compiles hier_linkage.hip a second time (the working matrix over
# linkage_scan.h's feat_tile, which must give libhsefr.so's bits, and the rounds with Ward's rule); its objects carry a geom_ prefix so
# that they do not replace libhsefr.so's.  The three update rules switch contraction off themselves (geom_rules.h), as lw2 does
GEOM_SRCS="geom_linkage.hip hier_linkage.hip"
GEOM_FLAGS="$FLAGS $DEVICE_STRIP -DHSEFR_GEOM_LIB"
LINT=1
HOST_STRIP=0
HOST_SIZE_FLAGS=""
if [ "${HSEFR_ASAN:-0}" = "1" ]; then
  # HSEFR_ASAN=1 build.sh   the HOST half of the same sources under the address + undefined-behaviour sanitizers (no device code is
  #                         compiled and none runs: GPU sanitizers are not available on this pool) -> build_asan/libhsefr_asan.so +
  #                         build_asan/fuzz_plan, the driver tests/test_plan_blob_fuzz_cpu.py runs.  The compiler flags of that mode live
  #                         in build_asan_flags.sh, which .gpurunignore keeps off the GPU boxes (their launcher refuses any tree whose
  #                         build scripts mention a sanitizer): a CPU-only recipe.
  OUT=build_asan/libhsefr_asan.so; BUILD=build_asan; LINT=0
  . ./build_asan_flags.sh
elif [ "${HSEFR_DEV:-0}" = "1" ]; then
  OUT=../libhsefr_dev.so; BUILD=build_dev; SRCS="$SRCS stem_fused.hip conv3x3_win_bf16.hip devtools.hip"; FLAGS="$FLAGS -DHSEFR_DEV $DEVICE_STRIP"
else
  # the product also ships without most of its host symbol table (.symtab / .strtab, about 70 KB of 100): the exported functions are in
  # .dynsym and the device kernels' symbols in .hip_fatbin, both untouched; of .symtab only the kernels' host-side handles stay, the data
  # symbols from which hsefr_plan_describe reads a launched kernel's name and template arguments (engine.hip, stub_names)
  # and the HOST half of every source but engine.hip (the forward call itself) is optimised for size: launchers and argument checks,
  # 28 KB less of them.  -Xarch_host reaches the host compilation only: the device side keeps -O3 and its code objects hold the same
  # instructions as without the flag
  OUT=../libhsefr.so; BUILD=build; FLAGS="$FLAGS $DEVICE_STRIP"; HOST_STRIP=1; HOST_SIZE_FLAGS="-Xarch_host -Os"
fi
OBJS=""
PIDS=""
mkdir -p "$BUILD"
for s in $SRCS; do
  o="$BUILD/${s%.hip}.o"
  # an object is stale against its source, EVERY header here (by glob: a new header needs no edit of this line), the public header and this script
  stale=0
  for dep in "$s" *.h ../../include/hsefr.h build.sh; do
    if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
  done
  if [ "$stale" = 1 ]; then
    rm -f "$o"
    host_flags="$HOST_SIZE_FLAGS"
    if [ "$s" = engine.hip ]; then host_flags=""; fi
    hipcc $FLAGS $host_flags ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o" &
    PIDS="$PIDS $!"
  fi
  OBJS="$OBJS $o"
done
for pid in $PIDS; do wait "$pid"; done     # a failed compile fails the build (set -e)
if [ "$LINT" = "0" ]; then
  # host-only objects still reference their translation unit's device image (__hip_fatbin_<id>, registered with the HIP runtime when the
  # library is loaded and parsed lazily at a first launch, which never happens here): empty images stand in for the device code that was
  # not compiled
  nm -u $OBJS | grep -o "__hip_fatbin_[0-9a-f]*" | sort -u |
    awk '{print "__attribute__((visibility(\"default\"), aligned(4096))) const char " $1 "[4096] = {0};"}' > "$BUILD/fatbin_stubs.c"
  /opt/rocm/lib/llvm/bin/clang -fPIC -c "$BUILD/fatbin_stubs.c" -o "$BUILD/fatbin_stubs.o"
  OBJS="$OBJS $BUILD/fatbin_stubs.o"
fi
hipcc $LINK -shared -fPIC -o "$OUT" $OBJS
if [ "$HOST_STRIP" = "1" ]; then
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN5hsefr*_kernel*' --keep-symbol='!*__device_stub__*' "$OUT"
fi
if [ "$LINT" = "1" ]; then
  # refuse a library with an unguarded gfx950 store-data hazard (see tools/isa_lint.py)
  python3 ../../tools/isa_lint.py "$OUT"
else
  hipcc $SAN_EXE_FLAGS -x c++ fuzz_plan.cc -o "$BUILD/fuzz_plan" -L"$BUILD" -lhsefr_asan -Wl,-rpath,"$(realpath $BUILD)"
fi
echo "built $(realpath $OUT)"
if [ "$LINT" = "1" ]; then
  # the second library (product and development builds alike; the host-only sanitizer recipe above has nothing of it): built, stripped
  # and linted as the first
  ALBUM_OUT=../libhsefr_album.so
  ALBUM_OBJS=""
  for s in $ALBUM_SRCS; do
    o="$BUILD/${s%.hip}.o"
    stale=0
    for dep in "$s" cv_linear_px.h ../../include/hsefr_album.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $ALBUM_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    ALBUM_OBJS="$ALBUM_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$ALBUM_OUT" $ALBUM_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$ALBUM_OUT"
  python3 ../../tools/isa_lint.py "$ALBUM_OUT"
  echo "built $(realpath $ALBUM_OUT)"
  # the third library: built, stripped and linted as the second
  FRAMES_OUT=../libhsefr_frames.so
  FRAMES_OBJS=""
  for s in $FRAMES_SRCS; do
    o="$BUILD/${s%.hip}.o"
    stale=0
    for dep in "$s" frames_px.h ../../include/hsefr_frames.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $FRAMES_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    FRAMES_OBJS="$FRAMES_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$FRAMES_OUT" $FRAMES_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$FRAMES_OUT"
  python3 ../../tools/isa_lint.py "$FRAMES_OUT"
  echo "built $(realpath $FRAMES_OUT)"
  # the fourth library: built, stripped and linted as the third
  FOREST_OUT=../libhsefr_forest.so
  FOREST_OBJS=""
  for s in $FOREST_SRCS; do
    o="$BUILD/${s%.hip}.o"
    stale=0
    for dep in "$s" ../../include/hsefr_forest.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $FOREST_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    FOREST_OBJS="$FOREST_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$FOREST_OUT" $FOREST_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$FOREST_OUT"
  python3 ../../tools/isa_lint.py "$FOREST_OUT"
  echo "built $(realpath $FOREST_OUT)"
  # the fifth library: built, stripped and linted as the fourth; stale against the headers it shares with libhsefr.so too
  RAGGED_OUT=../libhsefr_ragged.so
  RAGGED_OBJS=""
  for s in $RAGGED_SRCS; do
    o="$BUILD/${s%.hip}.o"
    stale=0
    for dep in "$s" mtcnn_post_frame.h area_resize_px.h ../../include/hsefr_ragged.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $RAGGED_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    RAGGED_OBJS="$RAGGED_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$RAGGED_OUT" $RAGGED_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$RAGGED_OUT"
  python3 ../../tools/isa_lint.py "$RAGGED_OUT"
  echo "built $(realpath $RAGGED_OUT)"
  # the sixth library: built, stripped and linted as the fifth; stale against the headers it shares with the second and the third too
  MIXED_OUT=../libhsefr_mixed.so
  MIXED_OBJS=""
  for s in $MIXED_SRCS; do
    o="$BUILD/${s%.hip}.o"
    stale=0
    for dep in "$s" cv_linear_px.h frames_px.h ../../include/hsefr_mixed.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $MIXED_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    MIXED_OBJS="$MIXED_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$MIXED_OUT" $MIXED_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$MIXED_OUT"
  python3 ../../tools/isa_lint.py "$MIXED_OUT"
  echo "built $(realpath $MIXED_OUT)"
  # the seventh library: built, stripped and linted as the sixth; stale against the headers it shares with libhsefr.so too
  SPLIT_OUT=../libhsefr_split.so
  SPLIT_OBJS=""
  for s in $SPLIT_SRCS; do
    o="$BUILD/${s%.hip}.o"
    stale=0
    for dep in "$s" linkage_scan.h mfma_dot.h common.h ../../include/hsefr.h ../../include/hsefr_split.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $SPLIT_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    SPLIT_OBJS="$SPLIT_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$SPLIT_OUT" $SPLIT_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$SPLIT_OUT"
  python3 ../../tools/isa_lint.py "$SPLIT_OUT"
  echo "built $(realpath $SPLIT_OUT)"
  # the eighth library: built, stripped and linted as the seventh; stale against the headers it shares with libhsefr.so too
  GEOM_OUT=../libhsefr_geom.so
  GEOM_OBJS=""
  for s in $GEOM_SRCS; do
    o="$BUILD/geom_${s%.hip}.o"
    stale=0
    for dep in "$s" hier_build.h geom_rules.h linkage_scan.h mfma_dot.h common.h ../../include/hsefr.h ../../include/hsefr_geom.h build.sh; do
      if [ ! -f "$o" ] || [ "$dep" -nt "$o" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
      rm -f "$o"
      hipcc $GEOM_FLAGS -Xarch_host -Os ${HSEFR_EXTRA_FLAGS:-} -c "$s" -o "$o"
    fi
    GEOM_OBJS="$GEOM_OBJS $o"
  done
  hipcc $LINK -shared -fPIC -o "$GEOM_OUT" $GEOM_OBJS
  /opt/rocm/lib/llvm/bin/llvm-strip --strip-all -w --keep-symbol='_ZN*_kernel*' --keep-symbol='!*__device_stub__*' "$GEOM_OUT"
  python3 ../../tools/isa_lint.py "$GEOM_OUT"
  echo "built $(realpath $GEOM_OUT)"
fi
