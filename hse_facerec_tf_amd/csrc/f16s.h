// What the split-f16 kernels state once: the vocabulary of pwconv_f16s.hip, dwpw_f16s.hip, pwblk_stream.hip, pwconv_ps.hip, dwconv.hip's
// SPLIT instances and, through stem_patch.h, the fused stems.  (The scheme itself -- why two f16 halves, the ranges, the weight image --
// is the head comment of pwconv_f16s.hip.)
//
//   split    an fp32 value v, already scaled by 2^a_log2, is hi = f16(v), lo = f16(v - hi): v = hi + lo to 2^-22
//   row      32 values of one tile row (a pixel or an output channel, one K-tile of BK = 32 input channels) are one 128-byte "split
//            row" [hi 32 x f16 | lo 32 x f16] = eight 16-byte chunks: 0..3 hold the hi halves of k = 8 c .., 4..7 the lo halves.  In LDS
//            chunk c of row r sits at chunk position c ^ swz_key(r): the ds_read_b128 fragment reads of 32 consecutive rows and the
//            ds_write_b64 staging writes of adjacent rows (the key's row-parity term) are both free of bank conflicts
//   product  x * w ~= wh*xl + wl*xh + wh*xh, three f16 MFMAs into ONE fp32 accumulator IN THAT ORDER, whichever of the two is the
//            MFMA's first operand: the order of the three additions is part of every kernel's bits (tests/test_f16s_bits_gpu.py,
//            tests/test_stem_bits_gpu.py)
//
// Only __device__ __forceinline__ functions, types and constants.  Deliberately NOT here: anything a kernel owns -- tiling, pipelines,
// sched_group_barrier lists, epilogues, other swizzles (ringb, swz32), and the stems' single-product exact conv1 MFMAs.
#pragma once
#include "common.h"

namespace hsefr {
namespace f16s {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int BK = 32;          // input channels per K-tile = values per split row
constexpr int ROWB = 128;       // bytes per split row: 32 hi halves | 32 lo halves

// swizzle key of a tile row (depends on row & 15 only), and the byte offset of 16-B chunk `chunk` of tile row `row`: chunk ^ key, spelt
// as two exclusive-ors from the left (with the key in parentheses hipcc schedules every kernel here differently)
__device__ __forceinline__ int swz_key(int row) { return ((row >> 1) & 7) ^ ((row & 1) << 2); }
__device__ __forceinline__ int swzb(int row, int chunk) { return row * ROWB + 16 * (chunk ^ ((row >> 1) & 7) ^ ((row & 1) << 2)); }

__device__ __forceinline__ float relu6(float v) { return fminf(fmaxf(v, 0.f), 6.f); }

// the split of four scaled values (round to nearest even, twice)
__device__ __forceinline__ void split(f32x4 v, f16x4& hi, f16x4& lo) {
    hi = __builtin_convertvector(v, f16x4);
    lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), f16x4);
}

// one split quad -- values k = 4 q .. 4 q + 3 of tile row `row` -- into the tile: 8 bytes of the hi half-row, 8 of the lo half-row
__device__ __forceinline__ void put_quad(unsigned char* tile, int row, int q, f16x4 hi, f16x4 lo) {
    *(f16x4*)(tile + swzb(row, q >> 1) + 8 * (q & 1)) = hi;
    *(f16x4*)(tile + swzb(row, 4 + (q >> 1)) + 8 * (q & 1)) = lo;
}

// MFMA fragment: 16-B chunk `chunk` of tile row `row`.  The 32x32x16 step s (0 | 1) of a K-tile takes, in lane half lh, the 8 halves
// k = 16 s + 8 lh ..: chunk 2 s + lh of the hi half-row and chunk 4 + 2 s + lh of the lo half-row; the 16x16x32 MFMA takes the whole
// K-tile at once: chunks lq and 4 + lq of lane quarter lq.  (The chunk is formed at the call: formed in here, hipcc compiles
// dwpw_f16s.hip's kernels differently.)
__device__ __forceinline__ f16x8 frag(const unsigned char* tile, int row, int chunk) { return *(const f16x8*)(tile + swzb(row, chunk)); }

// The three-MFMA product, 32x32x16.  mac3: the weights are the MFMA's first operand (lane (li, lh) then holds pixel li and, in accumulator
// register r, channel acc_row(r, lh) of the 32 x 32 block); mac3_t: the activations are (pixel acc_row(r, lh), channel li).  The same
// three products in the same order either way.  Two kernels spell the same six lines out, each in one place of its own, because hipcc
// compiles them differently through a call: pwblk_stream.hip (`mfmas`) and pwconv_ps.hip (`mfma_block`, two accumulators alternating).
__device__ __forceinline__ void mac3(const f16x8& wh, const f16x8& wl, const f16x8& xh, const f16x8& xl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh, acc, 0, 0, 0);
}
__device__ __forceinline__ void mac3_t(const f16x8& xh, const f16x8& xl, const f16x8& wh, const f16x8& wl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, wh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, wh, acc, 0, 0, 0);
}
// ... and on the 16x16x32 MFMA (a whole K-tile per instruction), weights first
__device__ __forceinline__ void mac3_16(const f16x8& wh, const f16x8& wl, const f16x8& xh, const f16x8& xl, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
}

// Row (or column) of a 32 x 32 accumulator block that register r = 0..15 of lane half lh holds along the FIRST operand's dimension: four
// runs of four, 8 apart, the two lane halves 4 apart.  The other dimension's index is the lane's li = lane & 31.  (A register's run of
// four is what the epilogues park with one 16-byte LDS write: v[e] = acc[4 j + e] is rows acc_row(4 j, lh) .. + 3.)
__device__ __forceinline__ constexpr int acc_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

}  // namespace f16s
}  // namespace hsefr
