// What the LDS-DMA bf16 convolution kernels state once: conv_dma_bf16.hip (the general implicit GEMM), conv3x3_win_bf16.hip and
// conv3x3_w2_bf16.hip (the window 3x3 kernels), conv1x1_w4_bf16.hip (the four-wave 1x1 and its PROJ form); conv1x1_pair_bf16.hip
// shares the epilogue and the weight-row permutation.  All of them promise one results contract,
//
//   y = bf16( act( bf16( fma(acc, scale, shift) ) + R ) ),      R = residual | bf16(projection) | nothing
//
// and it is epilogue8 / park8 below, so "same rounding points in every kernel" holds by construction
// (tests/test_resnet50_rounding_gpu.py pins the rounding, tests/test_bf16_dma_bits_gpu.py every output bit).  A kernel keeps what is
// tuned per kernel: its loop skeleton, LDS layout, issue schedule, sched_group_barrier sequences and register pins.
#pragma once
#include "common.h"

namespace hsefr {
namespace bf16_dma {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int ROWB = 128;                 // bytes per LDS row: 64 bf16 = one K-step of one pixel / one weight row
constexpr unsigned OOR = 0x80000000u;     // a byte offset beyond every buffer resource (tensors < 2 GiB): the DMA writes zeros for it, loads return
                                          // zeros and move no bytes, stores are dropped

// ---- address helpers ----
// the row-keyed chunk swizzle (conflict-free ds_read_b128 for 16 rows that start at a multiple of 4; the four-wave kernels, whose
// fragments start anywhere, key on row & 6 instead: conv3x3_w2_bf16.hip)
__device__ __forceinline__ int swz_key(int row) { return ((row >> 1) & 7) ^ ((row & 1) << 2); }
__device__ __forceinline__ float bfround(float f) { return __uint_as_float(hsefr_bf16_bits(f) << 16); }      // round-to-nearest-even (common.h)
// the workgroup barrier WITHOUT __syncthreads()'s waits: LDS reads of the next step may stay in flight across it (conv3x3_w2_bf16.hip's
// header); the "memory" clobber keeps hipcc from moving LDS accesses over it
__device__ __forceinline__ void step_barrier() { asm volatile("s_barrier" ::: "memory"); }

// A buffer resource whose words are pinned to SGPRs: the inline-asm DMA / store take it under an "s" constraint, and with the
// parameter block behind by-reference lambdas hipcc otherwise keeps (selects between) resources in VGPRs -- which assembles to
// an invalid instruction, not to a waterfall loop.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_sgpr(const void* ptr, long long bytes) {
    const unsigned long long a = (unsigned long long)ptr;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const unsigned n = __builtin_amdgcn_readfirstlane(bytes <= 0 ? 0u : (bytes > 0xffffffffll ? 0xffffffffu : (unsigned)bytes));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((unsigned long long)hi << 32) | lo), 0, n, 0x00020000);
}

// LDS row R of a weight image <-> output channel, per 32 channels (the four-wave kernels and the pair): rows 16 b + i of a pair of
// 16-row blocks hold channel 8 (i >> 2) + 4 b + (i & 3), so that with the weights as the first MFMA operand accumulator element e
// of block b in lane (l16, lq) is channel 8 lq + 4 b + e -- a lane owns 8 CONSECUTIVE channels per pair of blocks: 16-byte stores
// straight from the accumulators.  (conv_dma / conv3x3_win keep the rows in natural order and read them permuted instead.)
__device__ __forceinline__ int perm_channel(int R) {
    const int i = R & 15, b = (R >> 4) & 1;
    return (R & ~31) + 8 * (i >> 2) + 4 * b + (i & 3);
}

// ---- the LDS-DMA piece: 64 lanes x 16 bytes from r[voff (+ soff)] to the KiB at lds_addr (uniform; M0 carries it) ----
// Two assembler forms: the literal 0 costs the kernels without a uniform offset no SGPR and no move; conv_dma passes its soff.
__device__ __forceinline__ void dma_piece(const __amdgpu_buffer_rsrc_t& r, unsigned lds_addr, unsigned voff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff), "s"(r)
                 : "memory", "m0");
}
__device__ __forceinline__ void dma_piece(const __amdgpu_buffer_rsrc_t& r, unsigned lds_addr, unsigned voff, unsigned soff) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(__builtin_amdgcn_readfirstlane(lds_addr)), "v"(voff),
                 "s"(r), "s"(__builtin_amdgcn_readfirstlane(soff))
                 : "memory", "m0");
}

// ---- a tile's epilogue constants ----
// By LDS-DMA into 2 KiB at lds_dst: scale[n0 .. n0 + 127] as lanes 0-31 of one piece, shift[..] as lanes 32-63 of a second one (the
// other lanes' offsets are out of range: zeros).  One loader wave issues them AHEAD of a step's pieces, so that step's counted
// wait covers them; the kernels keep two copies by tile parity.
__device__ __forceinline__ void stage_scale_shift(const __amdgpu_buffer_rsrc_t& r_scale, const __amdgpu_buffer_rsrc_t& r_shift, unsigned lds_dst, int lane) {
    dma_piece(r_scale, lds_dst, lane < 32 ? 16u * lane : OOR);
    dma_piece(r_shift, lds_dst + 1024, lane >= 32 ? 16u * (unsigned)(lane - 32) : OOR);
}
struct ScaleShift { f32x4 sc, sh; };
// ... and four channels' constants read back from that layout (shift: the second KiB, behind the 32 lanes x 16 bytes of zeros)
__device__ __forceinline__ ScaleShift read_scale_shift(const unsigned char* consts, int channel) {
    return ScaleShift{*(const f32x4*)(consts + channel * 4), *(const f32x4*)(consts + 1024 + 512 + channel * 4)};
}

// ---- the epilogue of the eight consecutive channels a lane owns: accumulators a0 (channels 0-3, constants c0) and a1 (4-7, c1) ----
// Its three stages, in the contract's order.  conv3x3_w2 loads its residual inside its own `if` and calls them one by one; conv_dma
// spells the first two out and says why.
__device__ __forceinline__ void scale_shift8(float (&v)[8], const f32x4& a0, const f32x4& a1, const ScaleShift& c0, const ScaleShift& c1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(a0[e], c0.sc[e], c0.sh[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 + e] = fmaf(a1[e], c1.sc[e], c1.sh[e]);
}
// res: the residual's four packed bf16 pairs
__device__ __forceinline__ void add_residual8(float (&v)[8], const f32x4& res) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const unsigned rw = __float_as_uint(res[d]);
        v[2 * d] = bfround(v[2 * d]) + __uint_as_float(rw << 16);
        v[2 * d + 1] = bfround(v[2 * d + 1]) + __uint_as_float(rw & 0xFFFF0000u);
    }
}
// -> the four packed bf16 pairs to store
__device__ __forceinline__ f32x4 clamp_pack8(const float (&v)[8], float act_lo, float act_hi) {
    f32x4 o;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const float f0 = fminf(fmaxf(v[2 * d], act_lo), act_hi), f1 = fminf(fmaxf(v[2 * d + 1], act_lo), act_hi);
        o[d] = __uint_as_float(hsefr_pack_bf16x2(f0, f1));
    }
    return o;
}
__device__ __forceinline__ f32x4 epilogue8(const f32x4& a0, const f32x4& a1, const ScaleShift& c0, const ScaleShift& c1, bool has_res, const f32x4& res,
                                           float act_lo, float act_hi) {
    float v[8];
    scale_shift8(v, a0, a1, c0, c1);
    if (has_res) add_residual8(v, res);
    return clamp_pack8(v, act_lo, act_hi);
}
// The projected shortcut's eight channels, scaled, shifted and rounded to bf16 where its tensor used to be stored: parked as the packed
// pairs epilogue8 takes for its residual.
__device__ __forceinline__ f32x4 park8(const f32x4& a0, const f32x4& a1, const ScaleShift& c0, const ScaleShift& c1) {
    float v[8];
    scale_shift8(v, a0, a1, c0, c1);
    f32x4 o;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = __uint_as_float(hsefr_pack_bf16x2(v[2 * d], v[2 * d + 1]));
    return o;
}

// ---- the persistent tile walk: workgroup b of g takes tiles b, b + g, ...; past its last tile the prefetch cursors stay on it ----
__device__ __forceinline__ unsigned tiles_of_workgroup(unsigned total) { return (total - blockIdx.x + gridDim.x - 1) / gridDim.x; }
__device__ __forceinline__ unsigned tile_index(unsigned i, unsigned ntile, unsigned total, int reverse) {
    return xcd_remap_dir(blockIdx.x + (i < ntile ? i : ntile - 1) * gridDim.x, total, reverse);
}

// ---- host side ----
// clamp bounds of an activation: (-inf, +inf) none, (0, +inf) ReLU, (0, 6) ReLU6
inline int act_bounds(int act, const char* name, float* lo, float* hi) {
    HSEFR_REQUIRE(act == HSEFR_ACT_NONE || act == HSEFR_ACT_RELU || act == HSEFR_ACT_RELU6, HSEFR_ERR_UNSUPPORTED, "%s: act %d", name, act);
    *lo = act == HSEFR_ACT_NONE ? -INFINITY : 0.f;
    *hi = act == HSEFR_ACT_RELU6 ? 6.f : INFINITY;
    return HSEFR_OK;
}
// one persistent workgroup per CU: tile indices are 32-bit
inline int persistent_grid(long long total, const char* name, unsigned* total_tiles, unsigned* grid) {
    HSEFR_REQUIRE(total < (1ll << 31), HSEFR_ERR_UNSUPPORTED, "%s: too many tiles", name);
    *total_tiles = (unsigned)total;
    *grid = (unsigned)(total < 256 ? total : 256);
    return HSEFR_OK;
}

// ---- stamps.  Diagnostic build only (HSEFR_DEV=1 HSEFR_EXTRA_FLAGS=-DHSEFR_CD_STAMPS build.sh): per-wave s_memtime sums of the step
// phases, 8 words per wave (six phases, the wave's lifetime, its step count) for the first 256 workgroups; tools/cd_stamps.py reads them ----
#ifdef HSEFR_CD_STAMPS
#define BF16_STAMP_ARRAY(stamps, waves) __device__ unsigned long long stamps[256 * (waves) * 8]
#define BF16_STAMP_SYMBOL(stamps) HIP_SYMBOL(stamps), sizeof(stamps)
#define BF16_STAMP_DECL unsigned long long st[6] = {0, 0, 0, 0, 0, 0}; unsigned long long tprev = __builtin_amdgcn_s_memtime(); const unsigned long long tstart = tprev
#define BF16_STAMP(i) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); st[i] += _t - tprev; tprev = _t; } while (0)
#define BF16_STAMP_FLUSH(stamps, waves) do { if (lane == 0 && blockIdx.x < 256) { unsigned long long* o = stamps + (blockIdx.x * (waves) + wave) * 8; \
    for (int i_ = 0; i_ < 6; ++i_) o[i_] = st[i_]; o[6] = __builtin_amdgcn_s_memtime() - tstart; o[7] = nsteps; } } while (0)
#else
#define BF16_STAMP_ARRAY(stamps, waves) static_assert(true, "")
#define BF16_STAMP_SYMBOL(stamps) nullptr, 0
#define BF16_STAMP_DECL do { } while (0)
#define BF16_STAMP(i) do { } while (0)
#define BF16_STAMP_FLUSH(stamps, waves) do { } while (0)
#endif
// read_*_stamps: read_stamps_impl(BF16_STAMP_SYMBOL(array), "read_*_stamps", host_out, bytes)
inline int read_stamps_impl(const void* symbol, size_t capacity, const char* name, void* host_out, size_t bytes) {
    if (!symbol) {
        set_error("%s: library built without -DHSEFR_CD_STAMPS", name);
        return HSEFR_ERR_UNSUPPORTED;
    }
    HSEFR_REQUIRE(bytes <= capacity, HSEFR_ERR_INVALID, "%s: too many bytes", name);
    HSEFR_HIP_CHECK(hipMemcpyFromSymbol(host_out, symbol, bytes));
    return HSEFR_OK;
}

}  // namespace bf16_dma
}  // namespace hsefr
