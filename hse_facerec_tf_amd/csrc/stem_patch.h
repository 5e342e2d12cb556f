// What the fused MobileNet stems state once.  namespace stem: the vector types and one-line helpers of every generation
// (stem2_fused.hip .. stem5_stream.hip).  namespace stem::patch: the 4 x 8 patch kernels (stem2_fused.hip, stem3_fused.hip,
// stem4_fused.hip) -- their geometry, the persistent loop's patch cursor, the stages behind conv1 and the launchers' common part.
// A generation is its front end (gather / window, conv1) and its history; stages C-E of stem3 and stem4 are these functions, so
// "same operation order, same bits for equal conv1 results" holds by construction (tests/test_stem_bits_gpu.py pins the bits).
// The split-f16 vocabulary -- vector types, the split rows' swzb, relu6, split -- is f16s.h's.
#pragma once
#include "f16s.h"

namespace hsefr {
namespace stem {

using f16s::f32x4;
using f16s::f16x4;
using f16s::f16x8;
using f16s::swzb;
using f16s::relu6;
using f16s::split;
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(4))) F3 { float a, b, c; };
struct __attribute__((packed, aligned(4))) Frag4 { f16x8 v; };      // a 16-byte MFMA fragment at a 4-byte-aligned LDS address

__device__ __forceinline__ int swz32(int row, int chunk) { return row * 32 + 4 * (chunk ^ ((row >> 1) & 7) ^ ((row & 1) << 2)); }       // floats
// 4-wide fused multiply-add on vector types: lowers to two v_pk_fma_f32 (same rounding as fmaf, half the instructions);
// used where no MFMA shares the issue slots (the depthwise stages).
__device__ __forceinline__ f32x4 vfma(f32x4 a, f32x4 b, f32x4 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f32x4 as_v(float4 a) { return (f32x4){a.x, a.y, a.z, a.w}; }
// A value the compiler cannot see through.  The patch kernels take the thread index through it once per patch: every stage's LDS
// addresses are then re-derived (a few VALU) instead of being hoisted out of the loop as ~100 loop-invariant VGPRs -- which had
// the compiler spill to scratch.
template <class T>
__device__ __forceinline__ T opaque(T v) { asm volatile("" : "+v"(v)); return v; }

namespace patch {

constexpr int PH = 4, PW = 8;                         // output patch (of the stride-2 depthwise)
constexpr int R1H = 2 * PH + 1, R1W = 2 * PW + 1;     // block-1 region 9 x 17
constexpr int R1PIX = R1H * R1W;                      // 153
constexpr int R1ROWS = 160;                           // 10 MFMA row blocks of 16
constexpr int R0H = R1H + 2, R0W = R1W + 2;           // conv1 region 11 x 19
constexpr int R0PIX = R0H * R0W;                      // 209
constexpr int R0ROWS = 224;                           // 14 MFMA row blocks of 16
constexpr int COP = 36;                               // floats per pixel row of the conv1 region in LDS (32 + 4): taps sit at
                                                      // compile-time offsets from one base (no per-tap swizzle arithmetic)
constexpr int P1P = 68;                               // floats per pixel row of the 96x96x64 patch in LDS (64 + 4: rows 4 banks apart)
static_assert(R0ROWS * COP <= R1PIX * P1P, "the conv1 region fits in the 96x96x64 patch's LDS");

// What every generation's Params holds behind its own front end's fields (the launchers fill it with fill_params)
struct PatchParams {
    const float4* wd1;     // depthwise 1 [9][8] float4
    const float4* d1scale; // [8]
    const float4* d1shift; // [8]
    const float* wsplit;   // pointwise split rows [64][1][64 f16]
    const float* descale;  // [64]
    const float* pshift;   // [64]
    const float4* wd2;     // depthwise 2 [9][16] float4
    const float4* d2scale; // [16]
    const float4* d2shift; // [16]
    float* y;              // [N,OH2,OW2,64]
    int H, W, H1, W1, OH2, OW2, tiles_w, tiles_h;
    unsigned total;        // patches of the launch
    float a_scale;         // 2^a_log2
    int reverse;           // engine.hip's alternating sweep (0 for a plan's first launch, which the stem is)
    unsigned long long* stamps;    // diagnostic builds (-DHSEFR_STEM_STAMPS) only
};

// ---- patch cursor of the persistent loop (advanced with carries: no divisions in the loop) ----
struct Cur { int n, th, tw; };
__device__ __forceinline__ Cur decode(const PatchParams& p, unsigned t) {
    const unsigned lt = xcd_remap_dir(t, p.total, p.reverse);
    Cur c;
    c.tw = lt % p.tiles_w;
    c.th = (lt / p.tiles_w) % p.tiles_h;
    c.n = lt / (p.tiles_w * p.tiles_h);
    return c;
}
__device__ __forceinline__ Cur cursor_step(const PatchParams& p) {     // what one trip round the grid adds to a cursor
    const int stride_lt = gridDim.x / 8;             // launch guarantees gridDim.x % 8 == 0 whenever the kernel loops
    Cur d;
    d.tw = stride_lt % p.tiles_w; d.th = (stride_lt / p.tiles_w) % p.tiles_h; d.n = stride_lt / (p.tiles_w * p.tiles_h);
    return d;
}
__device__ __forceinline__ Cur advance(const PatchParams& p, Cur c, const Cur& d) {
    if (!p.reverse) {
        c.tw += d.tw; if (c.tw >= p.tiles_w) { c.tw -= p.tiles_w; c.th += 1; }
        c.th += d.th; if (c.th >= p.tiles_h) { c.th -= p.tiles_h; c.n += 1; }
        c.n += d.n;
    } else {
        c.tw -= d.tw; if (c.tw < 0) { c.tw += p.tiles_w; c.th -= 1; }
        c.th -= d.th; if (c.th < 0) { c.th += p.tiles_h; c.n -= 1; }
        c.n -= d.n;
    }
    return c;
}

// ---- stage C: depthwise 1.  Thread = (channel quad, run of <= 6 pixels of one region row): 3 x 8 taps read once ----
// Co: the conv1 region, W1: the depthwise-1 weights [9][8], As: the GEMM A tile (split-f16 rows).  Depthwise 1 feeds the split:
// d1sc / d1sh carry the 2^a_log2 pre-scale and cap6 = 6 * 2^a_log2 (a power of two commutes with every rounding here:
// relu6(s * sc + sh) * 2^a == clamp(s * (sc 2^a) + sh 2^a, 0, 6 * 2^a) bit for bit).
__device__ __forceinline__ void stage_dw1(const float* Co, const float4* W1, unsigned char* As, int tid, int c4l, f32x4 d1sc, f32x4 d1sh, float cap6) {
    const int grp = tid >> 3;                              // 27 runs: row = grp / 3, columns 6 * (grp % 3) ..
    if (grp < 27) {
        const int ry = grp / 3, c0 = 6 * (grp - 3 * ry);
        // row by row: 8 taps of a region row feed 6 running sums (the products of a pixel are added in the order
        // dy = 0 (dx 0,1,2), dy = 1, dy = 2 of stem2_fused.hip / dwconv.hip: same bits)
        f32x4 sum[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) sum[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            f32x4 tap[8];
#pragma unroll
            // (the last run is 5 pixels wide: its eighth tap is the next row's first pixel, read and never used --
            // all 24 addresses are one base plus a constant)
            for (int col = 0; col < 8; ++col) tap[col] = *(const f32x4*)(&Co[((ry + dy) * R0W + c0 + col) * COP + 4 * c4l]);
            const f32x4 w0 = as_v(W1[(dy * 3 + 0) * 8 + c4l]), w1 = as_v(W1[(dy * 3 + 1) * 8 + c4l]), w2 = as_v(W1[(dy * 3 + 2) * 8 + c4l]);
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                sum[j] = vfma(tap[j], w0, sum[j]);
                sum[j] = vfma(tap[j + 1], w1, sum[j]);
                sum[j] = vfma(tap[j + 2], w2, sum[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            if (c0 + j < R1W) {
                const f32x4 o = vfma(sum[j], d1sc, d1sh);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf(o[e], 0.f), cap6);
                f16x4 hi, lo;
                split(v, hi, lo);
                const int q = ry * R1W + c0 + j;
                *(f16x4*)(&As[swzb(q, c4l >> 1) + 8 * (c4l & 1)]) = hi;
                *(f16x4*)(&As[swzb(q, 4 + (c4l >> 1)) + 8 * (c4l & 1)]) = lo;
            }
        }
    }
}

// ---- stage D: pointwise on the f16 MFMA (K = 32 in one instruction); wave w = channels 16w..16w+15, all 10 row blocks ----
// As: the A tile (rows 153..159 hold stale bytes: their products are never stored), P1: the 96x96x64 patch, Pv: 1 = block-1 pixel
// inside its map (read only where !interior); bh / bl: the wave's weight fragments, pds / psh: its descale / shift.
__device__ __forceinline__ void stage_pw(const unsigned char* As, float* P1, const float* Pv, bool interior, int wave, int l16, int q4, f16x8 bh,
                                         f16x8 bl, f32x4 pds, f32x4 psh) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f16x8 ah[5], al[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            ah[i] = *(const f16x8*)(&As[swzb((5 * half + i) * 16 + l16, q4)]);
            al[i] = *(const f16x8*)(&As[swzb((5 * half + i) * 16 + l16, 4 + q4)]);
        }
        f32x4 acc[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pdt = 0; pdt < 3; ++pdt)
#pragma unroll
            for (int i = 0; i < 5; ++i)
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pdt == 1 ? bl : bh, pdt == 0 ? al[i] : ah[i], acc[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            // lane: block-1 pixel m = 16*mb + l16, channels 16*wave + 4*q4 + (0..3)
            const int m = (5 * half + i) * 16 + l16;
            if (m < R1PIX) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = relu6(fmaf(acc[i][e], pds[e], psh[e]));
                if (!interior) o = o * Pv[m];
                *(f32x4*)(&P1[m * P1P + wave * 16 + 4 * q4]) = o;
            }
        }
    }
}

// ---- stage E: depthwise 2 (stride 2) from LDS -> global; both output pixels of a thread in flight together ----
// P1: the 96x96x64 patch, W2: the depthwise-2 weights [9][16].
template <int ACT>
__device__ __forceinline__ void stage_dw2(const PatchParams& p, const Cur& cur, const float* P1, const float4* W2, int tid, int c4o, f32x4 d2sc, f32x4 d2sh) {
    const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y + (size_t)cur.n * p.OH2 * p.OW2 * 64, (long long)p.OH2 * p.OW2 * 256);
    f32x4 tp[2][9];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int px = (tid >> 4) + 16 * it, i = px >> 3, j = px & 7;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) tp[it][dy * 3 + dx] = *(const f32x4*)(&P1[((2 * i + dy) * R1W + 2 * j + dx) * P1P + 4 * c4o]);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int px = (tid >> 4) + 16 * it, i = px >> 3, j = px & 7;
        f32x4 s = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 9; ++k) s = vfma(tp[it][k], as_v(W2[k * 16 + c4o]), s);
        const f32x4 o = vfma(s, d2sc, d2sh);
        f32x4 v;
        v[0] = apply_act<ACT>(o[0]); v[1] = apply_act<ACT>(o[1]); v[2] = apply_act<ACT>(o[2]); v[3] = apply_act<ACT>(o[3]);
        const int oh = cur.th * PH + i, ow = cur.tw * PW + j;
        // a pixel outside the map gets an offset beyond the resource and the store is dropped (no branch)
        const unsigned voff = (oh < p.OH2 && ow < p.OW2) ? (unsigned)(oh * p.OW2 + ow) * 256u + 16u * c4o : 0x80000000u;
        bstore16(v, ry, voff, 0);
    }
}

// ---- the launchers' common part ----
// ranges of the power-of-two pre-scales: 2^a_log2 in front of the pointwise split, 2^in_log2 in front of conv1's
inline bool a_log2_ok(int a_log2) { return a_log2 > 0 && a_log2 <= 12; }
inline bool in_log2_ok(int in_log2) { return in_log2 >= -8 && in_log2 <= 14; }

// `kernel` names the generation in the error message
inline int fill_params(PatchParams& p, const char* kernel, const float* wd1, const float* d1scale, const float* d1shift, const void* wsplit, const float* descale,
                       const float* pshift, const float* wd2, const float* d2scale, const float* d2shift, float* y, int n, int h, int w, int h1,
                       int w1, int oh2, int ow2, int a_log2, hipStream_t s) {
    p.wd1 = (const float4*)wd1; p.d1scale = (const float4*)d1scale; p.d1shift = (const float4*)d1shift;
    p.wsplit = (const float*)wsplit; p.descale = descale; p.pshift = pshift;
    p.wd2 = (const float4*)wd2; p.d2scale = (const float4*)d2scale; p.d2shift = (const float4*)d2shift; p.y = y;
    p.H = h; p.W = w; p.H1 = h1; p.W1 = w1; p.OH2 = oh2; p.OW2 = ow2;
    p.tiles_w = (ow2 + PW - 1) / PW; p.tiles_h = (oh2 + PH - 1) / PH;
    const long long total = (long long)n * p.tiles_w * p.tiles_h;
    HSEFR_REQUIRE(total < (1ll << 31), HSEFR_ERR_UNSUPPORTED, "%s: grid too large", kernel);
    p.total = (unsigned)total;
    p.a_scale = ldexpf(1.f, a_log2);
    p.reverse = sweep_reverse();
    p.stamps = nullptr;
#ifdef HSEFR_STEM_STAMPS
    p.stamps = stamp_buffer(s);
#endif
    return HSEFR_OK;
}

// the three activations a stem kernel is instantiated for: common.h's switch (`kernel` names the generation in the error message)
#define HSEFR_STEM_ACT_DISPATCH(kernel, act, LAUNCH) HSEFR_ACT_SWITCH(act, kernel, LAUNCH)

}  // namespace patch
}  // namespace stem
}  // namespace hsefr
