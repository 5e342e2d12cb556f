// MobileNet's stem and the depthwise half of its second block in one kernel -- fourth generation (round 3):
//   conv1 3x3/2 (3 -> 32, + shift + ReLU6) -> depthwise 3x3/1 (+ scale + shift + ReLU6) -> pointwise 1x1 (32 -> 64, + shift +
//   ReLU6) -> depthwise 3x3/2 (+ scale + shift + act),                                              NHWC, gfx950.
//
// Replaces graph nodes #30-#55 (conv1 .. conv_dw_2_relu), run by tf_sess.run at facerec_test.py:120 / facial_analysis.py:109,
// and -- in the uint8 form -- the float conversion, channel reversal and mean subtraction in front of them
// (facerec_test.py:95-106, facial_analysis.py:98-107).  Same patch geometry as stem3_fused.hip (4 x 8 output pixels per
// workgroup step), same patch cursor and stages C-E (depthwise 1, pointwise, depthwise 2): stem_patch.h's, same bits for equal
// conv1 results.  What changed is everything in front of them (72.6 M VALU against 3.8 M MFMA wave-instructions,
// the im2col stage alone 3.1-3.5 k of a patch's 15 k cycles):
//
//   * NO im2col.  stem3 cut 209 rows of 27 values out of the input window with scalar LDS reads (27 ds_read_b32 + ~230 VALU
//     per thread: every input value converted 2.25 times) and wrote them back as MFMA rows.  Here the window is converted ONCE,
//     while it is parked: a thread's 16-byte piece of an image row becomes four f16 (hi) + four f16 (lo) and goes to LDS with
//     two ds_write_b64 -- the window in LDS is the image rows themselves, [row][x][rgb] as f16, hi plane and lo plane.
//   * conv1 reads its MFMA operands STRAIGHT FROM THE WINDOW.  Kernel row dy of a conv pixel is 9 consecutive values of one
//     window row (3 pixels x 3 channels), so the K = 27 contraction is laid out as two 32-deep steps whose 8-value lane slices
//     are contiguous, 4-byte-aligned 16-byte LDS reads:
//         step 0, slice dy (0..2): values 0..7 of kernel row dy        step 1, slice dy: value 8 of kernel row dy (+ 7 whose
//         slice 3: weights zero                                         weights are zero: the next pixel's bytes, finite)
//     -- the pattern of stem7x7_pool.hip.  Two steps x three products = 6 MFMAs of 16 cycles per (16 pixels x 16 channels).
//   * Columns outside the image are whole 16-byte pieces (3 * 32 is a multiple of 4): they are masked like rows outside it, by
//     an out-of-range buffer offset that returns zeros -- no per-value masks.
//   * The next patch's window is loaded during stages B-D, converted and parked during stage E (its LDS region is dead from
//     stage B's barrier on): 4 barriers per patch instead of 7.
//   * The bound check (DESIGN.md lesson 24) runs on the f16 hi halves with packed integer maxima: 1 VALU per value.
//
// uint8 form (U8 = true; SURVEY 8f-1 "fused into conv1's input read"): x is the RESIZED image as the decoder's RGB bytes
// [N,H,W,3].  A byte is exact in ONE f16, so the window has one plane and a product is two MFMAs (wh * a, wl * a).  The mean
// and the channel reversal are folded into constants: the weight image is packed channel-reversed, and
//     conv1(u8 - mean) = sum_valid w * u8  -  sum_valid w * mean          (taps on SAME padding contribute neither)
// where the second sum depends only on which taps are valid: 4 cases (pixel in the last conv row / column or not), prepared
// on the host in float64 as 4 shift vectors.  Error: products are exact, the fp32 accumulation runs over values up to 255
// instead of 151 -- the same 2^-24-scale round-off as the fp32 path (tested at the same 2e-6 bar).
//
// Shapes: H % 4 == 0 and W % 4 == 0 (no top / left padding in either stride-2 step, window rows start 8 bytes into a
// 16-byte unit for every patch); anything else takes stem3_fused.hip.
#include <type_traits>

#include "stem_patch.h"

namespace hsefr {

using namespace stem;
using namespace stem::patch;

namespace {

struct Stem4Params : PatchParams {
    const void* x;         // [N,H,W,3] fp32 (preprocessed) or uint8 RGB (U8)
    const void* cw4;       // conv1 split rows in the two-step K layout: [2 steps][32 channels][hi 32 x f16 | lo 32 x f16]
    const float* cdescale; // [32]  2^-(e_n + in_log2)
    const float* cshift;   // [32]; U8: [4][32] = shift - sum_valid w * mean for (last row ? 2 : 0) + (last column ? 1 : 0)
    int* overflow;         // set to 1 if an input value breaks the declared bound (may be null; fp32 form only)
    float in_scale;
    long long x_bytes;             // size of the whole input tensor
};

constexpr int RAWH = 2 * R0H + 1;                     // input window: 23 rows x 39 pixels
constexpr int RAWQ = 30;                              // 4-value pieces per window row (2 + 39 * 3 = 119 values -> 120)
constexpr int WRP = 256;                              // bytes per window row and plane in LDS: 120 f16 + 8 that stay zero
constexpr int WPLANE = RAWH * WRP;                    // 5888
constexpr int WSHIFT = 2;                             // a window row starts this many values into its first piece

template <int ACT, bool U8>
__global__ __launch_bounds__(256, 2) void stem4_fused_kernel(Stem4Params p) {
    // LDS: U1 = the input window as f16 (hi plane | lo plane: parked in a patch's stage E, read by the next patch's stage B),
    //      then the GEMM A tile (C-D); U2 = conv1 region (B-C), then the 96x96x64 patch (D-E)
    __shared__ __attribute__((aligned(16))) unsigned char U1[R1ROWS * 128];            // 20 KB
    static_assert(2 * WPLANE <= R1ROWS * 128, "the window planes fit in U1");
    unsigned char* Wn = U1;
    __shared__ __attribute__((aligned(16))) float U2[R1PIX * P1P];                      // 41 KB
    __shared__ __attribute__((aligned(16))) float4 W2[9 * 16];                          // depthwise-2 weights
    __shared__ __attribute__((aligned(16))) float4 W1[9 * 8];                           // depthwise-1 weights
    // per-channel constants (read where they are used: as per-thread registers they lived through every stage and spilled)
    __shared__ __attribute__((aligned(16))) float Kc[64 + 64 + 128 + 128];              // conv1 descale | shift, dw1 scale | shift (x 2^a), pointwise descale | shift, dw2 scale | shift
    __shared__ float Cv[R0ROWS];                                                        // 1 = conv1 pixel inside its map
    __shared__ float Pv[R1ROWS];                                                        // 1 = block-1 pixel inside its map
    __shared__ __attribute__((aligned(16))) float Ct[U8 ? 4 * 32 : 4];                  // U8: the four shift vectors
    __shared__ int Cc[U8 ? R0ROWS : 4];                                                 // U8: case of a conv1 pixel, times 32
    float* Co = U2;
    float* P1 = U2;
    unsigned char* As = U1;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q4 = lane >> 4;

    // ---- constants, once per workgroup ----
    if (tid < 9 * 16) W2[tid] = p.wd2[tid];
    if (tid < 9 * 8) W1[tid] = p.wd1[tid];
    if (U8 && tid < 4 * 32) Ct[tid] = p.cshift[tid];
    // (depthwise 1's scale / shift carry the 2^a_log2 pre-scale of the split: stage_dw1)
    if (tid < 32) { Kc[tid] = p.cdescale[tid]; Kc[32 + tid] = p.cshift[tid]; }
    else if (tid < 64) { Kc[32 + tid] = ((const float*)p.d1scale)[tid - 32] * p.a_scale; Kc[64 + tid] = ((const float*)p.d1shift)[tid - 32] * p.a_scale; }
    else if (tid < 128) { Kc[64 + tid] = p.descale[tid - 64]; Kc[128 + tid] = p.pshift[tid - 64]; }
    else if (tid < 192) { Kc[128 + tid] = ((const float*)p.d2scale)[tid - 128]; Kc[192 + tid] = ((const float*)p.d2shift)[tid - 128]; }
    const float cap6 = 6.f * p.a_scale;
    // conv1: lane (n = 16 nb + l16, k-slice q4) holds the weight fragments of both K steps and both channel blocks for good
    f16x8 cwh[2][2], cwl[2][2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            cwh[st][nb] = *(const f16x8*)((const unsigned char*)p.cw4 + (size_t)(st * 32 + nb * 16 + l16) * 128 + 16 * q4);
            cwl[st][nb] = *(const f16x8*)((const unsigned char*)p.cw4 + (size_t)(st * 32 + nb * 16 + l16) * 128 + 64 + 16 * q4);
        }
    }
    // pointwise: wave w owns channels 16w .. 16w+15
    const f16x8 bh = *(const f16x8*)((const unsigned char*)p.wsplit + (size_t)(wave * 16 + l16) * 128 + 16 * q4);
    const f16x8 bl = *(const f16x8*)((const unsigned char*)p.wsplit + (size_t)(wave * 16 + l16) * 128 + 64 + 16 * q4);

    // conv1 operand addresses, patch-invariant: row block ri of this wave, pixel m = 16 (rb0 + ri) + l16 (pixels past the 209th
    // repeat the last one), K slice q4 = kernel row min(q4, 2): byte offset of the slice's first value in the hi plane
    const int rb0 = (wave * 7) >> 1;
    unsigned caddr[4];
#pragma unroll
    for (int ri = 0; ri < 4; ++ri) {
        const int m = min((rb0 + ri) * 16 + l16, R0PIX - 1);
        const int ry = m / R0W, rx = m - ry * R0W;
        caddr[ri] = (unsigned)((2 * ry + min(q4, 2)) * WRP + 2 * WSHIFT + 12 * rx);
    }

    const Cur step = cursor_step(p);

    // ---- the input window of a patch: 23 rows x 30 four-value pieces (fp32: 16 bytes, uint8: 4 bytes), three per thread ----
    // A window row starts at image column iw0 = 32 tw - 2, i.e. at value 3 (row W + iw0) = 2 (mod 4) of the tensor: piece q of a
    // row holds window values 4 q - 2 .. 4 q + 1 (the first two belong to the pixel on the left and are never read).  Rows
    // outside the image and pieces that lie wholly in columns outside it (3 * 32 = 0 mod 4: a column edge is a piece edge) get
    // an out-of-range offset: the buffer returns zeros -- SAME padding costs no instruction.
    // (row, piece) of a thread's three items are re-derived from an opaque copy of the thread index where they are used: as
    // loop invariants they, and the address arithmetic hipcc hoisted with them, lived through every stage and spilled
    auto item_rq = [&](int k, int& row, int& q) __attribute__((always_inline)) {
        const int item = opaque((int)threadIdx.x) + 256 * k;
        row = item / RAWQ;
        q = item - row * RAWQ;
    };
    typedef typename std::conditional<U8, unsigned, f32x4>::type raw_t;
    raw_t rawv[3];
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, p.x_bytes);
    constexpr int VB = U8 ? 1 : 4;                    // bytes per value
    auto load_window = [&](const Cur& c) {
        const int ih0 = 4 * c.th * PH - 2, iw0 = 4 * c.tw * PW - 2;
        const int q_hi = (3 * (p.W - iw0) + WSHIFT) >> 2;        // first piece wholly right of the image
        const int q_lo = iw0 < 0 ? (3 * (-iw0) + WSHIFT) >> 2 : 0;  // pieces wholly left of it
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int row, q;
            item_rq(k, row, q);
            const int ih = ih0 + row;
            const bool ok = row < RAWH && ih >= 0 && ih < p.H && q >= q_lo && q < q_hi;
            const int first = ((c.n * p.H + ih) * p.W + iw0) * 3 - WSHIFT + 4 * q;   // value index, = 0 (mod 4); < 2^29 (launcher)
            const unsigned voff = ok ? (unsigned)(first * VB) : 0x80000000u;
            if constexpr (U8) rawv[k] = __builtin_amdgcn_raw_buffer_load_b32(rx, voff, 0, 0);
            else rawv[k] = bload16(rx, voff, 0);
        }
    };
    u16x2 amax_pk = {0, 0};
    auto park_window = [&]() {
        // the last 16 bytes of every window row are written by no piece (and the A tile passes through this memory): zero, so
        // that the step-1 reads of a row's last pixels meet finite bytes under their zero weights
        if (threadIdx.x < RAWH * (U8 ? 1 : 2)) {
            const float z = opaque(0.f);       // (a hoisted zero vector is what hipcc spilled here)
            *(f32x4*)(&Wn[threadIdx.x * WRP + WRP - 16]) = (f32x4){z, z, z, z};
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int row, q;
            item_rq(k, row, q);
            if (row < RAWH) {
                unsigned char* dst = &Wn[row * WRP + 8 * q];
                if constexpr (U8) {
                    const unsigned b = rawv[k];
                    f32x4 v;
                    v[0] = (float)(b & 255u); v[1] = (float)((b >> 8) & 255u); v[2] = (float)((b >> 16) & 255u); v[3] = (float)(b >> 24);
                    *(f16x4*)dst = __builtin_convertvector(v, f16x4);               // exact
                } else {
                    f16x4 hi, lo;
                    split(rawv[k] * p.in_scale, hi, lo);                             // (the scale is a power of two: exact)
                    *(f16x4*)dst = hi;
                    *(f16x4*)(dst + WPLANE) = lo;
                    // bound check on the hi halves: |v| < 2^15 <=> (bits & 0x7fff) < 0x7800; an Inf / NaN has all exponent bits set
                    const u32x2 hb = __builtin_bit_cast(u32x2, hi);
                    amax_pk = __builtin_elementwise_max(amax_pk, __builtin_bit_cast(u16x2, hb.x & 0x7FFF7FFFu));
                    amax_pk = __builtin_elementwise_max(amax_pk, __builtin_bit_cast(u16x2, hb.y & 0x7FFF7FFFu));
                }
            }
        }
    };
    // validity of the conv1 / block-1 pixels of a patch (read only by patches that touch the map's border)
    auto border_tables = [&](const Cur& c, int t) {
        const int y10 = 2 * c.th * PH, x10 = 2 * c.tw * PW;
        if (t < R0ROWS) {
            const int rp = t < R0PIX ? t : R0PIX - 1;
            const int ry = rp / R0W, rxx = rp - ry * R0W;
            const int cy = y10 - 1 + ry, cx = x10 - 1 + rxx;
            Cv[t] = (t < R0PIX && cy >= 0 && cy < p.H1 && cx >= 0 && cx < p.W1) ? 1.f : 0.f;
            if constexpr (U8) Cc[t] = 32 * ((cy == p.H1 - 1 ? 2 : 0) + (cx == p.W1 - 1 ? 1 : 0));
        }
        if (t < R1ROWS) {
            const int q = t < R1PIX ? t : 0;
            const int y1 = y10 + q / R1W, x1 = x10 + q % R1W;
            Pv[t] = (t < R1PIX && y1 >= 0 && y1 < p.H1 && x1 >= 0 && x1 < p.W1) ? 1.f : 0.f;
        }
    };

    unsigned t = blockIdx.x;
    if (t >= p.total) return;
    Cur cur = decode(p, t);
    load_window(cur);
    park_window();
    border_tables(cur, tid);
    __syncthreads();

    STEM_STAMP_DECL;
    while (true) {
        const unsigned tn = t + gridDim.x;
        const bool more = tn < p.total;
        const Cur nxt = advance(p, cur, step);
        const int y10 = 2 * cur.th * PH, x10 = 2 * cur.tw * PW;
        // a patch whose conv1 region lies inside the map has no pixel to zero: the validity factors are all 1 (uniform test);
        // U8: ... and strictly inside its last row / column, where the taps on the padding change the folded mean term
        const bool interior = y10 - 1 >= 0 && x10 - 1 >= 0 && y10 - 1 + R0H <= p.H1 - (U8 ? 1 : 0) && x10 - 1 + R0W <= p.W1 - (U8 ? 1 : 0);
        STEM_STAMP(0);
        const int tid = opaque((int)threadIdx.x), lane = tid & 63, l16 = lane & 15, q4 = lane >> 4, c4l = tid & 7, c4o = tid & 15;
        STEM_STAMP(7);

        // ---- stage B: conv1 straight from the window; 14 row blocks x 2 channel blocks = 28 pairs, 7 per wave ----
        // pair pr = 7 * wave + i covers row block pr >> 1, channel block pr & 1: the (row block, channel block) of slot i
        // depends on the parity of the wave only -- two unrolled variants, register indices all static
        auto conv_stage = [&](auto ODDC) __attribute__((always_inline)) {
            constexpr int ODD = decltype(ODDC)::value;
            // all fragments of the wave's four row blocks first (one LDS round trip), then the MFMAs with the seven accumulators
            // interleaved: consecutive MFMAs never depend on each other
            f16x8 ah[2][4], al[2][4];
#pragma unroll
            for (int ri = 0; ri < 4; ++ri) {
                const unsigned char* a0 = Wn + caddr[ri];
                ah[0][ri] = ((const Frag4*)(a0))->v;
                ah[1][ri] = ((const Frag4*)(a0 + 16))->v;
                if constexpr (!U8) { al[0][ri] = ((const Frag4*)(a0 + WPLANE))->v; al[1][ri] = ((const Frag4*)(a0 + WPLANE + 16))->v; }
            }
            f32x4 acc[7];
#pragma unroll
            for (int i = 0; i < 7; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int pdt = U8 ? 1 : 0; pdt < 3; ++pdt)
#pragma unroll
                    for (int i = 0; i < 7; ++i) {
                        constexpr int dummy = 0; (void)dummy;
                        const int ri = (i + ODD) >> 1, nb = (i + ODD) & 1;
                        // per K step the products in the order (wh*al, wl*ah, wh*ah) of the pointwise kernels; a byte has no lo term
                        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pdt == 1 ? cwl[st][nb] : cwh[st][nb], pdt == 0 ? al[st][ri] : ah[st][ri], acc[i], 0, 0, 0);
                    }
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                // lane: pixel m = 16 * rb + l16, channels nb*16 + 4*q4 + (0..3)   (operands swapped: weights first)
                const int ri = (i + ODD) >> 1, nb = (i + ODD) & 1;
                const int m = (rb0 + ri) * 16 + l16;
                const f32x4 ds = *(const f32x4*)(&Kc[nb * 16 + 4 * q4]);
                f32x4 sh = *(const f32x4*)(&Kc[32 + nb * 16 + 4 * q4]);
                if constexpr (U8) { if (!interior) sh = *(const f32x4*)(&Ct[Cc[m] + nb * 16 + 4 * q4]); }
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = relu6(fmaf(acc[i][e], ds[e], sh[e]));
                if (!interior) o = o * Cv[m];
                *(f32x4*)(&Co[m * COP + 4 * (nb * 4 + q4)]) = o;
            }
        };
        if (wave & 1) conv_stage(std::integral_constant<int, 1>());
        else conv_stage(std::integral_constant<int, 0>());
        STEM_STAMP(3);
        __syncthreads();     // conv1 region complete; the window is dead
        STEM_STAMP(2);
        if (more) load_window(nxt);      // next patch's window: in flight during stages C-D, parked in stage E

        // stage C: depthwise 1 -> split-f16 A tile
        stage_dw1(Co, W1, As, tid, c4l, *(const f32x4*)(&Kc[64 + 4 * c4l]), *(const f32x4*)(&Kc[96 + 4 * c4l]), cap6);
        STEM_STAMP(4);
        __syncthreads();     // A tile complete; conv1 region dead
        STEM_STAMP(2);

        // stage D: pointwise -> 96x96x64 patch
        stage_pw(As, P1, Pv, interior, wave, l16, q4, bh, bl, *(const f32x4*)(&Kc[128 + wave * 16 + 4 * q4]), *(const f32x4*)(&Kc[192 + wave * 16 + 4 * q4]));
        STEM_STAMP(5);
        __syncthreads();     // 96x96x64 patch complete; A tile dead
        STEM_STAMP(2);

        // the next patch's window (loaded during B-D) and border tables first: their LDS is dead since stage B / D of this patch,
        // and the piece registers are free before the depthwise's taps need them
        if (more) {
            park_window();
            const int ny = 2 * nxt.th * PH, nx = 2 * nxt.tw * PW;
            if (!(ny - 1 >= 0 && nx - 1 >= 0 && ny - 1 + R0H <= p.H1 - (U8 ? 1 : 0) && nx - 1 + R0W <= p.W1 - (U8 ? 1 : 0))) border_tables(nxt, tid);
        }
        STEM_STAMP(1);
        // stage E: depthwise 2 -> global
        stage_dw2<ACT>(p, cur, P1, W2, tid, c4o, *(const f32x4*)(&Kc[256 + 4 * c4o]), *(const f32x4*)(&Kc[320 + 4 * c4o]));
        STEM_STAMP(6);
        STEM_STAMP_COUNT;
        if (!more) break;
        __syncthreads();     // the 96x96x64 patch is dead; window and tables of the next patch complete
        t = tn;
        cur = nxt;
    }
    if constexpr (!U8) {
        const unsigned am = max((unsigned)amax_pk[0], (unsigned)amax_pk[1]);
        if (am >= 0x7800u && p.overflow) atomicOr(p.overflow, 1);
    }
    STEM_STAMP_FLUSH(p.stamps, (int)(threadIdx.x & 63), wave);
}

}  // namespace

HSEFR_KNOB(g_stem4_grid, "stem4_grid", 512);      // dev builds: persistent workgroups of the launch (256 = one per CU: latency experiments)

bool stem4_fused_supported(int cin, int c1, int c2, int conv_stride, int dw1_stride, int dw2_stride, int kh, int kw, int h, int w) {
    return cin == 3 && c1 == 32 && c2 == 64 && conv_stride == 2 && dw1_stride == 1 && dw2_stride == 2 && kh == 3 && kw == 3 &&
           h >= 4 && w >= 4 && h % 4 == 0 && w % 4 == 0;
}

int launch_stem4_fused(const void* x, int x_is_u8, const void* cw4, const float* cdescale, const float* cshift, const float* wd1,
                       const float* d1scale, const float* d1shift, const void* wsplit, const float* descale, const float* pshift,
                       const float* wd2, const float* d2scale, const float* d2shift, float* y, int* overflow, int n, int h, int w,
                       int in_log2, int a_log2, int act, hipStream_t s) {
    HSEFR_REQUIRE(n >= 0 && h >= 4 && w >= 4 && h % 4 == 0 && w % 4 == 0, HSEFR_ERR_INVALID,
                  "stem4_fused: %dx%d input (both edges must be multiples of 4; other sizes take stem3_fused)", h, w);
    HSEFR_REQUIRE(a_log2_ok(a_log2), HSEFR_ERR_INVALID, "stem4_fused: a_log2=%d", a_log2);
    HSEFR_REQUIRE(x_is_u8 ? in_log2 == 0 : in_log2_ok(in_log2), HSEFR_ERR_INVALID, "stem4_fused: in_log2=%d", in_log2);
    HSEFR_REQUIRE((long long)n * h * w * 12 < (1ll << 31) - 64, HSEFR_ERR_UNSUPPORTED,
                  "stem4_fused: the input batch must stay below 2 GB (its offsets travel in 32 bits, 2^31 marks a masked piece)");
    if (n == 0) return HSEFR_OK;
    Stem4Params p;
    p.x = x; p.cw4 = cw4; p.cdescale = cdescale; p.cshift = cshift; p.overflow = overflow;
    if (const int rc = fill_params(p, "stem4_fused", wd1, d1scale, d1shift, wsplit, descale, pshift, wd2, d2scale, d2shift, y, n, h, w, h / 2, w / 2,
                                   h / 4, w / 4, a_log2, s)) return rc;
    p.in_scale = ldexpf(1.f, in_log2);
    p.x_bytes = (long long)n * h * w * 3 * (x_is_u8 ? 1 : 4);
    const unsigned g = p.total < (unsigned)g_stem4_grid ? p.total : (unsigned)g_stem4_grid;      // % 8 == 0: the kernel's incremental patch cursor relies on it
#define HSEFR_STEM4(A)                                                                                   \
    do {                                                                                                 \
        if (x_is_u8) HSEFR_LAUNCH((stem4_fused_kernel<A, true>), dim3(g), dim3(256), 0, s, p);     \
        else HSEFR_LAUNCH((stem4_fused_kernel<A, false>), dim3(g), dim3(256), 0, s, p);            \
    } while (0)
    HSEFR_STEM_ACT_DISPATCH("stem4_fused", act, HSEFR_STEM4);
#undef HSEFR_STEM4
    return launch_status("stem4_fused");
}

}  // namespace hsefr
