// conv_pw_2 and the 48 x 48 depthwise-pointwise block behind it as ONE row-streaming launch, NHWC fp32, gfx950:
//
//   x [n,H,W,64] (ReLU6-bounded) -> pointwise 64 -> 128 + shift + ReLU6 -> depthwise 3x3 stride 1 SAME + scale + shift + ReLU6
//                                -> pointwise 128 -> 128 + shift + act -> y [n,H,W,128]
//
// (graph nodes Conv2D 1x1 ... Maximum of conv_pw_2, then DepthwiseConv2dNative ... Maximum of conv_dw_3 / conv_pw_3, run by tf_sess.run at
// facerec_test.py:120 / facial_analysis.py:109.)  As two launches (pwconv_f16s.hip, then dwpw_f16s.hip) the 128-channel tensor between
// them is written and read back: at batch 256 x 192 that is 302 + 305 MB of the 1068 MB the two launches move.  Here it lives in LDS, one
// map row at a time.  A map row (W <= 48 pixels) is the whole width, so a kernel that walks DOWN the image needs no halo in either
// direction: every conv_pw_2 pixel is computed exactly once per work item.
//
// One persistent workgroup of 8 waves per CU.  A work item is (image, row segment); its rows form one flat sequence with the rows of
// the workgroup's other items.  A segment of output rows [r0, r1) takes the conv_pw_2 rows r0 - 1 .. r1 (a segment inside the map
// recomputes one row above and one below itself; rows outside the map are ZERO rows that go through the same arithmetic).  Row k of the
// flat sequence passes through four stages, one step (= one workgroup barrier) apart:
//   step k      producers   the input row (16-byte buffer loads issued one step earlier) x 2^a_log2 -> f16 hi / lo -> stage A2
//   step k + 1  consumers   conv_pw_2: A2 x resident weight fragments on the MFMA -> descale, shift, ReLU6 -> fp32 row in the LDS ring
//                           (two rows of W + 2 cells: the cells at x = -1 and x = W stay zero)
//   step k + 2  producers   depthwise: the newest ring row adds its three taps to the partial sums a lane keeps in registers
//                           (top + middle of the row below, top of the row after that), closes the row above -> scale, shift, ReLU6,
//                           x 2^a_log2 -> f16 hi / lo -> stage A3
//   step k + 3  consumers   conv_pw_3: A3 x resident weight fragments -> wave-private scratch -> 128-byte-line stores, issued between
//                           the K-steps of the same step's conv_pw_2 product
// The four PRODUCER waves (one per SIMD) own the vector ALU work, the four CONSUMER waves the matrix work: consumer c holds the split
// weight rows of output channels [32 c, 32 c + 32) of BOTH pointwise layers in registers for the life of the workgroup (96 VGPRs) and
// runs the products with the weights FIRST, so a lane ends up with four runs of four consecutive channels of one pixel.
//
// Bit for bit the two launches: per pointwise product the K-steps of 16 ascend, and each adds wh*al, wl*ah, wh*ah to ONE accumulator
// (pwconv_f16s.hip's step; dwpw_f16s.hip's stride-2 kernel shows that swapping the MFMA operands keeps the bits); the depthwise forms
// t = x0*w0, fma(x1,w1,t), fma(x2,w2,t) per input row, (row0 + row1) + row2, fma(sum, scale, shift), ReLU6, x 2^a_log2, hi = f16(v),
// lo = f16(v - hi) (dwpw3_f16s_kernel's producer).  A row's arithmetic does not depend on the segment it is in, nor on the batch.
// LDS: ring 2 x 25.6 KB + A2 2 x 12 KB + A3 2 x 24 KB + scratch 4 x 8 KB + 1 KB constants + 1 KB item table = 156 KB.
// Row layout, split and product: f16s.h.
#include "f16s.h"

#ifndef PB_ABLATE
#define PB_ABLATE 0     // knock-out builds (tools/build_ko.sh; timing only, wrong results): 1 no products, 2 no depthwise, 4 no input loads / split, 8 no stores
#endif
namespace hsefr {

namespace {

using namespace f16s;

constexpr int PB_CIN = 64, PB_C = 128, PB_COUT = 128;   // the one shape: conv_pw_2 64 -> 128, block 128 -> 128
constexpr int PB_WMAX = 48;                             // widest map row the LDS budget takes
constexpr unsigned PB_GRID = 256;                       // persistent workgroups: one per CU of the MI355X
constexpr int PB_CELLB = PB_C * 4;                      // a ring cell: one pixel's 128 fp32 channels
constexpr int PB_RING = (PB_WMAX + 2) * PB_CELLB;       // one ring row
constexpr int PB_KT = PB_WMAX * ROWB;                // one K-tile (32 channels) of a stage: 48 pixel rows of 128 B
constexpr int PB_A2 = (PB_CIN / 32) * PB_KT, PB_A3 = (PB_C / 32) * PB_KT;
// (the second 32-pixel column block reads pixel rows 32..63 of a K-tile: rows 48..63 are the next K-tile's, the next stage's or -- behind
// the last A3 stage -- the scratch's first bytes: finite or not, a column of the product depends on its own pixel row alone and columns
// beyond W are never stored)
constexpr int PB_A2_OFF = 2 * PB_RING, PB_A3_OFF = PB_A2_OFF + 2 * PB_A2, PB_S_OFF = PB_A3_OFF + 2 * PB_A3;
constexpr int PB_ITEMS = 64;                            // items per workgroup and launch (their table sits in LDS; the launcher deals larger batches out over launches)
constexpr int PB_E_OFF = PB_S_OFF + 4 * 8192, PB_T_OFF = PB_E_OFF + 2 * PB_C * 4, PB_LDS = PB_T_OFF + PB_ITEMS * 16;
static_assert(PB_LDS <= 160 * 1024, "LDS budget");

struct PwBlkParams {
    const float* x;         // [n,H,W,64]
    const float* w2;        // conv_pw_2 split rows [128][2][64 f16]
    const float* ds2;       // its descale, shift [128]
    const float* sh2;
    const f32x4* wd;        // depthwise [9][32]
    const f32x4* dscale;    // [32]
    const f32x4* dshift;
    const float* w3;        // conv_pw_3 split rows [128][4][64 f16]
    const float* ds3;
    const float* sh3;
    float* y;               // [n,H,W,128]
    int nimg, H, W, S;      // S: row segments per image
    unsigned total;         // nimg * S work items
    float a_scale2, a_scale3;
    int reverse;            // sweep direction (common.h)
    int act;                // conv_pw_3's activation: HSEFR_ACT_NONE | _RELU | _RELU6
    hsefr_udiv kS;          // exact division by S (S >= 2)
};

// ring cell `cell` (pixel + 1), 16-byte chunk `chunk` (channel quad): eight neighbouring cells spread one chunk over 128 contiguous bytes
__device__ __forceinline__ int ringb(int cell, int chunk) { return cell * PB_CELLB + 16 * (chunk ^ (cell & 7)); }

// One instantiation: a row is always two 32-pixel column blocks (rows of at most 32 pixels compute a block they never store) and the last
// activation is a run-time choice between three uniform branches -- the product library has no room for six copies of this kernel
// (tests/test_abi_cpu.py keeps it below 4 MB).
constexpr int NB = 2;

__global__ __launch_bounds__(512, 1) void pwblk_stream_f16s_kernel(PwBlkParams p) {
    __shared__ __attribute__((aligned(1024))) unsigned char smem[PB_LDS];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W;
    const unsigned OOB = 0xFFFFFFF0u;
    for (int i = tid; i < 2 * PB_RING / 16; i += 512) ((f32x4*)smem)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
        float* el = (float*)(smem + PB_E_OFF);
        if (tid < PB_C) { el[tid] = p.ds2[tid]; el[PB_C + tid] = p.sh2[tid]; }
    }
    // the workgroup's items and their rows: item i is image n, output rows r0 .., R = rows + 2 conv_pw_2 rows (decoded once, into LDS); a
    // cursor is (item ordinal, row s of the item's R): row s is map row r0 - 1 + s.  Past the end a cursor stays on the last item.
    const unsigned nitem = (p.total - blockIdx.x + gridDim.x - 1) / gridDim.x;
    int* itab = (int*)(smem + PB_T_OFF);
    if (tid < (int)nitem) {
        const unsigned lt = xcd_remap_dir(blockIdx.x + (unsigned)tid * gridDim.x, p.total, p.reverse);
        const bool one = p.S == 1;
        const unsigned n = one ? lt : hsefr_udiv_do(lt, p.kS), seg = lt - n * (unsigned)p.S;
        const int r0 = one ? 0 : (int)hsefr_udiv_do(seg * (unsigned)H, p.kS);
        itab[4 * tid] = (int)n;
        itab[4 * tid + 1] = r0;
        itab[4 * tid + 2] = (one ? H : (int)hsefr_udiv_do((seg + 1u) * (unsigned)H, p.kS)) - r0 + 2;
    }
    __syncthreads();
    struct Cur { unsigned i; int s, R, n, r0; };
    auto open = [&](Cur& c) {
        const int* e = itab + 4 * (c.i < nitem ? c.i : nitem - 1);
        c.n = __builtin_amdgcn_readfirstlane(e[0]);
        c.r0 = __builtin_amdgcn_readfirstlane(e[1]);
        c.R = __builtin_amdgcn_readfirstlane(e[2]);
        c.s = 0;
    };
    auto next = [&](Cur& c) {
        if (++c.s == c.R) { ++c.i; open(c); }
    };
    int nflat = 0;
    for (unsigned i = 0; i < nitem; ++i) nflat += __builtin_amdgcn_readfirstlane(itab[4 * i + 2]);
    const int nsteps = nflat + 3;
    __syncthreads();

    if (wave < 4) {
        // =============================== producers: input split + depthwise ===============================
        const __amdgpu_buffer_rsrc_t rx = make_rsrc(p.x, (long long)p.nimg * H * W * PB_CIN * 4);
        // input row: W x 16 quads of 16 bytes, three per lane; quad i = pixel i / 16, channels 4 (i % 16) ..
        unsigned xv[3];
        int a2o[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = tid + 256 * j;
            xv[j] = i < W * 16 ? (unsigned)i * 16u : OOB;
            const int cq = i & 15, skq = cq & 7;
            a2o[j] = (cq >> 3) * PB_KT + swzb(i >> 4, skq >> 1) + 8 * (skq & 1);      // hi half-row; the lo half-row is this ^ 64
        }
        f32x4 xr[3];                          // the row in flight
        Cur cl;
        cl.i = 0;
        open(cl);
        auto gload = [&]() {                  // the load cursor's row; past the last item (the three drain steps) nothing is fetched
            const int q = cl.r0 - 1 + cl.s;
            const bool ok = q >= 0 && q < H && cl.i < nitem;
            const unsigned so = __builtin_amdgcn_readfirstlane(ok ? (unsigned)((cl.n * H + q) * W) * (unsigned)(PB_CIN * 4) : 0u);
#pragma unroll
            for (int j = 0; j < 3; ++j) xr[j] = bload16(rx, ok ? xv[j] : OOB, so);
            next(cl);
        };
        auto split = [&](unsigned char* At) {      // pwconv_f16s.hip's staging arithmetic
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                f16x4 hi, lo;
                f16s::split(xr[j] * p.a_scale2, hi, lo);
                *(f16x4*)(At + a2o[j]) = hi;
                *(f16x4*)(At + (a2o[j] ^ 64)) = lo;
            }
        };
        // depthwise: a lane owns channel quad `quad` at pixels pg, pg + 8, .. with its taps, scale and shift in registers
        const int quad = tid & 31, pg = tid >> 5;
        f32x4 wk[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) wk[i] = p.wd[i * (PB_C / 4) + quad];
        const f32x4 dsc = p.dscale[quad], dsh = p.dshift[quad];
        int ro[3];                            // ring offsets of cells pg + t (pixels pg - 1, pg, pg + 1); eight pixels on: + 8 cells, same swizzle
#pragma unroll
        for (int t = 0; t < 3; ++t) ro[t] = ringb(pg + t, quad);
        // stage A3 offsets of pixel pg + 8 j: swzb's row term (row >> 1) & 7 = (pg >> 1) ^ 4 (j & 1) -- odd j land in the other half-row
        const int a3e = (quad >> 3) * PB_KT + swzb(pg, (quad & 7) >> 1) + 8 * (quad & 1);
        f32x4 top[6], mid[6];                 // per pixel: top taps of the newest row; top of the row before + middle of the newest
#pragma unroll
        for (int j = 0; j < 6; ++j) top[j] = mid[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        auto depthwise = [&](const unsigned char* rs, unsigned char* At) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const f32x4 h0 = *(const f32x4*)(rs + ro[0] + j * 8 * PB_CELLB), h1 = *(const f32x4*)(rs + ro[1] + j * 8 * PB_CELLB),
                            h2 = *(const f32x4*)(rs + ro[2] + j * 8 * PB_CELLB);
                auto row_sum = [&](int b) {
                    f32x4 t = h0 * wk[b];
                    t = __builtin_elementwise_fma(h1, wk[b + 1], t);
                    return __builtin_elementwise_fma(h2, wk[b + 2], t);
                };
                const f32x4 sa = row_sum(0), sb = row_sum(3), sc = row_sum(6);
                const f32x4 sacc = mid[j] + sc;          // (row0 + row1) + row2 of the output row above the newest ring row
                mid[j] = top[j] + sb;
                top[j] = sa;
                const f32x4 o = __builtin_elementwise_fma(sacc, dsc, dsh);
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu6(o[e]);
                f16x4 hi, lo;
                f16s::split(v * p.a_scale3, hi, lo);
                const int ao = (a3e ^ (64 * (j & 1))) + j * 8 * ROWB;
                *(f16x4*)(At + ao) = hi;
                *(f16x4*)(At + (ao ^ 64)) = lo;
            }
        };
        gload();
        // row g leaves the registers first (the consumers need it in the next step) and they are refilled with row g + 1 at once: the
        // loads have the depthwise of row g - 2 and the step's barrier to land -- a step lasts as long as the consumers' products, longer
        // than a trip to HBM -- and one loop body serves every step
#pragma nounroll
        for (int g = 0; g < nsteps; ++g) {
            if (!(PB_ABLATE & 4)) {
                if (g < nflat) split(smem + PB_A2_OFF + (g & 1) * PB_A2);
                gload();
            }
            if (!(PB_ABLATE & 2) && g >= 2 && g < nflat + 2) depthwise(smem + (g & 1) * PB_RING, smem + PB_A3_OFF + (g & 1) * PB_A3);
            __syncthreads();
        }
    } else {
        // =============================== consumers: the two pointwise products ===============================
        const int cw = wave - 4;
        const int li = lane & 31, lh = lane >> 5;
        const int erow = lane >> 3, ech = lane & 7;
        const __amdgpu_buffer_rsrc_t ry = make_rsrc(p.y, (long long)p.nimg * H * W * PB_COUT * 4);
        // resident weight fragments: MFMA step s of K-tile kt takes the 8 halves [16 s + 8 lh, + 8) of the hi and of the lo half-row
        f16x8 w2h[4], w2l[4], w3h[8], w3l[8];
        {
            const unsigned char* r2 = (const unsigned char*)p.w2 + (size_t)(32 * cw + li) * (PB_CIN * 4);
            const unsigned char* r3 = (const unsigned char*)p.w3 + (size_t)(32 * cw + li) * (PB_C * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                w2h[s] = *(const f16x8*)(r2 + (s >> 1) * 128 + (2 * (s & 1) + lh) * 16);
                w2l[s] = *(const f16x8*)(r2 + (s >> 1) * 128 + 64 + (2 * (s & 1) + lh) * 16);
            }
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                w3h[s] = *(const f16x8*)(r3 + (s >> 1) * 128 + (2 * (s & 1) + lh) * 16);
                w3l[s] = *(const f16x8*)(r3 + (s >> 1) * 128 + 64 + (2 * (s & 1) + lh) * 16);
            }
        }
        f32x4 ds3 = *(const f32x4*)(p.ds3 + 32 * cw + 4 * ech), sh3 = *(const f32x4*)(p.sh3 + 32 * cw + 4 * ech);
        // the resident operands are IN their registers before the loop: hipcc otherwise sinks each load's vmcnt wait to its first use inside
        // the loop, where the counter also counts this wave's own output stores (asm statements it does not see) -- every step's
        // conv_pw_2 product then waited for the stores of the conv_pw_3 row just issued
#pragma unroll
        for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(w2h[s]), "+v"(w2l[s]));
#pragma unroll
        for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(w3h[s]), "+v"(w3l[s]));
        asm volatile("" : "+v"(ds3), "+v"(sh3));
        const float* el = (const float*)(smem + PB_E_OFF);
        unsigned char* scr = smem + PB_S_OFF + cw * 8192;        // 4 KB per column block
        Cur c1, c3;
        c1.i = 0;
        open(c1);
        c3 = c1;
        // weights first: lane (li, lh) holds pixel li of column block b, channels acc_row(r, lh) of the wave's 32
        f32x16 acc2[NB], acc3[NB];             // conv_pw_2's and conv_pw_3's accumulators (both live: see the step below)
        f16x8 fh[2][NB], fl[2][NB];            // activation fragments, two K-steps
        auto zero = [&](f32x16* acc) {
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        };
        auto fragments = [&](const unsigned char* St, int s, int buf) {
            const unsigned char* row = St + (s >> 1) * PB_KT;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                fh[buf][b] = frag(row, b * 32 + li, 2 * (s & 1) + lh);
                fl[buf][b] = frag(row, b * 32 + li, 4 + 2 * (s & 1) + lh);
            }
        };
        auto mfmas = [&](f32x16* acc, const f16x8& wh, const f16x8& wl, int buf) {      // one K-step: wh*al, wl*ah, wh*ah into one accumulator
#pragma unroll
            for (int b = 0; b < NB; ++b) {      // (f16s.h's mac3, spelt out: through the helper hipcc numbers this kernel's registers differently)
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, fl[buf][b], acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, fh[buf][b], acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, fh[buf][b], acc[b], 0, 0, 0);
            }
        };
        // (the fragments of K-step s + 1 are requested before the MFMAs of step s: one LDS round trip is hidden behind 6 MFMAs)
        auto product3 = [&](const unsigned char* St) {
            zero(acc3);
            fragments(St, 0, 0);
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (s + 1 < 8) fragments(St, s + 1, (s + 1) & 1);
                mfmas(acc3, w3h[s], w3l[s], s & 1);
            }
        };
        // conv_pw_3's way out, in three pieces per column block: accumulators -> scratch, scratch -> 8 lanes per pixel row, -> 128-byte lines
        unsigned sv[NB][4];
        f32x4 rv[4];
        auto out_park = [&](int b) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc3[b][4 * j + e];
                *(f32x4*)(scr + b * 4096 + li * 128 + 16 * ((2 * j + lh) ^ (li & 7))) = v;
            }
        };
        auto out_fetch = [&](int b) {          // (all reads before the first store: a store is an asm statement the LDS reads do not cross)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rr = erow + 8 * i;
                rv[i] = *(const f32x4*)(scr + b * 4096 + rr * 128 + 16 * (ech ^ (rr & 7)));
            }
        };
        auto out_store = [&](int b) {          // (one uniform choice of the activation per column block, not one per store)
            f32x4 o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = __builtin_elementwise_fma(rv[i], ds3, sh3);
            if (p.act == HSEFR_ACT_RELU6) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[i][e] = apply_act<HSEFR_ACT_RELU6>(o[i][e]);
            } else if (p.act == HSEFR_ACT_RELU) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[i][e] = apply_act<HSEFR_ACT_RELU>(o[i][e]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (!(PB_ABLATE & 8)) bstore16_welded(o[i], ry, sv[b][i], 0u);
        };
#pragma nounroll
        for (int g = 0; g < nsteps; ++g) {
            const int par = (g + 1) & 1;                   // the stages and the ring row the producers filled in the last step
            // conv_pw_3 of row g - 3: output row r0 + s - 2 (an item's first two rows only fill the depthwise window)
            const bool emit = !(PB_ABLATE & 1) && g >= 3 && g < nflat + 3 && c3.s >= 2;
            // conv_pw_2 of row g - 1 into the ring; a row outside the map is a row of zeros
            const bool feed = !(PB_ABLATE & 1) && g >= 1 && g < nflat + 1;
            const int q = c1.r0 - 1 + c1.s;
            const bool inside = feed && q >= 0 && q < H;
            unsigned char* slot = smem + par * PB_RING;
            const unsigned char* A2s = smem + PB_A2_OFF + par * PB_A2;
            if (emit) {
                const int r = c3.r0 + c3.s - 2;
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int px = b * 32 + erow + 8 * i;
                        sv[b][i] = px < W ? ((unsigned)((c3.n * H + r) * W + px) * (unsigned)PB_COUT + (unsigned)(32 * cw + 4 * ech)) * 4u : OOB;
                    }
                product3(smem + PB_A3_OFF + par * PB_A3);
                out_park(0);
                out_park(1);
            }
            // conv_pw_3's row leaves UNDER conv_pw_2's MFMAs: its accumulators are parked at once (so the two products' accumulators are
            // never live together), the scratch reads and the stores sit between conv_pw_2's K-steps (uniform branches: a step at the
            // edge of an item has only one of the two)
            if (inside) {
                zero(acc2);
                fragments(A2s, 0, 0);
                fragments(A2s, 1, 1);
                mfmas(acc2, w2h[0], w2l[0], 0);
            }
            if (emit) out_fetch(0);
            if (inside) {
                fragments(A2s, 2, 0);
                mfmas(acc2, w2h[1], w2l[1], 1);
            }
            if (emit) { out_store(0); out_fetch(1); }
            if (inside) {
                fragments(A2s, 3, 1);
                mfmas(acc2, w2h[2], w2l[2], 0);
            }
            if (emit) out_store(1);
            if (inside) mfmas(acc2, w2h[3], w2l[3], 1);
            if (inside) {
                f32x4 ds[4], sh[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    ds[j] = *(const f32x4*)(el + 32 * cw + 8 * j + 4 * lh);
                    sh[j] = *(const f32x4*)(el + PB_C + 32 * cw + 8 * j + 4 * lh);
                }
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = relu6(fmaf(acc2[b][4 * j + e], ds[j][e], sh[j][e]));
                        if (b * 32 + li < W) *(f32x4*)(slot + ringb(b * 32 + li + 1, 8 * cw + 2 * j + lh)) = v;
                    }
            } else if (feed) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (b * 32 + li < W) *(f32x4*)(slot + ringb(b * 32 + li + 1, 8 * cw + 2 * j + lh)) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (!(PB_ABLATE & 1) && g >= 3 && g < nflat + 3) next(c3);
            if (feed) next(c1);
            __syncthreads();
        }
    }
}

}  // namespace

// shapes the row-streaming launch covers (what HSEFR_OPF_PWBLK_NEXT runs): 64 -> 128 -> 128 channels on rows of at most 48 pixels
bool pwblk_covered(int cin, int cmid, int cout, int w) { return cin == PB_CIN && cmid == PB_C && cout == PB_COUT && w >= 1 && w <= PB_WMAX; }

// segs: 0 = as many row segments per image as fill the CUs (a segment recomputes two conv_pw_2 rows: at least four rows each), s > 0 = s
// segments (at most h).  The result does not depend on it.
int launch_pwblk_f16s(const float* x, const void* w2split, const float* descale2, const float* shift2, const float* wd, const float* dscale,
                      const float* dshift, const void* w3split, const float* descale3, const float* shift3, float* y, int n, int h, int w,
                      int a_log2, int a_log2_blk, int act, int segs, hipStream_t s) {
    HSEFR_REQUIRE(n >= 0 && h > 0 && w > 0 && w <= PB_WMAX, HSEFR_ERR_UNSUPPORTED, "pwblk_f16split: map %d x %d not covered (rows of at most %d pixels)",
                  h, w, PB_WMAX);
    HSEFR_REQUIRE(a_log2 > 0 && a_log2 <= 12 && a_log2_blk > 0 && a_log2_blk <= 12, HSEFR_ERR_INVALID, "pwblk_f16split: a_log2=%d / %d (1..12)", a_log2,
                  a_log2_blk);
    HSEFR_REQUIRE(segs >= 0, HSEFR_ERR_INVALID, "pwblk_f16split: segs=%d", segs);
    if (n == 0) return HSEFR_OK;
    HSEFR_REQUIRE((long long)n * h * w * PB_COUT * 4 < (1ll << 32) - 16, HSEFR_ERR_UNSUPPORTED, "pwblk_f16split: tensors beyond 4 GB");
    PwBlkParams p;
    p.x = x; p.w2 = (const float*)w2split; p.ds2 = descale2; p.sh2 = shift2;
    p.wd = (const f32x4*)wd; p.dscale = (const f32x4*)dscale; p.dshift = (const f32x4*)dshift;
    p.w3 = (const float*)w3split; p.ds3 = descale3; p.sh3 = shift3; p.y = y;
    p.nimg = n; p.H = h; p.W = w;
    int S = segs;
    if (S == 0) {
        const int fill = (int)((PB_GRID + (unsigned)n - 1) / (unsigned)n), most = h / 4 > 1 ? h / 4 : 1;
        S = fill < most ? fill : most;
    }
    p.S = S < h ? S : h;
    if (p.S > PB_ITEMS) p.S = PB_ITEMS;
    p.kS = hsefr_udiv_make(p.S >= 2 ? (unsigned)p.S : 2u);
    p.a_scale2 = ldexpf(1.f, a_log2);
    p.a_scale3 = ldexpf(1.f, a_log2_blk);
    p.reverse = sweep_reverse();
    HSEFR_REQUIRE(act == HSEFR_ACT_RELU6 || act == HSEFR_ACT_RELU || act == HSEFR_ACT_NONE, HSEFR_ERR_UNSUPPORTED, "pwblk_f16split: act %d", act);
    p.act = act;
    // a workgroup's item table holds PB_ITEMS items: a batch beyond PB_GRID * PB_ITEMS items (16384 images in one segment) goes out in slices
    const int per = (int)(PB_GRID * PB_ITEMS) / p.S;
    for (int n0 = 0; n0 < n; n0 += per) {
        p.nimg = n - n0 < per ? n - n0 : per;
        p.x = x + (size_t)n0 * h * w * PB_CIN;
        p.y = y + (size_t)n0 * h * w * PB_COUT;
        p.total = (unsigned)p.nimg * (unsigned)p.S;
        const unsigned g = p.total < PB_GRID ? p.total : PB_GRID;
        HSEFR_LAUNCH(pwblk_stream_f16s_kernel, dim3(g), dim3(512), 0, s, p);
    }
    return launch_status("pwblk_f16split");
}

}  // namespace hsefr
