// Pointwise (1x1) convolution + shift + act as a SPLIT-f16 MFMA GEMM with fp32-grade results, NHWC fp32, gfx950.
//
// Same graph nodes as pwconv_f32.hip (Conv2D 1x1 -> Add shift -> Relu -> Minimum 6 -> Maximum 0, run by tf_sess.run at
// facerec_test.py:120 / facial_analysis.py:109), same fp32 activations in HBM, same fp32 accumulators.  What changes is
// how each product is formed.  gfx950 has no fp32 matrix rate worth the name (v_mfma_f32_32x32x2_f32: 157 TF/s, 1/16 of
// the f16 rate), so every fp32 operand is written as the exact sum of two f16 numbers plus a residual below 2^-22,
//
//     a = ah + al (+ ra),  w = wh + wl (+ rw),   ah = f16(a), al = f16(a - ah)      (round to nearest even)
//     a*w  ~=  ah*wh + ah*wl + al*wh            dropped: al*wl, ra*w, a*rw  --  each <= 2^-22 |a*w|
//
// and the three products go through v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator (f16 x f16 products are exact in
// fp32).  Error per product <= 3 * 2^-22 (7e-7) worst case, ~2e-7 typical -- the size of an fp32 rounding or two;
// end-to-end embeddings stay at 1e-6 of the fp64 oracle (bar: 1e-4).  3 MFMAs at 16x the rate = 5.3x fewer matrix
// cycles than the fp32 MFMA kernel, which turns the pointwise layers from matrix-bound into memory-bound.
//
// Range (f16 tops out at 65504 and loses precision below 6.1e-5): operands are moved into the top of the f16 range by
// exact power-of-two scalings that the epilogue undoes --
//   * activations: |x| <= bound is a PRECONDITION (the lowering takes it from the graph: the producer ends in ReLU6),
//     x' = x * 2^a_log2 with bound * 2^a_log2 < 32768;
//   * weights: per output channel n, w' = w * 2^e_n with max_k |w'| in [8192, 16384), split on the host into the two
//     f16 planes; descale[n] = 2^-(e_n + a_log2).
// With that, f16 subnormals (or their flushing) only touch |x| < 1.5e-8: absolute errors far below one fp32 ulp of any
// output.  Unbounded inputs take the fp32 MFMA kernel instead (pwconv_f32.hip).
//
// Weight image ("split rows"): for output channel n and K-tile kt (32 input channels) one 128-byte row
//   [ wh(k = 32kt .. 32kt+31) : 32 x f16 | wl(same k) : 32 x f16 ]      -> [Cout][K/32][64] f16, byte-compatible with a
// [Cout][K] fp32 matrix, so it is staged with the same full-line 16-B copies and lands in LDS in MFMA-ready form.  The
// activation tile is split by the staging threads (4 values each: scale, 2 x cvt, subtract) on its way into the same
// row format.  The row layout, its LDS swizzle, the split and the three-MFMA product are f16s.h's, shared with every other
// split-f16 kernel.
#include <type_traits>

#include "f16s.h"

#ifndef PWS_AAUX
#define PWS_AAUX 0     // cache policy of the activation loads (buffer aux bits: 1 glc, 2 slc)
#endif
namespace hsefr {

namespace {

using namespace f16s;

#ifdef HSEFR_PWS_STAMPS
// Diagnostic build only (build.sh HSEFR_EXTRA_FLAGS=-DHSEFR_PWS_STAMPS): per-wave s_memtime sums of the step phases.
__device__ unsigned long long g_pws_stamps[1024 * 8 * 8];
#define PWS_STAMP(i) do { const unsigned long long _t = __builtin_amdgcn_s_memtime(); st[i] += _t - tprev; tprev = _t; } while (0)
#else
#define PWS_STAMP(i) do { } while (0)
#endif

// sched_group_barrier masks
#define SG_VALU 0x002
#define SG_MFMA 0x008
#define SG_VMEM_RD 0x020
#define SG_DS_RD 0x100
#define SG_DS_WR 0x200

template <int BM, int BN, int WAVES_N, int OCC, int ACT>
__global__ __launch_bounds__(128 * WAVES_N, OCC) void pwconv_f16s_kernel(const float* __restrict__ x, const float* __restrict__ wsplit,
                                                               const float* __restrict__ descale,
                                                               const float* __restrict__ shift, float* __restrict__ y,
                                                               long long M, int K, int Cout, float a_scale,
                                                               unsigned tiles_n, unsigned total_tiles, int reverse) {
    constexpr int NT = 128 * WAVES_N;                 // threads: 2 x WAVES_N waves
    constexpr int WM = BM / 2, WN = BN / WAVES_N;     // wave tile
    constexpr int MI = WM / 32, NI = WN / 32;
    constexpr int SR = NT / 8;                        // rows staged per pass (8 threads = one 128-B row)
    constexpr int AP = BM / SR, BP = BN / SR;         // staging passes
    constexpr int NMFMA = MI * NI * 6;                // per wave and step
    static_assert(WAVES_N == 2 && (BM + BN) * ROWB >= 4 * 4096, "epilogue scratch: 4 KB per wave inside one stage");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2][(BM + BN) * ROWB];   // stage = A rows, then B rows
    __shared__ __attribute__((aligned(16))) float Et[2][2][BN];   // epilogue constants [tile parity][descale | shift][n]
    auto As = [&](int st) { return &smem[st][0]; };
    auto Bs = [&](int st) { return &smem[st][BM * ROWB]; };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int li = lane & 31, lh = lane >> 5;
    const int srow = tid >> 3, skq = tid & 7;
    const int KT = K / BK;

    if (blockIdx.x >= total_tiles) return;
    // The (tile, K-tile) steps of this persistent workgroup form ONE flat sequence g = 0 .. nsteps-1.  With the f16
    // MFMA a step's matrix work (24 MFMAs per wave at 128x128) is shorter than a global-load round trip, so the loads
    // run TWO steps ahead of the MFMAs (two register sets, by step parity); a prefetch cursor of its own walks the same
    // sequence and simply keeps re-reading the last tile once it runs off the end (harmless, never consumed).
    const unsigned ntile = (total_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x;
    const unsigned nsteps = ntile * KT;
    const unsigned rowbytes = (unsigned)K * 4u;
    const unsigned voff = (unsigned)srow * rowbytes + 16u * skq;     // this thread's 16 B of a staged 8-row group

    const bool tn_pow2 = (tiles_n & (tiles_n - 1u)) == 0u;
    const int tn_shift = __builtin_ctz(tiles_n);
    auto tile_origin = [&](unsigned i, long long& mm0, int& nn0) {
        const unsigned lt = xcd_remap_dir(blockIdx.x + (i < ntile ? i : ntile - 1) * gridDim.x, total_tiles, reverse);
        // tiles_n is a power of two for every MobileNet / ResNet layer: two shifts instead of two 32-bit divisions, four times per tile
        const unsigned tm = tn_pow2 ? lt >> tn_shift : lt / tiles_n;
        mm0 = (long long)tm * BM;
        nn0 = (lt - tm * tiles_n) * BN;
    };
    __amdgpu_buffer_rsrc_t ra_rsrc, rb_rsrc;
    unsigned pf_i = 0;   // prefetch cursor: tile ordinal, K-tile
    int pf_kt = 0;
    auto setup_rsrc = [&](unsigned i) {
        long long mm0;
        int nn0;
        tile_origin(i, mm0, nn0);
        ra_rsrc = make_rsrc(x + mm0 * K, (M - mm0) * (long long)rowbytes);
        rb_rsrc = make_rsrc(wsplit + (long long)nn0 * K, (long long)(Cout - nn0) * rowbytes);
    };

    f32x4 ra[2][AP], rb[2][BP];
    auto gload = [&](auto SET) {   // loads of the prefetch cursor's step into register set SET
        constexpr int S = decltype(SET)::value;
        const unsigned so = (unsigned)pf_kt * (BK * 4u);
#pragma unroll
        for (int p = 0; p < AP; ++p) ra[S][p] = __builtin_bit_cast(hsefr_f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra_rsrc, voff, so + (unsigned)(SR * p) * rowbytes, PWS_AAUX));
#pragma unroll
        for (int p = 0; p < BP; ++p) rb[S][p] = bload16(rb_rsrc, voff, so + (unsigned)(SR * p) * rowbytes);
    };
    auto advance_prefetch = [&]() {
        if (++pf_kt == KT) {
            pf_kt = 0;
            setup_rsrc(++pf_i);
        }
    };
    // activations: 4 fp32 -> 4 hi halves (8 B at k-offset 4*skq of the hi half-row) + 4 lo halves (same place, lo half-row)
    auto swrite = [&](auto SET, int buf) {
        constexpr int S = decltype(SET)::value;
#pragma unroll
        for (int p = 0; p < AP; ++p) {
            f16x4 hi, lo;
            split(ra[S][p] * a_scale, hi, lo);
            put_quad(As(buf), srow + SR * p, skq, hi, lo);
        }
#pragma unroll
        for (int p = 0; p < BP; ++p) *(f32x4*)(Bs(buf) + swzb(srow + SR * p, skq)) = rb[S][p];
    };

    f32x16 acc[MI][NI];
    auto zero_acc = [&]() {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    };
    zero_acc();

    typedef std::integral_constant<int, 0> S0;
    typedef std::integral_constant<int, 1> S1;
    long long m0;
    int n0;
    unsigned ci = 0;   // compute cursor
    int ckt = 0;
    tile_origin(0, m0, n0);
    setup_rsrc(0);
    gload(S0());
    advance_prefetch();
    gload(S1());
    advance_prefetch();
    swrite(S0(), 0);
    __syncthreads();
    const int arow = wm * WM + li, brow = wn * WN + li;
    // Epilogue geometry.  The MFMAs run with the weights first: lane (li, lh) then owns output row m = li of a 32 x 32
    // block and, in accumulator register r, column n = acc_row(r, lh): four runs of 4 consecutive channels = four
    // ds_write_b128 into a wave-private 32 x 128 B scratch (the LDS stage the tile's last step has just finished with).
    // Read back 8 lanes per row, a block leaves as 4 stores of 8 rows x 128 B: whole lines, a quarter of the store
    // instructions of the register-per-row layout.
    const int erow = lane >> 3, ech = lane & 7;
    const unsigned yvoff = ((unsigned)(wm * WM + erow) * (unsigned)Cout + (unsigned)(wn * WN + 4 * ech)) * 4u;

#ifdef HSEFR_PWS_STAMPS
    unsigned long long st[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long tprev = __builtin_amdgcn_s_memtime();
    const unsigned long long tstart = tprev;
#endif
    // one step: compute from LDS stage P, refill register set P with step g+2, move set 1-P (step g+1) into stage 1-P
    auto step = [&](auto PAR) {
        constexpr int P = decltype(PAR)::value;
        PWS_STAMP(5);
        // the tile's epilogue constants go to LDS during its first step (ahead of that step's prefetch in the load queue)
        f32x4 ec;
        const bool fill = ckt == 0 && tid < BN / 2;
        if (fill) {
            const int j = tid < BN / 4 ? tid : tid - BN / 4;
            ec = *(const f32x4*)((tid < BN / 4 ? descale : shift) + n0 + 4 * j);
        }
        // ---- one scheduling region: MFMAs as the backbone, everything else in their shadow -------------------------
        f16x8 ah[2][MI], al[2][MI], bh[2][NI], bl[2][NI];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                ah[s][mi] = frag(As(P), arow + mi * 32, 2 * s + lh);
                al[s][mi] = frag(As(P), arow + mi * 32, 4 + 2 * s + lh);
            }
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                bh[s][ni] = frag(Bs(P), brow + ni * 32, 2 * s + lh);
                bl[s][ni] = frag(Bs(P), brow + ni * 32, 4 + 2 * s + lh);
            }
        }
        gload(PAR);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) mac3(bh[s][ni], bl[s][ni], ah[s][mi], al[s][mi], acc[mi][ni]);
        swrite(std::integral_constant<int, 1 - P>(), 1 - P);
        // desired order: fragments, then one prefetch load per MFMA, then the conversion VALU + LDS writes of the
        // next stage spread under the remaining MFMAs (the wave never queues up 12 loads at once, and the ~60 VALU
        // of the split are hidden instead of following the MFMAs)
        __builtin_amdgcn_sched_group_barrier(SG_DS_RD, 4 * (MI + NI), 0);
#pragma unroll
        for (int i = 0; i < AP + BP; ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VMEM_RD, 1, 0);
        }
#pragma unroll
        for (int i = 0; i < NMFMA - (AP + BP); ++i) {
            __builtin_amdgcn_sched_group_barrier(SG_MFMA, 1, 0);
            __builtin_amdgcn_sched_group_barrier(SG_VALU, (14 * AP + NMFMA - (AP + BP) - 1) / (NMFMA - (AP + BP)), 0);
            __builtin_amdgcn_sched_group_barrier(SG_DS_WR, 1, 0);
        }
        if (fill) *(f32x4*)(&Et[ci & 1][tid < BN / 4 ? 0 : 1][4 * (tid < BN / 4 ? tid : tid - BN / 4)]) = ec;
        PWS_STAMP(1);
        __syncthreads();
        PWS_STAMP(3);
        advance_prefetch();
        if (++ckt == KT) {
            const float* et = &Et[ci & 1][0][0];
            const __amdgpu_buffer_rsrc_t ry = make_rsrc(y + m0 * Cout + n0, ((M - m0) * Cout - n0) * 4ll);
            unsigned char* scr = &smem[P][wave * 4096];       // stage P: every wave is past its last read (barrier above)
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int nl = wn * WN + ni * 32 + 4 * ech;
                const f32x4 ds = *(const f32x4*)(et + nl), sh = *(const f32x4*)(et + BN + nl);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4 v;
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = acc[mi][ni][4 * j + e];
                        *(f32x4*)(scr + li * 128 + 16 * ((2 * j + lh) ^ (li & 7))) = v;
                    }
                    // (all four reads before the first store: the store's hazard guard is an asm statement the LDS reads do not cross,
                    // and with a read per store the wave waited out one LDS round trip per 16 bytes)
                    f32x4 rv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int r = erow + 8 * i;
                        rv[i] = *(const f32x4*)(scr + r * 128 + 16 * (ech ^ (r & 7)));
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int e = 0; e < 4; ++e) rv[i][e] = apply_act<ACT>(fmaf(rv[i][e], ds[e], sh[e]));
                    // (the four stores back to back, after all the arithmetic: no vector write lands in a store's data registers
                    // inside its hazard window -- tools/isa_lint.py)
#pragma unroll
                    for (int i = 0; i < 4; ++i)   // rows beyond M fall outside the resource and are dropped by the hardware
                        bstore16(rv[i], ry, yvoff, (unsigned)(mi * 32 + 8 * i) * (unsigned)Cout * 4u + (unsigned)(ni * 32) * 4u);
                }
            }
            __syncthreads();   // the scratch is the stage the next step refills
            zero_acc();
            ckt = 0;
            ++ci;
            tile_origin(ci, m0, n0);
        }
    };
    for (unsigned g = 0; g < nsteps; g += 2) {
        step(S0());
        PWS_STAMP(4);
        if (g + 1 >= nsteps) break;
        step(S1());
        PWS_STAMP(4);
    }
#ifdef HSEFR_PWS_STAMPS
    if (lane == 0 && blockIdx.x < 1024) {
        unsigned long long* o = g_pws_stamps + (blockIdx.x * 8 + wave) * 8;
        for (int i = 0; i < 6; ++i) o[i] = st[i];
        o[6] = __builtin_amdgcn_s_memtime() - tstart;
        o[7] = nsteps;
    }
#endif
}

struct TileCfg { int bm, bn, occ; double eff; };

// Candidate tiles and their relative speed per output element (measured, tools/kbench.py pws: bigger tiles move fewer
// L2->LDS bytes per MFMA).  Resident workgroups per CU: LDS 64/48/32 KB and the launch bounds below.
const TileCfg kCands[3] = {{128, 128, 2, 1.00}, {128, 64, 3, 0.77}, {64, 64, 3, 0.60}};

// Persistent workgroups deal the tiles out in rounds of 256 CUs x occ.  A partly empty last round does not cost a whole
// tile time: the workgroups that finish early leave their CU to the stragglers, which then run faster (measured on
// 36864x512x512: 2.25 rounds of 128x128 beat 3.0 rounds of 128x64; on 9216x1024x1024 1.125 rounds beat 1.5).
int choose_tile(long long m, int cout, int forced) {
    int best = -1;
    double best_cost = 0;
    for (int i = 0; i < 3; ++i) {
        const TileCfg& c = kCands[i];
        if (cout % c.bn || (forced >= 0 && forced != i)) continue;
        const double rounds = (double)(((m + c.bm - 1) / c.bm) * (cout / c.bn)) / (256.0 * c.occ);
        const double up = (double)(long long)(rounds + 0.999999);
        const double makespan = rounds <= 1.0 ? 1.0 : up - 0.35 * (up - rounds);
        const double cost = makespan * c.occ * c.bm * c.bn / c.eff;
        if (best < 0 || cost < best_cost) { best = i; best_cost = cost; }
    }
    return best;
}

HSEFR_KNOB(g_forced_tile, "pws_tile", -1);  // dev builds: 0 = 128x128, 1 = 128x64, 2 = 64x64

template <int BM, int BN, int WAVES_N, int OCC>
int launch_cfg(const float* x, const void* wsplit, const float* descale, const float* shift, float* y, long long m, int k,
               int cout, float a_scale, int act, hipStream_t s) {
    const long long tiles_m = (m + BM - 1) / BM;
    const unsigned tiles_n = cout / BN;
    const long long total = tiles_m * tiles_n;
    HSEFR_REQUIRE(total < (1ll << 31), HSEFR_ERR_UNSUPPORTED, "pwconv_f16split: too many tiles");
    const long long g = total < 256ll * OCC ? total : 256ll * OCC;
    dim3 grid((unsigned)g), block(128 * WAVES_N);
#define HSEFR_PWS_LAUNCH(A)                                                                                         \
    HSEFR_LAUNCH((pwconv_f16s_kernel<BM, BN, WAVES_N, OCC, A>), grid, block, 0, s, x, (const float*)wsplit, descale, shift, \
                       y, m, k, cout, a_scale, tiles_n, (unsigned)total, sweep_reverse())
    HSEFR_ACT_SWITCH(act, "pwconv_f16split", HSEFR_PWS_LAUNCH);
#undef HSEFR_PWS_LAUNCH
    return launch_status("pwconv_f16split");
}

}  // namespace


int read_pws_stamps(void* host_out, size_t bytes) {
#ifdef HSEFR_PWS_STAMPS
    HSEFR_REQUIRE(bytes <= sizeof(unsigned long long) * 1024 * 8 * 8, HSEFR_ERR_INVALID, "read_pws_stamps: too many bytes");
    HSEFR_HIP_CHECK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_pws_stamps), bytes));
    return HSEFR_OK;
#else
    (void)host_out; (void)bytes;
    set_error("read_pws_stamps: library built without -DHSEFR_PWS_STAMPS");
    return HSEFR_ERR_UNSUPPORTED;
#endif
}

int launch_pwconv_f16s(const float* x, const void* wsplit, const float* descale, const float* shift, float* y,
                       long long m, int k, int cout, int a_log2, int act, hipStream_t s) {
    HSEFR_REQUIRE(k > 0 && k % BK == 0, HSEFR_ERR_UNSUPPORTED, "pwconv_f16split: k=%d must be a multiple of %d", k, BK);
    HSEFR_REQUIRE(cout > 0 && cout % 64 == 0, HSEFR_ERR_UNSUPPORTED, "pwconv_f16split: cout=%d must be a multiple of 64", cout);
    HSEFR_REQUIRE(a_log2 >= -24 && a_log2 <= 24, HSEFR_ERR_INVALID, "pwconv_f16split: a_log2=%d", a_log2);
    HSEFR_REQUIRE(m >= 0, HSEFR_ERR_INVALID, "pwconv_f16split: m=%lld", m);
    if (m == 0) return HSEFR_OK;
    const float a_scale = ldexpf(1.f, a_log2);
    switch (choose_tile(m, cout, g_forced_tile)) {
        case 0: return launch_cfg<128, 128, 2, 2>(x, wsplit, descale, shift, y, m, k, cout, a_scale, act, s);
        case 1: return launch_cfg<128, 64, 2, 3>(x, wsplit, descale, shift, y, m, k, cout, a_scale, act, s);
        case 2: return launch_cfg<64, 64, 2, 3>(x, wsplit, descale, shift, y, m, k, cout, a_scale, act, s);
    }
    set_error("pwconv_f16split: no tile configuration for cout=%d", cout);
    return HSEFR_ERR_UNSUPPORTED;
}

}  // namespace hsefr
