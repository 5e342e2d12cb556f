// Post-extract identification on device: L2 row normalisation and brute-force 1-NN and k-NN, gfx950.
//
// Replaces preprocessing.normalize(X, 'l2') (facerec_test.py:401),
// KNeighborsClassifier(n_neighbors=1, p=2).fit(gallery).kneighbors(probe)
// (facerec_test.py:422 scored through classifier_tester :200-207) and the 3-NN classifiers of
// facerec_test.py:269-288 (kneighbors and the uniform-weight predict: launch_knn at the end of this file), and the same
// search under the study's chi-square and KL distances (facerec_test.py:157-164, :275-276, :424-425: metric_dist_tile_kernel,
// launch_knn_metric).
//
// 1-NN = a [nq x ng x d] contraction (4582 x 4582 x 1024 for LFW, 43 GFLOP) -> fp32 MFMA:
//   dist2[q, g] = |q|^2 + |g|^2 - 2 q.g ,  arg-min over g, ties to the lowest gallery index.
// One workgroup = 32 probe rows x the whole gallery; its 4 waves take gallery tiles of 32 rows
// round-robin, each keeps a per-lane running (min, index) for its 16 accumulator rows, and the
// candidates meet once at the end (wavefront shuffles, then LDS across the 4 waves).  Row norms
// are accumulated from the very fragments that feed the MFMAs.
#include <atomic>

#include "common.h"
#include "mfma_dot.h"

namespace hsefr {

namespace {

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(256) void l2_normalize_kernel(const float* __restrict__ x, float* __restrict__ y, int n, int d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const float* xr = x + (size_t)row * d;
    float ss = 0.f;
    for (int j = lane; j < d; j += 64) ss = fmaf(xr[j], xr[j], ss);
    ss = wave_sum64(ss);
    float nrm = sqrtf(ss);
    if (nrm == 0.f) nrm = 1.f;  // sklearn: zero rows are left as they are
    for (int j = lane; j < d; j += 64) y[(size_t)row * d + j] = xr[j] / nrm;
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void nn1_kernel(const float* __restrict__ q, const float* __restrict__ g, int nq,
                                                  int ng, int d, int* __restrict__ nn_index,
                                                  float* __restrict__ nn_dist2) {
    __shared__ float s_val[4][32];
    __shared__ int s_idx[4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.x * 32;
    const int qrow = min(q0 + li, nq - 1);
    const float* qp = q + (size_t)qrow * d + 4 * lh;

    float best_v[16];
    int best_i[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { best_v[r] = INFINITY; best_i[r] = 0x7fffffff; }

    float qq = 0.f;  // |q_row|^2, accumulated on the first gallery tile only
    bool qq_done = false;
    const int gtiles = (ng + 31) / 32;
    for (int gt = wave; gt < gtiles; gt += 4) {
        const int gcol = gt * 32 + li;
        const int grow = min(gcol, ng - 1);
        const float* gp = g + (size_t)grow * d + 4 * lh;
        f32x16 acc;
        float gg, qs;
        mfma_dot_32x32(qp, gp, d, acc, qs, gg);
        gg += __shfl_xor(gg, 32);
        if (!qq_done) { qq = qs + __shfl_xor(qs, 32); qq_done = true; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;  // probe row of this accumulator register
            const float qr = __shfl(qq, rr);
            const float v = fmaxf(qr + gg - 2.f * acc[r], 0.f);
            if (gcol < ng && better(v, gcol, best_v[r], best_i[r])) { best_v[r] = v; best_i[r] = gcol; }
        }
    }
    // arg-min across the 32 gallery columns held by the lanes of each half-wave
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(best_v[r], m);
            const int oi = __shfl_xor(best_i[r], m);
            if (better(ov, oi, best_v[r], best_i[r])) { best_v[r] = ov; best_i[r] = oi; }
        }
    }
    if (li == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
            s_val[wave][rr] = best_v[r];
            s_idx[wave][rr] = best_i[r];
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && q0 + threadIdx.x < nq) {
        float bv = s_val[0][threadIdx.x];
        int bi = s_idx[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (better(s_val[w][threadIdx.x], s_idx[w][threadIdx.x], bv, bi)) { bv = s_val[w][threadIdx.x]; bi = s_idx[w][threadIdx.x]; }
        nn_index[q0 + threadIdx.x] = bi;
        if (nn_dist2) nn_dist2[q0 + threadIdx.x] = bv;
    }
}

// One wave's 32 x 32 tile of squared distances max(|x_i|^2 + |y_j|^2 - 2 x_i.y_j, 0) between rows i0.. of x [n,d] and j0.. of y [m,d]: the MFMA
// contraction, operand arrangement and sum of nn1_kernel (so the same bits), handed to emit(row, col, dist2) for every element inside.
template <class Emit>
__device__ __forceinline__ void dist2_tile_32x32(const float* __restrict__ x, const float* __restrict__ y, int n, int m, int d, int i0, int j0,
                                                 Emit emit) {
    const int lane = threadIdx.x & 63;
    const int li = lane & 31, lh = lane >> 5;
    const float* xp = x + (size_t)min(i0 + li, n - 1) * d + 4 * lh;
    const float* yp = y + (size_t)min(j0 + li, m - 1) * d + 4 * lh;
    f32x16 acc;
    float xx, yy;
    mfma_dot_32x32(xp, yp, d, acc, xx, yy);
    xx += __shfl_xor(xx, 32);
    yy += __shfl_xor(yy, 32);
    const int col = j0 + li;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float xr = __shfl(xx, rr);
        const int row = i0 + rr;
        const float v = fmaxf(xr + yy - 2.f * acc[r], 0.f);
        if (row < n && col < m) emit(row, col, v);
    }
}

// Full Euclidean distance matrix D[i,j] = |x_i - y_j| (sklearn pairwise_distances at
// facial_clustering_test.py:396; the feature term of process_photos.py:46-51's O(N^2) Python loop),
// same MFMA contraction as nn1_kernel.  Workgroup = 64x64 outputs, wave = 32x32.
__global__ __launch_bounds__(256) void pairwise_dist_kernel(const float* __restrict__ x, const float* __restrict__ y, int n, int m,
                                                            int d, float* __restrict__ out, int same) {
    const int wave = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 64 + (wave >> 1) * 32, j0 = blockIdx.x * 64 + (wave & 1) * 32;
    if (i0 >= n || j0 >= m) return;
    dist2_tile_32x32(x, y, n, m, d, i0, j0, [=](int row, int col, float v2) {
        out[(size_t)row * m + col] = same && row == col ? 0.f : sqrtf(v2);     // pairwise_distances(X) has an exact zero diagonal
    });
}

// The k-NN search of everything the split-f16 GEMM does not take: the finished squared distances of a block of probe rows, [n, ld].
__global__ __launch_bounds__(256) void knn_dist2_tile_kernel(const float* __restrict__ q, const float* __restrict__ g, int n, int ng, int d,
                                                             float* __restrict__ out, int ld) {
    const int wave = threadIdx.x >> 6;
    const int i0 = blockIdx.y * 64 + (wave >> 1) * 32, j0 = blockIdx.x * 64 + (wave & 1) * 32;
    if (i0 >= n || j0 >= ng) return;
    dist2_tile_32x32(q, g, n, ng, d, i0, j0, [=](int row, int col, float v2) { out[(size_t)row * ld + col] = v2; });
}

// ---------------------------------------------------------------------------------------------------------------------
// Large searches (the LFW protocol: 4582 probes x 4582 gallery rows x 1024): the contraction on the split-f16
// GEMM of pwconv_f16s.hip (three f16 MFMA products per fp32 product, error <= 3 * 2^-22 per product -- the arithmetic every
// pointwise layer of the network runs on) instead of the fp32 matrix pipe (29 TFLOP/s in nn1_kernel):
//   1. row norms |q|^2 and the largest |q| of the whole probe matrix (one device scalar: the probes are scaled by the power of
//      two that brings them into [-1, 1], which is what the GEMM's fixed activation scale 2^12 assumes);
//   2. the gallery as the GEMM's WEIGHTS: every row scaled by its own power of two into [8192, 16384), split hi / lo into
//      "split rows" [row][k / 32][hi 32 x f16 | lo 32 x f16]; descale[g] = -2 * 2^(Eq - 12 - e_g), shift[g] = |g|^2 -- so
//      the GEMM's own epilogue returns |g|^2 - 2 q.g; rows that pad the gallery to a multiple of 64 get descale 0 and a huge shift;
//   3. the GEMM -> [nq, ng_pad] fp32 (84 MB for LFW: written and read once at HBM speed);
//   4. row arg-min of max(|q|^2 + that, 0), ties to the lowest gallery index (the rule of nn1_kernel and of scikit-learn).
__global__ __launch_bounds__(256) void nn1_prep_queries_kernel(const float* __restrict__ q, int nq, int d, float* __restrict__ qq,
                                                               unsigned* __restrict__ qmax_bits) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq) return;
    const float* r = q + (size_t)row * d;
    float ss = 0.f, mx = 0.f;
    for (int j = lane; j < d; j += 64) { const float v = r[j]; ss = fmaf(v, v, ss); mx = fmaxf(mx, fabsf(v)); }
    ss = wave_sum64(ss);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    if (lane == 0) {
        qq[row] = ss;
        atomicMax(qmax_bits, __float_as_uint(mx));          // non-negative floats order like their bit patterns (a NaN row wins: results NaN, as before)
    }
}

__device__ __forceinline__ int pow2_above(float mx) {      // e with mx * 2^-e in [0.5, 1)  (0 for mx = 0 / Inf / NaN)
    int e = 0;
    if (mx > 0.f && mx < INFINITY) (void)frexpf(mx, &e);
    return e;
}

__global__ __launch_bounds__(256) void nn1_scale_queries_kernel(const float* __restrict__ q, float* __restrict__ qs, long long n4,
                                                                const unsigned* __restrict__ qmax_bits) {
    const float sc = ldexpf(1.f, -pow2_above(__uint_as_float(*qmax_bits)));
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) ((f32x4*)qs)[i] = ((const f32x4*)q)[i] * sc;
}

__global__ __launch_bounds__(256) void nn1_split_gallery_kernel(const float* __restrict__ g, int ng, int ng_pad, int d,
                                                                unsigned short* __restrict__ wsplit, float* __restrict__ descale,
                                                                float* __restrict__ shift, const unsigned* __restrict__ qmax_bits) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= ng_pad) return;
    unsigned short* w = wsplit + (size_t)row * d * 2;
    if (row >= ng) {
        for (int j = lane; j < 2 * d; j += 64) w[j] = 0;
        if (lane == 0) { descale[row] = 0.f; shift[row] = 3.0e38f; }
        return;
    }
    const float* r = g + (size_t)row * d;
    float ss = 0.f, mx = 0.f;
    for (int j = lane; j < d; j += 64) { const float v = r[j]; ss = fmaf(v, v, ss); mx = fmaxf(mx, fabsf(v)); }
    ss = wave_sum64(ss);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    const int eg = 14 - pow2_above(mx);                      // mx * 2^eg in [8192, 16384)
    const float sc = ldexpf(1.f, eg);
    for (int j = lane; j < d; j += 64) {
        const float v = r[j] * sc;                           // exact
        const _Float16 hi = (_Float16)v;
        const _Float16 lo = (_Float16)(v - (float)hi);
        const int grp = j >> 5, k = j & 31;
        w[grp * 64 + k] = __builtin_bit_cast(unsigned short, hi);
        w[grp * 64 + 32 + k] = __builtin_bit_cast(unsigned short, lo);
    }
    if (lane == 0) {
        const int eq = pow2_above(__uint_as_float(*qmax_bits));
        descale[row] = -2.f * ldexpf(1.f, eq - 12 - eg);
        shift[row] = ss;
    }
}

__global__ __launch_bounds__(256) void nn1_row_argmin_kernel(const float* __restrict__ y, int nq, int ng, int ng_pad,
                                                             const float* __restrict__ qq, int* __restrict__ nn_index,
                                                             float* __restrict__ nn_dist2) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq) return;
    const float* r = y + (size_t)row * ng_pad;
    const float qr = qq[row];
    float bv = INFINITY;
    int bi = 0x7fffffff;
    for (int j = lane; j < ng; j += 64) {
        const float v = fmaxf(qr + r[j], 0.f);
        if (better(v, j, bv, bi)) { bv = v; bi = j; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) {
        nn_index[row] = bi;
        if (nn_dist2) nn_dist2[row] = bv;
    }
}

// k nearest rows of a slice y [nq, ld] of squared distances (qq == nullptr: finished, from knn_dist2_tile_kernel) or of |g|^2 - 2 q.g (the
// split-f16 GEMM's epilogue; qq = |q|^2, finished here exactly as nn1_row_argmin_kernel does), one wave per probe row.  Distances are
// never NaN (fmaxf(., 0) on both paths, as in nn1).  Each lane strides over the row with a list of its CAP >= k best candidates sorted
// by (dist2, index) in registers -- insertion and pop are unrolled compare-and-shift, no register is indexed at run time; a comparison
// with the list's last entry gates the insertion.  The 64 lists are merged by k wave arg-mins over their heads under the same order
// (the winning lane pops): result t lands in lane t, which writes it, and the lanes below k then hold the neighbours' labels for the
// vote -- most occurrences, equal counts to the smallest label value (scikit-learn's uniform-weight predict).
template <int CAP>
__global__ __launch_bounds__(256) void knn_select_kernel(const float* __restrict__ y, int nq, int ng, int ld, const float* __restrict__ qq,
                                                         int k, int* __restrict__ nn_index, float* __restrict__ nn_dist2,
                                                         const int* __restrict__ g_label, int* __restrict__ pred) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nq) return;
    const float* r = y + (size_t)row * ld;
    const float qr = qq ? qq[row] : 0.f;
    float lv[CAP];
    int li[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) { lv[i] = INFINITY; li[i] = 0x7fffffff; }
    for (int j0 = lane; j0 < ng; j0 += 256) {
        float in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) in[u] = j0 + 64 * u < ng ? r[j0 + 64 * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = j0 + 64 * u;
            const float v = qq ? fmaxf(qr + in[u], 0.f) : in[u];
            // better(v, j, entry) for THIS lane's entries: its columns ascend, so an equal value never goes in front of a held one, and
            // an empty entry (INFINITY, the sentinel index) gives way to every candidate, one at distance INFINITY included
            if (j < ng && (v < lv[CAP - 1] || li[CAP - 1] == 0x7fffffff)) {
                bool front[CAP];
#pragma unroll
                for (int i = 0; i < CAP; ++i) front[i] = v < lv[i] || li[i] == 0x7fffffff;
#pragma unroll
                for (int i = CAP - 1; i >= 0; --i) {
                    // entry i takes its upper neighbour when the candidate goes in front of that one, the candidate when it goes exactly here
                    const bool above = i > 0 && front[i > 0 ? i - 1 : 0];
                    lv[i] = above ? lv[i > 0 ? i - 1 : 0] : front[i] ? v : lv[i];
                    li[i] = above ? li[i > 0 ? i - 1 : 0] : front[i] ? j : li[i];
                }
            }
        }
    }
    float out_v = INFINITY;
    int out_i = 0x7fffffff;
    for (int t = 0; t < k; ++t) {
        float bv = lv[0];
        int bi = li[0];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == t) { out_v = bv; out_i = bi; }
        if (li[0] == bi) {                                   // gallery indices are unique: one lane holds the winner (none is left: all hold the sentinel)
#pragma unroll
            for (int i = 0; i + 1 < CAP; ++i) { lv[i] = lv[i + 1]; li[i] = li[i + 1]; }
            lv[CAP - 1] = INFINITY;
            li[CAP - 1] = 0x7fffffff;
        }
    }
    if (lane < k) {
        nn_index[(size_t)row * k + lane] = out_i;
        if (nn_dist2) nn_dist2[(size_t)row * k + lane] = out_v;
    }
    if (!g_label) return;
    const bool found = lane < k && out_i < ng;               // k <= ng results exist; the test keeps the label read in bounds regardless
    const int lab = found ? g_label[out_i] : 0x7fffffff;
    int cnt = 0;
    for (int t = 0; t < k; ++t) {
        const int other = __shfl(lab, t);
        const bool other_found = __shfl((int)found, t) != 0;
        cnt += found && other_found && other == lab;
    }
    int bl = lab;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int oc = __shfl_xor(cnt, m);
        const int ol = __shfl_xor(bl, m);
        if (oc > cnt || (oc == cnt && ol < bl)) { cnt = oc; bl = ol; }
    }
    if (lane == 0) pred[row] = bl;
}

// ---------------------------------------------------------------------------------------------------------------------
// The study's other two k-NN distances (chi2dist and KL_dist, facerec_test.py:157-164, the metric= callables of :275-276 and :424-425).
// Neither is a dot product, so the tile is vector-ALU work: a workgroup takes 64 probe rows x 64 gallery rows, thread (ty, tx) the 4 x 4
// pairs of probe rows ty + 16 i and gallery rows tx + 16 j in registers.  Both row blocks go through the LDS in chunks of METRIC_KC
// columns with a row stride of METRIC_KC + 4 floats: the sixteen gallery rows that the sixteen lanes of one 16-byte LDS read's group ask
// for then start at 36 tx mod 64 dwords, sixteen different 4-bank slots (the group's other operand, a probe row, is one or two
// addresses, which broadcast).  A metric is a functor: PX values per probe element and one per gallery element, computed when a chunk is
// staged (the logs of kl: once per row element and tile, never per pair), and the per-element term.
//
// A distance is a function of its two rows alone: every pair adds its d terms to one accumulator in column order by the same
// instructions, whatever the tile, n, m, ld or the query slice; rows and columns that pad a tile are clamped copies whose results are not
// written, and the columns of a last partial chunk are not visited at all.  Identical gallery rows therefore tie bit for bit, a search
// done in halves gives the same bits, and a NaN sum is written as +INFINITY (knn_select_kernel's order has no place for a NaN).
constexpr int METRIC_KC = 32, METRIC_LD = METRIC_KC + 4;

// chi2: sum_c (x - y)^2 / (x + y) over the columns with x + y > 0 (np.where(sum > 0, ., 0): a zero, negative or NaN sum adds 0).
// Four roundings per term (sum, difference, square, the correctly rounded IEEE quotient: exact wherever the quotient is representable,
// so features in {0, 1, 3} give the integer distances) and d - 1 additions of non-negative terms: |error| <= (d + 3) u D, u = 2^-24.
// Equal rows: every difference is 0, the distance exactly 0.
struct Chi2Metric {
    static constexpr int PX = 1;
    static __device__ __forceinline__ void stage_x(float x, float* v) { v[0] = x; }
    static __device__ __forceinline__ float stage_y(float y) { return y; }
    static __device__ __forceinline__ float add(float acc, const float* x, float y) {
        const float s = x[0] + y, df = x[0] - y;
        const float t = df * df / s;                         // for every s: a select, not a branch per term, drops the others
        return acc + (s > 0.f ? t : 0.f);
    }
};

// kl: sum_c a (log a - log b), a = fl32(x + 0.001f), b = fl32(y + 0.001f) -- (x+0.001)*log((x+0.001)/(y+0.001)) on float32 arrays, not
// symmetric (x the probe, y the gallery row), not clamped at 0.  One logf (ocml's, within 1 ulp = 2 u |log|) serves both sides, so equal
// rows give log a - log b = 0 and the distance exactly 0.  Per term: the two logs 2 u a (|log a| + |log b|), their difference u |t|; the
// product and the addition are one fma, d roundings of partial sums that are at most sum |t|:
// |error| <= u [(d + 1) sum |t_c| + 2 sum a_c (|log a_c| + |log b_c|)].  An entry <= -0.001 has a <= 0 (or b: log b = -inf or NaN): the
// sum is NaN or +inf, written as +INFINITY.
struct KlMetric {
    static constexpr int PX = 2;
    static __device__ __forceinline__ void stage_x(float x, float* v) { v[0] = x + 0.001f; v[1] = logf(v[0]); }
    static __device__ __forceinline__ float stage_y(float y) { return logf(y + 0.001f); }
    static __device__ __forceinline__ float add(float acc, const float* x, float y) { return fmaf(x[0], x[1] - y, acc); }
};

template <class M>
__global__ __launch_bounds__(256) void metric_dist_tile_kernel(const float* __restrict__ q, const float* __restrict__ g, int n, int ng, int d,
                                                               float* __restrict__ out, int ld) {
    __shared__ __attribute__((aligned(16))) float sx[M::PX][64 * METRIC_LD];
    __shared__ __attribute__((aligned(16))) float sy[64 * METRIC_LD];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
    // staging: this thread's 4 columns (lc) of rows lr and lr + 32 of both blocks; rows past the end are copies of the last one
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    const float* qp[2];
    const float* gp[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        qp[h] = q + (size_t)min(i0 + lr + 32 * h, n - 1) * d + lc;
        gp[h] = g + (size_t)min(j0 + lr + 32 * h, ng - 1) * d + lc;
    }
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 rq[2], rg[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {                            // d is a multiple of 4: a thread's 4 columns are inside or outside together
        rq[h] = lc < d ? *(const f32x4*)qp[h] : zero;
        rg[h] = lc < d ? *(const f32x4*)gp[h] : zero;
    }
    for (int c0 = 0; c0 < d; c0 += METRIC_KC) {
        __syncthreads();                                     // the previous chunk has been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 vx[M::PX], vy;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v[M::PX];
                M::stage_x(rq[h][e], v);
#pragma unroll
                for (int p = 0; p < M::PX; ++p) vx[p][e] = v[p];
                vy[e] = M::stage_y(rg[h][e]);
            }
            const int at = (lr + 32 * h) * METRIC_LD + lc;
#pragma unroll
            for (int p = 0; p < M::PX; ++p) *(f32x4*)&sx[p][at] = vx[p];
            *(f32x4*)&sy[at] = vy;
        }
        __syncthreads();
        const int cn = c0 + METRIC_KC + lc;                  // the next chunk's loads fly during this one's arithmetic
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            rq[h] = cn < d ? *(const f32x4*)(qp[h] + c0 + METRIC_KC) : zero;
            rg[h] = cn < d ? *(const f32x4*)(gp[h] + c0 + METRIC_KC) : zero;
        }
        const int kc = min(METRIC_KC, d - c0);
        for (int c = 0; c < kc; c += 4) {
            f32x4 x[4][M::PX], y[4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int p = 0; p < M::PX; ++p) x[i][p] = *(const f32x4*)&sx[p][(ty + 16 * i) * METRIC_LD + c];
#pragma unroll
            for (int j = 0; j < 4; ++j) y[j] = *(const f32x4*)&sy[(tx + 16 * j) * METRIC_LD + c];
#pragma unroll
            for (int e = 0; e < 4; ++e)                      // column order, one accumulator per pair
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float xe[M::PX];
#pragma unroll
                    for (int p = 0; p < M::PX; ++p) xe[p] = x[i][p][e];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = M::add(acc[i][j], xe, y[j][e]);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = i0 + ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = j0 + tx + 16 * j;
            const float v = acc[i][j];
            if (row < n && col < ng) out[(size_t)row * ld + col] = v != v ? INFINITY : v;
        }
    }
}

}  // namespace

int launch_pairwise_dist(const float* x, const float* y, int n, int m, int d, float* out, hipStream_t s) {
    HSEFR_REQUIRE(d > 0 && d % 8 == 0, HSEFR_ERR_UNSUPPORTED, "pairwise_dist: d=%d must be a multiple of 8", d);
    HSEFR_REQUIRE(n >= 0 && m >= 0, HSEFR_ERR_INVALID, "pairwise_dist: bad shape");
    if (n == 0 || m == 0) return HSEFR_OK;
    dim3 grid((m + 63) / 64, (n + 63) / 64), block(256);
    HSEFR_LAUNCH(pairwise_dist_kernel, grid, block, 0, s, x, y, n, m, d, out, x == y ? 1 : 0);
    return launch_status("pairwise_dist");
}

int launch_l2_normalize(const float* x, float* y, int n, int d, hipStream_t s) {
    HSEFR_REQUIRE(n >= 0 && d > 0, HSEFR_ERR_INVALID, "l2_normalize: bad shape");
    if (n == 0) return HSEFR_OK;
    dim3 grid((n + 3) / 4), block(256);
    HSEFR_LAUNCH(l2_normalize_kernel, grid, block, 0, s, x, y, n, d);
    return launch_status("l2_normalize");
}

HSEFR_KNOB(g_nn1_y_mb, "nn1_y_mb", 256, [](int v) { return v > 0 ? v : 1; });      // dev builds: bound of the distance-matrix slice in MiB (tests force several query blocks with a small one)
#define NN1_Y_BYTES ((long long)g_nn1_y_mb << 20)

static std::atomic<long long> g_nn1_fallbacks{0};
long long nn1_fallbacks() { return g_nn1_fallbacks.load(); }

// The split-f16 GEMM search shared by launch_nn1 and launch_knn: its workspace (scaled probes, split gallery, a [block, ng_pad] slice of
// |g|^2 - 2 q.g) is stream-ordered.  The matrix is walked in QUERY BLOCKS so that it stays bounded (NN1_Y_BYTES: 100 000 x 100 000 would
// be 40 GB in one piece -- ADVICE r4); rows are independent, so the blocking changes no bit.  select(y, m, ng_pad, qq, q0) reduces the
// slice of probe rows q0 .. q0 + m (qq = their |q|^2) and returns its status.  Returns false when not even the smallest workspace could be
// had (the caller's allocator may hold the memory) and nothing was launched: the caller runs its other path -- not an error, but COUNTED
// and described, so a perf cliff or a last-bit difference can be traced to it (hsefr_nn1_fallbacks, hsefr_last_error_string).
template <class Select>
static bool split_f16_search(const char* what, const float* q, const float* g, int nq, int ng, int d, hipStream_t s, int& rc, Select select) {
    const int ng_pad = (ng + 63) / 64 * 64;
    const long long y_rows_max = NN1_Y_BYTES / ((long long)ng_pad * 4);
    int qb = (int)(y_rows_max >= nq ? nq : (y_rows_max < 256 ? 256 : y_rows_max / 256 * 256));     // query rows per block
    const size_t b_qs = (size_t)nq * d * 4, b_w = (size_t)ng_pad * d * 4;
    size_t b_y = (size_t)qb * ng_pad * 4;
    const size_t b_small = ((size_t)nq + 2 * (size_t)ng_pad + 64) * 4;
    char* ws = nullptr;
    // a failed allocation is retried with HALF the query block, down to 256 rows (the slice of the distance matrix is
    // the only part of the workspace that can shrink), before the search gives up on this path
    while (hipMallocAsync((void**)&ws, b_qs + b_w + b_y + b_small, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        ws = nullptr;
        if (qb <= 256) break;
        qb = qb / 2 < 256 ? 256 : qb / 2 / 256 * 256;
        b_y = (size_t)qb * ng_pad * 4;
    }
    if (!ws) {
        g_nn1_fallbacks.fetch_add(1);
        set_error("%s: no stream-ordered workspace (%zu bytes) for the split-f16 search of %d x %d x %d; ran the fp32 kernel", what,
                  b_qs + b_w + b_y + b_small, nq, ng, d);
        return false;
    }
    float* qs = (float*)ws;
    unsigned short* w = (unsigned short*)(ws + b_qs);
    float* y = (float*)(ws + b_qs + b_w);
    float* qq = (float*)(ws + b_qs + b_w + b_y);
    float* descale = qq + nq;
    float* shift = descale + ng_pad;
    unsigned* qmax = (unsigned*)(shift + ng_pad);
    rc = HSEFR_OK;
    if (hipMemsetAsync(qmax, 0, 4, s) != hipSuccess) rc = HSEFR_ERR_HIP;
    if (rc == HSEFR_OK) {
        HSEFR_LAUNCH(nn1_prep_queries_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, q, nq, d, qq, qmax);
        HSEFR_LAUNCH(nn1_split_gallery_kernel, dim3((ng_pad + 3) / 4), dim3(256), 0, s, g, ng, ng_pad, d, w, descale, shift, qmax);
        const long long n4 = (long long)nq * d / 4;
        HSEFR_LAUNCH(nn1_scale_queries_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, q, qs, n4, qmax);
        rc = launch_status("split-f16 search preparation");
    }
    for (int q0 = 0; q0 < nq && rc == HSEFR_OK; q0 += qb) {
        const int m = nq - q0 < qb ? nq - q0 : qb;
        rc = launch_pwconv_f16s(qs + (size_t)q0 * d, w, descale, shift, y, m, d, ng_pad, 12, HSEFR_ACT_NONE, s);
        if (rc == HSEFR_OK) rc = select(y, m, ng_pad, qq + q0, q0);
    }
    (void)hipFreeAsync(ws, s);
    return true;
}

static bool split_f16_shape(int nq, int ng, int d) { return d % 32 == 0 && (long long)nq * ng * d >= (1ll << 28); }

int launch_nn1(const float* q, const float* g, int nq, int ng, int d, int* nn_index, float* nn_dist2, hipStream_t s) {
    HSEFR_REQUIRE(d > 0 && d % 8 == 0, HSEFR_ERR_UNSUPPORTED, "nn1: d=%d must be a multiple of 8", d);
    HSEFR_REQUIRE(nq >= 0 && ng > 0, HSEFR_ERR_INVALID, "nn1: nq=%d ng=%d", nq, ng);
    if (nq == 0) return HSEFR_OK;
    int rc;
    if (split_f16_shape(nq, ng, d) &&
        split_f16_search("nn1", q, g, nq, ng, d, s, rc, [&](const float* y, int m, int ng_pad, const float* qq, int q0) {
            HSEFR_LAUNCH(nn1_row_argmin_kernel, dim3((m + 3) / 4), dim3(256), 0, s, y, m, ng, ng_pad, qq, nn_index + q0,
                               nn_dist2 ? nn_dist2 + q0 : nullptr);
            return launch_status("nn1 (row arg-min)");
        }))
        return rc;
    // every other search, and a large one without workspace, runs on nn1_kernel (no workspace; another summation order, far slower at
    // large sizes)
    dim3 grid((nq + 31) / 32), block(256);
    HSEFR_LAUNCH(nn1_kernel, grid, block, 0, s, q, g, nq, ng, d, nn_index, nn_dist2);
    return launch_status("nn1");
}

static int launch_knn_select(const float* y, int m, int ng, int ld, const float* qq, int k, int* nn_index, float* nn_dist2,
                             const int* g_label, int* pred, hipStream_t s) {
    // the list capacity is the kernel's cost in registers and in insertion work (nearly every column enters the list of SOME lane of its
    // wave): 4 entries serve the reference's 3-NN, 16 every k the entry point takes
    if (k <= 4) HSEFR_LAUNCH(knn_select_kernel<4>, dim3((m + 3) / 4), dim3(256), 0, s, y, m, ng, ld, qq, k, nn_index, nn_dist2, g_label, pred);
    else if (k <= 8) HSEFR_LAUNCH(knn_select_kernel<8>, dim3((m + 3) / 4), dim3(256), 0, s, y, m, ng, ld, qq, k, nn_index, nn_dist2, g_label, pred);
    else HSEFR_LAUNCH(knn_select_kernel<16>, dim3((m + 3) / 4), dim3(256), 0, s, y, m, ng, ld, qq, k, nn_index, nn_dist2, g_label, pred);
    return launch_status("knn (selection)");
}

constexpr int KNN_GRID_ROWS = 65535 * 64;                   // the distance-tile kernels' grid.y, in rows

// The searches on finished distance tiles: a stream-ordered slice y [qb, ng] of the distance matrix, of query rows bounded (NN1_Y_BYTES)
// and halved on a failed allocation like the GEMM path's, down to 64 rows; tiles(q0, m, y) launches the distances of probe rows
// q0 .. q0 + m into it, select(y, m, ng, nullptr, q0) reduces them.  Rows are independent, so the walk changes no bit.
template <class Select, class Tiles>
static int knn_slice_walk(const char* what, int nq, int ng, hipStream_t s, Select select, Tiles tiles) {
    const long long rows_max = NN1_Y_BYTES / ((long long)ng * 4);
    int qb = (int)(rows_max >= nq ? nq : (rows_max < 64 ? 64 : rows_max / 64 * 64));
    if (qb > KNN_GRID_ROWS) qb = KNN_GRID_ROWS;
    float* y = nullptr;
    while (hipMallocAsync((void**)&y, (size_t)qb * ng * 4, s) != hipSuccess || !y) {
        (void)hipGetLastError();
        y = nullptr;
        if (qb <= 64) break;
        qb = qb / 2 < 64 ? 64 : qb / 2 / 64 * 64;
    }
    HSEFR_REQUIRE(y, HSEFR_ERR_NOMEM, "%s: no stream-ordered workspace (%zu bytes) for a %d-row slice of the %d x %d distance matrix", what,
                  (size_t)qb * ng * 4, qb, nq, ng);
    int rc = HSEFR_OK;
    for (int q0 = 0; q0 < nq && rc == HSEFR_OK; q0 += qb) {
        const int m = nq - q0 < qb ? nq - q0 : qb;
        tiles(q0, m, y);
        rc = launch_status("knn (distance tiles)");
        if (rc == HSEFR_OK) rc = select(y, m, ng, nullptr, q0);
    }
    (void)hipFreeAsync(y, s);
    return rc;
}

int launch_knn(const float* q, const float* g, int nq, int ng, int d, int k, int* nn_index, float* nn_dist2, const int* g_label, int* pred,
               hipStream_t s) {
    HSEFR_REQUIRE(d > 0 && d % 8 == 0, HSEFR_ERR_UNSUPPORTED, "knn: d=%d must be a multiple of 8", d);
    HSEFR_REQUIRE(nq >= 0 && ng > 0 && ng <= 0x7fffffff - 512, HSEFR_ERR_INVALID, "knn: nq=%d ng=%d", nq, ng);
    HSEFR_REQUIRE(k >= 1 && k <= 16 && k <= ng, HSEFR_ERR_INVALID, "knn: k=%d must be in 1..16 and at most ng=%d", k, ng);
    if (nq == 0) return HSEFR_OK;
    const auto select = [&](const float* y, int m, int ld, const float* qq, int q0) {
        return launch_knn_select(y, m, ng, ld, qq, k, nn_index + (size_t)q0 * k, nn_dist2 ? nn_dist2 + (size_t)q0 * k : nullptr, g_label,
                                 pred ? pred + q0 : nullptr, s);
    };
    int rc;
    if (split_f16_shape(nq, ng, d) && split_f16_search("knn", q, g, nq, ng, d, s, rc, select)) return rc;
    // every other search (small by definition), and a large one without workspace: finished fp32 distances, nn1_kernel's own bits, then
    // the same selection.  A list of k candidates for each of nn1_kernel's 16 accumulator rows per lane would not fit its registers.
    return knn_slice_walk("knn", nq, ng, s, select, [&](int q0, int m, float* y) {
        HSEFR_LAUNCH(knn_dist2_tile_kernel, dim3((ng + 63) / 64, (m + 63) / 64), dim3(256), 0, s, q + (size_t)q0 * d, g, m, ng, d, y, ng);
    });
}

// metric: HSEFR_METRIC_CHI2 or HSEFR_METRIC_KL (checked by the callers); the tiles of probe rows x [n,d] against y [m,d] into out, row stride ld
static void launch_metric_tiles(int metric, const float* x, const float* y, int n, int m, int d, float* out, int ld, hipStream_t s) {
    const dim3 grid((m + 63) / 64, (n + 63) / 64), block(256);
    if (metric == HSEFR_METRIC_CHI2) HSEFR_LAUNCH(metric_dist_tile_kernel<Chi2Metric>, grid, block, 0, s, x, y, n, m, d, out, ld);
    else HSEFR_LAUNCH(metric_dist_tile_kernel<KlMetric>, grid, block, 0, s, x, y, n, m, d, out, ld);
}

static int check_metric_args(const char* what, int metric, int d) {
    HSEFR_REQUIRE(metric == HSEFR_METRIC_CHI2 || metric == HSEFR_METRIC_KL, HSEFR_ERR_INVALID,
                  "%s: metric=%d must be HSEFR_METRIC_CHI2 (1) or HSEFR_METRIC_KL (2)", what, metric);
    HSEFR_REQUIRE(d > 0 && d % 4 == 0, HSEFR_ERR_INVALID, "%s: d=%d must be a positive multiple of 4", what, d);
    return HSEFR_OK;
}

int launch_metric_dist(const float* x, const float* y, int n, int m, int d, int metric, float* out, hipStream_t s) {
    if (const int rc = check_metric_args("metric_dist", metric, d)) return rc;
    HSEFR_REQUIRE(n >= 0 && m >= 0 && n <= KNN_GRID_ROWS, HSEFR_ERR_INVALID, "metric_dist: n=%d m=%d (n at most %d)", n, m, KNN_GRID_ROWS);
    if (n == 0 || m == 0) return HSEFR_OK;
    launch_metric_tiles(metric, x, y, n, m, d, out, m, s);
    return launch_status("metric_dist");
}

int launch_knn_metric(const float* q, const float* g, int nq, int ng, int d, int k, int metric, int* nn_index, float* nn_dist, const int* g_label,
                      int* pred, hipStream_t s) {
    if (const int rc = check_metric_args("knn_metric", metric, d)) return rc;
    HSEFR_REQUIRE(nq >= 0 && ng > 0 && ng <= 0x7fffffff - 512, HSEFR_ERR_INVALID, "knn_metric: nq=%d ng=%d", nq, ng);
    HSEFR_REQUIRE(k >= 1 && k <= 16 && k <= ng, HSEFR_ERR_INVALID, "knn_metric: k=%d must be in 1..16 and at most ng=%d", k, ng);
    if (nq == 0) return HSEFR_OK;
    const auto select = [&](const float* y, int m, int ld, const float* qq, int q0) {
        return launch_knn_select(y, m, ng, ld, qq, k, nn_index + (size_t)q0 * k, nn_dist ? nn_dist + (size_t)q0 * k : nullptr, g_label,
                                 pred ? pred + q0 : nullptr, s);
    };
    return knn_slice_walk("knn_metric", nq, ng, s, select,
                          [&](int q0, int m, float* y) { launch_metric_tiles(metric, q + (size_t)q0 * d, g, m, ng, d, y, ng, s); });
}

}  // namespace hsefr
