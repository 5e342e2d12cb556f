// libhsefr_affinity.so (include/hsefr_affinity.h): sklearn.cluster.AffinityPropagation(...).fit on the device -- the last of the three fits
// the clustering study's scikit-learn branch names (facial_clustering_test.py:263), scikit-learn 1.7.2's _affinity_propagation operation by
// operation in fp64.
//
// State, all in the caller's workspace: S, A, R [n,n] fp64 (S with the preference on its diagonal and the noise added), the partial column
// sums [row blocks, n] and the column sums [n] of Rp = max(R, 0) with R's own diagonal, one 64-bit word of exemplar decisions per point,
// and O(n) words of the finish.  The start is: ap_norms_kernel + ap_sim_kernel (features: S = -|x_i - x_j|^2 on the fp64 MFMA) or
// ap_copy_kernel (dense), ap_minmax_kernel (are all off-diagonal similarities equal?), eight passes of ap_hist_kernel + ap_digit_kernel
// (the median: a radix select of the two middle entries on order-preserving keys), ap_prepare_kernel (the preference onto the diagonal,
// the noise).  An iteration is three launches:
//   ap_sweep_kernel    a workgroup per block of rows, a row at a time in two sweeps.  Sweep 1 finishes A's update of the PREVIOUS
//                      iteration (from R, the column sums and A as they stand), writes A, keeps S_ij in the row's LDS copy and reduces
//                      A_ij + S_ij to Y, Y2 and I.  Sweep 2 writes the new R from the LDS row and adds Rp into the thread's column sums,
//                      which stay in registers over the block's rows and are stored once: the block's partial sums
//   ap_colsum_kernel   a thread per column: the partial sums added in one fixed order, the diagonal of A's update (the same expression sweep 1
//                      will store), A_kk + R_kk, its sign shifted into the point's history
//   ap_stop_kernel     one workgroup: scikit-learn's stop test over the histories; the host reads its verdict (64 bytes)
// and the finish is ap_select_kernel (the exemplars in order), ap_assign_kernel (each point's exemplar of largest S), ap_member_sum_kernel +
// ap_winner_kernel + ap_relist_kernel (the refinement), ap_assign_kernel again, ap_select_kernel again (the refined exemplars ascending)
// and ap_labels_kernel.
//
// Nothing one workgroup writes is read by another in the same launch.  No grid-wide barriers, no cooperative launches, no spin-waits, no
// floating-point atomics; the integer atomics count or take an integer minimum / maximum, whose results do not depend on their order.
// An index read from device memory is compared with its bound before it is used; one out of bounds raises ctl[CTL_INTERNAL] and is not
// followed.  Every store is a vector store from plain C++.
#include <algorithm>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "common.h"
#include "lib_error.h"
#include "../../include/hsefr_affinity.h"

// scikit-learn's expressions round every operation on its own: no product is fused with the sum behind it anywhere in this file (the
// MFMA builtin is no contraction and is not affected)
#pragma clang fp contract(off)

namespace hsefr {

namespace {

typedef double ap_f64x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int TM = 32, TN = 64, TK = 16;             // a workgroup's tile of the product: 32 rows x 64 columns, 16 of the sum per LDS tile
constexpr int NONE = 0x7fffffff;
constexpr int CUS = 256;                             // compute units of an MI355X: what the row blocks are sized for (speed only)
constexpr int RADIX_PASSES = 8;                      // 8 bits of the key per pass
// where sweep 2 finds the row's similarities: in the workgroup's LDS copy (the product), or read again from memory (-DHSEFR_AFFINITY_ROW_IN_LDS=0,
// the alternative profiles/affinity_time.txt holds a time of: no LDS, so nothing but the threads bounds the workgroups of a CU)
#ifndef HSEFR_AFFINITY_ROW_IN_LDS
#define HSEFR_AFFINITY_ROW_IN_LDS 1
#endif
constexpr bool ROW_IN_LDS = HSEFR_AFFINITY_ROW_IN_LDS != 0;
// the control block: what the kernels report and the host reads
enum { CTL_NONFINITE = 0, CTL_INTERNAL = 1, CTL_STOP = 2, CTL_K = 3, CTL_UNCONVERGED = 4, CTL_WORDS = 16 };
// the 64-bit words beside it
enum { SEL_PREFIX = 0, SEL_RANK = 2, SEL_MIN = 4, SEL_MAX = 5, SEL_PREF = 6, SEL_WORDS = 8 };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// order-preserving key of a double that is no NaN (-0.0 counts as +0.0), and back
__device__ __forceinline__ u64 key_of(double v) {
    const u64 u = (u64)__double_as_longlong(v + 0.0);
    return u >> 63 ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double value_of(u64 k) {
    return __longlong_as_double((long long)(k >> 63 ? k & 0x7fffffffffffffffull : ~k));
}

// the header's noise factor g(seed, e)
__device__ __forceinline__ double noise_factor(u64 seed_term, u64 e) {
    u64 z = e + seed_term;
    z = (z ^ (z >> 30)) * HSEFR_AFFINITY_HASH_MUL1;
    z = (z ^ (z >> 27)) * HSEFR_AFFINITY_HASH_MUL2;
    z = z ^ (z >> 31);
    const double u = ((double)(z >> 12) + 0.5) * 0x1p-52;
    return (u * 2.0 - 1.0) * HSEFR_AFFINITY_SQRT3;
}

// ---- the similarities of the features ---------------------------------------------------------------------------------------------------
// the squared norms, a wave per row (d is a multiple of 4: a lane's pair is one 8-byte load)
__global__ __launch_bounds__(256) void ap_norms_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ xn, int* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    double s = 0.0;
    bool bad = false;
    for (int c = 2 * lane; c < d; c += 128) {
        const float2 f = *(const float2*)(x + (size_t)row * d + c);
        bad |= !(isfinite(f.x) && isfinite(f.y));
        s += (double)f.x * (double)f.x;
        s += (double)f.y * (double)f.y;
    }
    s = wave_sum(s);
    if (bad) ctl[CTL_NONFINITE] = 1;                 // (every writer stores the same 1)
    if (lane == 0) xn[row] = s;
}

__device__ __forceinline__ double x_load(const float* __restrict__ x, int row, int k, int n, int d) {
    return row < n && k < d ? (double)x[(size_t)row * d + k] : 0.0;
}

// S[i][j] = 0 - max(0, (N_i + N_j) - 2 <x_i, x_j>), S[i][i] = 0: 32 rows x 64 columns per workgroup (256 threads = 4 waves: wave w owns rows
// 16 (w & 1) .. and columns 32 (w >> 1) .., two 16 x 16 MFMA tiles).  Lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][column
// l & 15]; result register g of lane l is row (l >> 4) + 4 g, column l & 15.  An element's sum over k has one shape wherever its tile
// lies, and <x_i, x_j> and <x_j, x_i> are the same products added in the same order.  grid (ceil(n / 32), ceil(n / 64))
__global__ __launch_bounds__(256) void ap_sim_kernel(const float* __restrict__ x, const double* __restrict__ xn, int n, int d, double* __restrict__ S) {
    __shared__ double As[TK][TM + 1];
    __shared__ double Bs[TK][TN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32, r = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    const int kk = tid & 15, rr = tid >> 4;          // this thread's elements of a tile: column kk of rows rr + 16 e
    double va[TM / 16], vb[TN / 16];
#pragma unroll
    for (int e = 0; e < TM / 16; ++e) va[e] = x_load(x, m0 + rr + 16 * e, kk, n, d);
#pragma unroll
    for (int e = 0; e < TN / 16; ++e) vb[e] = x_load(x, n0 + rr + 16 * e, kk, n, d);
    ap_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += TK) {
        __syncthreads();                             // the previous tile has been read
#pragma unroll
        for (int e = 0; e < TM / 16; ++e) As[kk][rr + 16 * e] = va[e];
#pragma unroll
        for (int e = 0; e < TN / 16; ++e) Bs[kk][rr + 16 * e] = vb[e];
        __syncthreads();
        if (k0 + TK < d) {                           // the next tile travels while this one is multiplied
#pragma unroll
            for (int e = 0; e < TM / 16; ++e) va[e] = x_load(x, m0 + rr + 16 * e, k0 + TK + kk, n, d);
#pragma unroll
            for (int e = 0; e < TN / 16; ++e) vb[e] = x_load(x, n0 + rr + 16 * e, k0 + TK + kk, n, d);
        }
#pragma unroll
        for (int k = 0; k < TK; k += 4) {
            const double a = As[k + q][wm + r];
            const double b0v = Bs[k + q][wn + r], b1v = Bs[k + q][wn + 16 + r];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0v, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1v, acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const ap_f64x4 acc = t ? acc1 : acc0;
        const int j = n0 + wn + 16 * t + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = m0 + wm + q + 4 * g;
            if (i < n && j < n) S[(size_t)i * n + j] = i == j ? 0.0 : 0.0 - fmax(0.0, (xn[i] + xn[j]) - 2.0 * acc[g]);
        }
    }
}

// the dense path: the caller's matrix is copied, and a NaN or an infinity in it is reported
__global__ __launch_bounds__(256) void ap_copy_kernel(const double* __restrict__ src, size_t total, double* __restrict__ S, int* __restrict__ ctl) {
    bool bad = false;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const double v = src[e];
        bad |= !isfinite(v);
        S[e] = v;
    }
    if (bad) ctl[CTL_NONFINITE] = 1;
}

// the least and the largest off-diagonal similarity, as keys (sel[SEL_MIN] starts at all ones, sel[SEL_MAX] at 0)
__global__ __launch_bounds__(256) void ap_minmax_kernel(const double* __restrict__ S, int n, u64* __restrict__ sel) {
    __shared__ u64 s_lo[4], s_hi[4];
    const size_t total = (size_t)n * n;
    u64 lo = ~0ull, hi = 0ull;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        if (e % ((size_t)n + 1) == 0) continue;      // the diagonal
        const u64 k = key_of(S[e]);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const u64 ol = __shfl_xor(lo, o), oh = __shfl_xor(hi, o);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        atomicMin(&sel[SEL_MIN], lo);
        atomicMax(&sel[SEL_MAX], hi);
    }
}

// ---- the median: a radix select of the entries of ranks sel[SEL_RANK], sel[SEL_RANK + 1] among the n^2 keys ------------------------------
// pass p counts, for each of the two ranks, the digit (bits 56 - 8 p .. 63 - 8 p) of the keys whose higher bits equal the rank's prefix
__global__ __launch_bounds__(256) void ap_hist_kernel(const double* __restrict__ S, size_t total, int pass, const u64* __restrict__ sel,
                                                      unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[2][256];
    s_hist[0][threadIdx.x] = 0;
    s_hist[1][threadIdx.x] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 p0 = sel[SEL_PREFIX], p1 = sel[SEL_PREFIX + 1];
    const bool one = p0 == p1;                       // both ranks still in one bucket: count once
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const u64 k = key_of(S[e]);
        const unsigned digit = (unsigned)(k >> shift) & 255u;
        const u64 high0 = pass ? (k ^ p0) >> (shift + 8) : 0ull, high1 = pass ? (k ^ p1) >> (shift + 8) : 0ull;
        if (high0 == 0ull) atomicAdd(&s_hist[0][digit], 1u);
        if (!one && high1 == 0ull) atomicAdd(&s_hist[1][digit], 1u);
    }
    __syncthreads();
    unsigned* out = hist + (size_t)pass * 512;
    if (s_hist[0][threadIdx.x]) atomicAdd(&out[threadIdx.x], s_hist[0][threadIdx.x]);
    if (s_hist[1][threadIdx.x]) atomicAdd(&out[256 + threadIdx.x], s_hist[1][threadIdx.x]);
}

// the digit of each rank: the bucket its rank falls into; the rank becomes the rank within the bucket.  After the last pass the prefixes
// are the two keys, and the preference is the fp64 mean of their values (np.median); an explicit preference stands as given
__global__ void ap_digit_kernel(int pass, u64* __restrict__ sel, const unsigned* __restrict__ hist, int* __restrict__ ctl) {
    if (threadIdx.x != 0) return;
    const int shift = 56 - 8 * pass;
    const bool one = sel[SEL_PREFIX] == sel[SEL_PREFIX + 1];
    for (int r = 0; r < 2; ++r) {
        const unsigned* h = hist + (size_t)pass * 512 + (one ? 0 : 256 * r);
        u64 rank = sel[SEL_RANK + r], cum = 0;
        int digit = -1;
        for (int b = 0; b < 256; ++b) {
            if (rank < cum + h[b]) {
                digit = b;
                break;
            }
            cum += h[b];
        }
        if (digit < 0) {                             // (the counts do not hold the rank: not followed)
            ctl[CTL_INTERNAL] = 1;
            digit = 0;
            cum = rank;
        }
        sel[SEL_RANK + r] = rank - cum;
        sel[SEL_PREFIX + r] |= (u64)digit << shift;
    }
    if (pass == RADIX_PASSES - 1) {
        const double lo = value_of(sel[SEL_PREFIX]), hi = value_of(sel[SEL_PREFIX + 1]);
        sel[SEL_PREF] = (u64)__double_as_longlong((lo + hi) / 2.0);
    }
}

// S's diagonal = the preference, then the noise over the whole matrix (seed_on == 0: the diagonal only)
__global__ __launch_bounds__(256) void ap_prepare_kernel(double* __restrict__ S, int n, const u64* __restrict__ sel, int seed_on, u64 seed_term) {
    const double pref = __longlong_as_double((long long)sel[SEL_PREF]);
    const size_t total = (size_t)n * n;
    if (!seed_on) {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)n; i += (size_t)gridDim.x * 256) S[i * n + i] = pref;
        return;
    }
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const double s = e % ((size_t)n + 1) == 0 ? pref : S[e];
        S[e] = s + (0x1p-52 * s + 100.0 * DBL_MIN) * noise_factor(seed_term, (u64)e);
    }
}

// ---- an iteration -----------------------------------------------------------------------------------------------------------------------
struct Top {                                         // a row's largest value, where it stands first, and the largest of the others
    double y, y2;
    int i;
};
__device__ __forceinline__ Top top_merge(const Top a, const Top b) {
    Top o;
    if (a.y > b.y || (a.y == b.y && a.i < b.i)) {
        o.y = a.y;
        o.i = a.i;
        o.y2 = fmax(a.y2, b.y);
    } else {
        o.y = b.y;
        o.i = b.i;
        o.y2 = fmax(b.y2, a.y);
    }
    return o;
}

// Thread t owns the columns t + e * blockDim.x, e < EPT (EPT * blockDim.x >= n); the workgroup walks rows row0 .. row0 + rows_per - 1.
// Dynamic LDS: the row of n doubles.  damp / rest: damping and 1 - damping as the host rounds them.  cs: the column sums of the previous
// iteration's Rp (zeros before the first, as A and R).  part[blockIdx.x][j]: this block's sum of Rp_ij in row order
template <int EPT>
__global__ __launch_bounds__(1024) void ap_sweep_kernel(const double* __restrict__ S, double* __restrict__ A, double* __restrict__ R,
                                                        const double* __restrict__ cs, double* __restrict__ part, int n, int rows_per,
                                                        double damp, double rest) {
    extern __shared__ __attribute__((aligned(16))) double s_row[];
    __shared__ Top s_top[16];
    __shared__ Top s_all;
    const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wave = tid >> 6, waves = T >> 6;
    const int row0 = blockIdx.x * rows_per, row1 = min(row0 + rows_per, n);
    double sum[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) sum[e] = 0.0;
    for (int i = row0; i < row1; ++i) {
        const size_t at = (size_t)i * n;
        Top top = {-INFINITY, -INFINITY, NONE};
#pragma unroll 4                                     // (not EPT: sixteen columns' loads in flight at once do not fit the registers of 1024 threads)
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * T;
            if (j < n) {
                const double r = R[at + j], s = S[at + j];
                // tmp = Rp - column sum; its diagonal is kept, the rest clipped; A = A * damping - tmp * (1 - damping)
                double t = (i == j ? r : fmax(r, 0.0)) - cs[j];
                if (i != j) t = fmin(fmax(t, 0.0), INFINITY);
                const double a = A[at + j] * damp - t * rest;
                A[at + j] = a;
                if (ROW_IN_LDS) s_row[j] = s;
                const double v = a + s;
                if (v > top.y) {                     // (j rises: the first of equal values stays)
                    top.y2 = top.y;
                    top.y = v;
                    top.i = j;
                } else {
                    top.y2 = fmax(top.y2, v);
                }
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            Top other;
            other.y = __shfl_xor(top.y, o);
            other.y2 = __shfl_xor(top.y2, o);
            other.i = __shfl_xor(top.i, o);
            top = top_merge(top, other);
        }
        if (lane == 0) s_top[wave] = top;
        __syncthreads();
        if (tid == 0) {
            Top all = s_top[0];
            for (int w = 1; w < waves; ++w) all = top_merge(all, s_top[w]);
            s_all = all;
        }
        __syncthreads();
        const Top all = s_all;
        // R = R * damping + (S - Y, or S - Y2 at I) * (1 - damping); Rp = max(R, 0) with R's own diagonal
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * T;
            if (j < n) {
                const double s = ROW_IN_LDS ? s_row[j] : S[at + j];
                const double r = R[at + j] * damp + (s - (j == all.i ? all.y2 : all.y)) * rest;
                R[at + j] = r;
                sum[e] += i == j ? r : fmax(r, 0.0);
            }
        }
        __syncthreads();                             // s_row, s_top and s_all are free for the next row
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int j = tid + e * T;
        if (j < n) part[(size_t)blockIdx.x * n + j] = sum[e];
    }
}

// a thread per column k: cs[k] = the blocks' partial sums in one fixed order; the diagonal of A's update as the next sweep will store it;
// diag[k] = A_kk + R_kk; its sign enters the history
__global__ __launch_bounds__(256) void ap_colsum_kernel(const double* __restrict__ part, int blocks, const double* __restrict__ A,
                                                        const double* __restrict__ R, int n, double damp, double rest, double* __restrict__ cs,
                                                        double* __restrict__ diag, u64* __restrict__ history, int* __restrict__ eflag) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;    // four running sums over the blocks b = 0, 1, 2, 3 (mod 4): four loads in flight
    int b = 0;
    for (; b + 3 < blocks; b += 4) {
        s0 += part[(size_t)b * n + k];
        s1 += part[(size_t)(b + 1) * n + k];
        s2 += part[(size_t)(b + 2) * n + k];
        s3 += part[(size_t)(b + 3) * n + k];
    }
    for (; b < blocks; ++b) s0 += part[(size_t)b * n + k];
    const double s = (s0 + s1) + (s2 + s3);
    cs[k] = s;
    const double r = R[(size_t)k * n + k];
    const double a = A[(size_t)k * n + k] * damp - (r - s) * rest;
    const double v = a + r;
    diag[k] = v;
    history[k] = history[k] << 1 | (v > 0.0 ? 1ull : 0ull);
    eflag[k] = v > 0.0;
}

// scikit-learn's stop test (one workgroup): from iteration convergence_iter on, every point's last convergence_iter decisions are equal
// and there is an exemplar
__global__ __launch_bounds__(1024) void ap_stop_kernel(const u64* __restrict__ history, int n, int it, int convergence_iter, int* __restrict__ ctl) {
    __shared__ int s_un, s_k;
    if (threadIdx.x == 0) s_un = s_k = 0;
    __syncthreads();
    const u64 mask = convergence_iter >= 64 ? ~0ull : (1ull << convergence_iter) - 1ull;
    int un = 0, k = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const u64 h = history[i] & mask;
        un += h != 0ull && h != mask;
        k += (int)(history[i] & 1ull);
    }
    if (un) atomicAdd(&s_un, un);
    if (k) atomicAdd(&s_k, k);
    __syncthreads();
    if (threadIdx.x == 0) {
        ctl[CTL_UNCONVERGED] = s_un;
        ctl[CTL_K] = s_k;
        ctl[CTL_STOP] = it >= convergence_iter && s_un == 0 && s_k > 0;
    }
}

// ---- the finish -------------------------------------------------------------------------------------------------------------------------
// the flagged points in index order are the list; pos[i] = a flagged point's place in it, -1 for the others; one workgroup
__global__ __launch_bounds__(256) void ap_select_kernel(const int* __restrict__ flag, int n, int* __restrict__ list, int* __restrict__ pos,
                                                        int* __restrict__ count) {
    __shared__ int s_at[257];
    const int t = threadIdx.x, per = (n + 255) / 256;
    const int b = min(t * per, n), e = min(b + per, n);
    int c = 0;
    for (int i = b; i < e; ++i) c += flag[i] != 0;
    s_at[t + 1] = c;
    __syncthreads();
    if (t == 0) {
        s_at[0] = 0;
        for (int i = 1; i <= 256; ++i) s_at[i] += s_at[i - 1];
        *count = s_at[256];
    }
    __syncthreads();
    int o = s_at[t];
    for (int i = b; i < e; ++i) {
        if (flag[i] != 0) {
            list[o] = i;
            pos[i] = o++;
        } else {
            pos[i] = -1;
        }
    }
}

// a wave per point i: c[i] = the place k of the exemplar list[k] of largest S[i][list[k]], the first among equal values; an exemplar is
// assigned to itself
__global__ __launch_bounds__(256) void ap_assign_kernel(const double* __restrict__ S, int n, const int* __restrict__ list, const int* __restrict__ pos,
                                                        int K, int* __restrict__ c, int* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double best = -INFINITY;
    int bk = NONE;
    for (int k = lane; k < K; k += 64) {
        const int j = list[k];
        if ((unsigned)j >= (unsigned)n) {
            ctl[CTL_INTERNAL] = 1;
            continue;
        }
        const double v = S[(size_t)i * n + j];
        if (v > best || bk == NONE) {                // (k rises: the first of equal values stays)
            best = v;
            bk = k;
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double ov = __shfl_xor(best, o);
        const int ok = __shfl_xor(bk, o);
        if (ok != NONE && (bk == NONE || ov > best || (ov == best && ok < bk))) {
            best = ov;
            bk = ok;
        }
    }
    if (lane == 0) {
        const int own = pos[i];
        int k = own >= 0 ? own : bk;
        if ((unsigned)k >= (unsigned)K) {
            ctl[CTL_INTERNAL] = 1;
            k = 0;
        }
        c[i] = k;
    }
}

// a wave per point j of cluster k = c[j]: the sum of S[i][j] over the cluster's members i -- 64 members at a time in index order, a
// fixed tree within the 64, the chunks' sums added in order -- and the largest such sum of the cluster, as a key
__global__ __launch_bounds__(256) void ap_member_sum_kernel(const double* __restrict__ S, int n, const int* __restrict__ c, int K,
                                                            double* __restrict__ sums, u64* __restrict__ best) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const int k = c[j];
    double total = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool member = i < n && c[i] == k;
        if (__ballot(member) == 0ull) continue;      // (a chunk without a member would add zeros)
        total += wave_sum(member ? S[(size_t)i * n + j] : 0.0);
    }
    if (lane == 0) {
        sums[j] = total;
        if ((unsigned)k < (unsigned)K) atomicMax(&best[k], key_of(total));
    }
}
// the first member whose sum is its cluster's largest (winner starts at all ones)
__global__ __launch_bounds__(256) void ap_winner_kernel(const double* __restrict__ sums, const int* __restrict__ c, const u64* __restrict__ best,
                                                        int n, int K, unsigned* __restrict__ winner) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int k = c[j];
    if ((unsigned)k < (unsigned)K && key_of(sums[j]) == best[k]) atomicMin(&winner[k], (unsigned)j);
}
// the refined exemplars in cluster order: list2[k] = cluster k's winner, pos2 its place (pos2 starts at -1, flag2 at 0)
__global__ __launch_bounds__(256) void ap_relist_kernel(const unsigned* __restrict__ winner, int K, int n, int* __restrict__ list2,
                                                        int* __restrict__ pos2, int* __restrict__ flag2, int* __restrict__ ctl) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    unsigned w = winner[k];
    if (w >= (unsigned)n) {                          // (a cluster without a member: its exemplar is one)
        ctl[CTL_INTERNAL] = 1;
        w = 0;
    }
    list2[k] = (int)w;
    pos2[w] = k;
    flag2[w] = 1;
}
// labels[i] = the place of the point's refined exemplar among the exemplars in ascending order
__global__ __launch_bounds__(256) void ap_labels_kernel(const int* __restrict__ c, const int* __restrict__ list2, const int* __restrict__ rank,
                                                        int n, int K, int* __restrict__ labels, int* __restrict__ ctl) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = c[i];
    int label = -1;
    if ((unsigned)k < (unsigned)K) {
        const int e = list2[k];
        if ((unsigned)e < (unsigned)n) label = rank[e];
    }
    if ((unsigned)label >= (unsigned)K) {
        ctl[CTL_INTERNAL] = 1;
        label = -1;
    }
    labels[i] = label;
}

// the answers that need no iteration: every label -1 (mode 0), every point its own exemplar (mode 1), one cluster around point 0 (mode 2);
// mode 3 decides between 1 and 2 as scikit-learn does for equal similarities: n clusters if the preference exceeds S.flat[n - 1]
__global__ __launch_bounds__(256) void ap_trivial_kernel(int mode, const double* __restrict__ S, const u64* __restrict__ sel, int n,
                                                         int* __restrict__ exemplars, int* __restrict__ labels, double* __restrict__ diag,
                                                         int* __restrict__ ctl) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (mode == 3) {
        mode = __longlong_as_double((long long)sel[SEL_PREF]) > S[n - 1] ? 1 : 2;
        if (i == 0) ctl[CTL_K] = mode == 1 ? n : 1;
    }
    if (i >= n) return;
    if (mode == 0) {
        labels[i] = -1;
        return;
    }
    labels[i] = mode == 1 ? i : 0;
    if (mode == 1 || i == 0) exemplars[i] = i;
    diag[i] = 0.0;
}

__global__ void ap_info_kernel(const int* __restrict__ ctl, const u64* __restrict__ sel, int K, int n_iter, int converged, int equal,
                               int* __restrict__ info, double* __restrict__ preference) {
    const int t = threadIdx.x;
    if (t == 0) *preference = __longlong_as_double((long long)sel[SEL_PREF]);
    if (t >= HSEFR_AFFINITY_INFO_WORDS) return;
    int v = 0;
    if (t == HSEFR_AFFINITY_INFO_CLUSTERS) v = K;
    if (t == HSEFR_AFFINITY_INFO_N_ITER) v = n_iter;
    if (t == HSEFR_AFFINITY_INFO_CONVERGED) v = converged;
    if (t == HSEFR_AFFINITY_INFO_EQUAL) v = equal;
    if (t == HSEFR_AFFINITY_INFO_NONFINITE) v = ctl[CTL_NONFINITE];
    if (t == HSEFR_AFFINITY_INFO_INTERNAL) v = ctl[CTL_INTERNAL];
    info[t] = v;
}

// ---- the host -------------------------------------------------------------------------------------------------------------------------
constexpr size_t ALIGN = 256;
size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

// how the rows are dealt to the workgroups of ap_sweep_kernel
struct Sweep {
    int threads, ept, rows_per, blocks;
    size_t lds;
};
Sweep sweep_shape(int n) {
    Sweep w;
    w.threads = n <= 2048 ? 256 : 1024;
    w.ept = n <= 2048 ? 8 : 16;
    w.lds = ROW_IN_LDS ? (size_t)n * 8 : 0;
    // as many workgroups as the device holds at once (by LDS and by 2048 threads a CU), but blocks of rows deep enough that the partial
    // sums stay a small share of the traffic
    const int per_cu = (int)std::min<size_t>(2048 / w.threads, std::max<size_t>(1, (160 * 1024) / (w.lds + 1024)));
    const int slots = CUS * per_cu;
    w.rows_per = std::max((n + slots - 1) / slots, std::min(16, std::max(1, n / 512)));
    w.blocks = (n + w.rows_per - 1) / w.rows_per;
    return w;
}

struct Workspace {
    double *S, *A, *R, *part, *cs, *xn, *sums;
    u64 *history, *best, *sel;
    unsigned *hist, *winner;
    int *eflag, *list, *pos, *c, *list2, *pos2, *flag2, *ctl;
    size_t bytes;
};
// the layout; with base == null only the size
Workspace carve(char* base, int n) {
    Workspace w;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + at : nullptr;
        at += aligned(bytes);
        return p;
    };
    const size_t nn = (size_t)n * n * 8, n8 = (size_t)n * 8, n4 = (size_t)n * 4;
    w.S = (double*)take(nn);
    w.A = (double*)take(nn);
    w.R = (double*)take(nn);
    w.part = (double*)take((size_t)sweep_shape(n).blocks * n8);
    w.cs = (double*)take(n8);
    w.xn = (double*)take(n8);
    w.sums = (double*)take(n8);
    w.history = (u64*)take(n8);
    w.best = (u64*)take(n8);
    w.sel = (u64*)take(SEL_WORDS * 8);
    w.hist = (unsigned*)take(RADIX_PASSES * 512 * 4);
    w.winner = (unsigned*)take(n4);
    w.eflag = (int*)take(n4);
    w.list = (int*)take(n4);
    w.pos = (int*)take(n4);
    w.c = (int*)take(n4);
    w.list2 = (int*)take(n4);
    w.pos2 = (int*)take(n4);
    w.flag2 = (int*)take(n4);
    w.ctl = (int*)take(CTL_WORDS * 4);
    w.bytes = at;
    return w;
}

bool shape_supported(int n, int d) {
    return n >= 1 && n <= HSEFR_AFFINITY_MAX_N && d >= HSEFR_AFFINITY_D_MULTIPLE && d <= HSEFR_AFFINITY_MAX_D && d % HSEFR_AFFINITY_D_MULTIPLE == 0;
}

// the control block, read with the stream drained
int read_ctl(const int* ctl, int* host, hipStream_t s, const char* who, const char* what) {
    HSEFR_HIP_CHECK(hipMemcpyAsync(host, ctl, CTL_WORDS * 4, hipMemcpyDeviceToHost, s));
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error("%s: %s failed: %s", who, what, hipGetErrorString(e));
        return HSEFR_ERR_HIP;
    }
    return HSEFR_OK;
}

template <int EPT>
int launch_sweep(const Sweep& sw, const Workspace& w, int n, double damp, double rest, hipStream_t s) {
    if (sw.lds > 48 * 1024)
        HSEFR_HIP_CHECK(hipFuncSetAttribute((const void*)ap_sweep_kernel<EPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sw.lds));
    HSEFR_LAUNCH(ap_sweep_kernel<EPT>, dim3(sw.blocks), dim3(sw.threads), sw.lds, s, (const double*)w.S, w.A, w.R, (const double*)w.cs, w.part, n,
                 sw.rows_per, damp, rest);
    return HSEFR_OK;
}

// x (features) or dense (similarities): exactly one is set
int fit(const char* who, const float* x, const double* dense, int n, int d, double damping, int max_iter, int convergence_iter,
        double preference_in, long long noise_seed, int* exemplars, int* labels, double* diag, double* preference, int* info, void* workspace,
        size_t workspace_bytes, hipStream_t s) {
    HSEFR_REQUIRE((x || dense) && exemplars && labels && diag && preference && info && workspace, HSEFR_ERR_INVALID, "%s: null pointer", who);
    HSEFR_REQUIRE(n >= 1, HSEFR_ERR_INVALID, "%s: n=%d", who, n);
    HSEFR_REQUIRE(damping >= 0.5 && damping < 1.0, HSEFR_ERR_INVALID, "%s: damping=%g must lie in [0.5, 1)", who, damping);
    HSEFR_REQUIRE(convergence_iter >= 1 && convergence_iter <= HSEFR_AFFINITY_MAX_CONVERGENCE_ITER, HSEFR_ERR_INVALID,
                  "%s: convergence_iter=%d (1 .. %d)", who, convergence_iter, HSEFR_AFFINITY_MAX_CONVERGENCE_ITER);
    HSEFR_REQUIRE(!__builtin_isinf(preference_in), HSEFR_ERR_INVALID, "%s: preference=%g must be finite (a NaN: the median)", who, preference_in);
    HSEFR_REQUIRE(noise_seed >= -1, HSEFR_ERR_INVALID, "%s: noise_seed=%lld (-1: no noise)", who, noise_seed);
    HSEFR_REQUIRE(shape_supported(n, d), HSEFR_ERR_UNSUPPORTED, "%s: n=%d, d=%d (n <= %d, d a multiple of %d up to %d)", who, n, d,
                  HSEFR_AFFINITY_MAX_N, HSEFR_AFFINITY_D_MULTIPLE, HSEFR_AFFINITY_MAX_D);
    HSEFR_REQUIRE(max_iter >= 1 && max_iter <= HSEFR_AFFINITY_MAX_ITER, HSEFR_ERR_UNSUPPORTED, "%s: max_iter=%d (1 .. %d)", who, max_iter,
                  HSEFR_AFFINITY_MAX_ITER);
    HSEFR_REQUIRE((uintptr_t)workspace % 16 == 0 && (uintptr_t)x % 8 == 0 && (uintptr_t)dense % 8 == 0 && (uintptr_t)diag % 8 == 0 &&
                      (uintptr_t)preference % 8 == 0,
                  HSEFR_ERR_INVALID, "%s: misaligned pointer (workspace: 16 bytes, x, diag and preference: 8)", who);
    const Workspace w = carve((char*)workspace, n);
    HSEFR_REQUIRE(workspace_bytes >= w.bytes, HSEFR_ERR_INVALID, "%s: workspace of %zu bytes, %zu needed (hsefr_affinity_workspace_bytes)", who,
                  workspace_bytes, w.bytes);
    const size_t total = (size_t)n * n;
    const dim3 blk(256), per_point((n + 255) / 256), per_wave((n + 3) / 4);
    const dim3 stream_grid((unsigned)std::min<size_t>((total + 255) / 256, 4096));
    const Sweep sw = sweep_shape(n);
    const double rest = 1.0 - damping;
    int host[CTL_WORDS];
    int rc;

    HSEFR_HIP_CHECK(hipMemsetAsync(w.ctl, 0, CTL_WORDS * 4, s));
    HSEFR_HIP_CHECK(hipMemsetAsync(w.sel, 0, SEL_WORDS * 8, s));
    HSEFR_HIP_CHECK(hipMemsetAsync(w.sel + SEL_MIN, 0xff, 8, s));
    HSEFR_HIP_CHECK(hipMemsetAsync(w.hist, 0, RADIX_PASSES * 512 * 4, s));
    if (x) {
        HSEFR_LAUNCH(ap_norms_kernel, per_wave, blk, 0, s, x, n, d, w.xn, w.ctl);
        HSEFR_LAUNCH(ap_sim_kernel, dim3((n + TM - 1) / TM, (n + TN - 1) / TN), blk, 0, s, x, (const double*)w.xn, n, d, w.S);
    } else {
        HSEFR_LAUNCH(ap_copy_kernel, stream_grid, blk, 0, s, dense, total, w.S, w.ctl);
    }
    HSEFR_LAUNCH(ap_minmax_kernel, stream_grid, blk, 0, s, (const double*)w.S, n, w.sel);
    if ((rc = launch_status("the similarities")) != HSEFR_OK) return rc;
    u64 sel[SEL_WORDS];
    HSEFR_HIP_CHECK(hipMemcpyAsync(sel, w.sel, sizeof sel, hipMemcpyDeviceToHost, s));
    if ((rc = read_ctl(w.ctl, host, s, who, "the similarities")) != HSEFR_OK) return rc;
    if (host[CTL_NONFINITE]) {
        HSEFR_LAUNCH(ap_info_kernel, dim3(1), dim3(64), 0, s, (const int*)w.ctl, (const u64*)w.sel, 0, 0, 0, 0, info, preference);
        (void)hipStreamSynchronize(s);
        set_error("%s: non-finite input (a NaN or an infinity among the %s)", who, x ? "features" : "similarities");
        return HSEFR_ERR_INVALID;
    }
    const bool equal = n == 1 || sel[SEL_MIN] == sel[SEL_MAX];

    // the preference: the median of all n^2 entries, or the caller's
    if (preference_in != preference_in) {
        sel[SEL_PREFIX] = sel[SEL_PREFIX + 1] = 0;
        sel[SEL_RANK] = (total - 1) / 2;             // the two middle entries (one entry twice for an odd count)
        sel[SEL_RANK + 1] = total / 2;
        HSEFR_HIP_CHECK(hipMemcpyAsync(w.sel, sel, 4 * 8, hipMemcpyHostToDevice, s));
        for (int pass = 0; pass < RADIX_PASSES; ++pass) {
            HSEFR_LAUNCH(ap_hist_kernel, stream_grid, blk, 0, s, (const double*)w.S, total, pass, (const u64*)w.sel, w.hist);
            HSEFR_LAUNCH(ap_digit_kernel, dim3(1), dim3(64), 0, s, pass, w.sel, (const unsigned*)w.hist, w.ctl);
        }
    } else {
        HSEFR_HIP_CHECK(hipMemcpyAsync(w.sel + SEL_PREF, &preference_in, 8, hipMemcpyHostToDevice, s));
    }

    int K = 0, n_iter = 0, converged = 0;
    bool internal = false;
    if (equal) {
        HSEFR_LAUNCH(ap_trivial_kernel, per_point, blk, 0, s, 3, (const double*)w.S, (const u64*)w.sel, n, exemplars, labels, diag, w.ctl);
        if ((rc = launch_status("ap_trivial_kernel")) != HSEFR_OK) return rc;
        if ((rc = read_ctl(w.ctl, host, s, who, "the equal similarities")) != HSEFR_OK) return rc;
        K = host[CTL_K];
        converged = 1;
        internal = host[CTL_INTERNAL] || (K != 1 && K != n);
    } else {
        const u64 seed_term = (u64)noise_seed * HSEFR_AFFINITY_HASH_SEED_MUL + HSEFR_AFFINITY_HASH_GAMMA;
        HSEFR_LAUNCH(ap_prepare_kernel, noise_seed >= 0 ? stream_grid : per_point, blk, 0, s, w.S, n, (const u64*)w.sel, noise_seed >= 0 ? 1 : 0,
                     seed_term);
        HSEFR_HIP_CHECK(hipMemsetAsync(w.A, 0, total * 8, s));
        HSEFR_HIP_CHECK(hipMemsetAsync(w.R, 0, total * 8, s));
        HSEFR_HIP_CHECK(hipMemsetAsync(w.cs, 0, (size_t)n * 8, s));
        HSEFR_HIP_CHECK(hipMemsetAsync(w.history, 0, (size_t)n * 8, s));
        for (int it = 0; it < max_iter; ++it) {
            rc = sw.ept == 8 ? launch_sweep<8>(sw, w, n, damping, rest, s) : launch_sweep<16>(sw, w, n, damping, rest, s);
            if (rc != HSEFR_OK) return rc;
            HSEFR_LAUNCH(ap_colsum_kernel, per_point, blk, 0, s, (const double*)w.part, sw.blocks, (const double*)w.A, (const double*)w.R, n, damping,
                         rest, w.cs, diag, w.history, w.eflag);
            HSEFR_LAUNCH(ap_stop_kernel, dim3(1), dim3(1024), 0, s, (const u64*)w.history, n, it, convergence_iter, w.ctl);
            if ((rc = launch_status("the iteration's kernels")) != HSEFR_OK) return rc;
            if ((rc = read_ctl(w.ctl, host, s, who, "an iteration")) != HSEFR_OK) return rc;
            n_iter = it + 1;
            if (host[CTL_INTERNAL]) break;
            if (host[CTL_STOP]) {
                converged = 1;
                break;
            }
        }
        K = host[CTL_K];
        internal = host[CTL_INTERNAL] || K < 0 || K > n;
        if (!internal && K == 0) {
            HSEFR_LAUNCH(ap_trivial_kernel, per_point, blk, 0, s, 0, (const double*)w.S, (const u64*)w.sel, n, exemplars, labels, diag, w.ctl);
        } else if (!internal) {
            HSEFR_HIP_CHECK(hipMemsetAsync(w.best, 0, (size_t)n * 8, s));
            HSEFR_HIP_CHECK(hipMemsetAsync(w.winner, 0xff, (size_t)n * 4, s));
            HSEFR_HIP_CHECK(hipMemsetAsync(w.pos2, 0xff, (size_t)n * 4, s));
            HSEFR_HIP_CHECK(hipMemsetAsync(w.flag2, 0, (size_t)n * 4, s));
            HSEFR_LAUNCH(ap_select_kernel, dim3(1), blk, 0, s, (const int*)w.eflag, n, w.list, w.pos, w.ctl + CTL_K);
            HSEFR_LAUNCH(ap_assign_kernel, per_wave, blk, 0, s, (const double*)w.S, n, (const int*)w.list, (const int*)w.pos, K, w.c, w.ctl);
            HSEFR_LAUNCH(ap_member_sum_kernel, per_wave, blk, 0, s, (const double*)w.S, n, (const int*)w.c, K, w.sums, w.best);
            HSEFR_LAUNCH(ap_winner_kernel, per_point, blk, 0, s, (const double*)w.sums, (const int*)w.c, (const u64*)w.best, n, K, w.winner);
            HSEFR_LAUNCH(ap_relist_kernel, dim3((K + 255) / 256), blk, 0, s, (const unsigned*)w.winner, K, n, w.list2, w.pos2, w.flag2, w.ctl);
            HSEFR_LAUNCH(ap_assign_kernel, per_wave, blk, 0, s, (const double*)w.S, n, (const int*)w.list2, (const int*)w.pos2, K, w.c, w.ctl);
            HSEFR_LAUNCH(ap_select_kernel, dim3(1), blk, 0, s, (const int*)w.flag2, n, exemplars, w.pos, w.ctl + CTL_K);
            HSEFR_LAUNCH(ap_labels_kernel, per_point, blk, 0, s, (const int*)w.c, (const int*)w.list2, (const int*)w.pos, n, K, labels, w.ctl);
        }
        if ((rc = launch_status("the finish")) != HSEFR_OK) return rc;
        if ((rc = read_ctl(w.ctl, host, s, who, "the finish")) != HSEFR_OK) return rc;
        internal = internal || host[CTL_INTERNAL] || host[CTL_K] != K;      // (both selections count K points)
    }
    HSEFR_LAUNCH(ap_info_kernel, dim3(1), dim3(64), 0, s, (const int*)w.ctl, (const u64*)w.sel, K, n_iter, converged, equal ? 1 : 0, info,
                 preference);
    if ((rc = launch_status("ap_info_kernel")) != HSEFR_OK) return rc;
    if (internal) {
        const int one = 1;
        (void)hipMemcpyAsync(info + HSEFR_AFFINITY_INFO_INTERNAL, &one, 4, hipMemcpyHostToDevice, s);
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error("%s: the finish failed: %s", who, hipGetErrorString(e));
        return HSEFR_ERR_HIP;
    }
    if (internal) {
        set_error("%s: internal error: an index or a count left its bound on the device (K=%d of n=%d)", who, K, n);
        return HSEFR_ERR_HIP;
    }
    return HSEFR_OK;
}

}  // namespace

}  // namespace hsefr

extern "C" {

__attribute__((visibility("default"))) int hsefr_affinity_version(void) { return HSEFR_AFFINITY_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_affinity_last_error(void) { return hsefr::g_error; }

__attribute__((visibility("default"))) size_t hsefr_affinity_workspace_bytes(int n, int d) {
    return hsefr::shape_supported(n, d) ? hsefr::carve(nullptr, n).bytes : 0;
}

__attribute__((visibility("default"))) int hsefr_affinity_fit(const float* x, int n, int d, double damping, int max_iter, int convergence_iter,
                                                              double preference_in, long long noise_seed, int32_t* exemplars, int32_t* labels,
                                                              double* diag, double* preference, int32_t* info, void* workspace,
                                                              size_t workspace_bytes, void* stream) {
    if (!x) {
        hsefr::set_error("affinity_fit: null pointer");
        return HSEFR_ERR_INVALID;
    }
    return hsefr::fit("affinity_fit", x, nullptr, n, d, damping, max_iter, convergence_iter, preference_in, noise_seed, exemplars, labels, diag,
                      preference, info, workspace, workspace_bytes, (hipStream_t)stream);
}

__attribute__((visibility("default"))) int hsefr_affinity_fit_dense(const double* s, int n, double damping, int max_iter, int convergence_iter,
                                                                    double preference_in, long long noise_seed, int32_t* exemplars,
                                                                    int32_t* labels, double* diag, double* preference, int32_t* info,
                                                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!s) {
        hsefr::set_error("affinity_fit_dense: null pointer");
        return HSEFR_ERR_INVALID;
    }
    return hsefr::fit("affinity_fit_dense", nullptr, s, n, HSEFR_AFFINITY_D_MULTIPLE, damping, max_iter, convergence_iter, preference_in,
                      noise_seed, exemplars, labels, diag, preference, info, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
