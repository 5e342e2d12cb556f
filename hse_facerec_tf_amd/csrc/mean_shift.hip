// libhsefr_shift.so (include/hsefr_shift.h): sklearn.cluster.MeanShift(bandwidth=h).fit / .predict on the device -- the third method of
// the clustering study's scikit-learn branch (facial_clustering_test.py:264), with every row of X a seed and all seeds advanced together.
//
// State, all in the caller's workspace: M [n,d] fp64 the seeds' means (M = X at the start), S [n,d] fp64 the member sums of an iteration's
// active rows (and, at the finish, the ordered means), the BIT matrix [n][W = ceil(n/64)] (row = a seed: bit j = face j is a member), the
// squared norms of X's rows and of M's, per seed its count and completed iterations, and the active list twice.  An iteration over the
// na seeds still active is four launches:
//   ms_member_kernel   32 active seeds x 64 faces per workgroup: <m, x> on the fp64 MFMA, D2 = N(m) + N(x) - 2 <m, x> <= h^2 -> one 64-bit
//                      word of the bit matrix per seed and workgroup
//   ms_means_kernel    32 active seeds x 64 columns per workgroup: sum_j bit(seed, j) X[j, c] on the same MFMA, the bits expanded to 0.0 / 1.0
//                      in registers; ONE accumulator per element walks the faces in index order (a chunk of 64 faces none of the tile's seeds
//                      holds is skipped: it would add zeros), so equal member sets give equal bits of the mean
//   ms_step_kernel     a wave per active seed: count = the row's set bits, mean = sum / count, the shift |new - old|, the stop test,
//                      completed, keep[row]
//   ms_compact_kernel  one workgroup: the kept rows, in order, are the next active list; its length is what the host reads (64 bytes)
// and the finish is: ms_rank_kernel twice (which seeds hold the last copy of their mean; each such mean's place under (count, coordinates)
// descending), ms_gather_kernel (the ordered means and their norms), ms_member_kernel over them (the centre-to-centre bit matrix),
// ms_suppress_kernel (one workgroup, the suppressed set in LDS, sequential over the kept centres), ms_centers_kernel (the outputs) and
// ms_assign_kernel (each face's nearest centre by D2, then its distance from the differences) -- hsefr_shift_assign's kernel.
//
// Nothing one workgroup writes is read by another in the same launch.  No grid-wide barriers, no cooperative launches, no spin-waits,
// no floating-point atomics; the integer atomics count.  An index read from device memory is compared with its bound before it is used;
// one out of bounds raises ctl[CTL_INTERNAL] and is not followed.  Every store is a vector store from plain C++.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "common.h"
#include "lib_error.h"
#include "../../include/hsefr_shift.h"

namespace hsefr {

namespace {

typedef double ms_f64x4 __attribute__((ext_vector_type(4)));
typedef double ms_f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned long long u64;

constexpr int TM = 32, TN = 64, TK = 16;             // a workgroup's tile of a product: 32 rows x 64 columns, 16 of the sum per LDS tile
constexpr int NONE = 0x7fffffff;
// the control block: what the kernels report and the host reads
enum { CTL_ACTIVE = 0, CTL_NONFINITE = 1, CTL_INTERNAL = 2, CTL_MAX_ITER = 3, CTL_DISTINCT = 4, CTL_CENTERS = 5, CTL_WORDS = 16 };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool F64>
__device__ __forceinline__ double ms_load(const void* p, int row, int k, int d) {
    if (row < 0 || k >= d) return 0.0;
    const size_t at = (size_t)row * d + k;
    return F64 ? ((const double*)p)[at] : (double)((const float*)p)[at];
}

// ---- the start: M = X, the squared norms, every seed active -------------------------------------------------------------------------
// a wave per row; d is a multiple of 4, so a lane's pair of doubles is one 16-byte store
__global__ __launch_bounds__(256) void ms_prep_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ M, double* __restrict__ xn,
                                                      double* __restrict__ mn, int* __restrict__ cnt, int* __restrict__ completed,
                                                      int* __restrict__ active, int* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    double s = 0.0;
    bool bad = false;
    for (int c = 2 * lane; c < d; c += 128) {
        const float2 f = *(const float2*)(x + (size_t)row * d + c);
        const ms_f64x2 v = {(double)f.x, (double)f.y};
        bad |= !(isfinite(f.x) && isfinite(f.y));
        s += v.x * v.x;
        s += v.y * v.y;
        *(ms_f64x2*)(M + (size_t)row * d + c) = v;
        hsefr_store_guard();
    }
    s = wave_sum(s);
    if (bad) ctl[CTL_NONFINITE] = 1;                 // (every writer stores the same 1)
    if (lane == 0) {
        xn[row] = s;
        mn[row] = s;
        cnt[row] = 0;
        completed[row] = 0;
        active[row] = row;
    }
}

// the squared norms of the rows of a [rows, d] matrix, fp32 or fp64, in ms_prep_kernel's shape of sum
template <bool F64>
__global__ __launch_bounds__(256) void ms_norms_kernel(const void* __restrict__ a, int rows, int d, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    double s = 0.0;
    for (int c = 2 * lane; c < d; c += 128) {
        const double v0 = ms_load<F64>(a, row, c, d), v1 = ms_load<F64>(a, row, c + 1, d);
        s += v0 * v0;
        s += v1 * v1;
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

// ---- the product tile -----------------------------------------------------------------------------------------------------------------
// acc0 / acc1 += sum_k A[s_arow[i], k] B[b0 + j, k] for the workgroup's 32 x 64 tile (256 threads = 4 waves: wave w owns rows
// 16 (w & 1) .. and columns 32 (w >> 1) .., two 16 x 16 MFMA tiles).  Lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][column
// l & 15]; result register g of lane l is row (l >> 4) + 4 g, column l & 15.  s_arow (LDS, filled behind a barrier): the row of A of each
// tile row, or -1 (reads as zeros); rows of B at or past nb read as zeros.  The sum over k of an element has one shape wherever its tile lies.
template <bool A64, bool B64>
__device__ __forceinline__ void tile_dot(const void* __restrict__ A, const int* s_arow, const void* __restrict__ B, int b0, int nb, int d,
                                         double (*As)[TM + 1], double (*Bs)[TN + 1], ms_f64x4& acc0, ms_f64x4& acc1) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32, r = lane & 15, q = lane >> 4;
    const int kk = tid & 15, rr = tid >> 4;          // this thread's elements of a tile: column kk of rows rr + 16 e
    double va[TM / 16], vb[TN / 16];
    int arow[TM / 16], brow[TN / 16];
#pragma unroll
    for (int e = 0; e < TM / 16; ++e) arow[e] = s_arow[rr + 16 * e];
#pragma unroll
    for (int e = 0; e < TN / 16; ++e) brow[e] = b0 + rr + 16 * e < nb ? b0 + rr + 16 * e : -1;
#pragma unroll
    for (int e = 0; e < TM / 16; ++e) va[e] = ms_load<A64>(A, arow[e], kk, d);
#pragma unroll
    for (int e = 0; e < TN / 16; ++e) vb[e] = ms_load<B64>(B, brow[e], kk, d);
    for (int k0 = 0; k0 < d; k0 += TK) {
        __syncthreads();                             // the previous tile has been read
#pragma unroll
        for (int e = 0; e < TM / 16; ++e) As[kk][rr + 16 * e] = va[e];
#pragma unroll
        for (int e = 0; e < TN / 16; ++e) Bs[kk][rr + 16 * e] = vb[e];
        __syncthreads();
        if (k0 + TK < d) {                           // the next tile travels while this one is multiplied
#pragma unroll
            for (int e = 0; e < TM / 16; ++e) va[e] = ms_load<A64>(A, arow[e], k0 + TK + kk, d);
#pragma unroll
            for (int e = 0; e < TN / 16; ++e) vb[e] = ms_load<B64>(B, brow[e], k0 + TK + kk, d);
        }
#pragma unroll
        for (int k = 0; k < TK; k += 4) {
            const double a = As[k + q][wm + r];
            const double b0v = Bs[k + q][wn + r], b1v = Bs[k + q][wn + 16 + r];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0v, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1v, acc1, 0, 0, 0);
        }
    }
}

// the rows of a tile: s_row[i] = the row of the matrix behind list entry m0 + i (rows == null: the entry itself), -1 past the list's end or
// for an entry outside 0 .. limit - 1, which raises ctl[CTL_INTERNAL].  Ends behind a barrier.
__device__ __forceinline__ void tile_rows(const int* __restrict__ rows, int m0, int nrows, int limit, int* s_row, int* __restrict__ ctl) {
    if (threadIdx.x < TM) {
        const int e = m0 + threadIdx.x;
        int row = -1;
        if (e < nrows) {
            row = rows ? rows[e] : e;
            if ((unsigned)row >= (unsigned)limit) {
                ctl[CTL_INTERNAL] = 1;
                row = -1;
            }
        }
        s_row[threadIdx.x] = row;
    }
    __syncthreads();
}

// ---- membership: one bit per pair -----------------------------------------------------------------------------------------------------
// rows: the listed rows of A [., d] fp64 (the active seeds' means, or the ordered means) with their squared norms an (by row of A);
// columns: the ncols rows of B (the faces, fp32, or the ordered means, fp64) with bn.  bits[row of A][blockIdx.y] = the 64 decisions
// D2 <= h2 of this workgroup's columns (0 past ncols).  grid (ceil(nrows / 32), ceil(ncols / 64)); W = the bit rows' stride in words.
template <bool B64>
__global__ __launch_bounds__(256) void ms_member_kernel(const double* __restrict__ A, const double* __restrict__ an, const int* __restrict__ rows,
                                                        int nrows, int limit, const void* __restrict__ B, const double* __restrict__ bn, int ncols,
                                                        int d, double h2, u64* __restrict__ bits, int W, int* __restrict__ ctl) {
    __shared__ double As[TK][TM + 1];
    __shared__ double Bs[TK][TN + 1];
    __shared__ int s_row[TM];
    __shared__ unsigned short s_part[TM][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32, r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.y * TN;
    tile_rows(rows, blockIdx.x * TM, nrows, limit, s_row, ctl);
    ms_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    tile_dot<true, B64>(A, s_row, B, n0, ncols, d, As, Bs, acc0, acc1);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const ms_f64x4 acc = t ? acc1 : acc0;
        const int j = n0 + wn + 16 * t + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = wm + q + 4 * g, row = s_row[i];
            bool in = false;
            if (row >= 0 && j < ncols) in = (an[row] + bn[j]) - 2.0 * acc[g] <= h2;
            const u64 b = __ballot(in);              // bit l: row (l >> 4) + 4 g of this wave's 16, column l & 15
            if (r == 0) s_part[i][(wn >> 4) + t] = (unsigned short)(b >> (16 * q));
        }
    }
    __syncthreads();
    if (tid < TM && s_row[tid] >= 0)
        bits[(size_t)s_row[tid] * W + blockIdx.y] = (u64)s_part[tid][0] | (u64)s_part[tid][1] << 16 | (u64)s_part[tid][2] << 32 | (u64)s_part[tid][3] << 48;
}

// ---- the member sums ------------------------------------------------------------------------------------------------------------------
// S[list entry e][c] = sum over the faces j in index order of bit(rows[e], j) X[j, c].  grid (ceil(nrows / 32), ceil(d / 64))
__global__ __launch_bounds__(256) void ms_means_kernel(const u64* __restrict__ bits, int W, const int* __restrict__ rows, int nrows, int n,
                                                       const float* __restrict__ x, int d, double* __restrict__ S, int* __restrict__ ctl) {
    __shared__ double Bs[TK][TN + 1];
    __shared__ u64 s_w[TM];
    __shared__ int s_row[TM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32, r = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.x * TM, c0 = blockIdx.y * TN;
    tile_rows(rows, m0, nrows, n, s_row, ctl);
    ms_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    const int cc = tid & 63, kr = tid >> 6;          // this thread's elements of a tile of X: column cc of faces kr + 4 e
    for (int w = 0; w < W; ++w) {
        __syncthreads();                             // the previous words have been read
        if (tid < TM) s_w[tid] = s_row[tid] >= 0 ? bits[(size_t)s_row[tid] * W + w] : 0ull;
        __syncthreads();
        if (__ballot(lane < TM && s_w[lane & (TM - 1)] != 0ull) == 0ull) continue;      // the same answer in every wave
        const u64 mine = s_w[wm + r];
#pragma unroll 1
        for (int sub = 0; sub < 64 / TK; ++sub) {
            const int j0 = w * 64 + sub * TK;
            if (j0 >= n) break;
            double v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = j0 + kr + 4 * e, c = c0 + cc;
                v[e] = j < n && c < d ? (double)x[(size_t)j * d + c] : 0.0;
            }
            __syncthreads();                         // the previous tile has been read
#pragma unroll
            for (int e = 0; e < 4; ++e) Bs[kr + 4 * e][cc] = v[e];
            __syncthreads();
#pragma unroll
            for (int k = 0; k < TK; k += 4) {
                const double a = (mine >> (sub * TK + k + q)) & 1ull ? 1.0 : 0.0;
                const double b0v = Bs[k + q][wn + r], b1v = Bs[k + q][wn + 16 + r];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0v, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1v, acc1, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const ms_f64x4 acc = t ? acc1 : acc0;
        const int c = c0 + wn + 16 * t + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = wm + q + 4 * g;
            if (m0 + i < nrows && c < d) S[(size_t)(m0 + i) * d + c] = acc[g];
        }
    }
}

// ---- the step of every active seed ----------------------------------------------------------------------------------------------------
// a wave per list entry: count, mean, shift, stop test.  A stopped seed's mean and count are final
__global__ __launch_bounds__(256) void ms_step_kernel(const double* __restrict__ S, const u64* __restrict__ bits, int W, const int* __restrict__ rows,
                                                      int nrows, int n, int d, double* __restrict__ M, double* __restrict__ mn,
                                                      int* __restrict__ cnt, int* __restrict__ completed, int* __restrict__ keep, double stop,
                                                      int max_iter, int* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= nrows) return;
    const int seed = rows[e];
    if ((unsigned)seed >= (unsigned)n) {
        if (lane == 0) {
            ctl[CTL_INTERNAL] = 1;
            keep[e] = 0;
        }
        return;
    }
    int c = 0;
    for (int w = lane; w < W; w += 64) c += __popcll(bits[(size_t)seed * W + w]);
    c = wave_sum(c);
    if (c < 1) {                                     // no member (scikit-learn drops such a seed): it stops and is no centre
        if (lane == 0) {
            cnt[seed] = 0;
            keep[e] = 0;
        }
        return;
    }
    const double count = (double)c;
    double s2 = 0.0, nn = 0.0;
    for (int k = lane; k < d; k += 64) {
        const double nw = S[(size_t)e * d + k] / count, df = nw - M[(size_t)seed * d + k];
        s2 += df * df;
        nn += nw * nw;
        M[(size_t)seed * d + k] = nw;
    }
    s2 = wave_sum(s2);
    nn = wave_sum(nn);
    if (lane == 0) {
        mn[seed] = nn;
        cnt[seed] = c;
        const bool converged = sqrt(s2) <= stop;
        const int done = completed[seed];
        if (converged || done >= max_iter) {
            if (!converged) atomicAdd(&ctl[CTL_MAX_ITER], 1);
            keep[e] = 0;
        } else {
            completed[seed] = done + 1;
            keep[e] = 1;
        }
    }
}

// the kept entries of the list, in order, are the next list; one workgroup
__global__ __launch_bounds__(256) void ms_compact_kernel(const int* __restrict__ rows, const int* __restrict__ keep, int nrows, int* __restrict__ next,
                                                         int* __restrict__ ctl) {
    __shared__ int s_at[257];
    const int t = threadIdx.x, per = (nrows + 255) / 256;
    const int b = min(t * per, nrows), e = min(b + per, nrows);
    int c = 0;
    for (int i = b; i < e; ++i) c += keep[i] != 0;
    s_at[t + 1] = c;
    __syncthreads();
    if (t == 0) {
        s_at[0] = 0;
        for (int i = 1; i <= 256; ++i) s_at[i] += s_at[i - 1];
        ctl[CTL_ACTIVE] = s_at[256];
    }
    __syncthreads();
    int o = s_at[t];
    for (int i = b; i < e; ++i)
        if (keep[i] != 0) next[o++] = rows[i];
}

// ---- the finish -------------------------------------------------------------------------------------------------------------------------
// whether mean a comes before mean b in scikit-learn's order of the centres, (count, coordinates) descending; equal: neither
__device__ __forceinline__ int mean_compare(const double* __restrict__ M, int d, int a, int b) {      // 1: a's tuple is greater, -1: less, 0: equal
    for (int k = 0; k < d; ++k) {
        const double va = M[(size_t)a * d + k], vb = M[(size_t)b * d + k];
        if (va != vb) return va > vb ? 1 : -1;
    }
    return 0;
}
// a workgroup per seed i.  pass 0: isrep[i] = it has members and no later seed has an equal mean (scikit-learn's dict keyed by the mean
// keeps the last writer's count).  pass 1, for such a seed: its place = how many such seeds come before it; order[place] = i
__global__ __launch_bounds__(256) void ms_rank_kernel(const double* __restrict__ M, const int* __restrict__ cnt, int n, int d, int pass,
                                                      int* __restrict__ isrep, int* __restrict__ order, int* __restrict__ ctl) {
    __shared__ int s_count;
    const int i = blockIdx.x, t = threadIdx.x;
    if (pass == 0) {
        int later = 0;
        for (int j = i + 1 + t; j < n; j += 256)
            if (cnt[j] > 0 && mean_compare(M, d, j, i) == 0) later = 1;
        later = __syncthreads_or(later);
        if (t == 0) isrep[i] = cnt[i] > 0 && !later;
        return;
    }
    if (!isrep[i]) return;
    if (t == 0) s_count = 0;
    __syncthreads();
    const int ci = cnt[i];
    int before = 0;
    for (int j = t; j < n; j += 256) {
        if (j == i || !isrep[j]) continue;
        const int cj = cnt[j];
        before += cj > ci || (cj == ci && mean_compare(M, d, j, i) > 0);
    }
    before = wave_sum(before);
    if ((t & 63) == 0) atomicAdd(&s_count, before);
    __syncthreads();
    if (t == 0) {
        order[s_count] = i;                          // (s_count < n: it counts other seeds)
        atomicAdd(&ctl[CTL_DISTINCT], 1);
    }
}

// the ordered means: C[c] = M[order[c]] with its squared norm and count; a wave per row
__global__ __launch_bounds__(256) void ms_gather_kernel(const double* __restrict__ M, const int* __restrict__ order, int k2, int n, int d,
                                                        const int* __restrict__ cnt, double* __restrict__ C, double* __restrict__ cn,
                                                        int* __restrict__ cint, int* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= k2) return;
    const int src = order[c];
    const bool ok = (unsigned)src < (unsigned)n;
    if (!ok && lane == 0) ctl[CTL_INTERNAL] = 1;     // a place no seed took: the row reads as zeros
    double s = 0.0;
    for (int k = 2 * lane; k < d; k += 128) {
        const ms_f64x2 v = ok ? *(const ms_f64x2*)(M + (size_t)src * d + k) : ms_f64x2{0.0, 0.0};
        s += v.x * v.x;
        s += v.y * v.y;
        *(ms_f64x2*)(C + (size_t)c * d + k) = v;
        hsefr_store_guard();
    }
    s = wave_sum(s);
    if (lane == 0) {
        cn[c] = s;
        cint[c] = ok ? cnt[src] : 0;
    }
}

// In order, a centre not yet suppressed suppresses every later centre whose bit it holds.  One workgroup, the suppressed set in LDS;
// sequential over the kept centres only (a suppressed one costs a read).  klist = the kept centres, ctl[CTL_CENTERS] their number
constexpr int MAX_WORDS = (HSEFR_SHIFT_MAX_N + 63) / 64;
__global__ __launch_bounds__(256) void ms_suppress_kernel(const u64* __restrict__ bits, int W, int k2, int* __restrict__ klist, int* __restrict__ ctl) {
    __shared__ u64 s_supp[MAX_WORDS];
    __shared__ int s_at[MAX_WORDS];
    const int t = threadIdx.x, words = (k2 + 63) / 64;
    if (k2 < 1 || words > MAX_WORDS || words > W) {  // (a launch the host did not make)
        if (t == 0) ctl[CTL_INTERNAL] = 1;
        return;
    }
    for (int w = t; w < words; w += 256) s_supp[w] = 0ull;
    __syncthreads();
    for (int i = 0; i < k2; ++i) {
        const int wi = i >> 6;
        if ((s_supp[wi] >> (i & 63)) & 1ull) continue;                      // the same word in every thread, written behind a barrier
        __syncthreads();                                                     // every thread has read it
        for (int w = wi + t; w < words; w += 256) {
            u64 v = bits[(size_t)i * W + w];
            if (w == wi) v &= ~((2ull << (i & 63)) - 1ull);                  // the later centres only
            s_supp[w] |= v;
        }
        __syncthreads();
    }
    __syncthreads();
    if (t == 0) {
        int o = 0;
        for (int w = 0; w < words; ++w) {
            const u64 valid = (w == words - 1 && (k2 & 63)) ? (1ull << (k2 & 63)) - 1ull : ~0ull;
            s_supp[w] = ~s_supp[w] & valid;
            s_at[w] = o;
            o += __popcll(s_supp[w]);
        }
        ctl[CTL_CENTERS] = o;
    }
    __syncthreads();
    for (int w = t; w < words; w += 256) {
        u64 kept = s_supp[w];
        int o = s_at[w];
        while (kept) {                                                       // at most 64 turns
            klist[o++] = w * 64 + __ffsll((long long)kept) - 1;
            kept &= kept - 1ull;
        }
    }
}

// the outputs: centers[c] = C[klist[c]] with its norm and intensity; a wave per centre
__global__ __launch_bounds__(256) void ms_centers_kernel(const double* __restrict__ C, const double* __restrict__ cn, const int* __restrict__ cint,
                                                         const int* __restrict__ klist, int k, int k2, int d, double* __restrict__ centers,
                                                         double* __restrict__ cn_out, int* __restrict__ intensity, int* __restrict__ ctl) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= k) return;
    const int src = klist[c];
    const bool ok = (unsigned)src < (unsigned)k2;
    if (!ok && lane == 0) ctl[CTL_INTERNAL] = 1;
    for (int j = 2 * lane; j < d; j += 128) {
        *(ms_f64x2*)(centers + (size_t)c * d + j) = ok ? *(const ms_f64x2*)(C + (size_t)src * d + j) : ms_f64x2{0.0, 0.0};
        hsefr_store_guard();
    }
    if (lane == 0) {
        cn_out[c] = ok ? cn[src] : 0.0;
        intensity[c] = ok ? cint[src] : 0;
    }
}

// ---- the nearest centre (the labels of fit, and predict) ------------------------------------------------------------------------------
// 32 rows of q per workgroup against all k centres: the least (D2, index), then the distance itself from the differences
__global__ __launch_bounds__(256) void ms_assign_kernel(const float* __restrict__ q, const double* __restrict__ qn, int nq, const double* __restrict__ C,
                                                        const double* __restrict__ cn, int k, int d, int* __restrict__ labels,
                                                        double* __restrict__ dist) {
    __shared__ double As[TK][TM + 1];
    __shared__ double Bs[TK][TN + 1];
    __shared__ int s_row[TM];
    __shared__ double s_bd[2][TM];
    __shared__ int s_bi[2][TM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32, r = lane & 15, qq = lane >> 4;
    const int m0 = blockIdx.x * TM;
    if (tid < TM) s_row[tid] = m0 + tid < nq ? m0 + tid : -1;
    __syncthreads();
    double bd[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    int bi[4] = {NONE, NONE, NONE, NONE};
    for (int n0 = 0; n0 < k; n0 += TN) {
        ms_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
        tile_dot<false, true>(q, s_row, C, n0, k, d, As, Bs, acc0, acc1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const ms_f64x4 acc = t ? acc1 : acc0;
            const int j = n0 + wn + 16 * t + r;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = s_row[wm + qq + 4 * g];
                if (row < 0 || j >= k) continue;
                const double d2 = (qn[row] + cn[j]) - 2.0 * acc[g];
                if (d2 < bd[g] || (d2 == bd[g] && j < bi[g])) {
                    bd[g] = d2;
                    bi[g] = j;
                }
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int o = 8; o; o >>= 1) {                // over the 16 lanes of a row
            const double od = __shfl_xor(bd[g], o);
            const int oi = __shfl_xor(bi[g], o);
            if (od < bd[g] || (od == bd[g] && oi < bi[g])) {
                bd[g] = od;
                bi[g] = oi;
            }
        }
        if (r == 0) {
            s_bd[wave >> 1][wm + qq + 4 * g] = bd[g];
            s_bi[wave >> 1][wm + qq + 4 * g] = bi[g];
        }
    }
    __syncthreads();
    if (tid < TM) {
        const bool second = s_bd[1][tid] < s_bd[0][tid] || (s_bd[1][tid] == s_bd[0][tid] && s_bi[1][tid] < s_bi[0][tid]);
        s_bi[0][tid] = s_bi[second][tid];
    }
    __syncthreads();
    for (int i = wave; i < TM; i += 4) {             // a wave per row: its distance to the chosen centre
        const int row = s_row[i], c = s_bi[0][i];
        if (row < 0) continue;
        const bool ok = (unsigned)c < (unsigned)k;   // (no centre won: a non-finite row)
        double s = 0.0;
        if (ok)
            for (int j = lane; j < d; j += 64) {
                const double df = (double)q[(size_t)row * d + j] - C[(size_t)c * d + j];
                s += df * df;
            }
        s = wave_sum(s);
        if (lane == 0) {
            labels[row] = ok ? c : -1;
            dist[row] = ok ? sqrt(s) : (double)NAN;
        }
    }
}

__global__ void ms_info_kernel(const int* __restrict__ ctl, int n_iter, int work, int* __restrict__ info) {
    const int t = threadIdx.x;
    if (t >= HSEFR_SHIFT_INFO_WORDS) return;
    int v = 0;
    if (t == HSEFR_SHIFT_INFO_CENTERS) v = ctl[CTL_CENTERS];
    if (t == HSEFR_SHIFT_INFO_N_ITER) v = n_iter;
    if (t == HSEFR_SHIFT_INFO_DISTINCT) v = ctl[CTL_DISTINCT];
    if (t == HSEFR_SHIFT_INFO_MAX_ITER) v = ctl[CTL_MAX_ITER];
    if (t == HSEFR_SHIFT_INFO_NONFINITE) v = ctl[CTL_NONFINITE];
    if (t == HSEFR_SHIFT_INFO_INTERNAL) v = ctl[CTL_INTERNAL];
    if (t == HSEFR_SHIFT_INFO_WORK) v = work;
    info[t] = v;
}

// ---- the host -------------------------------------------------------------------------------------------------------------------------
constexpr size_t ALIGN = 256;
size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

struct Workspace {
    double *M, *S, *xn, *mn, *cn, *cn_out;
    u64* bits;
    int *cnt, *completed, *active[2], *keep, *isrep, *order, *cint, *klist, *ctl;
    size_t bytes;
};
// the layout; with base == null only the size
Workspace carve(char* base, int n, int d) {
    Workspace w;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + at : nullptr;
        at += aligned(bytes);
        return p;
    };
    const size_t nd = (size_t)n * d * 8, words = (size_t)(n + 63) / 64;
    w.M = (double*)take(nd);
    w.S = (double*)take(nd);
    w.bits = (u64*)take((size_t)n * words * 8);
    w.xn = (double*)take((size_t)n * 8);
    w.mn = (double*)take((size_t)n * 8);
    w.cn = (double*)take((size_t)n * 8);
    w.cn_out = (double*)take((size_t)n * 8);
    w.cnt = (int*)take((size_t)n * 4);
    w.completed = (int*)take((size_t)n * 4);
    w.active[0] = (int*)take((size_t)n * 4);
    w.active[1] = (int*)take((size_t)n * 4);
    w.keep = (int*)take((size_t)n * 4);
    w.isrep = (int*)take((size_t)n * 4);
    w.order = (int*)take((size_t)n * 4);
    w.cint = (int*)take((size_t)n * 4);
    w.klist = (int*)take((size_t)n * 4);
    w.ctl = (int*)take(CTL_WORDS * 4);
    w.bytes = at;
    return w;
}

bool shape_supported(int n, int d) {
    return n >= 1 && n <= HSEFR_SHIFT_MAX_N && d >= HSEFR_SHIFT_D_MULTIPLE && d <= HSEFR_SHIFT_MAX_D && d % HSEFR_SHIFT_D_MULTIPLE == 0;
}

// the control block, read with the stream drained
int read_ctl(const int* ctl, int* host, hipStream_t s, const char* what) {
    HSEFR_HIP_CHECK(hipMemcpyAsync(host, ctl, CTL_WORDS * 4, hipMemcpyDeviceToHost, s));
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error("shift_fit: %s failed: %s", what, hipGetErrorString(e));
        return HSEFR_ERR_HIP;
    }
    return HSEFR_OK;
}

int assign(const float* q, const double* qn, int nq, const double* centers, const double* cn, int k, int d, int* labels, double* dist,
           hipStream_t s) {
    HSEFR_LAUNCH(ms_assign_kernel, dim3((nq + TM - 1) / TM), dim3(256), 0, s, q, qn, nq, centers, cn, k, d, labels, dist);
    return launch_status("ms_assign_kernel");
}

int shift_fit(const float* x, int n, int d, double h, int max_iter, double* centers, int* intensity, int* labels, double* label_dist, int* info,
              void* workspace, size_t workspace_bytes, hipStream_t s) {
    HSEFR_REQUIRE(x && centers && intensity && labels && label_dist && info && workspace, HSEFR_ERR_INVALID, "shift_fit: null pointer");
    HSEFR_REQUIRE(n >= 1, HSEFR_ERR_INVALID, "shift_fit: n=%d", n);
    HSEFR_REQUIRE(__builtin_isfinite(h) && h > 0.0, HSEFR_ERR_INVALID, "shift_fit: bandwidth=%g must be finite and > 0", h);
    HSEFR_REQUIRE(shape_supported(n, d), HSEFR_ERR_UNSUPPORTED, "shift_fit: n=%d, d=%d (n <= %d, d a multiple of %d up to %d)", n, d,
                  HSEFR_SHIFT_MAX_N, HSEFR_SHIFT_D_MULTIPLE, HSEFR_SHIFT_MAX_D);
    HSEFR_REQUIRE(max_iter >= 0 && max_iter <= HSEFR_SHIFT_MAX_ITER, HSEFR_ERR_UNSUPPORTED, "shift_fit: max_iter=%d (0 .. %d)", max_iter,
                  HSEFR_SHIFT_MAX_ITER);
    HSEFR_REQUIRE((uintptr_t)workspace % 16 == 0 && (uintptr_t)centers % 16 == 0 && (uintptr_t)x % 8 == 0, HSEFR_ERR_INVALID,
                  "shift_fit: misaligned pointer (workspace and centers: 16 bytes, x: 8)");
    const Workspace w = carve((char*)workspace, n, d);
    HSEFR_REQUIRE(workspace_bytes >= w.bytes, HSEFR_ERR_INVALID, "shift_fit: workspace of %zu bytes, %zu needed (hsefr_shift_workspace_bytes)",
                  workspace_bytes, w.bytes);
    const int W = (n + 63) / 64;
    const double h2 = h * h, stop = 1e-3 * h;
    const dim3 blk(256), per_row((n + 3) / 4);
    int host[CTL_WORDS];

    HSEFR_HIP_CHECK(hipMemsetAsync(w.ctl, 0, CTL_WORDS * 4, s));
    HSEFR_HIP_CHECK(hipMemsetAsync(intensity, 0, (size_t)n * 4, s));
    HSEFR_HIP_CHECK(hipMemsetAsync(w.order, 0xff, (size_t)n * 4, s));
    HSEFR_LAUNCH(ms_prep_kernel, per_row, blk, 0, s, x, n, d, w.M, w.xn, w.mn, w.cnt, w.completed, w.active[0], w.ctl);
    int rc = launch_status("ms_prep_kernel");
    if (rc != HSEFR_OK) return rc;
    if ((rc = read_ctl(w.ctl, host, s, "the first pass")) != HSEFR_OK) return rc;
    if (host[CTL_NONFINITE]) {
        HSEFR_LAUNCH(ms_info_kernel, dim3(1), dim3(64), 0, s, w.ctl, 0, 0, info);
        (void)hipStreamSynchronize(s);
        set_error("shift_fit: non-finite input (a NaN or an infinity among the features)");
        return HSEFR_ERR_INVALID;
    }

    int na = n, n_iter = 0, work = 0, cur = 0;
    for (int it = 0; it <= max_iter && na > 0; ++it) {               // at most max_iter + 1 passes: a seed with max_iter completed stops
        const dim3 rows((na + TM - 1) / TM);
        HSEFR_LAUNCH(ms_member_kernel<false>, dim3(rows.x, W), blk, 0, s, w.M, w.mn, w.active[cur], na, n, (const void*)x, w.xn, n, d, h2, w.bits,
                     W, w.ctl);
        HSEFR_LAUNCH(ms_means_kernel, dim3(rows.x, (d + TN - 1) / TN), blk, 0, s, w.bits, W, w.active[cur], na, n, x, d, w.S, w.ctl);
        HSEFR_LAUNCH(ms_step_kernel, dim3((na + 3) / 4), blk, 0, s, w.S, w.bits, W, w.active[cur], na, n, d, w.M, w.mn, w.cnt, w.completed, w.keep,
                     stop, max_iter, w.ctl);
        HSEFR_LAUNCH(ms_compact_kernel, dim3(1), blk, 0, s, w.active[cur], w.keep, na, w.active[cur ^ 1], w.ctl);
        if ((rc = launch_status("the iteration's kernels")) != HSEFR_OK) return rc;
        if ((rc = read_ctl(w.ctl, host, s, "an iteration")) != HSEFR_OK) return rc;
        work += na;
        na = host[CTL_ACTIVE];
        if (host[CTL_INTERNAL] || na < 0 || na > n) break;
        if (na > 0) n_iter = it + 1;
        cur ^= 1;
    }
    bool internal = host[CTL_INTERNAL] || na != 0;

    int k2 = 0, k = 0;
    if (!internal) {
        HSEFR_LAUNCH(ms_rank_kernel, dim3(n), blk, 0, s, w.M, w.cnt, n, d, 0, w.isrep, w.order, w.ctl);
        HSEFR_LAUNCH(ms_rank_kernel, dim3(n), blk, 0, s, w.M, w.cnt, n, d, 1, w.isrep, w.order, w.ctl);
        if ((rc = launch_status("ms_rank_kernel")) != HSEFR_OK) return rc;
        if ((rc = read_ctl(w.ctl, host, s, "the ordering")) != HSEFR_OK) return rc;
        k2 = host[CTL_DISTINCT];
        internal = host[CTL_INTERNAL] || k2 < 1 || k2 > n;
    }
    if (!internal) {
        HSEFR_LAUNCH(ms_gather_kernel, dim3((k2 + 3) / 4), blk, 0, s, w.M, w.order, k2, n, d, w.cnt, w.S, w.cn, w.cint, w.ctl);
        HSEFR_LAUNCH(ms_member_kernel<true>, dim3((k2 + TM - 1) / TM, (k2 + 63) / 64), blk, 0, s, w.S, w.cn, (const int*)nullptr, k2, n,
                     (const void*)w.S, w.cn, k2, d, h2, w.bits, W, w.ctl);
        HSEFR_LAUNCH(ms_suppress_kernel, dim3(1), blk, 0, s, w.bits, W, k2, w.klist, w.ctl);
        if ((rc = launch_status("the suppression")) != HSEFR_OK) return rc;
        if ((rc = read_ctl(w.ctl, host, s, "the suppression")) != HSEFR_OK) return rc;
        k = host[CTL_CENTERS];
        internal = host[CTL_INTERNAL] || k < 1 || k > k2;
    }
    if (!internal) {
        HSEFR_LAUNCH(ms_centers_kernel, dim3((k + 3) / 4), blk, 0, s, w.S, w.cn, w.cint, w.klist, k, k2, d, centers, w.cn_out, intensity, w.ctl);
        if ((rc = assign(x, w.xn, n, centers, w.cn_out, k, d, labels, label_dist, s)) != HSEFR_OK) return rc;
    }
    HSEFR_LAUNCH(ms_info_kernel, dim3(1), dim3(64), 0, s, w.ctl, n_iter, work, info);
    if ((rc = launch_status("ms_info_kernel")) != HSEFR_OK) return rc;
    if ((rc = read_ctl(w.ctl, host, s, "the finish")) != HSEFR_OK) return rc;
    if (internal || host[CTL_INTERNAL]) {
        if (!host[CTL_INTERNAL]) {                   // a count the host refused: say so in info as well
            const int one = 1;
            (void)hipMemcpyAsync(info + HSEFR_SHIFT_INFO_INTERNAL, &one, 4, hipMemcpyHostToDevice, s);
            (void)hipStreamSynchronize(s);
        }
        set_error("shift_fit: internal error: an index or a count left its bound on the device (active=%d, means=%d, centres=%d of n=%d)", na, k2,
                  k, n);
        return HSEFR_ERR_HIP;
    }
    return HSEFR_OK;
}

int shift_assign(const float* q, int nq, int d, const double* centers, int k, int* labels, double* dist, hipStream_t s) {
    HSEFR_REQUIRE(q && centers && labels && dist, HSEFR_ERR_INVALID, "shift_assign: null pointer");
    HSEFR_REQUIRE(nq >= 1 && k >= 1, HSEFR_ERR_INVALID, "shift_assign: nq=%d, k=%d", nq, k);
    HSEFR_REQUIRE(shape_supported(nq, d) && k <= HSEFR_SHIFT_MAX_N, HSEFR_ERR_UNSUPPORTED,
                  "shift_assign: nq=%d, k=%d, d=%d (nq, k <= %d, d a multiple of %d up to %d)", nq, k, d, HSEFR_SHIFT_MAX_N, HSEFR_SHIFT_D_MULTIPLE,
                  HSEFR_SHIFT_MAX_D);
    double* norms = nullptr;
    const size_t bytes = (size_t)(nq + k) * 8;
    if (hipMallocAsync((void**)&norms, bytes, s) != hipSuccess || !norms) {
        (void)hipGetLastError();
        set_error("shift_assign: no stream-ordered workspace (%zu bytes)", bytes);
        return HSEFR_ERR_NOMEM;
    }
    HSEFR_LAUNCH(ms_norms_kernel<false>, dim3((nq + 3) / 4), dim3(256), 0, s, (const void*)q, nq, d, norms);
    HSEFR_LAUNCH(ms_norms_kernel<true>, dim3((k + 3) / 4), dim3(256), 0, s, (const void*)centers, k, d, norms + nq);
    const int rc = assign(q, norms, nq, centers, norms + nq, k, d, labels, dist, s);
    (void)hipFreeAsync(norms, s);
    return rc;
}

}  // namespace

}  // namespace hsefr

extern "C" {

__attribute__((visibility("default"))) int hsefr_shift_version(void) { return HSEFR_SHIFT_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_shift_last_error(void) { return hsefr::g_error; }

__attribute__((visibility("default"))) size_t hsefr_shift_workspace_bytes(int n, int d) {
    return hsefr::shape_supported(n, d) ? hsefr::carve(nullptr, n, d).bytes : 0;
}

__attribute__((visibility("default"))) int hsefr_shift_fit(const float* x, int n, int d, double bandwidth, int max_iter, double* centers,
                                                           int32_t* intensity, int32_t* labels, double* label_dist, int32_t* info,
                                                           void* workspace, size_t workspace_bytes, void* stream) {
    return hsefr::shift_fit(x, n, d, bandwidth, max_iter, centers, intensity, labels, label_dist, info, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

__attribute__((visibility("default"))) int hsefr_shift_assign(const float* q, int nq, int d, const double* centers, int k, int32_t* labels,
                                                              double* dist, void* stream) {
    return hsefr::shift_assign(q, nq, d, centers, k, labels, dist, (hipStream_t)stream);
}

}  // extern "C"
