// Scores of flat clusterings on the device, for the clustering study's threshold sweeps (facial_clustering_test.py:416-499):
// hsefr_flat_cuts turns one dendrogram's leaf order and gap heights into a row of labels per threshold, hsefr_partition_scores turns
// rows of labels into the integer counts and fp64 sums behind ARI, AMI, homogeneity / completeness / V-measure and B-cubed.
//
// No R x C contingency table is formed.  A row's non-zero cells are the runs of its sorted (cluster, class) keys:
//   0. lf[m] = lgamma(m + 1) for m = 0 .. n (the hypergeometric weights of the expected mutual information read it)
//   1. classes   one workgroup sorts (y_true, item) keys; the runs give every item its class index t, the class sizes a, H_true,
//                sum a^2, and through a histogram of the sizes the DISTINCT class sizes with their multiplicities
//   2. rows      one workgroup per row sorts (cluster key << 32 | t) -- a negative label's cluster key is 2^31 + item, a cluster of its
//                own -- then ranks the cell starts and the cluster starts by ballot scans, reduces the cell and cluster sums, compacts
//                the histogram of cluster sizes into the distinct sizes, and evaluates the EMI once per pair of distinct sizes,
//                weighted by the product of the multiplicities (at most about sqrt(2n) distinct sizes a side).
// The sort is a bitonic network over the keys padded to a power of two: in LDS up to 16384 keys (128 KiB of the CU's 160 KiB; 8-byte
// keys read at unit stride by a wave's lanes, the partner run at a power-of-two distance, touch every one of the 64 4-byte banks twice per
// access, which is what a ds_read_b64 costs anyway), in the row's global workspace above that.  Equal keys are equal values, so the
// sorted array does not depend on how the network treats ties.
// Bit-identical results: integer atomics only (the size histograms and each class's sum of n_ij^2, whose sums do not depend on the
// order of the additions; the first B-cubed sum is added class by class from the latter, so exact ties between labellings stay ties), every
// fp64 sum is a fixed per-thread sequence followed by a fixed tree, and a row reads nothing another row writes.
// Workspace O(rows * n), stream-ordered, refused before any launch; nothing is synchronised.
#include <math.h>

#include "common.h"

namespace hsefr {

namespace {

typedef unsigned long long u64;
constexpr int NT = 1024;                 // threads of the sorting, class and flat-cut workgroups
constexpr int RT = 512;                  // threads of a row's scoring workgroup (256 registers a lane: the EMI loop does not spill)
constexpr int LDS_KEYS = 16384;          // keys the LDS sort holds (128 KiB)

struct ClassInfo {                       // what the class pass leaves for the rows
    long long sum_a2;
    double h_true;
    int classes, distinct;
};

// exclusive rank of this thread's flag among the flags of the workgroup's chunk, on top of `base`; base becomes the running total.
// Every thread of the workgroup (T threads) calls it.  s_w = T / 64 ints.
template <int T>
__device__ inline int chunk_rank(bool flag, int& base, int* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 m = __ballot(flag);
    if (lane == 0) s_w[wave] = __popcll(m);
    __syncthreads();
    int before = base, total = base;
#pragma unroll
    for (int w = 0; w < T / 64; ++w) {
        before += w < wave ? s_w[w] : 0;
        total += s_w[w];
    }
    __syncthreads();                     // s_w is rewritten by the next call
    base = total;
    return before + __popcll(m & ((1ull << lane) - 1));
}

// sums over the workgroup in a fixed shape: a butterfly per wave (lane 0's association is the one kept), the wave sums in order
template <int NTH, class T>
__device__ inline T block_sum(T v, T* s_t) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0) s_t[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = 0;
#pragma unroll
    for (int w = 0; w < NTH / 64; ++w) r += s_t[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void ps_lgamma_kernel(double* __restrict__ lf, int n) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m <= n) lf[m] = lgamma((double)m + 1.0);
}

// keys [blockIdx.x][P] = the sorted keys of row blockIdx.x of src [rows][n], padded with ~0.  t == null: (value, item) keys of the class
// pass; else (cluster key, t[item]).  LDS: the network runs in LDS (P <= LDS_KEYS), else in the output array itself.
template <bool LDS>
__global__ __launch_bounds__(NT) void ps_sort_kernel(const int* __restrict__ src, const int* __restrict__ t, int n, int P,
                                                     u64* __restrict__ keys) {
    __shared__ u64 s_keys[LDS ? LDS_KEYS : 1];
    const int* row = src + (size_t)blockIdx.x * n;
    u64* out = keys + (size_t)blockIdx.x * P;
    u64* k = LDS ? s_keys : out;
    for (int i = threadIdx.x; i < P; i += NT) {
        u64 key = ~0ull;
        if (i < n) {
            const int v = row[i];
            if (!t) key = ((u64)(unsigned)v << 32) | (unsigned)i;
            else key = ((u64)(v >= 0 ? (unsigned)v : 0x80000000u | (unsigned)i) << 32) | (unsigned)t[i];
        }
        k[i] = key;
    }
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int idx = threadIdx.x; idx < P / 2; idx += NT) {
                const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1));
                const int l = i | j;
                const u64 a = k[i], b = k[l];
                if ((a > b) == ((i & kk) == 0)) {
                    k[i] = b;
                    k[l] = a;
                }
            }
            __syncthreads();
        }
    }
    if (LDS)
        for (int i = threadIdx.x; i < P; i += NT) out[i] = k[i];
}

// hist[s] = how many groups have size s (1 <= s <= n) -> the sizes present, ascending, with their counts; returns how many.  The counts
// were added by atomics, which live in L2: they are read there too, past an L1 line a neighbouring array's load may have brought in
template <int T>
__device__ inline int compact_sizes(const int* __restrict__ hist, int n, int* __restrict__ sizes, int* __restrict__ mult, int* s_w) {
    int base = 0;
    for (int c0 = 1; c0 <= n; c0 += T) {
        const int s = c0 + threadIdx.x;
        const int h = s <= n ? __hip_atomic_load(&hist[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        const int r = chunk_rank<T>(h > 0, base, s_w);
        if (h > 0) {
            sizes[r] = s;
            mult[r] = h;
        }
    }
    return base;
}

// the class pass, one workgroup: keys = the sorted (y_true, item) keys
__global__ __launch_bounds__(NT) void ps_class_kernel(const u64* __restrict__ keys, int n, int* __restrict__ t, int* __restrict__ a,
                                                      int* __restrict__ cpos, int* __restrict__ hist, int* __restrict__ sa,
                                                      int* __restrict__ ma, ClassInfo* __restrict__ info) {
    __shared__ int s_w[NT / 64];
    __shared__ double s_d[NT / 64];
    __shared__ long long s_l[NT / 64];
    int R = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int p = c0 + threadIdx.x;
        const u64 key = p < n ? keys[p] : 0;
        const bool start = p < n && (p == 0 || (unsigned)(keys[p - 1] >> 32) != (unsigned)(key >> 32));
        const int r = chunk_rank<NT>(start, R, s_w);
        if (p < n) t[(unsigned)key] = r + start - 1;
        if (start) cpos[r] = p;
    }
    if (threadIdx.x == 0) cpos[R] = n;
    __syncthreads();
    const double ln_n = log((double)n);
    double h = 0;
    long long a2 = 0;
    for (int c = threadIdx.x; c < R; c += NT) {
        const int sz = cpos[c + 1] - cpos[c];
        a[c] = sz;
        atomicAdd(&hist[sz], 1);
        a2 += (long long)sz * sz;
        h -= (double)sz / n * (log((double)sz) - ln_n);
    }
    h = block_sum<NT>(h, s_d);
    a2 = block_sum<NT>(a2, s_l);             // (its barriers also publish hist)
    const int da = compact_sizes<NT>(hist, n, sa, ma, s_w);
    if (threadIdx.x == 0) {
        info->sum_a2 = a2;
        info->h_true = h;
        info->classes = R;
        info->distinct = da;
    }
}

// ints of one row's arrays (RowWs), even so that every row's 8-byte array stays aligned
__host__ __device__ inline size_t row_stride(int n) { return (8 * (size_t)n + 5 + 1) & ~(size_t)1; }

struct RowWs {                           // one row's arrays
    u64* cls_nij2;                       // [n] sum of n_ij^2 over each class's cells, zeroed by the caller
    int* cellpos;                        // [n + 1] where each cell starts in the sorted keys
    int* cluspos;                        // [n + 1] where each cluster starts
    int* cellclu;                        // [n] the cluster of each cell
    int* hist;                           // [n + 1] clusters per size, zeroed by the caller
    int* sb;                             // [n + 1] distinct cluster sizes
    int* mb;                             // [n + 1] their multiplicities
};

// one workgroup per row: keys = the row's sorted (cluster key, class) keys
__global__ __launch_bounds__(RT) void ps_row_kernel(const u64* __restrict__ keys_all, int n, int P, const int* __restrict__ a,
                                                    const int* __restrict__ sa, const int* __restrict__ ma,
                                                    const ClassInfo* __restrict__ info, const double* __restrict__ lf,
                                                    int* __restrict__ row_ints, long long* __restrict__ counts,
                                                    double* __restrict__ stats) {
    __shared__ int s_w[RT / 64];
    __shared__ double s_d[RT / 64];
    __shared__ long long s_l[RT / 64];
    const int row = blockIdx.x;
    const u64* keys = keys_all + (size_t)row * P;
    const size_t n1 = (size_t)n + 1;
    RowWs w;
    int* base = row_ints + (size_t)row * row_stride(n);
    w.cls_nij2 = (u64*)base;
    w.hist = base + 2 * (size_t)n;       // (the two arrays that start at zero lie together: one clear covers them)
    w.cellpos = w.hist + n1;
    w.cluspos = w.cellpos + n1;
    w.sb = w.cluspos + n1;
    w.mb = w.sb + n1;
    w.cellclu = w.mb + n1;

    int cells = 0, clusters = 0;
    for (int c0 = 0; c0 < n; c0 += RT) {
        const int p = c0 + threadIdx.x;
        const u64 key = p < n ? keys[p] : 0;
        const u64 prev = p > 0 && p < n ? keys[p - 1] : 0;
        const bool cell = p < n && (p == 0 || prev != key);
        const bool clus = p < n && (p == 0 || (unsigned)(prev >> 32) != (unsigned)(key >> 32));
        const int rc = chunk_rank<RT>(cell, cells, s_w);
        const int rj = chunk_rank<RT>(clus, clusters, s_w);
        if (cell) {
            w.cellpos[rc] = p;
            w.cellclu[rc] = rj + clus - 1;
        }
        if (clus) w.cluspos[rj] = p;
    }
    if (threadIdx.x == 0) {
        w.cellpos[cells] = n;
        w.cluspos[clusters] = n;
    }
    __syncthreads();

    const double dn = (double)n, ln_n = log(dn);
    double h_pred = 0;
    long long b2 = 0, big = 0, nonneg = 0;
    for (int j = threadIdx.x; j < clusters; j += RT) {
        const int p = w.cluspos[j], b = w.cluspos[j + 1] - p;
        atomicAdd(&w.hist[b], 1);
        b2 += (long long)b * b;
        big += b >= 2;
        nonneg += !(keys[p] >> 63);
        h_pred -= (double)b / dn * (log((double)b) - ln_n);
    }
    double mi = 0, s_a = 0, s_b = 0;
    long long nij2 = 0;
    for (int c = threadIdx.x; c < cells; c += RT) {
        const int p = w.cellpos[c], nij = w.cellpos[c + 1] - p, j = w.cellclu[c];
        const int ai = a[(unsigned)keys[p]], bj = w.cluspos[j + 1] - w.cluspos[j];
        const double sq = (double)nij * nij;
        nij2 += (long long)nij * nij;
        mi += (double)nij / dn * log(dn * nij / ((double)ai * bj));
        atomicAdd(&w.cls_nij2[(unsigned)keys[p]], (u64)nij * nij);
        s_b += sq / bj / dn;
    }
    h_pred = block_sum<RT>(h_pred, s_d);     // (the barriers also publish hist and cls_nij2)
    mi = block_sum<RT>(mi, s_d);
    // the first B-cubed sum class by class, from integer sums: two labellings that give every class the same sum of squares (a merge
    // of clusters that share no class does) get the same bits, so a threshold selection sees the tie the exact values have
    for (int c = threadIdx.x; c < info->classes; c += RT)
        s_a += (double)__hip_atomic_load(&w.cls_nij2[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / a[c] / dn;
    s_a = block_sum<RT>(s_a, s_d);
    s_b = block_sum<RT>(s_b, s_d);
    b2 = block_sum<RT>(b2, s_l);
    big = block_sum<RT>(big, s_l);
    nonneg = block_sum<RT>(nonneg, s_l);
    nij2 = block_sum<RT>(nij2, s_l);

    // expected mutual information, once per pair of distinct sizes
    const int db = compact_sizes<RT>(w.hist, n, w.sb, w.mb, s_w);
    __syncthreads();
    const int da = info->distinct;
    const double lf_n = lf[n];
    double emi = 0;
    for (long long q = threadIdx.x; q < (long long)da * db; q += RT) {
        const int ia = (int)(q / db), ib = (int)(q - (long long)ia * db);
        const int ai = sa[ia], bj = w.sb[ib];
        const double ab = (double)ai * bj;
        const double fixed = lf[ai] + lf[bj] + lf[n - ai] + lf[n - bj] - lf_n;
        const int lo = max(1, ai + bj - n), hi = min(ai, bj);
        double acc = 0;
        for (int k = lo; k <= hi; ++k) {
            const double g = fixed - lf[k] - lf[ai - k] - lf[bj - k] - lf[n - ai - bj + k];
            acc += (double)k / dn * log(dn * k / ab) * exp(g);
        }
        emi += (double)ma[ia] * w.mb[ib] * acc;
    }
    emi = block_sum<RT>(emi, s_d);

    if (threadIdx.x == 0) {
        long long* c = counts + (size_t)row * 8;
        c[0] = info->classes;
        c[1] = clusters;
        c[2] = big;
        c[3] = nonneg;
        c[4] = cells;
        c[5] = nij2;
        c[6] = info->sum_a2;
        c[7] = b2;
        double* st = stats + (size_t)row * 6;
        st[0] = info->h_true;
        st[1] = h_pred;
        st[2] = mi;
        st[3] = emi;
        st[4] = s_a;
        st[5] = s_b;
    }
}

// labels[r][order[p]] = 1 + #{q < p : gaps[q] > thresholds[r]}, one workgroup per threshold
__global__ __launch_bounds__(NT) void ps_flat_cuts_kernel(const int* __restrict__ order, const double* __restrict__ gaps, int n,
                                                          const double* __restrict__ thresholds, int* __restrict__ labels) {
    __shared__ int s_w[NT / 64];
    const double thr = thresholds[blockIdx.x];
    int* out = labels + (size_t)blockIdx.x * n;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += NT) {
        const int p = c0 + threadIdx.x;
        const bool cut = p >= 1 && p < n && gaps[p - 1] > thr;
        const int r = chunk_rank<NT>(cut, base, s_w);
        if (p < n) {
            const int o = order[p];
            if ((unsigned)o < (unsigned)n) out[o] = 1 + r + cut;
        }
    }
}

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

}  // namespace

int launch_flat_cuts(const int* order, const double* gaps, int n, const double* thresholds, int rows, int* labels, hipStream_t s) {
    HSEFR_LAUNCH(ps_flat_cuts_kernel, dim3(rows), dim3(NT), 0, s, order, gaps, n, thresholds, labels);
    return launch_status("flat_cuts");
}

int launch_partition_scores(const int* y_true, const int* labels, int n, int rows, long long* counts, double* stats, hipStream_t s) {
    int P = 2;
    while (P < n) P <<= 1;
    const size_t n1 = (size_t)n + 1, row_ints = row_stride(n), class_ints = 2 * (size_t)n + 4 * n1;
    // 8-byte arrays first: lf, the class keys, the rows' keys, the class info; then the class pass's ints and the rows' ints
    const size_t off_ckeys = n1 * 8, off_rkeys = off_ckeys + (size_t)P * 8, off_info = off_rkeys + (size_t)rows * P * 8;
    const size_t off_cints = off_info + align8(sizeof(ClassInfo)), off_rints = off_cints + align8(class_ints * 4);
    const size_t bytes = off_rints + (size_t)rows * row_ints * 4;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("partition_scores: no stream-ordered workspace (%zu bytes) for n=%d, rows=%d", bytes, n, rows);
        return HSEFR_ERR_NOMEM;
    }
    double* lf = (double*)ws;
    u64* ckeys = (u64*)(ws + off_ckeys);
    u64* rkeys = (u64*)(ws + off_rkeys);
    ClassInfo* info = (ClassInfo*)(ws + off_info);
    int* t = (int*)(ws + off_cints);
    int* a = t + n;
    int* cpos = a + n;
    int* chist = cpos + n1;
    int* sa = chist + n1;
    int* ma = sa + n1;
    int* rints = (int*)(ws + off_rints);

    int rc = HSEFR_OK;
    if (!route_probe()) {
        // the size histograms start at zero (the other arrays are written before they are read)
        hipError_t e = hipMemsetAsync(chist, 0, n1 * 4, s);
        if (e == hipSuccess) e = hipMemset2DAsync(rints, row_ints * 4, 0, (2 * (size_t)n + n1) * 4, rows, s);
        if (e != hipSuccess) {
            set_error("partition_scores: clearing the histograms failed: %s", hipGetErrorString(e));
            rc = HSEFR_ERR_HIP;
        }
    }
    if (rc == HSEFR_OK) {
        HSEFR_LAUNCH(ps_lgamma_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, s, lf, n);
        if (P <= LDS_KEYS) HSEFR_LAUNCH(ps_sort_kernel<true>, dim3(1), dim3(NT), 0, s, y_true, (const int*)nullptr, n, P, ckeys);
        else HSEFR_LAUNCH(ps_sort_kernel<false>, dim3(1), dim3(NT), 0, s, y_true, (const int*)nullptr, n, P, ckeys);
        HSEFR_LAUNCH(ps_class_kernel, dim3(1), dim3(NT), 0, s, ckeys, n, t, a, cpos, chist, sa, ma, info);
        if (P <= LDS_KEYS) HSEFR_LAUNCH(ps_sort_kernel<true>, dim3(rows), dim3(NT), 0, s, labels, (const int*)t, n, P, rkeys);
        else HSEFR_LAUNCH(ps_sort_kernel<false>, dim3(rows), dim3(NT), 0, s, labels, (const int*)t, n, P, rkeys);
        HSEFR_LAUNCH(ps_row_kernel, dim3(rows), dim3(RT), 0, s, rkeys, n, P, a, sa, ma, info, lf, rints, counts, stats);
        rc = launch_status("partition_scores");
    }
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace hsefr
