// DBSCAN on device (sklearn.cluster.DBSCAN(eps, min_samples, metric="precomputed") of get_facial_clusters, facial_clustering.py:260-265)
// with scikit-learn's labels, from linkage_scan.h's two distance sources and without an N x N matrix on the features path.
//
// The rule has no traversal order in it.  N(i) = {j : w(i,j) <= eps} + {i}; i is core when |N(i)| >= min_samples.  Core clusters are the
// connected components of the core points joined by core-core edges with w <= eps; the seed of a cluster is its smallest core index,
// and clusters are numbered in increasing seed order.  A non-core point with a core neighbour takes the cluster of the smallest seed
// among its core neighbours (dbscan_inner expands clusters from the lowest unlabelled core index and a border point keeps its first
// label); every other point is noise (-1).  A call:
//   1. degree        per row: |{j != i : w <= eps}| + 1 >= min_samples -> core[i]           (one row scan)
//   2. Boruvka       linkage.hip's rounds with the filter "both ends core and w <= eps": label[] = core component roots
//                    (rounds used + 1 row scans; the first round that hooks nothing ends the rest)
//   3. seeds         atomicMin of the core index per root, then cs[j] = that seed for core j, INT_MAX for the rest
//   4. border        per non-core row: min cs[j] over w <= eps                                (one row scan)
//   5. numbering     one workgroup ranks the seeds (core && cs[i] == i) by a ballot scan; labels[i] = rank[seed of i] or -1.
// Features are compared as w <= eps_f, eps_f the largest float <= eps: for a float w that is (double)w <= eps.  Workspace O(n),
// stream-ordered, refused before any launch; nothing is synchronised.
#include <math.h>

#include "linkage_scan.h"

namespace hsefr {

namespace {

constexpr int NONE = 0x7fffffff;

__global__ __launch_bounds__(256) void db_init_kernel(int* __restrict__ seed, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) seed[i] = NONE;
}

// BORDER == false: core[i] = |{j != i : w <= eps}| + 1 >= min_samples.  BORDER == true: out[i] = min cs[j] over j != i with w <= eps,
// for the workgroups that hold a non-core row.  The rows are FeatScan's; each keeps a count or a minimum.
template <bool BORDER>
__global__ __launch_bounds__(256) void db_scan_feat_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ born,
                                                           const float* __restrict__ year, float eps, int min_samples,
                                                           const int* __restrict__ cs, unsigned char* __restrict__ core,
                                                           int* __restrict__ out) {
    __shared__ int s_acc[4][32];
    const int q0 = blockIdx.x * 32;
    if (BORDER && !__syncthreads_or(threadIdx.x < 32 && q0 + (int)threadIdx.x < n && !core[q0 + threadIdx.x])) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31;
    link::FeatScan fs(x, n, d, born, year);
    int acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = BORDER ? NONE : 0;

    const int tiles = (n + 31) / 32;
    for (int gt = wave; gt < tiles; gt += 4) {
        const int gcol = gt * 32 + li;
        const int grow = min(gcol, n - 1);
        const int gcs = BORDER ? cs[grow] : 0;
        float v[16];
        fs.tile(grow, v);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool hit = gcol < n && gcol != q0 + fs.rr(r) && v[r] <= eps;
            if (BORDER) acc[r] = hit ? min(acc[r], gcs) : acc[r];
            else acc[r] += hit;
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            const int o = __shfl_xor(acc[r], m);
            acc[r] = BORDER ? min(acc[r], o) : acc[r] + o;
        }
    }
    if (li == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_acc[wave][fs.rr(r)] = acc[r];
    }
    __syncthreads();
    const int i = q0 + threadIdx.x;
    if (threadIdx.x < 32 && i < n) {
        if (BORDER) {
            out[i] = min(min(s_acc[0][threadIdx.x], s_acc[1][threadIdx.x]), min(s_acc[2][threadIdx.x], s_acc[3][threadIdx.x]));
        } else {
            const int deg = s_acc[0][threadIdx.x] + s_acc[1][threadIdx.x] + s_acc[2][threadIdx.x] + s_acc[3][threadIdx.x] + 1;
            core[i] = deg >= min_samples;
        }
    }
}

// the same two passes on the dense source (linkage_scan.h's upper-triangle tiles)
template <bool BORDER>
__global__ __launch_bounds__(256) void db_scan_dense_kernel(const double* __restrict__ D, int n, double eps, int min_samples,
                                                            const int* __restrict__ cs, unsigned char* __restrict__ core,
                                                            int* __restrict__ out) {
    __shared__ double s_t[64][65];
    __shared__ int s_cs[64];
    const int t = threadIdx.x, ri = t >> 2, sub = t & 3;
    const int r0 = blockIdx.x * 64, row = r0 + ri;
    if (BORDER && !__syncthreads_or(t < 64 && r0 + t < n && !core[r0 + t])) return;
    int acc = BORDER ? NONE : 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        __syncthreads();                                     // the previous tile has been read
        link::dense_stage(D, n, r0, c0, s_t);
        if (BORDER && t < 64) s_cs[t] = c0 + t < n ? cs[c0 + t] : NONE;
        __syncthreads();
#pragma unroll 4
        for (int m = 0; m < 16; ++m) {
            const int cj = sub + 4 * m, col = c0 + cj;
            const bool hit = col < n && col != row && link::dense_at(s_t, r0, c0, ri, cj) <= eps;
            if (BORDER) acc = hit ? min(acc, s_cs[cj]) : acc;
            else acc += hit;
        }
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
        const int o = __shfl_xor(acc, m);
        acc = BORDER ? min(acc, o) : acc + o;
    }
    if (sub == 0 && row < n) {
        if (BORDER) out[row] = acc;
        else core[row] = acc + 1 >= min_samples;
    }
}

__global__ __launch_bounds__(256) void db_seed_kernel(const int* __restrict__ label, const unsigned char* __restrict__ core,
                                                      int* __restrict__ seed, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && core[i]) atomicMin(&seed[label[i]], i);
}

__global__ __launch_bounds__(256) void db_cs_kernel(const int* __restrict__ label, const unsigned char* __restrict__ core,
                                                    const int* __restrict__ seed, int* __restrict__ cs, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) cs[i] = core[i] ? seed[label[i]] : NONE;
}

// rank[i] = the number of seeds before i, by one workgroup of 1024 in chunks: a ballot per wave, the 16 wave counts through LDS
__global__ __launch_bounds__(1024) void db_rank_kernel(const unsigned char* __restrict__ core, const int* __restrict__ cs,
                                                       int* __restrict__ rank, int n) {
    __shared__ int s_w[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 1024) {
        const int i = c0 + threadIdx.x;
        const bool seed = i < n && core[i] && cs[i] == i;
        const unsigned long long m = __ballot(seed);
        if (lane == 0) s_w[wave] = __popcll(m);
        __syncthreads();
        int before = base, total = base;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0;
            total += s_w[w];
        }
        if (i < n) rank[i] = before + __popcll(m & ((1ull << lane) - 1));
        base = total;
        __syncthreads();                                     // s_w is rewritten by the next chunk
    }
}

__global__ __launch_bounds__(256) void db_label_kernel(const unsigned char* __restrict__ core, const int* __restrict__ cs,
                                                       const int* __restrict__ border, const int* __restrict__ rank,
                                                       int* __restrict__ labels, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = core[i] ? cs[i] : border[i];
    labels[i] = s == NONE ? -1 : rank[s];
}

}  // namespace

int launch_dbscan(const DistSource& src, double eps, int min_samples, int* labels, unsigned char* core, hipStream_t s) {
    const int n = src.n;
    // Boruvka's workspace, then int arrays seed, cs, border, rank, then the core flags when the caller keeps none
    const size_t bytes = boruvka_bytes(n) + (size_t)n * 4 * 4 + (core ? 0 : (size_t)n);
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("dbscan: no stream-ordered workspace (%zu bytes) for n=%d", bytes, n);
        return HSEFR_ERR_NOMEM;
    }
    int* seed = (int*)(ws + boruvka_bytes(n));
    int* cs = seed + n;
    int* border = cs + n;
    int* rank = border + n;
    if (!core) core = (unsigned char*)(rank + n);
    float eps_f = (float)eps;
    if ((double)eps_f > eps) eps_f = nextafterf(eps_f, 0.f);

    const dim3 blk(256), g1((n + 255) / 256), gf((n + 31) / 32), gd((n + 63) / 64);
    HSEFR_LAUNCH(db_init_kernel, g1, blk, 0, s, seed, n);
    if (src.dense)
        HSEFR_LAUNCH(db_scan_dense_kernel<false>, gd, blk, 0, s, src.dense, n, eps, min_samples, cs, core, border);
    else
        HSEFR_LAUNCH(db_scan_feat_kernel<false>, gf, blk, 0, s, src.x, n, src.d, src.born, src.year, eps_f, min_samples, cs, core, border);
    const int* label = boruvka_rounds(src, core, eps_f, eps, ws, nullptr, nullptr, nullptr, s);
    HSEFR_LAUNCH(db_seed_kernel, g1, blk, 0, s, label, core, seed, n);
    HSEFR_LAUNCH(db_cs_kernel, g1, blk, 0, s, label, core, seed, cs, n);
    if (src.dense)
        HSEFR_LAUNCH(db_scan_dense_kernel<true>, gd, blk, 0, s, src.dense, n, eps, min_samples, cs, core, border);
    else
        HSEFR_LAUNCH(db_scan_feat_kernel<true>, gf, blk, 0, s, src.x, n, src.d, src.born, src.year, eps_f, min_samples, cs, core, border);
    HSEFR_LAUNCH(db_rank_kernel, dim3(1), dim3(1024), 0, s, core, cs, rank, n);
    HSEFR_LAUNCH(db_label_kernel, g1, blk, 0, s, core, cs, border, rank, labels, n);
    const int rc = launch_status("dbscan");
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace hsefr
